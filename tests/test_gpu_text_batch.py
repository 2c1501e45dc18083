"""The batched text loop on the device (GeneratorBase._generate_text_batch: ragged prefill, text-feedback chunks, retirement at EOS /
max_frames, admission into freed rows): every utterance's text equals its own single-row run through _generate_text — the
one-by-one loop this change does not touch — greedy, n-gram-filtered and sampled under per-utterance keys, and the reference's
golden ids where they exist.  Toy model, chunk_frames = 4 so that a session crosses many boundaries in a few frames."""
import pytest
import torch

from helpers import build_toy_module, load_golden_lm, toy_state_dict
from test_gpu_ngram import _asr_prompt, _decided_prefix, _prompt
from test_ngram import TA, load_golden

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
MAX_FRAMES = [10, 3, 4, 5, 9, 1, 8]
_gens, _single = {}, {}


def generator(dtype):
    """One asr Generator per dtype and process (the parameters' dtype selects the plan), chunk_frames = 4."""
    if dtype not in _gens:
        from uniaudio2_amd.evaluation.asr_task import Generator
        m = build_toy_module()
        m.load_state_dict(toy_state_dict(load_golden_lm()[1]))
        gen = Generator(m.to("cuda").to(dtype), TA, text_tokenizer_path="ids")
        gen.chunk_frames = 4
        _gens[dtype] = gen
    return _gens[dtype]


def prompts7():
    """asr1 of the reference's golden and six prompts of the golden's shape, seven distinct lengths."""
    d, _ = load_golden_lm()
    asr1 = (torch.from_numpy(d["asr1_tokens"]).long(), torch.from_numpy(d["asr1_mask"]).bool())
    rest = [_asr_prompt(70 + i, n_text, n_audio) for i, (n_text, n_audio) in enumerate([(3, 5), (6, 11), (2, 3), (8, 8), (5, 19), (4, 2)])]
    out = [asr1] + rest
    assert len({int(t.shape[0]) for t, _ in out}) == 7
    return out


def single(dtype, tag, b, prompt, max_frames, topk=1, temperature=1.0, seed=None, top_p=0.0, ngram=0, fallback=499):
    """The reference of every comparison: utterance b alone through _generate_text (B = 1, the shared sampler stream keyed by `seed`),
    computed once per (dtype, tag, b, ...) and shared."""
    key = (dtype, tag, b, max_frames, topk, temperature, seed, top_p, ngram)
    if key not in _single:
        gen = generator(dtype)
        m = gen._model
        m.set_sampling(1)                                        # whatever key comes next is a new one: the draw index rewinds
        m.sampling_seed, gen.top_p = seed, top_p
        try:
            _single[key] = gen._generate_text(prompt[0], prompt[1], topk=topk, temperature=temperature, max_frames=max_frames,
                                              no_repeat_ngram_size=ngram, ngram_fallback=fallback)
        finally:
            m.sampling_seed, gen.top_p = None, 0.0
            gen._set_sampling(1, 1.0)                            # the nucleus filter off again
    return _single[key]


# ---- 1. greedy -----------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("batch_size", [2, 3, 6, None])
def test_greedy_texts_equal_their_single_row_runs(dtype, batch_size):
    """batch_size 6 and None take the live row count across the 5 / 6 switch between the few-row and the weights-stationary kernel
    while rows retire."""
    gen, ps = generator(dtype), prompts7()
    want = [single(dtype, "p7", b, ps[b], MAX_FRAMES[b]) for b in range(7)]
    got = gen._generate_text_batch(ps, topk=1, max_frames=MAX_FRAMES, batch_size=batch_size)
    assert [len(t.split()) for t in got] == MAX_FRAMES           # the toy vocabulary has no EOS: every utterance runs its frames
    assert got == want
    if dtype == torch.float32:
        assert [int(t) for t in got[0].split()] == load_golden_lm()[0]["asr1_samples"][:, 0, 0].tolist()
    assert len(set(got)) == 7


# ---- 2. n-gram -----------------------------------------------------------------------------------------------------------------
NG_FRAMES = [24, 16, 24, 12, 20]                                 # 96 frames in all through two rows, capacity 24: no row passes it


def _ngram_prompts():
    g = load_golden()
    return [_prompt(g, "ng2"), _prompt(g, "ng3"), _prompt(g, "ng3b"), _asr_prompt(61, 4, 9), _asr_prompt(62, 7, 13)]


def _one_by_one_ngram(dtype, n, b, prompt):
    """generate_asr_with_ngram_sampling for utterance b alone (its 500 frames), once per (dtype, n, b)."""
    key = (dtype, "ngram-method", n, b)
    if key not in _single:
        gen = generator(dtype)
        tp, rt, st = torch.tensor([128000, 1, 128001]), torch.zeros(2, 8), torch.zeros(3, 8)
        gen.prepare_asr_task = lambda a, r, s: prompt            # the prompt stands in for prepare_asr_task's layout
        try:
            _single[key] = gen.generate_asr_with_ngram_sampling(tp, "asr", semantic_token=st, reason_token=rt, topk=1,
                                                                no_repeat_ngram_size=n, fallback_token=499)
        finally:
            del gen.prepare_asr_task
    return _single[key]


@pytest.mark.parametrize("n", [2, 3])
def test_ngram_session_longer_than_the_capacity_equals_one_by_one(n):
    dtype = torch.float32
    gen, ps = generator(dtype), _ngram_prompts()
    d, meta = load_golden()
    assert meta["fallback"] == 499 and sum(NG_FRAMES) > max(NG_FRAMES)
    got = gen._generate_text_batch(ps, topk=1, max_frames=NG_FRAMES, no_repeat_ngram_size=n, ngram_fallback=499, batch_size=2)    # not refused
    assert gen._model._ngram is None                             # the filter is off after the call
    for b, text in enumerate(got):
        ids = text.split()
        assert len(ids) == NG_FRAMES[b]
        assert ids == _one_by_one_ngram(dtype, n, b, ps[b]).split()[:NG_FRAMES[b]], b          # the filter is causal: a prefix of the 500 frames
    assert any("499" in t.split() for t in got)                 # bans fired
    banned = 0                                                   # bans of the reference inside the compared frames
    for b, name in enumerate(["ng2", "ng3", "ng3b"]):
        if {c["name"]: c["n"] for c in meta["cases"]}[name] == n:
            k = min(_decided_prefix((d, meta), name), NG_FRAMES[b])
            assert [int(t) for t in got[b].split()][:k] == d[f"{name}_final"][:k].tolist(), name
            banned += int((d[f"{name}_cand"][:k] != d[f"{name}_final"][:k]).sum())
    assert banned >= 1


def test_ngram_bound_follows_the_rows_and_a_plain_session_is_refused_where_it_was():
    gen = generator(torch.float32)
    m, ps = gen._model, [(t.cuda(), k.cuda()) for t, k in _ngram_prompts()]
    if m._st["B"] < 2:
        m.setup_caches(2)
    m.set_sampling(1)
    try:
        # a single session without admission: refused exactly at its capacity
        m.begin_ragged(ps[:1])
        m.set_ngram(3, 499, capacity=20)
        m.generate_frames(16, 1, 1)
        with pytest.raises(ValueError, match="n-gram history full: 16 \\+ 8"):
            m.generate_frames(8, 1, 1)
        m.generate_frames(4, 1, 1)
        with pytest.raises(ValueError, match="n-gram history full: 20 \\+ 1"):
            m.generate_frames(1, 1, 1)
        # with admission the bound is the longest LIVE row's: 14 frames in all under capacity 8
        m.begin_ragged(ps[:2])
        m.set_ngram(3, 499, capacity=8)
        m.generate_frames(6, 2, 1)
        m.retire_rows([1], 2)
        m.admit_rows(ps[2:3], 1)
        assert m._st["ngram_len"][:2].tolist() == [6, 0]
        m.generate_frames(2, 2, 1)                               # row 0 is full now, the admitted row holds 2
        with pytest.raises(ValueError, match="n-gram history full: 8 \\+ 1"):
            m.generate_frames(1, 2, 1)
        m.retire_rows([1], 2)
        m.generate_frames(6, 1, 1)                               # the admitted row alone: 2 + 6
        assert int(m._st["ngram_len"][0]) == 8
        with pytest.raises(ValueError, match="n-gram history full: 8 \\+ 1"):
            m.generate_frames(1, 1, 1)
    finally:
        m.set_ngram(0)


# ---- 3. sampled ----------------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("top_p", [0.0, 0.8], ids=["topk", "topk+topp"])
def test_sampled_texts_equal_their_single_runs_under_their_own_keys(dtype, top_p):
    gen, ps = generator(dtype), prompts7()
    seeds = [0x5EED0000FFFFFFF0 + 977 * b for b in range(7)]
    want = [single(dtype, "p7", b, ps[b], MAX_FRAMES[b], topk=5, temperature=0.9, seed=seeds[b], top_p=top_p) for b in range(7)]
    greedy = [single(dtype, "p7", b, ps[b], MAX_FRAMES[b]) for b in range(7)]
    assert want != greedy                                        # sampling is at work
    gen.top_p = top_p
    try:
        for batch_size in (2, 4):
            got = gen._generate_text_batch(ps, topk=5, temperature=0.9, max_frames=MAX_FRAMES, seeds=seeds, batch_size=batch_size)
            assert got == want, batch_size
    finally:
        gen.top_p = 0.0
        gen._set_sampling(1, 1.0)
    assert not gen._model._row_streams


# ---- 4. the expert skip around admissions -------------------------------------------------------------------------------------------
@DTYPES
def test_keeping_the_audio_experts_gives_the_same_ids(dtype, monkeypatch):
    """By default every frame but the first after the prefill and after each admission skips the audio experts; with
    UA2_KEEP_AUDIO_EXPERTS=1 none does.  Same ids: the skip never covers a row that still holds a prompt step."""
    gen, ps = generator(dtype), prompts7()
    default = gen._generate_text_batch(ps, topk=1, max_frames=MAX_FRAMES, batch_size=2)
    monkeypatch.setenv("UA2_KEEP_AUDIO_EXPERTS", "1")
    kept = gen._generate_text_batch(ps, topk=1, max_frames=MAX_FRAMES, batch_size=2)
    assert kept == default == [single(dtype, "p7", b, ps[b], MAX_FRAMES[b]) for b in range(7)]
