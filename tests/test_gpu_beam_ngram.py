"""The no-repeat-n-gram ban inside the beam search on the device (include/ua2hip.h ua2_beam_step_groups_ngram,
ua2_stage3_set_beam_ngram; Model_stage3.beam_search[_batch](no_repeat_ngram_size=n); --beam_no_repeat_ngram).

(a) On every launch of tests/beam_ngram_cases.py the step under the ban equals ua2_beam_step_groups on the host-masked logits bit for
    bit — cand_logp, cand_id, score, fin, len, parent, token, log, ctrl — and the float64 rule in ids, parents, fin and len;
(b) the written history set of every new live slot holds the float64 rule's ids, the read set and everything else keeps its words;
(c) n = 0 and ng = NULL are ua2_beam_step_groups; (d) bad arguments return non-zero with a message and launch nothing;
(e) beam_search(no_repeat_ngram_size=n) on the golden toy LM against the float64 search over the CPU oracle, in cases where the
    reference with and without the ban end in different beams, under test_gpu_beam.py's tolerance 2 * 5e-5 * factor * steps;
(f) identities without margins: chunking, graphs, expert skipping, the batch against the single searches, W = 1 against the greedy
    loop under set_ngram up to the step at which that filter first fires, the page tables afterwards;
(g) the command line writes the text of the model-level search."""
import ctypes as C

import numpy as np
import pytest
import torch

import beam_ngram_cases as nc
import beam_ngram_ref
import beam_ref
from beam_ref import FINISHED, LIVE
from helpers import build_oracle, build_product_model, build_toy_module, load_golden_lm, toy_state_dict
from test_gpu_beam import asr1, greedy_ids, scaled_sd, tiled_prompt
from test_gpu_beam_groups import DeviceBeams, four_prompts

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -3                                                                  # what no step writes into a history


@pytest.fixture(scope="module")
def golden():
    return load_golden_lm()


@pytest.fixture(scope="module")
def sd(golden):
    return toy_state_dict(golden[1])


def _bits(t):
    return t.view(torch.int32).cpu().numpy().copy()


class Launch:
    """The caller-owned state of one launch of G groups (tests/test_gpu_beam_groups.py's DeviceBeams, a guard group behind the last
    one) and, under the ban, the histories [G + 1][2][8][cap] with 64 guard words behind them."""

    def __init__(self, cases, ban=True):
        from uniaudio2_amd._lib import BeamNgram
        c0 = cases[0]
        self.cases, self.W, self.G, self.cap = cases, c0.W, len(cases), c0.cap
        self.st = DeviceBeams(c0.W, self.G, cap=nc.LOG_CAP, lp_n=c0.lp_n)
        for g, c in enumerate(cases):
            self.st.load(g, c.beam, c.step)
        self.hist = torch.full(((self.G + 1) * 2 * 8 * self.cap + 64,), SENT, dtype=torch.int32, device=DEV)
        sets = self.hist[:(self.G + 1) * 2 * 8 * self.cap].view(self.G + 1, 2, 8, self.cap)
        for g, c in enumerate(cases):
            for j, b in enumerate(c.beam):                                 # every slot's text, a finished slot's too: it must not ban
                ids = b.ids[:self.cap]
                sets[g, c.step & 1, j, :len(ids)] = torch.tensor(ids, dtype=torch.int32)
        self.sets, self.before = sets, self.hist.cpu().numpy().copy()
        self.ng = BeamNgram(c0.n if ban else 0, self.cap, self.hist.data_ptr())

    def run(self, x, ng="own"):
        """One step of all groups on x [G * W, ld] (numpy fp32): through the new entry point (ng: "own", None = NULL) or, ng = "plain",
        through ua2_beam_step_groups.  Returns the logits' bits after the launch."""
        from uniaudio2_amd import ops
        from uniaudio2_amd._lib import check, lib
        c0 = self.cases[0]
        logits = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
        if ng == "plain":
            check(lib.ua2_beam_step_groups(logits.data_ptr(), c0.ld, c0.V, self.W, self.G, c0.eos, C.byref(self.st.c), self.st.token.data_ptr(), 9,
                                           ops.stream()), "ua2_beam_step_groups")
        else:
            check(lib.ua2_beam_step_groups_ngram(logits.data_ptr(), c0.ld, c0.V, self.W, self.G, c0.eos, C.byref(self.st.c),
                                                 C.byref(self.ng) if ng == "own" else None, self.st.token.data_ptr(), 9, ops.stream()),
                  "ua2_beam_step_groups_ngram")
        torch.cuda.synchronize()
        return _bits(logits)

    def everything(self):
        """All a step may write, the guard group included, as integers."""
        return dict(groups=[self.st.fields(g) for g in range(self.G + 1)], cand_logp=_bits(self.st.cand_logp).tolist(),
                    cand_id=self.st.cand_id.cpu().tolist())


def _check_launch(cases):
    """(a) and (b) for one launch of len(cases) groups."""
    x = np.concatenate([c.x for c in cases])
    xm = np.concatenate([nc.masked(c) for c in cases])
    ban, plain = Launch(cases), Launch(cases)
    assert np.array_equal(ban.run(x), x.view(np.int32))                    # the logits stay read-only
    plain.run(xm, "plain")
    got, want = ban.everything(), plain.everything()
    for k in want:
        assert got[k] == want[k], (cases[0].name, k)
    assert np.array_equal(plain.hist.cpu().numpy(), plain.before)
    hist = ban.hist.cpu().numpy()
    expect = ban.before.copy().reshape(-1)
    sets = expect[:(ban.G + 1) * 2 * 8 * ban.cap].reshape(ban.G + 1, 2, 8, ban.cap)
    for g, c in enumerate(cases):
        new, parents, fed = nc.after(c)
        f = got["groups"][g]
        assert f["fin"][:c.W] == [b.fin for b in new] and f["len"][:c.W] == [b.len for b in new], c.name
        assert f["parent"][:c.W] == parents and [r[0] for r in f["token"]] == fed, c.name
        for t, b in enumerate(new):                                        # the other set: the text of every new live slot, up to cap
            if b.fin == LIVE:
                ids = b.ids[:c.cap]
                sets[g, (c.step & 1) ^ 1, t, :len(ids)] = ids
    assert np.array_equal(hist, expect), cases[0].name                     # the read set, the rows of other slots, the guards


@pytest.mark.parametrize("W", nc.WIDTHS)
@pytest.mark.parametrize("V", nc.SMALL)
def test_banned_step_equals_the_step_on_masked_logits(V, W):
    for case in nc.single_cases(V, W):
        _check_launch([case])


@pytest.mark.parametrize("W", nc.WIDTHS)
@pytest.mark.parametrize("V", nc.SMALL)
def test_three_groups_in_one_launch_and_each_alone(V, W):
    cases = nc.group_cases(V, W)
    _check_launch(cases)
    x = np.concatenate([c.x for c in cases])
    both = Launch(cases)
    both.run(x)
    for g, c in enumerate(cases):                                          # a group's result depends only on its own rows and history
        one = Launch([c])
        one.run(c.x)
        assert one.st.fields(0) == both.st.fields(g), c.name
        assert np.array_equal(_bits(one.st.cand_logp[0]), _bits(both.st.cand_logp[g])) and torch.equal(one.st.cand_id[0], both.st.cand_id[g])
        assert torch.equal(one.sets[0], both.sets[g]), c.name


def test_long_prefix_released_vocabulary_second_trip_and_over_capacity():
    for case in nc.special_cases():
        _check_launch([case])


def test_ban_off_is_the_existing_step():
    for case in nc.single_cases(9217, 5)[:4] + nc.group_cases(9217, 5)[:1]:
        want = Launch([case])
        want.run(case.x, "plain")
        for ng, ban in (("own", False), (None, True)):                     # n = 0 in the struct; no struct at all
            got = Launch([case], ban=ban)
            got.run(case.x, ng)
            assert got.everything() == want.everything(), (case.name, ng)
            assert np.array_equal(got.hist.cpu().numpy(), got.before)


def test_bad_arguments_launch_nothing():
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import BeamNgram, lib
    case = nc.single_cases(9217, 5)[0]
    L = Launch([case])
    before = L.everything()
    logits = torch.from_numpy(case.x).to(DEV)

    def call(ng, W=case.W, G=1, V=case.V, ld=case.ld, logits_ptr=logits.data_ptr()):
        rc = lib.ua2_beam_step_groups_ngram(logits_ptr, ld, V, W, G, case.eos, C.byref(L.st.c), C.byref(ng), L.st.token.data_ptr(), 9, ops.stream())
        return rc, lib.ua2_last_error().decode()
    h = L.hist.data_ptr()
    for ng, kw, what in [(BeamNgram(1, L.cap, h), {}, "2..16"), (BeamNgram(17, L.cap, h), {}, "2..16"), (BeamNgram(-3, L.cap, h), {}, "2..16"),
                         (BeamNgram(3, 0, h), {}, "capacity"), (BeamNgram(0, 0, h), {}, "capacity"), (BeamNgram(3, L.cap, None), {}, "NULL history"),
                         (BeamNgram(3, L.cap, h), dict(W=9), "beam width"), (BeamNgram(3, L.cap, h), dict(G=13), "groups"),
                         (BeamNgram(3, L.cap, h), dict(ld=case.V - 1), "W <= V <= ld"), (BeamNgram(3, L.cap, h), dict(logits_ptr=None), "NULL logits"),
                         (BeamNgram(3, L.cap, h), dict(V=48 * 1024 * 8 + 1, ld=48 * 1024 * 8 + 1), "bitmap")]:
        rc, msg = call(ng, **kw)
        assert rc != 0 and what in msg, (kw, msg)
    torch.cuda.synchronize()
    assert L.everything() == before and np.array_equal(L.hist.cpu().numpy(), L.before)


def test_six_steps_with_a_swap_and_a_fan_out():
    """The histories carried on the device from step to step (two slots swap parents, one parent has three children): after every
    step the written set holds the reference's texts, and the log walks back to them."""
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import BeamNgram, check, lib
    seq, plain = nc.sequence()
    rows = nc.sequence_rows()
    W, V, cap = nc.SEQ_W, nc.SEQ_V, nc.SEQ_CAP
    assert any(nc.has_swap(s["parents"]) for s in seq) and any(nc.has_fan_out(s["parents"]) for s in seq[1:])
    st = DeviceBeams(W, 1, cap=nc.SEQ_STEPS, lp_n=64)
    st.load(0, beam_ref.start(W), 0)
    hist = torch.full((2, 2, 8, cap), SENT, dtype=torch.int32, device=DEV)                # + a guard group
    ng = BeamNgram(nc.SEQ_N, cap, hist.data_ptr())
    for t, s in enumerate(seq):
        logits = torch.from_numpy(rows[t]).to(DEV)
        check(lib.ua2_beam_step_groups_ngram(logits.data_ptr(), V, V, W, 1, V + 3, C.byref(st.c), C.byref(ng), st.token.data_ptr(), 9, ops.stream()), "step")
        torch.cuda.synchronize()
        f = st.fields(0)
        assert f["parent"][:W] == s["parents"] and [r[0] for r in f["token"]] == s["fed"], t
        assert f["len"][:W] == [b.len for b in s["beam"]] and f["fin"][:W] == [b.fin for b in s["beam"]], t
        got = hist[0, (t & 1) ^ 1].cpu().tolist()
        for j, b in enumerate(s["beam"]):
            assert got[j][:b.len] == b.ids, (t, j)
    log = np.array(st.fields(0)["log"])
    assert [beam_ref.backtrack(log, j) for j in range(W)] == [b.ids for b in seq[-1]["beam"]] != plain
    assert (hist[1] == SENT).all() and (hist[0, :, W:] == SENT).all()


# ---- (e) end to end against the float64 rule over the CPU oracle --------------------------------------------------------------------
E2E = {   # name: (lm_head factor, W, max_length, n, EOS, prompt)
    "a": (4, 4, 12, 2, 128001, "asr1"), "b": (16, 2, 16, 2, 128001, "asr1"), "c": (16, 2, 24, 2, 128001, "asr1"),
    # n = 3, from a wider grid (tiled prompts, other EOS ids): the ban fires at steps 8 and 15; 5, 6, 7; 5, 6, 8
    "d": (8, 3, 16, 3, 16, "asr1"), "e": (8, 3, 16, 3, 128001, "t62"), "f": (16, 3, 24, 3, 13, "t62")}
_e2e = {}


def _prompt(golden, name):
    return asr1(golden) if name == "asr1" else tiled_prompt(golden, int(name[1:]))


def e2e_run(sd, golden, name):
    if name not in _e2e:
        s, W, ml, n, eos, prompt = E2E[name]
        tok, msk = _prompt(golden, prompt)
        o = build_oracle(scaled_sd(sd, s), "fp32", batch=W)
        _e2e[name] = (beam_ngram_ref.search(o, tok, msk, W, eos, n, max_length=ml), beam_ref.search(o, tok, msk, W, eos, max_length=ml))
    return _e2e[name]


@pytest.mark.parametrize("name", sorted(E2E))
def test_search_fp32_equals_the_banned_rule_over_the_oracle(sd, golden, name):
    s, W, ml, n, eos, prompt = E2E[name]
    ref, plain = e2e_run(sd, golden, name)
    steps = ref["steps"]
    tol = 2 * (5e-5 * s) * steps                  # test_gpu_beam.py's: the fp32 logit bar x the lm_head factor, twice per step
    print(f"  case {name}: steps {steps}, the ban fires at {ref['fired']}, oracle margins score / logit / final = "
          + " / ".join(f"{m:.3g}" for m in ref["margins"]) + f", tol {tol:.3g}")
    assert ref["margins"][0] >= tol and ref["margins"][2] >= tol and ref["margins"][1] >= 2 * 5e-5 * s and ref["margins"][1] >= tol
    assert ref["fired"] and [b.ids for b in ref["beam"]] != [b.ids for b in plain["beam"]]        # the ban decides the result
    tok, msk = _prompt(golden, prompt)
    m = build_product_model(scaled_sd(sd, s), torch.float32, batch=2 * W)
    ids, score, hyps = m.beam_search(tok, msk, beam_width=W, max_length=ml, eos_id=eos, no_repeat_ngram_size=n)
    worst = max(abs(h["score"] - b.score) for h, b in zip(hyps, ref["beam"]))
    print(f"  case {name}: worst score difference {worst:.3g}")
    assert [h["ids"] for h in hyps] == [b.ids for b in ref["beam"]]
    assert [h["finished"] for h in hyps] == [b.fin == FINISHED for b in ref["beam"]]
    assert worst <= tol
    assert ids == ref["beam"][ref["best"]].ids and score == hyps[ref["best"]]["score"]
    for h in hyps:                                                         # no hypothesis repeats an n-gram
        grams = [tuple(h["ids"][i:i + n]) for i in range(len(h["ids"]) - n + 1)]
        assert len(grams) == len(set(grams))
    without = m.beam_search(tok, msk, beam_width=W, max_length=ml, eos_id=eos)
    assert [h["ids"] for h in without[2]] == [b.ids for b in plain["beam"]]                       # and the default is the search as it was


# ---- (f) identities ------------------------------------------------------------------------------------------------------------------
KW = dict(beam_width=3, eos_id=13, max_length=24, no_repeat_ngram_size=2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_banned_search_does_not_depend_on_chunking_graph_or_expert_skipping(sd, golden, dtype):
    tok, msk = tiled_prompt(golden)
    W = 4
    m = build_product_model(scaled_sd(sd, 8), dtype, batch=2 * W)
    before = greedy_ids(m, tok, msk, 20)
    kw = dict(beam_width=W, max_length=40, eos_id=125, no_repeat_ngram_size=2)
    base = m.beam_search(tok, msk, chunk_frames=16, **kw)
    assert m.beam_search(tok, msk, chunk_frames=1, **kw) == base
    assert m.beam_search(tok, msk, use_graph=False, **kw) == base
    assert m.beam_search(tok, msk, skip_audio_experts=False, **kw) == base
    for h in base[2]:
        grams = [tuple(h["ids"][i:i + 2]) for i in range(len(h["ids"]) - 1)]
        assert len(grams) == len(set(grams))
    assert greedy_ids(m, tok, msk, 20) == before                           # the page tables are restored, the beam state detached
    for g in (m.audio_understanding_expert, m.backbone, m.audio_generation_expert):
        pt = g.kv_cache.page_table
        assert torch.equal(pt.flatten(), torch.arange(pt.numel(), dtype=torch.int32, device=DEV))
    assert m.beam_search(tok, msk, chunk_frames=16, **kw) == base          # and a second search starts from clean histories


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_batched_banned_search_equals_one_search_per_prompt(sd, golden, dtype):
    prompts = four_prompts(golden)[:3]
    m = build_product_model(scaled_sd(sd, 8), dtype, batch=2 * 3 * KW["beam_width"])
    single = [m.beam_search(t, k, **KW) for t, k in prompts]
    assert m.beam_search_batch(prompts, **KW) == single
    assert m.beam_search_batch(prompts[::-1], **KW) == single[::-1]
    for _, _, hyps in single:
        for h in hyps:
            grams = [tuple(h["ids"][i:i + 2]) for i in range(len(h["ids"]) - 1)]
            assert len(grams) == len(set(grams))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_beam_of_one_is_the_filtered_greedy_loop_until_the_filter_fires(sd, golden, dtype):
    """The two rules differ where the greedy filter fires (it substitutes `fallback`, the beam takes the next-best id): equality of
    the prefix before that step only."""
    tok, msk = asr1(golden)
    m = build_product_model(scaled_sd(sd, 16), dtype, batch=2)
    frames, fallback, n = 24, 499, 2
    m.set_ngram(n, fallback, capacity=frames)
    try:
        m.begin_ragged([(tok.to(DEV), msk.to(DEV))])
        want = m.generate_frames(frames, 1, 1, skip_audio_experts=True)[:, 0, 0].cpu().tolist()
    finally:
        m.set_ngram(0)
    first = next((i for i in range(frames) if want[i] == fallback and beam_ngram_ref.banned(want[:i], n)), frames)
    ids, _, _ = m.beam_search(tok, msk, beam_width=1, max_length=frames, eos_id=128001, no_repeat_ngram_size=n)
    assert ids[:first] == want[:first] and first >= n
    grams = [tuple(ids[i:i + n]) for i in range(len(ids) - n + 1)]
    assert len(ids) == frames and len(grams) == len(set(grams))


def test_values_and_combinations_are_refused(sd, golden):
    from uniaudio2_amd._lib import BeamNgram, lib
    tok, msk = asr1(golden)
    m = build_product_model(sd, torch.float32, batch=4)
    for bad in (1, 17, -2):
        with pytest.raises(ValueError, match="no_repeat_ngram_size"):
            m.beam_search(tok, msk, beam_width=2, max_length=4, no_repeat_ngram_size=bad)
        with pytest.raises(ValueError, match="no_repeat_ngram_size"):
            m.beam_search_batch([(tok, msk)], beam_width=2, max_length=4, no_repeat_ngram_size=bad)
    assert m._beam is None
    m.set_ngram(3, 499, capacity=8)
    with pytest.raises(ValueError, match="n-gram"):                        # the greedy filter and a beam still exclude each other
        m.beam_search(tok, msk, beam_width=2, max_length=4, no_repeat_ngram_size=3)
    m.set_ngram(0)
    hist = torch.zeros(2 * 8 * 4, dtype=torch.int32, device=DEV)
    ng = BeamNgram(3, 4, hist.data_ptr())
    assert lib.ua2_stage3_set_beam_ngram(m._h, C.byref(ng)) != 0 and b"no beam is attached" in lib.ua2_last_error()
    assert lib.ua2_stage3_set_beam_ngram(m._h, None) == 0                  # NULL = off: always valid
    m.begin_beams(tok, msk, beam_width=2, max_length=4)
    try:
        for bad, what in ((BeamNgram(1, 4, hist.data_ptr()), b"2..16"), (BeamNgram(3, 0, hist.data_ptr()), b"capacity"), (BeamNgram(3, 4, None), b"NULL history")):
            assert lib.ua2_stage3_set_beam_ngram(m._h, C.byref(bad)) != 0 and what in lib.ua2_last_error()
        assert lib.ua2_stage3_set_beam_ngram(m._h, C.byref(ng)) == 0
        m.generate_frames(4, 2, 3)
    finally:
        got = m.end_beams()
    assert len(got[0]) == 4
    assert m.beam_search(tok, msk, beam_width=2, max_length=4) == m.beam_search(tok, msk, beam_width=2, max_length=4, no_repeat_ngram_size=0)


# ---- (g) the command line ------------------------------------------------------------------------------------------------------------
def test_cli_writes_the_text_of_the_model_level_search(tmp_path, monkeypatch, sd):
    from test_ngram import TA
    from uniaudio2_amd import multi_task_inference as cli
    from uniaudio2_amd.evaluation.asr_task import Generator
    m = build_toy_module()
    m.load_state_dict(scaled_sd(sd, 16))
    m = m.to(DEV)
    g = torch.Generator().manual_seed(5)
    names = ["u0", "u1", "u2"]
    for i, name in enumerate(names):
        torch.save(torch.randint(0, 30, (8, 4 + i), generator=g, dtype=torch.int32), tmp_path / f"{name}_reason.pt")
        torch.save(torch.randint(0, 60, (8, 6 + 2 * i), generator=g, dtype=torch.int32), tmp_path / f"{name}_semantic.pt")
    monkeypatch.setattr(cli, "_load_config_and_llm", lambda args: (TA, m, torch.device(DEV)))
    base = ["--task", "ASR", "--token_dir", str(tmp_path), "--llm_train_config", "unused", "--text_tokenizer_path", "ids", "--prompt_text", "1 2",
            "--dtype", "fp32", "--beam_width", "3"]
    texts = {}
    for tag, extra in [("ban", ["--beam_no_repeat_ngram", "2"]), ("ban-batch", ["--beam_no_repeat_ngram", "2", "--batch_size", "2"]), ("plain", [])]:
        out = tmp_path / f"{tag}.txt"
        cli.main(base + extra + ["--results", str(out)])
        texts[tag] = out.read_text()
    assert texts["ban"] == texts["ban-batch"] != texts["plain"]
    gen = Generator(m, TA, text_tokenizer_path="ids")
    m.setup_caches(6)
    prompt = cli._get_prompt_tensor(cli.get_parser().parse_args(base), gen._text_tokenizer, "ASR")
    want = ""
    for name in names:
        reason, semantic = cli._load_token_pair(str(tmp_path), name)
        tok, msk = gen.prepare_asr_task(prompt, reason, semantic)
        ids, _, _ = m.beam_search(tok, msk.bool(), beam_width=3, length_penalty=0.6, max_length=500, eos_id=128001, no_repeat_ngram_size=2)
        grams = [tuple(ids[i:i + 2]) for i in range(len(ids) - 1)]
        assert len(grams) == len(set(grams))
        want += f"{name}\t{' '.join(str(k) for k in ids)}\n"
    assert texts["ban"] == want
