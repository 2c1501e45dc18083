"""Admission into a running decode session (Model_stage3.admit_rows, generate_ragged(batch_size=...), rewind_frame_log): every
sequence equals its own single run (row_stream_refs.single: the existing one-sequence path), greedy and under top-k with
per-sequence seeds, whatever was admitted or retired beside it."""
import pytest
import torch

from row_stream_refs import REF_FRAMES, TOPK, model, prompt, sampling, seed_of, single

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
TOPKS = pytest.mark.parametrize("topk", [1, TOPK], ids=["greedy", "topk5"])


def _begin(m, seqs, mode, topk, ngram=0):
    sampling(m, topk)
    m.begin_ragged([prompt(b, mode) for b in seqs])
    if ngram:
        m.set_ngram(ngram, 499, capacity=64)
    if topk > 1:
        m.set_row_seeds([seed_of(b) for b in seqs])


def _admit(m, seqs, batch, mode, topk):
    return m.admit_rows([prompt(b, mode) for b in seqs], batch, seeds=[seed_of(b) for b in seqs] if topk > 1 else None)


def _end(m):
    m.set_row_seeds(None)
    m.set_ngram(0)


@DTYPES
@TOPKS
def test_admit_a_third_sequence_after_three_frames(dtype, topk):
    m = model(dtype)
    _begin(m, [0, 1], 0, topk)
    a = m.generate_frames(3, 2, 0).clone().cpu()
    assert _admit(m, [2], 2, 0, topk) == 3
    b = m.generate_frames(5, 3, 0).clone().cpu()
    _end(m)
    for r in range(2):
        assert torch.equal(torch.cat([a[:, r], b[:, r]]), single(dtype, r, 0, topk)[:8]), r
    assert torch.equal(b[:, 2], single(dtype, 2, 0, topk)[:5])


@DTYPES
@TOPKS
def test_retire_one_then_admit_into_the_freed_row(dtype, topk):
    m = model(dtype)
    _begin(m, [0, 1, 2], 0, topk)
    a = m.generate_frames(3, 3, 0).clone().cpu()
    assert m.retire_rows([0, 2], 3) == 2
    assert _admit(m, [3], 2, 0, topk) == 3                        # row 2 holds the retired sequence's pages
    b = m.generate_frames(4, 3, 0).clone().cpu()
    _end(m)
    assert torch.equal(torch.cat([a[:, 0], b[:, 0]]), single(dtype, 0, 0, topk)[:7])
    assert torch.equal(torch.cat([a[:, 2], b[:, 1]]), single(dtype, 2, 0, topk)[:7])
    assert torch.equal(a[:, 1], single(dtype, 1, 0, topk)[:3])
    assert torch.equal(b[:, 2], single(dtype, 3, 0, topk)[:4])


@DTYPES
@TOPKS
def test_generate_ragged_five_prompts_two_rows(dtype, topk):
    m = model(dtype)
    sampling(m, topk)
    n_frames = [3, 7, 4, 6, 5]
    out = m.generate_ragged([prompt(b, 0) for b in range(5)], n_frames, mode=0, batch_size=2, seeds=[seed_of(b) for b in range(5)])
    for b in range(5):
        assert torch.equal(out[b].cpu(), single(dtype, b, 0, topk)[:n_frames[b]]), b


@DTYPES
@TOPKS
def test_ngram_text_loop_with_an_admission_keeps_the_live_histories(dtype, topk):
    m = model(dtype)
    _begin(m, [0, 1], 1, topk, ngram=3)
    a = m.generate_frames(6, 2, 1, skip_audio_experts=True).clone().cpu()
    lens = m._st["ngram_len"][:2].tolist()
    assert _admit(m, [2], 2, 1, topk) == 3
    assert m._st["ngram_len"][:3].tolist() == lens + [0] and not m._text_fed_back
    b = m.generate_frames(6, 3, 1, skip_audio_experts=True).clone().cpu()
    _end(m)
    for r in range(2):
        assert torch.equal(torch.cat([a[:, r, 0], b[:, r, 0]]), single(dtype, r, 1, topk, ngram=3)[:12, 0]), r
    assert torch.equal(b[:, 2, 0], single(dtype, 2, 1, topk, ngram=3)[:6, 0])
    # the greedy loops repeat themselves, so there the filter is at work: without it some id differs (14 sampled ids need not repeat)
    assert topk > 1 or any(not torch.equal(single(dtype, r, 1, topk, ngram=3)[:, 0], single(dtype, r, 1, topk)[:, 0]) for r in range(3))


@DTYPES
@TOPKS
def test_a_session_longer_than_the_frame_log(dtype, topk):
    """log_frames = 8 and 25 frames in all: the log slot is rewound between calls (greedy: under the deferred text head's ring)."""
    m = model(dtype, log_frames=8)
    sampling(m, topk)
    n_frames = [11, 5, 9, REF_FRAMES]
    out = m.generate_ragged([prompt(b, 0) for b in range(4)], n_frames, mode=0, batch_size=2, seeds=[seed_of(b) for b in range(4)])
    for b in range(4):
        assert torch.equal(out[b].cpu(), single(dtype, b, 0, topk)[:n_frames[b]]), b
    with pytest.raises(ValueError, match="frame log too small"):
        m.generate_frames(9, 1, 0)


@DTYPES
@TOPKS
def test_guided_pairs_admit_and_retire_two_rows(dtype, topk):
    """Mode 2: an utterance is a (conditional, unconditional) row pair with one key.  Two pairs start, one retires, a third is
    admitted into the freed rows; every pair equals its single-pair run (the B = 2 path test_gpu_lm pins against the golden)."""
    from helpers import load_golden_lm, product_decode_loop
    d, _ = load_golden_lm()
    t_a, m_a = torch.from_numpy(d["cfg2_tokens"]).long(), torch.from_numpy(d["cfg2_mask"]).bool()
    t_c = t_a.clone()
    t_c[:, 2:5, -1] = (t_c[:, 2:5, -1] + 7) % 100
    pairs = [(t_a, m_a), (t_a.flip(0), m_a.flip(0)), (t_c, m_a)]
    m = model(dtype)
    m.set_row_seeds(None)
    singles = []
    for p, (t, k) in enumerate(pairs):
        sampling(m, topk, seed_of(p))
        singles.append(product_decode_loop(m, t, k, 8, "audio", fast=True, cfg_scale=1.5)["samples"])
    rows = lambda p: [(pairs[p][0][j].cuda(), pairs[p][1][j].cuda()) for j in range(2)]
    keys = lambda ps: [seed_of(p) for p in ps for _ in range(2)] if topk > 1 else None
    sampling(m, topk)
    m.set_cfg(1.5)
    m.begin_ragged(rows(0) + rows(1))
    if topk > 1:
        m.set_row_seeds(keys([0, 1]))
    a = m.generate_frames(3, 4, 2).clone().cpu()
    assert m.retire_rows([2, 3], 4) == 2
    assert m.admit_rows(rows(2), 2, seeds=keys([2])) == 4
    b = m.generate_frames(5, 4, 2).clone().cpu()
    _end(m)
    m.set_cfg(1.0)
    assert torch.equal(a[:, 0:2], singles[0][:3])
    assert torch.equal(torch.cat([a[:, 2:4], b[:, 0:2]]), singles[1][:8])
    assert torch.equal(b[:, 2:4], singles[2][:5])


def test_over_full_admission_and_oversized_prompts_are_refused():
    m = model(torch.float32)
    _begin(m, [0, 1], 0, 1)
    with pytest.raises(ValueError, match="cannot admit"):
        m.admit_rows([prompt(b, 0) for b in range(5)], 2)         # 2 + 5 > the plan's 6
    limit = m.backbone.plan["max_seq"]
    long_t = torch.zeros(limit + 1, 9, dtype=torch.long)
    with pytest.raises(ValueError, match="max_seq_length"):
        m.admit_rows([(long_t, long_t.bool())], 2)
    m.set_row_seeds([1, 2])
    with pytest.raises(ValueError, match="one seed per prompt"):
        m.admit_rows([prompt(2, 0)], 2)
    m.set_row_seeds(None)
    assert m.admit_rows([], 2) == 2
