"""Nucleus sampling in the model (Model_stage3.set_top_p; include/ua2hip.h ua2_stage3_set_top_p) on the toy golden weights: the
smallest nucleus is the greedy run, the value selects the captured graph, and the row-invariance contract of row_stream_refs holds
with the switch on (batched rows, a retirement, an admission, guided pairs)."""
import pytest
import torch

from helpers import load_golden_lm, product_decode_loop
from row_stream_refs import REF_FRAMES, model, prompt, sampling, seed_of, single

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
TOP_P = 0.9
TOPK = 20                # (row_stream_refs' top-5 of the flat toy heads hold about 0.2 each: 0.9 would keep all five and filter nothing)
_singles = {}


def _run(m, b, mode, frames, topk, seed, use_graph=True):
    """Prompt b decoded alone on the shared stream from draw index 0."""
    m.set_row_seeds(None)
    sampling(m, topk, seed)
    m.begin_ragged([prompt(b, mode)])
    return m.generate_frames(frames, 1, mode, use_graph=use_graph, skip_audio_experts=(mode == 1)).clone()[:, 0].cpu()


def _single_p(dtype, b):
    """(REF_FRAMES, 9) ids of prompt b decoded alone under top-k TOPK, top_p TOP_P and seed_of(b); once per (dtype, b)."""
    if (dtype, b) not in _singles:
        m = model(dtype)
        m.set_top_p(TOP_P)
        try:
            _singles[dtype, b] = _run(m, b, 0, REF_FRAMES, TOPK, seed_of(b))
        finally:
            m.set_top_p(0.0)
    return _singles[dtype, b]


@DTYPES
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_smallest_nucleus_is_the_greedy_run(dtype, use_graph):
    """set_sampling(20, 0.9, seed) + set_top_p(1e-6): only the arg-max survives the filter, so every sampler returns the greedy id —
    audio columns and the text column of the audio loop, and the text loop's ids."""
    m = model(dtype)
    m.set_top_p(1e-6)
    try:
        audio = _run(m, 0, 0, 10, 20, 5, use_graph)
        text = _run(m, 1, 1, 10, 20, 5, use_graph)
    finally:
        m.set_top_p(0.0)
    assert torch.equal(audio, single(dtype, 0, 0, 1)[:10])
    assert torch.equal(text[:, 0], single(dtype, 1, 1, 1)[:10, 0])


@DTYPES
def test_top_p_selects_the_captured_graph(dtype):
    """top_p changes the ids against top-k alone, reproducibly; back at 0.0 the top-k-only ids return bit for bit with the graph
    cache warm, and a new value never replays a frame recorded under another (graph run == eager run at every value)."""
    m = model(dtype)
    try:
        plain = _run(m, 0, 0, 12, 20, 888)
        m.set_top_p(0.9)
        a = _run(m, 0, 0, 12, 20, 888)
        assert torch.equal(_run(m, 0, 0, 12, 20, 888), a) and not torch.equal(a, plain)
        assert (a[:, 1:] < 110).all() and (a[:, 0] < 512).all() and (a >= 0).all()
        m.set_top_p(0.0)
        assert torch.equal(_run(m, 0, 0, 12, 20, 888), plain)
        m.set_top_p(1.0)                                                  # off as well
        assert torch.equal(_run(m, 0, 0, 12, 20, 888), plain)
        m.set_top_p(0.3)
        b = _run(m, 0, 0, 12, 20, 888)
        assert torch.equal(b, _run(m, 0, 0, 12, 20, 888, use_graph=False)) and not torch.equal(b, a)
        m.set_top_p(0.9)
        assert torch.equal(_run(m, 0, 0, 12, 20, 888), a)
        assert torch.equal(_run(m, 0, 0, 12, 20, 888, use_graph=False), a)
        m.set_sampling(1, 1.0)                                            # greedy frames ignore top_p
        m.begin_ragged([prompt(0, 0)])
        assert torch.equal(m.generate_frames(8, 1, 0).clone()[:, 0].cpu(), single(dtype, 0, 0, 1)[:8])
    finally:
        m.set_top_p(0.0)
    with pytest.raises(ValueError, match="top_p"):
        m.set_top_p(1.5)
    assert m.top_p == 0.0


@DTYPES
def test_batched_rows_with_a_retirement_and_an_admission_equal_their_single_runs(dtype):
    """The contract of row_stream_refs with the nucleus on: under set_row_seeds every sequence draws what it draws alone under
    set_sampling(TOPK, T, seed=its key) and the same top_p — three rows start, one retires, a fourth is admitted into the freed row."""
    want = [_single_p(dtype, b) for b in range(4)]
    assert any(not torch.equal(want[b], single(dtype, b, 0, TOPK)) for b in range(4))      # the filter is at work in these runs
    m = model(dtype)
    m.set_top_p(TOP_P)
    try:
        sampling(m, TOPK)
        m.begin_ragged([prompt(b, 0) for b in range(3)])
        m.set_row_seeds([seed_of(b) for b in range(3)])
        a = m.generate_frames(3, 3, 0).clone().cpu()
        assert m.retire_rows([0, 2], 3) == 2
        assert m.admit_rows([prompt(3, 0)], 2, seeds=[seed_of(3)]) == 3
        b = m.generate_frames(4, 3, 0).clone().cpu()
    finally:
        m.set_row_seeds(None)
        m.set_top_p(0.0)
    assert torch.equal(torch.cat([a[:, 0], b[:, 0]]), want[0][:7])
    assert torch.equal(torch.cat([a[:, 2], b[:, 1]]), want[2][:7])
    assert torch.equal(a[:, 1], want[1][:3])
    assert torch.equal(b[:, 2], want[3][:4])


@DTYPES
def test_guided_pair_rows_draw_equal_ids(dtype):
    d, _ = load_golden_lm()
    t, k = torch.from_numpy(d["cfg2_tokens"]).long(), torch.from_numpy(d["cfg2_mask"]).bool()
    m = model(dtype)
    m.set_row_seeds(None)
    m.set_top_p(TOP_P)
    try:
        sampling(m, TOPK, seed_of(0))
        shared = product_decode_loop(m, t, k, 8, "audio", fast=True, cfg_scale=1.5)["samples"]
        sampling(m, TOPK, seed=9)
        m.set_row_seeds([seed_of(0), seed_of(0)])
        rows = product_decode_loop(m, t, k, 8, "audio", fast=True, cfg_scale=1.5)["samples"]
    finally:
        m.set_row_seeds(None)
        m.set_top_p(0.0)
    assert torch.equal(shared[:, 0], shared[:, 1]) and torch.equal(rows[:, 0], rows[:, 1])
    assert torch.equal(rows, shared)                                      # one key per pair: the pair's single run on the shared stream
