"""Per-row sampler streams in the model (Model_stage3.set_row_seeds; include/ua2hip.h ua2_stage3_set_row_streams): under top-k a
sequence decoded in a batch draws what it draws alone under set_sampling(topk, T, seed=its key).  The reference is always the
existing one-sequence path on the shared stream (row_stream_refs.single)."""
import pytest
import torch

from helpers import build_product_model, load_golden_lm, product_decode_loop
from row_stream_refs import T, TOPK, model, prompt, sampling, seed_of, single, state_dict

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])


@DTYPES
@pytest.mark.parametrize("mode", [0, 1])
def test_batched_rows_equal_their_single_runs_graph_on_and_off(dtype, mode):
    want = [single(dtype, b, mode, TOPK) for b in range(3)]
    m = model(dtype)
    runs = []
    for use_graph in (True, False):
        sampling(m, TOPK, seed=4242)                              # the shared seed is not read while row streams are on
        m.begin_ragged([prompt(b, mode) for b in range(3)])
        m.set_row_seeds([seed_of(b) for b in range(3)])
        shared_draw = int(m._st["counters"][1])
        runs.append(m.generate_frames(10, 3, mode, use_graph=use_graph, skip_audio_experts=(mode == 1)).clone().cpu())
        assert m._st["row_draw"][:3].tolist() == [10, 10, 10] and int(m._st["counters"][1]) == shared_draw
        m.set_row_seeds(None)
    for b in range(3):
        assert torch.equal(runs[0][:, b], want[b][:10]), (mode, b)
    assert torch.equal(runs[0], runs[1])
    if mode == 0:
        assert not torch.equal(want[0][:10], single(dtype, 0, mode, 1)[:10])   # the run is a sampled one


@DTYPES
@pytest.mark.parametrize("mode", [0, 1])
def test_generate_ragged_with_a_retirement_inside(dtype, mode):
    m = model(dtype)
    sampling(m, TOPK)
    n_frames = [4, 9, 12]
    out = m.generate_ragged([prompt(b, mode) for b in range(3)], n_frames, mode=mode, seeds=[seed_of(b) for b in range(3)])
    assert not m._row_streams                                     # the call's streams end with the call
    for b in range(3):
        assert torch.equal(out[b].cpu(), single(dtype, b, mode, TOPK)[:n_frames[b]]), (mode, b)
    # retire_rows carries a row's key and draw with it: a survivor moved to another row keeps its stream
    sampling(m, TOPK)
    m.begin_ragged([prompt(b, mode) for b in range(3)])
    m.set_row_seeds([seed_of(b) for b in range(3)])
    m.generate_frames(3, 3, mode)
    m.retire_rows([2, 1], 3)
    log = m.generate_frames(4, 2, mode).clone().cpu()
    m.set_row_seeds(None)
    assert torch.equal(log[:, 0], single(dtype, 2, mode, TOPK)[3:7]) and torch.equal(log[:, 1], single(dtype, 1, mode, TOPK)[3:7])


@DTYPES
def test_guided_pairs_batched_under_topk_equal_their_single_pair_runs(dtype):
    """The scenario of test_gpu_lm's batched-guidance test, where the shared stream lets only pair 0 reproduce its single run:
    with one key per pair every pair does."""
    d, _ = load_golden_lm()
    t_a, m_a = torch.from_numpy(d["cfg2_tokens"]).long(), torch.from_numpy(d["cfg2_mask"]).bool()
    t_c = t_a.clone()
    t_c[:, 2:5, -1] = (t_c[:, 2:5, -1] + 7) % 100
    pairs = [(t_a, m_a), (t_a.flip(0), m_a.flip(0)), (t_c, m_a)]
    m = model(dtype)
    m.set_row_seeds(None)
    singles = []
    for p, (t, k) in enumerate(pairs):
        sampling(m, TOPK, seed_of(p))
        singles.append(product_decode_loop(m, t, k, 8, "audio", fast=True, cfg_scale=1.5)["samples"])
    sampling(m, TOPK, seed=9)
    m.set_row_seeds([seed_of(p // 2) for p in range(6)])
    both = product_decode_loop(m, torch.cat([t for t, _ in pairs]), torch.cat([k for _, k in pairs]), 8, "audio", fast=True, cfg_scale=1.5)["samples"]
    m.set_row_seeds(None)
    for p in range(3):
        assert torch.equal(both[:, 2 * p:2 * p + 2], singles[p]), p
        assert torch.equal(both[:, 2 * p], both[:, 2 * p + 1])


def test_set_row_seeds_none_restores_the_shared_stream():
    """The scenario of test_model_topk_sampling_runs_and_is_reproducible: same seed, same ids as before row streams were ever on."""
    d, _ = load_golden_lm()
    tokens, mask = torch.from_numpy(d["tts1_tokens"]).long()[None], torch.from_numpy(d["tts1_mask"]).bool()[None]
    m = build_product_model(state_dict(), torch.bfloat16, batch=1)
    m.set_sampling(20, 0.9, seed=888)
    before = product_decode_loop(m, tokens, mask, 12, "audio", fast=True)["samples"]
    m.set_row_seeds([888])
    rows = product_decode_loop(m, tokens, mask, 12, "audio", fast=True)["samples"]
    assert torch.equal(rows, before)                              # one row keyed 888 at draw 0: the same stream
    again = product_decode_loop(m, tokens, mask, 12, "audio", fast=True)["samples"]
    assert not torch.equal(again, before)                         # the row's draw index kept counting
    m.set_row_seeds(None)
    m.set_sampling(20, 0.9, seed=889)
    m.set_sampling(20, 0.9, seed=888)                             # a new key rewinds the shared draw index
    after = product_decode_loop(m, tokens, mask, 12, "audio", fast=True)["samples"]
    assert torch.equal(after, before)
    m.set_sampling(1, 1.0)
    with pytest.raises(ValueError, match="distinct rows"):
        m.set_row_seeds([1, 2])                                   # a plan of one sequence


def test_streams_first_switched_on_inside_generate_ragged_stay_writable():
    """The arrays are allocated on first use, which may be inside an inference-mode call: later calls from plain code still write them."""
    m = build_product_model(state_dict(), torch.float32, batch=2)
    sampling(m, TOPK)
    out = m.generate_ragged([prompt(b, 0) for b in range(2)], [3, 2], mode=0, seeds=[seed_of(0), seed_of(1)])
    assert torch.equal(out[1].cpu(), single(torch.float32, 1, 0, TOPK)[:2])
    m.set_row_seeds([5, 6])
    m._st["row_draw"][:2] += 1
    assert m._st["row_draw"][:2].tolist() == [1, 1]
    m.set_row_seeds(None)
