"""The repetition penalty in the frame executor and the model (ua2_stage3_set_rep_penalty; Model_stage3.set_repetition_penalty) on the
toy golden weights.  Every sampled frame is replayed from the logits the frame left behind: the existing sampler on the host-penalised
row (tests/rep_penalty_ref.py) under the row's own key and draw must give the frame's id, and the device histories must be the
reference's rings.  Row invariance then carries retirement, admission and guided pairs."""
import numpy as np
import pytest
import torch

import rep_penalty_ref as rp
from helpers import load_golden_lm, product_decode_loop
from row_stream_refs import T, model, prompt, sampling, seed_of
from test_gpu_rep_penalty import _launch

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
W, TOPK, THETA = 4, 8, 1.5
FRAMES = 3 * W + 2
_singles = {}


class penalty:
    """with penalty(m, theta, window): the model's penalty for the block, cleared afterwards (the plans are shared between tests)."""

    def __init__(self, m, theta=THETA, window=W):
        self.m, self.a = m, (theta, window)

    def __enter__(self):
        self.m.set_repetition_penalty(*self.a)
        return self.m

    def __exit__(self, *exc):
        self.m.set_row_seeds(None)
        self.m.set_repetition_penalty(1.0)
        return False


def _u64(lo, hi):
    return (int(lo) & 0xFFFFFFFF) | ((int(hi) & 0xFFFFFFFF) << 32)


def _run(m, b, frames=FRAMES, topk=TOPK, seed=None, mode=0, use_graph=True):
    """Prompt b decoded alone on the shared stream from draw index 0 -> (frames, 9) ids (cpu)."""
    m.set_row_seeds(None)
    sampling(m, topk, seed_of(b) if seed is None else seed)
    m.begin_ragged([prompt(b, mode)])
    return m.generate_frames(frames, 1, mode, use_graph=use_graph, skip_audio_experts=(mode == 1)).clone()[:, 0].cpu()


def _single(dtype, b):
    """(FRAMES, 9) ids of prompt b alone under the penalty (THETA, W), top-k TOPK, seed_of(b); once per (dtype, b)."""
    if (dtype, b) not in _singles:
        m = model(dtype)
        with penalty(m):
            _singles[dtype, b] = _run(m, b)
    return _singles[dtype, b]


def _replayed_loop(m, B, use_graph):
    """FRAMES sampled frames of B rows (B == 1: the shared stream; B > 1: row streams), every frame replayed stream by stream.
    -> (FRAMES, B, 9) ids."""
    st = m._st
    ncb, va = st["ncb"], st["va"]
    sampling(m, TOPK, seed_of(0))
    m.begin_ragged([prompt(b, 0) for b in range(B)])
    if B > 1:
        m.set_row_seeds([seed_of(b) for b in range(B)])
    else:
        m.set_row_seeds(None)
    assert int(st["rep_len"][:B].abs().sum()) == 0                       # rows that start, start empty
    rings = [[(np.zeros(W, dtype=np.int32), 0) for _ in range(ncb + 1)] for _ in range(B)]
    out = []
    for f in range(FRAMES):
        if B > 1:
            keys = [_u64(*st["row_key"][b].tolist()) for b in range(B)]
            draws = st["row_draw"][:B].tolist()
            stream = dict(keys=keys, draws=draws)
            form = ("topk", "rows")
        else:
            stream = dict(seed=0, counter=tuple(st["counters"][1:4].tolist()))
            form = ("topk", "shared")
        forbid = st["forbid"][:B].tolist()
        ids = m.generate_frames(1, B, 0, use_graph=use_graph).clone()[0].cpu()
        tl = m.buffer("text_logits", B).cpu().numpy()
        al = m.buffer("audio_logits", B).cpu().numpy()
        vt = tl.shape[1]
        for s in range(ncb + 1):
            raw = tl if s == 0 else al[:, s - 1]
            pen = np.stack([rp.penalize(raw[b], rings[b][s][0], rings[b][s][1], W, THETA) for b in range(B)])
            want, _, _, _ = _launch(np.ascontiguousarray(pen), form, min(TOPK, vt) if s == 0 else TOPK, T, None if s == 0 else forbid, 0.0,
                                    entry="old", stream_id=s, **stream)
            assert want.tolist() == ids[:, s].tolist(), (f, s, want.tolist(), ids[:, s].tolist())
            for b in range(B):
                # replay_loop: one frame further from the ring so far, the draw being the twin launch's id
                tok, ring, n = rp.replay_loop([raw[b]], lambda _f, _l, b=b: want[b], W, THETA, *rings[b][s])[0]
                assert tok == int(ids[b, s])
                rings[b][s] = (ring, n)
        dev_h, dev_n = st["rep_hist"][:B].cpu().numpy(), st["rep_len"][:B].cpu().numpy()
        for b in range(B):
            for s in range(ncb + 1):
                # (the entries the ring stores: a slot not yet written since the row started holds whatever an earlier session left)
                assert dev_n[b, s] == rings[b][s][1] == f + 1, (f, b, s)
                assert np.array_equal(rp.window_ids(dev_h[b, s], f + 1, W), rp.window_ids(rings[b][s][0], f + 1, W)), (f, b, s)
        out.append(ids)
    return torch.stack(out)


@DTYPES
@pytest.mark.parametrize("B", [1, 3])
def test_sampled_loop_replays_frame_by_frame(dtype, B):
    """3 W + 2 frames, W = 4, top-k 8, theta 1.5: after every frame each stream's id is the existing sampler's on penalize(logits)
    under that row's key and draw, the histories are replay_loop's rings, and the eager executor gives the graph's ids."""
    m = model(dtype)
    with penalty(m):
        graph = _replayed_loop(m, B, True)
        eager = _replayed_loop(m, B, False)
    assert torch.equal(graph, eager)
    assert torch.equal(graph[:, 0], _single(dtype, 0))                    # row 0 is prompt 0's own run
    m.set_row_seeds(None)
    plain = _run(m, 0)
    assert not torch.equal(plain, graph[:, 0])                            # and the penalty is at work in it


@DTYPES
def test_batches_with_retirement_and_admission_equal_the_single_runs(dtype):
    """generate_ragged at batch 3 with seeds, and 4 prompts of different lengths through 2 rows: every sequence draws what it draws
    alone.  Then by hand: a surviving row keeps its history across retire_rows, an admitted one starts empty."""
    n_frames = [FRAMES, 6, 10, 8]
    want = [_single(dtype, b) for b in range(4)]
    m = model(dtype)
    with penalty(m):
        sampling(m, TOPK)
        got = m.generate_ragged([prompt(b, 0) for b in range(3)], [FRAMES] * 3, seeds=[seed_of(b) for b in range(3)])
        for b in range(3):
            assert torch.equal(got[b].cpu(), want[b]), b
        sampling(m, TOPK)
        got = m.generate_ragged([prompt(b, 0) for b in range(4)], n_frames, batch_size=2, seeds=[seed_of(b) for b in range(4)])
        for b in range(4):
            assert torch.equal(got[b].cpu(), want[b][:n_frames[b]]), b
        st = m._st
        sampling(m, TOPK)
        m.begin_ragged([prompt(b, 0) for b in range(3)])
        m.set_row_seeds([seed_of(b) for b in range(3)])
        a = m.generate_frames(3, 3, 0).clone().cpu()
        h2, n2 = st["rep_hist"][2].clone(), st["rep_len"][2].clone()
        assert n2.tolist() == [3] * 9
        assert m.retire_rows([0, 2], 3) == 2
        assert torch.equal(st["rep_hist"][1], h2) and torch.equal(st["rep_len"][1], n2)           # the survivor's history moved with it
        assert m.admit_rows([prompt(3, 0)], 2, seeds=[seed_of(3)]) == 3
        assert st["rep_len"][2].tolist() == [0] * 9 and st["rep_len"][:2].tolist() == [[3] * 9] * 2   # empty; the live rows' kept
        b_ = m.generate_frames(4, 3, 0).clone().cpu()
    assert torch.equal(torch.cat([a[:, 0], b_[:, 0]]), want[0][:7])
    assert torch.equal(torch.cat([a[:, 2], b_[:, 1]]), want[2][:7])
    assert torch.equal(a[:, 1], want[1][:3]) and torch.equal(b_[:, 2], want[3][:4])


@DTYPES
def test_guided_pair_rows_draw_and_append_equal_ids(dtype):
    d, _ = load_golden_lm()
    t, k = torch.from_numpy(d["cfg2_tokens"]).long(), torch.from_numpy(d["cfg2_mask"]).bool()
    m = model(dtype)
    st = m._st
    with penalty(m):
        m.set_row_seeds(None)
        sampling(m, TOPK, seed_of(0))
        shared = product_decode_loop(m, t, k, 2 * W, "audio", fast=True, cfg_scale=1.5)["samples"]
        hs, ns = st["rep_hist"][:2].clone(), st["rep_len"][:2].clone()
        sampling(m, TOPK, seed=9)
        m.set_row_seeds([seed_of(0), seed_of(0)])
        rows = product_decode_loop(m, t, k, 2 * W, "audio", fast=True, cfg_scale=1.5)["samples"]
        hr, nr = st["rep_hist"][:2].clone(), st["rep_len"][:2].clone()
    for s, h, n in ((shared, hs, ns), (rows, hr, nr)):
        assert torch.equal(s[:, 0], s[:, 1])
        assert torch.equal(h[0], h[1]) and torch.equal(n[0], n[1]) and n[0].tolist() == [2 * W] * 9
        ring = s[-W:, 0].T.contiguous().int()                            # 2 W frames: slot j of stream s holds the id of frame W + j
        assert torch.equal(h[0].cpu(), ring)
    assert torch.equal(rows, shared)
    sampling(m, TOPK, seed_of(0))                                         # the same key without the penalty: other ids
    plain = product_decode_loop(m, t, k, 2 * W, "audio", fast=True, cfg_scale=1.5)["samples"]
    assert not torch.equal(plain, shared)


@DTYPES
def test_clearing_and_switching_the_penalty(dtype):
    """set_repetition_penalty(1.0) after a penalised run gives the ids of a session that never enabled it; theta 1.5 -> 1.3 -> 1.5
    never replays a frame recorded under another value: each equals a fresh plan's ids, graph and eager."""
    m = model(dtype)
    never = _run(m, 0)
    fresh = {}
    f = model(dtype, log_frames=256)                                      # a fresh plan: nothing recorded, nothing remembered
    for theta in (1.5, 1.3):
        with penalty(f, theta):
            fresh[theta] = _run(f, 0)
    assert not torch.equal(fresh[1.5], fresh[1.3]) and not torch.equal(fresh[1.5], never)
    for theta in (1.5, 1.3, 1.5):
        m.set_repetition_penalty(theta, W)
        assert torch.equal(_run(m, 0), fresh[theta]), theta
        assert torch.equal(_run(m, 0, use_graph=False), fresh[theta]), theta
    m.set_repetition_penalty(1.5, 2)                                      # the window selects the frame as well
    two = _run(m, 0)
    assert torch.equal(two, _run(m, 0, use_graph=False)) and not torch.equal(two, fresh[1.5])
    m.set_repetition_penalty(1.0)
    assert torch.equal(_run(m, 0), never)
    assert m.repetition_penalty[0] == 1.0
    for bad, word in ((0.0, "penalty"), (float("nan"), "penalty"), (float("inf"), "penalty")):
        with pytest.raises(ValueError, match=word):
            m.set_repetition_penalty(bad)
    with pytest.raises(ValueError, match="window"):
        m.set_repetition_penalty(1.2, 513)
    assert torch.equal(_run(m, 0), never)


@DTYPES
def test_greedy_beam_and_score_ignore_the_penalty(dtype):
    m = model(dtype)
    tok, msk = prompt(1, 1)
    seq_t, seq_m = prompt(4, 0)
    kw = dict(beam_width=3, max_length=10, eos_id=13)

    def runs():
        m.set_row_seeds(None)
        greedy_audio = _run(m, 0, 10, topk=1)
        greedy_text = _run(m, 1, 10, topk=1, mode=1)
        sampling(m, 1)
        beam = m.beam_search(tok, msk, **kw)
        sampling(m, TOPK, 5)                                              # a sampled key is set while the sequence is scored
        sc = m.score_sequence(seq_t[None], seq_m[None])
        return greedy_audio, greedy_text, beam, sc["nll"].clone().cpu(), sc["pred"].clone().cpu()

    base = runs()
    with penalty(m):
        st = m._st
        st["rep_len"].zero_()
        got = runs()
        assert int(st["rep_len"].abs().sum()) == 0                        # and none of them appended an id
    assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
    assert got[2] == base[2]
    assert torch.equal(got[3].view(torch.int32), base[3].view(torch.int32)) and torch.equal(got[4], base[4])
