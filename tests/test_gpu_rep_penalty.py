"""ua2_sample_penalized (include/ua2hip.h; csrc/ua2_sample.hip) at kernel level through ctypes.  The contract's equivalence carries the
tests: a penalised launch on (logits, history) is bit for bit the EXISTING launch of the same form on the host-penalised logits of
tests/rep_penalty_ref.py — equal ids, equal gathered rows, no tolerance — and the ring afterwards is the reference's append."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import rep_penalty_ref as rp
import sampler_refs as sr

pytestmark = pytest.mark.gpu

CE, EMB_OFF, STREAM_ID = 8, 3, 2
OUT_LD, OUT_COL, OUT_FILL = 3, 1, -77
HIST_PAD, LEN_LD, RING_FILL = 3, 2, -9
FORMS = [("topk", "shared"), ("topk", "rows"), ("topp", "shared"), ("topp", "rows")]
KEYS = [0x0123456789ABCDEF, 7, 0xFFFFFFFFFFFFFFFF, 0x80000000, 0xDEADBEEF00000001]
DRAWS = [0, 1, 0x7FFFFFFF, 2, 6]


def _s32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= (1 << 31) else x


def _bits(t):
    return t.contiguous().view(torch.int32)


def _launch(lg, form, topk, T, forbid, top_p, hist=None, length=None, theta=1.0, W=1, entry="pen", keys=KEYS, draws=DRAWS, seed=888,
            counter=(5, 77, -3), dtype=torch.float32, key_shift=0, stream_id=STREAM_ID):
    """One launch.  lg [M, V] fp32 numpy; form (filter, stream); hist [M, cap] / length [M] numpy or None.  entry 'pen' = the new entry
    point, 'old' = the existing entry point of that form (no history).  -> (ids [M], next_h [M, CE], hist after, length after)."""
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import SampleArgs, check, lib
    M, V = lg.shape
    d_lg = torch.from_numpy(lg).cuda()
    out = torch.full((M, OUT_LD), OUT_FILL, dtype=torch.int32, device="cuda")
    emb = torch.randn(V + EMB_OFF, CE, generator=torch.Generator().manual_seed(5)).to(dtype).cuda()
    nh = torch.full((M, CE), -5.0, device="cuda")
    fb = None if forbid is None else torch.tensor(forbid, dtype=torch.int32).cuda()
    cnt = torch.tensor([_s32(w) for w in counter], dtype=torch.int32).cuda()
    rk = torch.tensor([[_s32(k), _s32(k >> 32)] for k in keys[:M]], dtype=torch.int32).cuda()
    rd = torch.tensor([_s32(d) for d in draws[:M]], dtype=torch.int32).cuda()
    ptr = lambda t: None if t is None else t.data_ptr()
    p = top_p if form[0] == "topp" else 0.0
    d_hist = d_len = None
    if entry == "pen":
        a = SampleArgs()
        a.dtype, a.M, a.logits, a.ld, a.V, a.topk, a.temperature, a.forbid = ops.dtype_code(dtype), M, d_lg.data_ptr(), V, V, topk, T, ptr(fb)
        a.stream_id, a.out_tokens, a.out_ld, a.out_col = stream_id, out.data_ptr(), OUT_LD, OUT_COL
        a.emb, a.emb_row_offset, a.C, a.next_h, a.top_p = emb.data_ptr(), EMB_OFF, CE, nh.data_ptr(), p
        if form[1] == "rows":
            a.row_key, a.row_draw = rk.data_ptr(), rd.data_ptr()
        else:
            a.seed, a.counter, a.row_key_shift = seed, cnt.data_ptr(), key_shift
        if hist is not None:
            cap = hist.shape[1]
            h_host = torch.full((M, cap + HIST_PAD), RING_FILL, dtype=torch.int32)
            h_host[:, :cap] = torch.from_numpy(hist)
            l_host = torch.full((M, LEN_LD), RING_FILL, dtype=torch.int32)
            l_host[:, 0] = torch.from_numpy(length)
            d_hist, d_len = h_host.cuda(), l_host.cuda()
            a.rep_penalty, a.rep_window, a.rep_cap, a.rep_hist_ld, a.rep_len_ld = theta, W, cap, cap + HIST_PAD, LEN_LD
            a.rep_hist, a.rep_len = d_hist.data_ptr(), d_len.data_ptr()
        check(lib.ua2_sample_penalized(C.byref(a), ops.stream()), "ua2_sample_penalized")
    else:
        head = (ops.dtype_code(dtype), M, d_lg.data_ptr(), V, V, topk, C.c_float(T), ptr(fb))
        tail = (stream_id, out.data_ptr(), OUT_LD, OUT_COL, emb.data_ptr(), EMB_OFF, CE, nh.data_ptr())
        if form[1] == "rows":
            args = head + (rk.data_ptr(), rd.data_ptr()) + tail
            if form[0] == "topp":
                check(lib.ua2_sample_topp_rows(*args, C.c_float(p), None, ops.stream()), "ua2_sample_topp_rows")
            else:
                check(lib.ua2_sample_topk_rows(*args, ops.stream()), "ua2_sample_topk_rows")
        else:
            args = head + (seed, cnt.data_ptr()) + tail + (key_shift,)
            if form[0] == "topp":
                check(lib.ua2_sample_topp(*args, C.c_float(p), None, ops.stream()), "ua2_sample_topp")
            else:
                check(lib.ua2_sample_topk(*args, ops.stream()), "ua2_sample_topk")
    torch.cuda.synchronize()
    o = out.cpu()
    ids = o[:, OUT_COL].clone()
    o[:, OUT_COL] = OUT_FILL
    assert bool((o == OUT_FILL).all()), "out_tokens was written outside column out_col"
    assert torch.equal(_bits(d_lg.cpu()), _bits(torch.from_numpy(lg))), "the logits were written"
    h_after = l_after = None
    if d_hist is not None:
        ha, la = d_hist.cpu(), d_len.cpu()
        assert bool((ha[:, hist.shape[1]:] == RING_FILL).all()) and bool((la[:, 1:] == RING_FILL).all()), "written outside the ring / the counter"
        h_after, l_after = ha[:, :hist.shape[1]].numpy(), la[:, 0].numpy()
    return ids.numpy().astype(np.int64), nh.cpu(), h_after, l_after


def _case(V, M, W, cap):
    """Rows with +0 / -0 / -inf columns (some of them in the history), one all-negative row; histories of lengths
    {0, 1, W - 1, W, 3 W + 2} holding duplicates, an id below forbid, ids 0 and V - 1 and the row's own largest columns."""
    rng = np.random.default_rng(V + W)
    lg = (rng.standard_normal((M, V)) * 2).astype(np.float32)
    if M > 2:
        lg[2] -= np.float32(9.0)                                          # every logit negative: the multiply branch decides the ids
    lg[:, 0], lg[:, V - 1], lg[:, 7], lg[:, 11], lg[:, 12] = -0.0, 0.0, -np.inf, 0.0, -np.inf
    forbid = [0, 3, 2, 0, 5][:M]
    lens = [0, 1, W - 1, W, 3 * W + 2][:M] if M > 1 else [3 * W + 2]
    hist, length = np.full((M, cap), RING_FILL, dtype=np.int32), np.zeros(M, dtype=np.int32)
    for m in range(M):
        top = np.argsort(lg[m])[::-1][:6].tolist()
        pattern = [top[0], 0, V - 1, top[0], 1, top[1], 7, top[2], top[1], top[3]]
        for j in range(lens[m]):
            hist[m], length[m] = rp.append(hist[m], length[m], pattern[(lens[m] - 1 - j) % len(pattern)])   # the newest ids are pattern[0 ..]
    return lg, forbid, hist, length


SHAPES = [(257, 5), (12296, 5), (128256, 1)]


@pytest.mark.parametrize("W", [1, 16, 512])
@pytest.mark.parametrize("V,M", SHAPES, ids=[f"V{v}" for v, _ in SHAPES])
def test_twin_launch_no_tolerance(V, M, W):
    """Each of the four forms: the new entry on (logits, hist) against the existing entry on penalize(logits) — ids equal, gathered
    rows equal, ring and counter afterwards equal to the reference's append.  (That the penalty moves ids at all is the anchor case's to
    show: tests/test_rep_penalty_host.py holds its reference ids to differ from the unpenalised ones.)"""
    cap = W + (5 if V == 257 else 0)                                      # a ring larger than the window as well
    lg, forbid, hist, length = _case(V, M, W, cap)
    topk, T, top_p = 50, 0.9, 0.8
    for theta in (1.3, 0.8):
        pen = np.stack([rp.penalize(lg[m], hist[m], length[m], W, theta) for m in range(M)])
        for form in FORMS:
            ids, nh, h_after, l_after = _launch(lg, form, topk, T, forbid, top_p, hist, length, theta, W)
            want, want_nh, _, _ = _launch(pen, form, topk, T, forbid, top_p, entry="old")
            assert np.array_equal(ids, want), (V, W, theta, form, ids, want)
            assert torch.equal(_bits(nh), _bits(want_nh)), (V, W, theta, form)
            for m in range(M):
                h, n = rp.append(hist[m], length[m], ids[m])
                assert np.array_equal(h_after[m], h) and int(l_after[m]) == n, (V, W, theta, form, m)
            assert all(int(ids[m]) >= forbid[m] for m in range(M))


def test_float64_anchor_case():
    """The launch tests/test_rep_penalty_host.py qualifies (0 rows outside the exact assertion, E_ref <= 1e-4), penalised on the device:
    every id is the float64 replay's on the host-penalised rows, under sampler_refs' assertion rule."""
    raw, hist, length, L = rp.anchor_case()
    a = rp.ANCHOR
    R = sr.replay(L)
    got, _, h_after, l_after = _launch(raw, ("topk", "shared"), L.topk, L.T, None, 0.0, hist, length, a["theta"], a["W"], seed=L.seed,
                                       counter=L.counter, stream_id=L.stream_id)
    print(R.line("rep-penalty-anchor"))
    bad = R.mismatches(got)
    assert not bad, [(m, int(got[m]), int(R.ids[m]), R.near[m].tolist()) for m in bad[:8]]
    assert int((~R.exact).sum()) <= sr.CAP * len(R.ids)
    for m in range(a["M"]):
        h, n = rp.append(hist[m], length[m], got[m])
        assert np.array_equal(h_after[m], h) and int(l_after[m]) == n


def test_row_invariance():
    """Row m of an M = 64 per-row-stream launch = a one-row launch with its history, key and draw: ids and appended histories."""
    M, V, W, theta = 64, 1030, 16, 1.3
    rng = np.random.default_rng(9)
    lg = (rng.standard_normal((M, V)) * 2).astype(np.float32)
    keys = [0x5EED0000FFFFFFF0 + 977 * m for m in range(M)]
    draws = [m % 7 for m in range(M)]
    forbid = [m % 4 for m in range(M)]
    hist, length = np.full((M, W), RING_FILL, dtype=np.int32), np.zeros(M, dtype=np.int32)
    for m in range(M):
        top = np.argsort(lg[m])[-8:]
        for tok in rng.choice(top, m % (2 * W + 3)):
            hist[m], length[m] = rp.append(hist[m], length[m], tok)
    for form in (("topk", "rows"), ("topp", "rows")):
        ids, nh, h_after, l_after = _launch(lg, form, 20, 0.9, forbid, 0.7, hist, length, theta, W, keys=keys, draws=draws)
        for m in range(M):
            one, one_nh, h1, l1 = _launch(lg[m:m + 1], form, 20, 0.9, forbid[m:m + 1], 0.7, hist[m:m + 1], length[m:m + 1], theta, W,
                                          keys=keys[m:m + 1], draws=draws[m:m + 1])
            assert int(one[0]) == int(ids[m]) and torch.equal(_bits(one_nh[0]), _bits(nh[m])), (form, m)
            assert np.array_equal(h1[0], h_after[m]) and int(l1[0]) == int(l_after[m]), (form, m)
            if m % 8:
                continue
            # ... and a one-row launch of the shared-stream form with that key in the device seed word and that draw in the counter
            sh, _, h2, _ = _launch(lg[m:m + 1], (form[0], "shared"), 20, 0.9, forbid[m:m + 1], 0.7, hist[m:m + 1], length[m:m + 1], theta, W,
                                   seed=0, counter=(draws[m], keys[m] & 0xFFFFFFFF, keys[m] >> 32))
            assert int(sh[0]) == int(ids[m]) and np.array_equal(h2[0], h_after[m]), (form, m)


def test_off_is_off():
    """rep_hist = NULL, and theta = 1 with a history supplied: the existing launch's ids and rows; the history is left untouched."""
    V, M, W = 333, 5, 16
    lg, forbid, hist, length = _case(V, M, W, W)
    for dtype in (torch.float32, torch.bfloat16):
        for form in FORMS:
            want, want_nh, _, _ = _launch(lg, form, 7, 0.9, forbid, 0.6, entry="old", dtype=dtype)
            ids, nh, _, _ = _launch(lg, form, 7, 0.9, forbid, 0.6, None, None, 1.3, W, dtype=dtype)
            assert np.array_equal(ids, want) and torch.equal(_bits(nh), _bits(want_nh)), form
            ids, nh, h_after, l_after = _launch(lg, form, 7, 0.9, forbid, 0.6, hist, length, 1.0, W, dtype=dtype)
            assert np.array_equal(ids, want) and torch.equal(_bits(nh), _bits(want_nh)), form
            assert np.array_equal(h_after, hist) and np.array_equal(l_after, length), form


def test_bad_arguments_are_refused_and_nothing_is_launched():
    from uniaudio2_amd._lib import SampleArgs, lib
    V = (1 << 17) + 1
    x = torch.zeros(1, V, device="cuda")
    out = torch.full((1,), -5, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(3, dtype=torch.int32, device="cuda")
    hist = torch.full((512,), -5, dtype=torch.int32, device="cuda")
    ln = torch.zeros(1, dtype=torch.int32, device="cuda")

    def call(v, theta, W, rows):
        a = SampleArgs()
        a.dtype, a.M, a.logits, a.ld, a.V, a.topk, a.temperature = 0, 1, x.data_ptr(), v, v, 2, 1.0
        a.out_tokens, a.out_ld = out.data_ptr(), 1
        if rows:
            a.row_key, a.row_draw = cnt.data_ptr(), cnt.data_ptr()
        else:
            a.seed, a.counter = 1, cnt.data_ptr()
        a.rep_penalty, a.rep_window, a.rep_cap, a.rep_hist_ld, a.rep_len_ld = theta, W, 512, 512, 1
        a.rep_hist, a.rep_len = hist.data_ptr(), ln.data_ptr()
        return lib.ua2_sample_penalized(C.byref(a), None)

    for rows in (False, True):
        for v, theta, W, word in ((64, 0.0, 16, "rep_penalty"), (64, -1.0, 16, "rep_penalty"), (64, math.nan, 16, "rep_penalty"),
                                  (64, math.inf, 16, "rep_penalty"), (64, 1.3, 0, "rep_window"), (64, 1.3, 513, "rep_window"),
                                  (64, 1.0, 0, "rep_window"), (V, 1.3, 16, "131072")):
            assert call(v, theta, W, rows) != 0, (v, theta, W)
            assert word in lib.ua2_last_error().decode(), (v, theta, W, lib.ua2_last_error())
    torch.cuda.synchronize()
    assert int(out[0]) == -5 and int(ln[0]) == 0 and bool((hist == -5).all())
    assert call(64, 1.3, 16, False) == 0 and call(64, 1.3, 512, True) == 0          # the same calls with good values run
    torch.cuda.synchronize()
    assert int(out[0]) in range(64) and int(ln[0]) == 2 and int(hist[0]) in range(64) and int(hist[1]) == int(out[0])
    assert bool((hist[2:] == -5).all())
