"""ua2_sample_topp / ua2_sample_topp_rows (nucleus sampling tail, include/ua2hip.h) at kernel level through ctypes.  The kept set is
checked EXACTLY, through keep_count and the drawn ids, against the float64 reference of tests/topp_ref.py on inputs whose decision
margin is far above what fp32 masses can move; the off path and the per-row form are checked against the entry points this change
leaves alone (ua2_sample_topk / ua2_sample_topk_rows)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import topp_ref

pytestmark = pytest.mark.gpu

V0, T0, FB0 = 1000, 0.7, 3
CE, EMB_OFF, STREAM_ID = 8, 3, 2
_cache = {}


def _base():
    """The inputs of test_gpu_lm's top-k kernel test: 1000 logits with one exact tie."""
    if "base" not in _cache:
        g = torch.Generator().manual_seed(0)
        base = torch.randn(V0, generator=g) * 2
        base[10] = base[11]
        _cache["base"] = base
    return _cache["base"]


def _ref(topk, p):
    """(kept mask, margin) of the float64 reference on the base row; computed once per case."""
    key = ("ref", topk, p)
    if key not in _cache:
        _cache[key] = topp_ref.kept_mask_f64(_base().double().numpy(), T0, FB0, topk, p)
    return _cache[key]


def _s32(x):
    return x - (1 << 32) if x >= (1 << 31) else x


def _words(k):
    return [_s32(k & 0xFFFFFFFF), _s32(k >> 32)]


def _emb(V, dtype):
    g = torch.Generator().manual_seed(5)
    return torch.randn(V + EMB_OFF, CE, generator=g).to(dtype).cuda()


def _shared(lg, topk, T, forbid, top_p, seed=888, counter=(0, 0, 0), emb=None, code=1, key_shift=0, count=True, entry="topp"):
    """One launch of the shared-stream form.  entry 'topk' = the existing ua2_sample_topk (top_p / count unused).
    -> (ids [M] cpu, next_h [M, CE] cpu or None, keep_count [M] cpu or None)."""
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import check, lib
    M, V = lg.shape
    out = torch.full((M, 2), -1, dtype=torch.int32, device="cuda")
    nh = torch.zeros(M, CE, device="cuda") if emb is not None else None
    cnt = torch.tensor(list(counter), dtype=torch.int32, device="cuda")
    fb = None if forbid is None else forbid.cuda()
    kc = torch.full((M,), -7, dtype=torch.int32, device="cuda") if count and entry == "topp" else None
    ptr = lambda t: None if t is None else t.data_ptr()
    head = (code, M, lg.data_ptr(), V, V, topk, C.c_float(T), ptr(fb), seed, cnt.data_ptr(), STREAM_ID, out.data_ptr(), 2, 1, ptr(emb), EMB_OFF,
            CE if emb is not None else 0, ptr(nh), key_shift)
    if entry == "topk":
        check(lib.ua2_sample_topk(*head, ops.stream()), "ua2_sample_topk")
    else:
        check(lib.ua2_sample_topp(*head, C.c_float(top_p), ptr(kc), ops.stream()), "ua2_sample_topp")
    assert bool((out[:, 0] == -1).all())
    return out[:, 1].cpu().long(), None if nh is None else nh.cpu(), None if kc is None else kc.cpu().long()


def _rows(lg, topk, T, forbid, top_p, keys, draws, emb=None, code=1, count=True, entry="topp"):
    """One launch of the per-row-stream form (entry 'topk' = the existing ua2_sample_topk_rows)."""
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import check, lib
    M, V = lg.shape
    out = torch.full((M, 2), -1, dtype=torch.int32, device="cuda")
    nh = torch.zeros(M, CE, device="cuda") if emb is not None else None
    rk = torch.tensor([_words(k) for k in keys], dtype=torch.int32, device="cuda")
    rd = torch.tensor(draws, dtype=torch.int32, device="cuda")
    fb = None if forbid is None else forbid.cuda()
    kc = torch.full((M,), -7, dtype=torch.int32, device="cuda") if count and entry == "topp" else None
    ptr = lambda t: None if t is None else t.data_ptr()
    head = (code, M, lg.data_ptr(), V, V, topk, C.c_float(T), ptr(fb), rk.data_ptr(), rd.data_ptr(), STREAM_ID, out.data_ptr(), 2, 1, ptr(emb),
            EMB_OFF, CE if emb is not None else 0, ptr(nh))
    if entry == "topk":
        check(lib.ua2_sample_topk_rows(*head, ops.stream()), "ua2_sample_topk_rows")
    else:
        check(lib.ua2_sample_topp_rows(*head, C.c_float(top_p), ptr(kc), ops.stream()), "ua2_sample_topp_rows")
    assert torch.equal(rk.cpu(), torch.tensor([_words(k) for k in keys], dtype=torch.int32))      # neither is written
    assert torch.equal(rd.cpu(), torch.tensor(draws, dtype=torch.int32))
    return out[:, 1].cpu().long(), None if nh is None else nh.cpu(), None if kc is None else kc.cpu().long()


def _tile(row, M):
    return row.unsqueeze(0).repeat(M, 1).contiguous().cuda()


@pytest.mark.parametrize("topk", [1000, 50, 8])
def test_kept_set_is_exactly_the_float64_nucleus(topk):
    """keep_count equals the float64 reference's kept size and every drawn id lies in its set, for every (topk, top_p).  The margin of
    every decision is asserted > 1e-4 (a condition on the inputs: smallest 1.40e-4 at topk 1000, p 0.95; kept sizes 1 .. 24), two
    orders above what fp32 expf, the division by T and the 2^-40 truncation move a mass ratio (about 1e-6)."""
    M = 512
    lg = _tile(_base(), M)
    forbid = torch.full((M,), FB0, dtype=torch.int32)
    for p in (0.1, 0.3, 0.5, 0.8, 0.95):
        mask, margin = _ref(topk, p)
        assert margin > 1e-4, (topk, p, margin)
        ids, _, kc = _shared(lg, topk, T0, forbid, p)
        print(f"topk {topk} top_p {p}: reference keeps {int(mask.sum())} (margin {margin:.3e}), keep_count {sorted(set(kc.tolist()))}")
        assert (kc == int(mask.sum())).all(), (topk, p, int(mask.sum()), sorted(set(kc.tolist())))
        assert set(ids.tolist()) <= set(np.nonzero(mask)[0].tolist()), (topk, p)
        assert np.array_equal(topp_ref.kept_mask_int(_base().numpy(), T0, FB0, topk, p), mask), (topk, p)


def test_frequencies_match_the_renormalised_nucleus():
    """16000 rows, top_p 0.8, topk = V: a nucleus of 5 (probabilities .495 / .303 / .069 / .067 / .066).  2e-2 is the bar of
    test_topk_sampling_kernel_distribution_and_threshold; at 16000 draws the largest per-class sigma is 0.004, so it is 5 sigma."""
    M = 16000
    mask, margin = _ref(V0, 0.8)
    keep = np.nonzero(mask)[0]
    assert keep.shape[0] == 5 and margin > 1e-4
    l = _base().double().numpy()[keep] / T0
    want = np.exp(l - l.max()); want /= want.sum()
    assert abs(np.sort(want)[::-1][0] - 0.495) < 1e-3 and math.sqrt(0.25 / M) < 0.004 + 1e-9
    ids, _, kc = _shared(_tile(_base(), M), V0, T0, torch.full((M,), FB0, dtype=torch.int32), 0.8)
    assert (kc == 5).all() and set(ids.tolist()) <= set(keep.tolist())
    freq = np.array([(ids == int(c)).float().mean().item() for c in keep])
    print("nucleus", keep.tolist(), "want", want.round(4).tolist(), "freq", freq.round(4).tolist())
    assert np.abs(freq - want).max() < 2e-2, (freq, want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_off_is_the_topk_launch_bit_for_bit(dtype):
    """top_p 0.0 and 1.0 through both new entry points: out_tokens and the gathered next_h of ua2_sample_topk / ua2_sample_topk_rows
    under the same seed and draw — with keep_count NULL (the top-k launch itself) and with it (the nucleus kernel, filter off)."""
    from uniaudio2_amd import ops
    code = ops.dtype_code(dtype)
    g = torch.Generator().manual_seed(3)
    M, V = 64, 333
    lg = (torch.randn(M, V, generator=g) * 1.5).cuda()
    forbid = torch.randint(0, 5, (M,), generator=g, dtype=torch.int32)
    emb = _emb(V, dtype)
    keys = [0x5EED0000FFFFFFF0 + 977 * m for m in range(M)]
    draws = [m % 7 for m in range(M)]
    for topk in (7, V):
        want, want_nh, _ = _shared(lg, topk, 0.9, forbid, 0.0, counter=(5, 77, -3), emb=emb, code=code, entry="topk")
        rwant, rwant_nh, _ = _rows(lg, topk, 0.9, forbid, 0.0, keys, draws, emb=emb, code=code, entry="topk")
        ksize = torch.tensor([int(topp_ref.topk_mask(lg[m].cpu().numpy() / np.float32(0.9), np.arange(V) >= int(forbid[m]), topk).sum())
                              for m in range(M)])
        for p in (0.0, 1.0):
            for count in (False, True):
                ids, nh, kc = _shared(lg, topk, 0.9, forbid, p, counter=(5, 77, -3), emb=emb, code=code, count=count)
                assert torch.equal(ids, want) and torch.equal(nh, want_nh), (topk, p, count)
                rids, rnh, rkc = _rows(lg, topk, 0.9, forbid, p, keys, draws, emb=emb, code=code, count=count)
                assert torch.equal(rids, rwant) and torch.equal(rnh, rwant_nh), (topk, p, count)
                if count:                                                 # filter off: every top-k column enters the race
                    assert torch.equal(kc, ksize) and torch.equal(rkc, ksize), (topk, p)
        assert torch.equal(want_nh, emb[(want + EMB_OFF).cuda()].float().cpu())


def test_nested_races_and_the_smallest_nucleus():
    """The per-column random numbers do not depend on the filter: with equal seed and draw, a row whose top-k-only id lies in the
    nucleus draws that id under top_p too.  top_p = 1e-6 leaves the arg-max of the admitted columns for every row."""
    M, topk = 2000, 50
    lg = _tile(_base(), M)
    forbid = torch.full((M,), FB0, dtype=torch.int32)
    plain, _, _ = _shared(lg, topk, T0, forbid, 0.0, entry="topk")
    for p in (0.5, 0.8, 0.95):
        mask, _ = _ref(topk, p)
        ids, _, _ = _shared(lg, topk, T0, forbid, p)
        inside = torch.from_numpy(mask)[plain]
        assert 0 < int(inside.sum()) < M, p                               # both kinds of rows occur
        assert torch.equal(ids[inside], plain[inside]), p
        assert bool(torch.from_numpy(mask)[ids].all())
    valid = _base().clone(); valid[:FB0] = float("-inf")
    ids, _, kc = _shared(lg, topk, T0, forbid, 1e-6)
    assert (ids == int(valid.argmax())).all() and (kc == 1).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_rows_form_equals_one_row_launches(dtype):
    """Row m of an M-row ua2_sample_topp_rows launch = a one-row ua2_sample_topp launch with seed 0, the key in the device seed word
    and the row's draw in the counter, bit for bit (ids, gathered rows, keep_count); equal (key, draw, logits) draw equal ids."""
    from uniaudio2_amd import ops
    code = ops.dtype_code(dtype)
    g = torch.Generator().manual_seed(11)
    V = 1030
    lg = torch.randn(7, V, generator=g) * 2
    lg[3] = (torch.arange(V) // 2).float()[torch.randperm(V, generator=g)] * 0.05       # ties everywhere
    lg[5] = float("-inf")
    lg[6] = lg[1]
    lg = lg.cuda()
    forbid = torch.tensor([0, 3, V // 2, 0, V - 1, 2, 3], dtype=torch.int32)
    keys = [0x0123456789ABCDEF, 7, 0xFFFFFFFFFFFFFFFF, 0x80000000, 0xDEADBEEF00000001, 12, 7]
    draws = [0, 1, 2 ** 31 - 1, 2, 1, 6, 1]
    emb = _emb(V, dtype)
    for topk, p in ((V, 0.9), (20, 0.5), (5, 0.999)):
        ids, nh, kc = _rows(lg, topk, 0.9, forbid, p, keys, draws, emb=emb, code=code)
        for m in range(7):
            one, one_nh, one_kc = _shared(lg[m:m + 1].contiguous(), topk, 0.9, forbid[m:m + 1], p, seed=0,
                                          counter=[draws[m]] + _words(keys[m]), emb=emb, code=code)
            assert int(one[0]) == int(ids[m]) and torch.equal(one_nh[0], nh[m]) and int(one_kc[0]) == int(kc[m]), (topk, p, m)
        assert torch.equal(nh, emb[(ids + EMB_OFF).cuda()].float().cpu())
        assert int(ids[6]) == int(ids[1]) and int(kc[6]) == int(kc[1])
        assert int(ids[4]) == V - 1 and int(kc[4]) == 1 and int(ids[5]) == 2 and int(kc[5]) == V - 2      # one column; all -inf: no filter
        assert bool((ids >= forbid).all()) and bool((ids < V).all())
        for m in (0, 1, 3):                                               # and the sets are the integer reference's
            want = topp_ref.kept_mask_int(lg[m].cpu().numpy(), 0.9, int(forbid[m]), topk, p)
            m64, margin = topp_ref.kept_mask_f64(lg[m].double().cpu().numpy(), 0.9, int(forbid[m]), topk, p)
            if margin > 1e-4:
                assert int(kc[m]) == int(m64.sum()) and bool(m64[int(ids[m])]), (topk, p, m)
            assert bool(want[int(ids[m])]) or margin <= 1e-4, (topk, p, m)


def test_flat_row_of_the_widest_head_keeps_every_column():
    """V = 131072 equal logits, top_p 0.5: every column ties at the threshold value and stays (keep_count == V); Z reaches 2^57, the
    headroom the V limit is sized for, and every column of a pass falls into one bucket."""
    V = 1 << 17
    lg = torch.full((2, V), 1.25, device="cuda")
    ids, _, kc = _shared(lg, V, 0.9, None, 0.5)
    assert kc.tolist() == [V, V] and bool((ids >= 0).all()) and bool((ids < V).all())
    assert int(ids[0]) != int(ids[1])                                     # (two rows, two streams: a 1-in-131072 coincidence otherwise)
    ids, _, kc = _shared(lg, 50, 0.9, torch.tensor([5, 0], dtype=torch.int32), 0.5)      # the top-k threshold ties as well
    assert kc.tolist() == [V - 5, V] and int(ids[0]) >= 5


def test_nan_and_inf_rows_follow_the_all_nan_rule():
    """As in ua2_sample_topk: a row whose scores are all NaN (a NaN row, a row of -inf) takes its first admitted column, Z == 0 switches
    the filter off, and a NaN next to finite values loses."""
    V = 257
    g = torch.Generator().manual_seed(2)
    lg = torch.randn(4, V, generator=g)
    lg[0] = float("nan")
    lg[1] = float("-inf")
    lg[2, 100] = float("nan")
    lg = lg.cuda()
    forbid = torch.tensor([4, 0, 2, 1], dtype=torch.int32)
    for p in (0.5, 1e-6):
        ids, _, kc = _shared(lg, V, 0.9, forbid, p)
        plain, _, _ = _shared(lg, V, 0.9, forbid, 0.0, entry="topk")
        assert ids[:2].tolist() == [4, 0] == plain[:2].tolist()
        assert kc[:2].tolist() == [V - 4, V]
        assert int(ids[2]) != 100 and 2 <= int(ids[2]) < V
    fin = lg[2].cpu().clone(); fin[100] = float("-inf"); fin[:2] = float("-inf")
    assert int(ids[2]) == int(fin.argmax()) and int(kc[2]) == 2           # top_p 1e-6: the finite maximum wins; the NaN column entered and lost
    fin3 = lg[3].cpu().clone(); fin3[:1] = float("-inf")
    assert int(ids[3]) == int(fin3.argmax()) and int(kc[3]) == 1


def test_bad_arguments_are_refused_and_nothing_is_launched():
    from uniaudio2_amd._lib import lib
    V = (1 << 17) + 1
    x = torch.zeros(1, V, device="cuda")
    out = torch.full((1,), -5, dtype=torch.int32, device="cuda")
    kc = torch.full((1,), -5, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(3, dtype=torch.int32, device="cuda")
    shared = lambda v, p: lib.ua2_sample_topp(0, 1, x.data_ptr(), v, v, 2, C.c_float(1.0), None, 1, cnt.data_ptr(), 0, out.data_ptr(), 1, 0, None,
                                              0, 0, None, 0, C.c_float(p), kc.data_ptr(), None)
    rows = lambda v, p: lib.ua2_sample_topp_rows(0, 1, x.data_ptr(), v, v, 2, C.c_float(1.0), None, cnt.data_ptr(), cnt.data_ptr(), 0,
                                                 out.data_ptr(), 1, 0, None, 0, 0, None, C.c_float(p), kc.data_ptr(), None)
    for call in (shared, rows):
        for v, p, word in ((V, 0.5, "131072"), (V, 0.0, "131072"), (64, -0.1, "top_p"), (64, 1.5, "top_p"), (64, math.nan, "top_p")):
            assert call(v, p) != 0
            assert word in lib.ua2_last_error().decode(), (v, p, lib.ua2_last_error())
    torch.cuda.synchronize()
    assert int(out[0]) == -5 and int(kc[0]) == -5
    assert shared(64, 0.5) == 0 and rows(64, 0.5) == 0                    # the same calls with good values run
    torch.cuda.synchronize()
    assert int(out[0]) in range(64) and int(kc[0]) >= 1
