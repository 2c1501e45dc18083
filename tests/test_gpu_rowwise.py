"""Kernel-level GPU tests of the row-wise glue kernels (csrc/ua2_misc.hip, ua2_codec.hip, ua2_sample.hip, dwconv1d of
ua2_conv.hip), which the whole-model goldens only reach at toy widths.

Two kinds of check (tests/kernel_refs.py):
  * kernels whose arithmetic is a documented sequence of singly-rounded fp32 operations equal a host float32 replay of that
    sequence bit for bit;
  * the others are compared with a float64 reference under bar = max(4 * E_ref, 8 * 2^-24 * scale), E_ref = error of the same
    formula in plain fp32 on the host on the very inputs of the case; every such case prints `case, err, E_ref, bar`.
Index-carrying inputs are generated in range and asserted in range on the host before a launch.  NaN reaches only the two
sampling tails, and only with emb = NULL (no gather: the one effect is the int32 written to out_tokens)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import kernel_refs as kr

pytestmark = pytest.mark.gpu

F64 = torch.float64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).numpy()


def _assert_same_bits(got, want, what=""):
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=what)


def _report(case, got, ref, ref32, rel_rows=False, quiet=False):
    """err / E_ref of `got` / `ref32` against the float64 `ref`: absolute with scale max(1, max |ref|), or relative to each row's
    max magnitude.  Prints the line and returns (err, bar)."""
    got, ref32 = got.detach().cpu().to(F64), ref32.to(F64)
    assert bool(torch.isfinite(got).all()), f"{case}: non-finite output"
    if rel_rows:
        scale = ref.abs().amax(dim=-1, keepdim=True).clamp_min(1e-30)
    else:
        scale = torch.tensor(max(1.0, float(ref.abs().max())), dtype=F64)
    err = float(((got - ref).abs() / scale).max())
    e_ref = float(((ref32 - ref).abs() / scale).max())
    b = kr.bar(e_ref)
    if not quiet:
        print(f"PARITY {case}: err {err:.3e} E_ref {e_ref:.3e} bar {b:.3e}")
    return err, b


class Handover(C.Structure):          # include/ua2hip.h ua2_handover
    _fields_ = [("norm_w", C.c_void_p), ("h", C.c_void_p), ("ldh", C.c_int32), ("packed", C.c_void_p), ("ssq", C.c_void_p)]


def _decode_packed_bf16(pk, M, K):
    """[ceil(M/16)][K/32][64 lanes][8 bf16]: element (m, c) in lane ((c & 31) >> 3) * 16 + (m & 15) of chunk c >> 5 (handover_emit8)."""
    return pk.view((M + 15) // 16, K // 32, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(-1, K)[:M]


def _check_handover(case, ho_h, ho_pk, ho_ssq, out, w):
    """h = RNE-bf16(out * norm_w) exactly (out = the kernel's own fp32 output), packed = the same values in fragment order,
    ssq = per-16-column sums of out^2 within fp32 sum-order noise."""
    M, Cc = out.shape
    want = (out * w).to(torch.bfloat16)                                   # one fp32 multiply, then RNE
    _assert_same_bits(ho_h, want, f"{case}: ho.h")
    _assert_same_bits(_decode_packed_bf16(ho_pk, M, Cc), want, f"{case}: ho.packed")
    o = out.cpu()
    ref = (o.to(F64) ** 2).view(M, Cc // 16, 16).sum(-1)
    ref32 = (o * o).view(M, Cc // 16, 16).sum(-1)
    scale = ref.clamp_min(1e-30)                                           # a row of zeros: ssq must be exactly zero
    err = float(((ho_ssq.cpu().to(F64) - ref).abs() / scale).max())
    e_ref = float(((ref32.to(F64) - ref).abs() / scale).max())
    b = kr.bar(e_ref)
    print(f"PARITY {case} ho.ssq: err {err:.3e} E_ref {e_ref:.3e} bar {b:.3e}")
    assert err <= b


# ---- bit-exact kernels ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1000, 4096 * 256 + 1000])
def test_ew_fma_equals_fp32_replay(n):
    """out = ((alpha * a) * b + c) + beta, each operation rounded once; broadcast by modulo; n not a multiple of 256, and beyond
    4096 * 256 (the grid-stride loop)."""
    from uniaudio2_amd import ops
    Cc, alpha, beta = 96, 1.7, -0.3
    g = _gen(n)
    for (use_b, use_c), (na, nb, nc) in itertools.product(itertools.product((False, True), repeat=2),
                                                          [(n, Cc, 1), (Cc, n, n), (1, 1, Cc), (n, n, Cc)]):
        a, b, c = (torch.randn(k, generator=g) for k in (na, nb, nc))
        out = torch.full((n,), float("nan"), device="cuda")
        ops.ew_fma(a.cuda(), b.cuda() if use_b else None, c.cuda() if use_c else None, alpha, beta, out=out, n=n)
        i = np.arange(n)
        v = np.float32(alpha) * a.numpy()[i % na]
        if use_b:
            v = v * b.numpy()[i % nb]
        if use_c:
            v = v + c.numpy()[i % nc]
        v = v + np.float32(beta)
        assert v.dtype == np.float32
        _assert_same_bits(out, torch.from_numpy(v), f"ew_fma b={use_b} c={use_c} n=({na},{nb},{nc})")


@pytest.mark.parametrize("V", [16, 17, 110, 255, 256, 257, 8193, 128256])
def test_cfg_mix_equals_fp32_replay_and_feeds_the_argmax(V):
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import check, lib
    ld, scale, nb = V + 3, 1.5, (V + 15) // 16
    for pairs, forbid in itertools.product((1, 5), [None] + sorted({f for f in (0, 5, 16, 40, V - 1) if f < V})):
        g = _gen(V + pairs)
        logits = torch.randn(2 * pairs, ld, generator=g)
        # exact ties of the guided value (l0 == l1 -> guided = l1 exactly): inside one group, and across groups at the row maximum
        for cols, val in (((3, 4), 1.25), ((V - 1, max(V - 1 - 16, 0), V // 2), 9.5)):
            for c in cols:
                logits[:, c] = val
        fb = None if forbid is None else torch.full((2 * pairs,), forbid, dtype=torch.int32)
        dev = logits.cuda()
        pmax = torch.full((2 * pairs, nb), float("nan"), device="cuda")
        pidx = torch.full((2 * pairs, nb), -1, dtype=torch.int32, device="cuda")
        check(lib.ua2_cfg_mix(dev.data_ptr(), ld, V, C.c_float(scale), None if fb is None else fb.cuda().data_ptr(), pmax.data_ptr(),
                              pidx.data_ptr(), pairs, ops.stream()), "ua2_cfg_mix")
        toks = torch.full((2 * pairs, 1), -1, dtype=torch.int32, device="cuda")
        assert int(pidx.min()) >= 0 and int(pidx.max()) < V                # the gather-free tail still gets in-range ids
        ops.argmax_embed(torch.float32, pmax, pidx, toks, 0)
        out = dev.cpu()
        for p in range(pairs):
            guided = kr.cfg_mix_ref(logits[2 * p, :V], logits[2 * p + 1, :V], scale, torch.float32)
            want_pm, want_pi = kr.argmax_partials(guided.numpy(), forbid or 0)
            masked = guided.numpy().copy()
            masked[:forbid or 0] = -np.inf
            for r in (2 * p, 2 * p + 1):
                what = f"cfg_mix V={V} pairs={pairs} forbid={forbid} row {r}"
                _assert_same_bits(out[r, :V], guided, what)
                _assert_same_bits(out[r, V:], logits[r, V:], what + " (columns past V)")
                _assert_same_bits(pmax[r], torch.from_numpy(want_pm), what + " part_max")
                np.testing.assert_array_equal(pidx[r].cpu().numpy(), want_pi, err_msg=what + " part_idx")
                assert int(toks[r, 0]) == int(masked.argmax()), what


def _embed_case(dtype, M, Cc, n_cb, va, seed, mask=None):
    g = _gen(seed)
    vt = 37
    tokens = torch.randint(0, va, (M, n_cb + 1), generator=g).to(torch.int32)
    tokens[:, n_cb] = torch.randint(0, vt, (M,), generator=g).to(torch.int32)
    tokens[0, :n_cb] = 0
    tokens[M - 1, :n_cb] = va - 1                                            # ids at both ends of a codebook
    tokens[0, n_cb], tokens[M - 1, n_cb] = vt - 1, 0
    if mask is None:
        mask = (torch.rand(M, n_cb + 1, generator=g) < 0.5).to(torch.uint8)
        mask[0] = 0
        mask[M - 1] = 1                                                       # all-off and all-on rows
    audio = torch.randn(n_cb * va, Cc, generator=g).to(dtype)
    wte = torch.randn(vt, Cc, generator=g).to(dtype)
    assert int(tokens[:, :n_cb].min()) >= 0 and int(tokens[:, :n_cb].max()) < va and int(tokens[:, n_cb].max()) < vt
    return tokens, mask, audio, wte


@pytest.mark.parametrize("Cc", [128, 256, 2048, 3072, 4104])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_embed_frame_fast_path_equals_fp32_replay(dtype, Cc):
    """n_cb = 8: the masked sum runs i = 0 .. 7 in fp32.  M in {1, 3, 64}, and all 256 mask patterns of a row at M = 256."""
    from uniaudio2_amd import ops
    va = 50
    allpat = torch.tensor([[(p >> i) & 1 for i in range(8)] + [1] for p in range(256)], dtype=torch.uint8)
    for M, mask in ((1, None), (3, None), (64, None), (256, allpat)):
        tokens, mask, audio, wte = _embed_case(dtype, M, Cc, 8, va, seed=M + Cc, mask=mask)
        a, t = ops.embed_frame(dtype, tokens.cuda(), mask.cuda(), audio.cuda(), wte.cuda(), va)
        ra, rt = kr.embed_frame_ref(tokens, mask, audio, wte, va, torch.float32)
        _assert_same_bits(a, ra, f"embed_frame {dtype} C={Cc} M={M} audio_sum")
        _assert_same_bits(t, rt, f"embed_frame {dtype} C={Cc} M={M} text")


@pytest.mark.parametrize("n_cb,Cc", [(1, 100), (4, 100), (9, 100), (4, 3072), (9, 3072), (8, 100)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_embed_frame_generic_path_equals_fp32_replay(dtype, n_cb, Cc):
    from uniaudio2_amd import ops
    for M in (1, 3, 64):
        tokens, mask, audio, wte = _embed_case(dtype, M, Cc, n_cb, 23, seed=M + n_cb)
        a, t = ops.embed_frame(dtype, tokens.cuda(), mask.cuda(), audio.cuda(), wte.cuda(), 23)
        ra, rt = kr.embed_frame_ref(tokens, mask, audio, wte, 23, torch.float32)
        _assert_same_bits(a, ra, f"embed_frame generic {dtype} n_cb={n_cb} C={Cc} M={M} audio_sum")
        _assert_same_bits(t, rt, f"embed_frame generic {dtype} n_cb={n_cb} C={Cc} M={M} text")


@pytest.mark.parametrize("Cc", [128, 2048, 3072])
def test_embed_frame_handover(Cc):
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import check, lib
    for M in (1, 3, 21):
        tokens, mask, audio, wte = _embed_case(torch.bfloat16, M, Cc, 8, 50, seed=M)
        mask[M - 1] = 1
        w = (torch.rand(Cc, generator=_gen(Cc)) + 0.5).cuda()
        a, t = torch.empty(M, Cc, device="cuda"), torch.empty(M, Cc, device="cuda")
        h = torch.zeros(M, Cc, dtype=torch.bfloat16, device="cuda")
        pk = torch.zeros((M + 15) // 16 * 16 * Cc, dtype=torch.bfloat16, device="cuda")
        ssq = torch.full((M, Cc // 16), float("nan"), device="cuda")
        ho = Handover(w.data_ptr(), h.data_ptr(), Cc, pk.data_ptr(), ssq.data_ptr())
        td, md, ad, wd = tokens.cuda(), mask.cuda(), audio.cuda(), wte.cuda()
        check(lib.ua2_embed_frame(1, M, Cc, 8, 50, td.data_ptr(), md.data_ptr(), ad.data_ptr(), wd.data_ptr(), a.data_ptr(), t.data_ptr(),
                                  C.addressof(ho), ops.stream()), "ua2_embed_frame")
        _assert_same_bits(a, kr.embed_frame_ref(tokens, mask, audio, wte, 50, torch.float32)[0], "audio_sum with hand-over")
        _check_handover(f"embed_frame C={Cc} M={M}", h, pk, ssq, a, w)


@pytest.mark.parametrize("Cc", [4, 100, 1024, 1028])
def test_gather_rows(Cc):
    from uniaudio2_amd import ops
    x = torch.randn(9, Cc, generator=_gen(Cc))
    idx = torch.tensor([3, -1, 3, 0, 8, -5, 8, 8, 1, -1, 7], dtype=torch.int32)
    assert int(idx.max()) < x.shape[0]
    out = ops.gather_rows(x.cuda(), idx.cuda())
    want = torch.where((idx >= 0)[:, None], x[idx.clamp_min(0).long()], torch.zeros(1))
    _assert_same_bits(out, want)


@pytest.mark.parametrize("n_part", [1, 7, 256, 257, 8016])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_argmax_embed_scenarios(dtype, n_part):
    """Maximum in the first / last partial and in each of the four waves (partial p is read by thread p % 256); exact ties across
    partials resolve to the lowest index; -inf everywhere except one partial; out_ld > 1 leaves the neighbouring columns alone;
    the emb gather in both dtypes with emb_row_offset."""
    from uniaudio2_amd import ops
    g = _gen(n_part)
    V = 16 * n_part
    spots = sorted({0, n_part - 1} | {p for p in (3, 64 + 3, 128 + 3, 192 + 3, 256) if p < n_part})
    rows_pm, rows_pi, want = [], [], []
    base_idx = (16 * torch.arange(n_part) + torch.randint(0, 16, (n_part,), generator=g)).to(torch.int32)
    for p in spots:                                                           # a unique maximum at partial p
        pm = torch.randn(n_part, generator=g)
        pm[p] = 50.0
        rows_pm.append(pm); rows_pi.append(base_idx.clone()); want.append(int(base_idx[p]))
    for p in spots:                                                           # -inf everywhere except partial p
        pm = torch.full((n_part,), float("-inf"))
        pm[p] = -3.0
        rows_pm.append(pm); rows_pi.append(base_idx.clone()); want.append(int(base_idx[p]))
    pm = torch.randn(n_part, generator=g)                                     # ties across partials / waves: the lowest INDEX wins,
    pm[spots] = 50.0                                                          # wherever it sits: indices descend with the partial here
    pi = (16 * torch.arange(n_part) + 15).flip(0).to(torch.int32).contiguous()
    rows_pm.append(pm); rows_pi.append(pi); want.append(int(pi[spots].min()))
    rows_pm.append(torch.full((n_part,), float("-inf"))); rows_pi.append(base_idx.clone()); want.append(int(base_idx.min()))
    pmax, pidx = torch.stack(rows_pm).cuda(), torch.stack(rows_pi).cuda()
    M, Cc, off = pmax.shape[0], 24, 5
    assert int(pidx.min()) >= 0 and int(pidx.max()) < V
    emb = torch.randn(off + V, Cc, generator=g).to(dtype)
    toks = torch.full((M, 3), -7, dtype=torch.int32, device="cuda")
    nxt = torch.full((M, Cc), float("nan"), device="cuda")
    ops.argmax_embed(dtype, pmax, pidx, toks, 1, emb=emb.cuda(), emb_row_offset=off, next_h=nxt)
    t = toks.cpu()
    assert t[:, 1].tolist() == want
    assert bool((t[:, 0] == -7).all()) and bool((t[:, 2] == -7).all())
    _assert_same_bits(nxt, emb[torch.tensor(want) + off].float())


# ---- the sampling tails on rows without a winner (emb = NULL: nothing is gathered) -----------------------------------------------

def test_argmax_tail_stays_in_range_on_nan_rows():
    """All-NaN, part-NaN and all -inf rows: 0 <= id < limit, deterministic; a row nobody wins takes its lowest candidate index
    (include/ua2hip.h).  The three tails share one helper (ua2_row_token), so this covers the code the gather forms run."""
    from uniaudio2_amd import ops
    n_part = 300
    V = 16 * n_part
    nan, inf = float("nan"), float("inf")
    idx = (16 * torch.arange(n_part) + 7).to(torch.int32)
    pm = torch.randn(5, n_part, generator=_gen(0))
    pm[0] = nan
    pm[1, ::2] = nan                                                          # part NaN: the finite maximum wins
    pm[2] = -inf
    pm[3, :-1] = nan                                                          # everything NaN but the last partial
    pm[4, 1:] = nan
    pi = idx.repeat(5, 1).contiguous()
    pi[0] = idx.flip(0)                                                       # the lowest index sits in the LAST partial
    assert int(pi.min()) >= 0 and int(pi.max()) < V
    finite = torch.where(torch.isnan(pm), torch.tensor(-inf), pm)
    want = [int(pi[0].min()), int(pi[1][finite[1].argmax()]), int(pi[2].min()), int(pi[3, -1]), int(pi[4, 0])]
    outs = []
    for _ in range(2):
        toks = torch.full((5, 1), -1, dtype=torch.int32, device="cuda")
        ops.argmax_embed(torch.float32, pm.cuda(), pi.cuda(), toks, 0)
        outs.append(toks.cpu()[:, 0])
    assert torch.equal(outs[0], outs[1])
    assert bool((outs[0] >= 0).all()) and bool((outs[0] < V).all())
    assert outs[0].tolist() == want


def _sample(logits, topk, T, forbid, cnt=0, seed=99):
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import check, lib
    M, V = logits.shape
    dev = logits.cuda()
    fb = None if forbid is None else torch.as_tensor(forbid, dtype=torch.int32).cuda()
    assert fb is None or (int(fb.min()) >= 0 and int(fb.max()) + topk <= V)
    out = torch.full((M, 1), -1, dtype=torch.int32, device="cuda")
    counter = torch.tensor([cnt, 0, 0], dtype=torch.int32, device="cuda")
    check(lib.ua2_sample_topk(0, M, dev.data_ptr(), V, V, topk, C.c_float(T), None if fb is None else fb.data_ptr(), seed, counter.data_ptr(),
                              1, out.data_ptr(), 1, 0, None, 0, 0, None, 0, ops.stream()), "ua2_sample_topk")
    return out.cpu()[:, 0].long()


def test_sample_topk_stays_in_range_on_nan_rows():
    V, nan, inf = 1000, float("nan"), float("inf")
    lg = torch.randn(4, V, generator=_gen(1))
    lg[0] = nan
    lg[1, ::3] = nan
    lg[2] = -inf
    lg[3, 5:] = nan
    forbid = [3, 0, 7, 2]
    for topk in (1, 50, V - 7):
        a, b = _sample(lg, topk, 0.8, forbid), _sample(lg, topk, 0.8, forbid)
        assert torch.equal(a, b)
        assert bool((a >= 0).all()) and bool((a < V).all()), a
        assert int(a[0]) == 3 and int(a[2]) == 7                            # no score could win: the lowest column the row may sample


@pytest.mark.parametrize("topk", [1, 50, 128256])
def test_sample_topk_set_membership_at_the_text_vocabulary(topk):
    """V = 128256; rows with -inf columns; forbid + topk == V on one row: every id lies in {c >= forbid : logit_c / T >= k-th
    largest of the admitted columns}, evaluated in fp32 on the host."""
    V, M, T = 128256, 16, 0.7
    lg = torch.randn(M, V, generator=_gen(topk)) * 3
    lg[1::2, ::5] = float("-inf")
    forbid = torch.zeros(M, dtype=torch.int32)
    forbid[2], forbid[3] = min(9, V - topk), V - topk                         # row 3: forbid + topk == V
    ids = _sample(lg, topk, T, forbid)
    scaled = lg / torch.tensor(T)                                             # fp32 division, as the kernel's
    for m in range(M):
        adm = scaled[m, int(forbid[m]):]
        kth = adm.topk(topk).values[-1]
        keep = set((torch.nonzero(adm >= kth).view(-1) + int(forbid[m])).tolist())
        assert int(ids[m]) in keep, (m, int(ids[m]))


def test_sample_topk_keeps_both_zeros_at_the_threshold():
    """`logits < topk_value` removes nothing at a tie, and -0.0 < +0.0 is false: with the threshold at +0.0 the -0.0 columns stay
    in the race.  One +0.0 among -0.0 columns, topk = 1: every column is kept, so 64 independent rows do not all draw that one."""
    V, M = 8, 64
    lg = torch.full((M, V), -0.0)
    lg[:, 5] = 0.0
    ids = _sample(lg, 1, 1.0, None)
    assert bool((ids >= 0).all()) and bool((ids < V).all())
    assert len(set(ids.tolist())) > 1, ids.tolist()


# ---- tolerance tests against the float64 references ---------------------------------------------------------------------------------

@pytest.mark.parametrize("Cc", [4, 128, 1020, 1024, 3072, 4096, 4100, 8192, 16384])
def test_rmsnorm_blend(Cc):
    """C > 4096 takes the path that re-reads the row.  Rows of magnitude 1e-3, 1 and 1e3; mask values 0 and 1 in both columns."""
    from uniaudio2_amd import ops
    for M in (1, 5):
        g = _gen(Cc + M)
        x = torch.randn(M, Cc, generator=g) * torch.tensor([1e-3, 1.0, 1e3, 1.0, 1e3])[:M, None]
        w, other = torch.rand(Cc, generator=g) + 0.5, torch.randn(M, Cc, generator=g)
        mask = torch.tensor([[1, 0, 1], [0, 1, 1], [1, 1, 0], [0, 0, 1], [1, 1, 1]], dtype=torch.uint8)[:M].contiguous()
        for (oth, ca, cb), want_n in itertools.product([(None, -1, -1), (None, 0, -1), (other, -1, 1), (other, 0, 1), (other, 2, 0)], (False, True)):
            r = ops.rmsnorm_blend(x.cuda(), w.cuda(), 1e-5, None if oth is None else oth.cuda(), mask.cuda() if (ca >= 0 or oth is not None) else None,
                                  ca, cb, want_n=want_n)
            o1, n = r if want_n else (r, None)
            ref1, refn = kr.rmsnorm_blend_ref(x, w, 1e-5, oth, mask, ca, cb)
            f1, fn = kr.rmsnorm_blend_ref(x, w, 1e-5, oth, mask, ca, cb, torch.float32)
            case = f"rmsnorm_blend C={Cc} M={M} other={oth is not None} col_a={ca} col_b={cb}"
            # rows blended to exactly zero have no magnitude to be relative to: absolute against the unblended norm's scale
            scale_ref = torch.maximum(ref1.abs().amax(-1, keepdim=True), refn.abs().amax(-1, keepdim=True))
            err = float(((o1.cpu().to(F64) - ref1).abs() / scale_ref).max())
            e_ref = float(((f1.to(F64) - ref1).abs() / scale_ref).max())
            b = kr.bar(e_ref)
            print(f"PARITY {case} out1: err {err:.3e} E_ref {e_ref:.3e} bar {b:.3e}")
            assert bool(torch.isfinite(o1).all()) and err <= b
            if want_n:
                err, b = _report(case + " out2", n, refn, fn, rel_rows=True)
                assert err <= b


@pytest.mark.parametrize("Cc", [128, 1024, 4096, 8192])
def test_rmsnorm_blend_handover(Cc):
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import check, lib
    for M in (1, 5):
        g = _gen(Cc * 3 + M)
        x, other = torch.randn(M, Cc, generator=g).cuda(), torch.randn(M, Cc, generator=g).cuda()
        w, nw = (torch.rand(Cc, generator=g) + 0.5).cuda(), (torch.rand(Cc, generator=g) + 0.5).cuda()
        mask = torch.tensor([[1, 1], [0, 1], [1, 0], [1, 1], [0, 0]], dtype=torch.uint8)[:M].contiguous().cuda()
        o1 = torch.empty(M, Cc, device="cuda")
        h = torch.zeros(M, Cc, dtype=torch.bfloat16, device="cuda")
        pk = torch.zeros((M + 15) // 16 * 16 * Cc, dtype=torch.bfloat16, device="cuda")
        ssq = torch.full((M, Cc // 16), float("nan"), device="cuda")
        ho = Handover(nw.data_ptr(), h.data_ptr(), Cc, pk.data_ptr(), ssq.data_ptr())
        check(lib.ua2_rmsnorm_blend(M, Cc, x.data_ptr(), w.data_ptr(), 1e-5, other.data_ptr(), mask.data_ptr(), 2, 0, 1, o1.data_ptr(), None,
                                    C.addressof(ho), ops.stream()), "ua2_rmsnorm_blend")
        plain = ops.rmsnorm_blend(x, w, 1e-5, other, mask, 0, 1)
        _assert_same_bits(o1, plain, "out1 with and without the hand-over")
        _check_handover(f"rmsnorm_blend C={Cc} M={M}", h, pk, ssq, o1, nw)     # the row blended to zero: h, packed and ssq exactly zero


@pytest.mark.parametrize("Cc", [1, 63, 64, 255, 256, 257, 1536, 4097])
def test_layernorm_rows(Cc):
    """Rows: unit scale; mean >> std (mean 1e3, std 1: the two-pass form must survive it); a constant row (variance 0: the output is
    b, or 0, and finite)."""
    from uniaudio2_amd import ops
    g = _gen(Cc)
    x = torch.randn(4, Cc, generator=g)
    x[1] += 1e3
    x[2] = 2.5
    x[3] *= 1e-3
    w, b = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g)
    for uw, ub in itertools.product((False, True), repeat=2):
        ww, bb = (w if uw else None), (b if ub else None)
        out = ops.layernorm_rows(x.cuda(), None if ww is None else ww.cuda(), None if bb is None else bb.cuda(), 1e-5)
        ref, ref32 = kr.layernorm_ref(x, ww, bb, 1e-5), kr.layernorm_ref(x, ww, bb, 1e-5, torch.float32)
        err, bar = _report(f"layernorm_rows C={Cc} w={uw} b={ub}", out, ref, ref32)
        assert err <= bar
        _assert_same_bits(out[2], bb if ub else torch.zeros(Cc), "constant row")


@pytest.mark.parametrize("Cc", [64, 1000])
@pytest.mark.parametrize("rpb", [1, 7])
def test_time_film(Cc, rpb):
    from uniaudio2_amd import ops
    g = _gen(Cc + rpb)
    B = 4
    R = B * rpb
    params = torch.randn(R, 2 * Cc, generator=g) * 4
    params[0, :8] = torch.tensor([20.0, -20.0, 0.0, 1e-4, 9.0, -9.0, 0.5, -0.5])       # tanh saturation
    x = torch.randn(R, Cc, generator=g)
    for bm in (None, torch.tensor([0, 1, 0, 1], dtype=torch.uint8)):
        out = ops.time_film(params.cuda(), x.cuda(), None if bm is None else bm.cuda(), rpb, 0.3)
        err, bar = _report(f"time_film C={Cc} rows_per_batch={rpb} mask={bm is not None}", out,
                           kr.time_film_ref(params, x, bm, rpb, 0.3), kr.time_film_ref(params, x, bm, rpb, 0.3, torch.float32))
        assert err <= bar
        if bm is not None:
            sel = (bm.bool()[torch.arange(R) // rpb])
            _assert_same_bits(out[sel.cuda()], x[sel], "masked batch elements pass x through")


@pytest.mark.parametrize("act", [1, 2, 3], ids=["silu", "sigmoid", "tanh"])
def test_ew_act(act):
    from uniaudio2_amd import ops
    x = torch.cat([torch.linspace(-100, 100, 4001), torch.tensor([0.0, -0.0, 100.0, -100.0, 88.0, -88.0, 1e-6, -1e-6])])
    out = ops.ew_act(x.cuda(), act)
    ref = kr.ew_act_ref(x, act)
    got = out.cpu().to(F64)
    assert bool(torch.isfinite(got).all())
    scale = ref.abs().clamp_min(1.0)                                          # absolute below 1, relative above (SiLU reaches 100)
    err = float(((got - ref).abs() / scale).max())
    e_ref = float(((kr.ew_act_ref(x, act, torch.float32).to(F64) - ref).abs() / scale).max())
    b = kr.bar(e_ref)
    print(f"PARITY ew_act act={act}: err {err:.3e} E_ref {e_ref:.3e} bar {b:.3e}")
    assert err <= b


def _bf16_nearest(x64):
    """float64 -> the nearest bf16 value (one rounding), as float64, and the bf16 ulp at that value."""
    b = x64.float().to(torch.bfloat16).to(F64)                                # within one ulp of the answer
    ulp = torch.pow(2.0, torch.floor(torch.log2(b.abs().clamp_min(2.0 ** -126))) - 7)
    cand = torch.stack([b - ulp, b, b + ulp])
    best = cand.gather(0, (cand - x64).abs().argmin(0, keepdim=True))[0]
    return best, ulp


@pytest.mark.parametrize("hs", [16, 32, 48, 64, 80, 96, 128, 192, 256])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_qknorm_rope_kv(dtype, hs):
    """One thread per head dim, 64-wide shuffles: head sizes that are not a multiple of 64 run partial waves.  Checks q_out, the
    K / V read back from the pool at the addressed slot, and that every other pool element still holds its sentinel."""
    from uniaudio2_amd import ops
    SENT = 640.0                                                              # exact in bf16
    B = 6
    pos = np.array([0, 63, 64, 65, 127, 128], dtype=np.int32)                 # both sides of two page edges
    g = _gen(hs)
    max_pos = 130
    n_diff = n_tot = 0
    worst = {}                                                                # per quantity: the case closest to its bar (64 cases per test)
    for n_head, norm, rot_dim, use_seq, ring in itertools.product((1, 6), (False, True), sorted({0, hs // 2, hs, 6}), (False, True), (0, 2)):
        maxp = ring if ring else 3
        n_pages = B * maxp + 2
        table = torch.randperm(n_pages, generator=g)[:B * maxp].to(torch.int32).view(B, maxp)
        seq = torch.randperm(B, generator=g).to(torch.int32) if use_seq else torch.arange(B, dtype=torch.int32)
        assert int(table.min()) >= 0 and int(table.max()) < n_pages and sorted(seq.tolist()) == list(range(B))
        assert ring or int(pos.max()) // 64 < maxp
        qkv = torch.randn(B, 3 * n_head * hs, generator=g) + 0.5
        qw, qb, kw, kb = (torch.randn(hs, generator=g) for _ in range(4))
        half = max(rot_dim // 2, 1)
        ang = torch.arange(max_pos, dtype=F64)[:, None] * (10000.0 ** (-torch.arange(half, dtype=F64) / half))[None, :]
        cos, sin = ang.cos().float(), ang.sin().float()
        kp = torch.full((n_pages, n_head, 64, hs), SENT, dtype=dtype, device="cuda")
        vp = torch.full((n_pages, n_head, 64, hs), SENT, dtype=dtype, device="cuda")
        tab = table.cuda()
        geom = ops.kv_geom(kp, vp, tab, n_head, n_head, hs, ring_pages=ring)
        q_out = torch.full((B, n_head * hs), float("nan"), device="cuda")
        nw = dict(qw=qw.cuda(), qb=qb.cuda(), kw=kw.cuda(), kb=kb.cuda()) if norm else {}
        ops.qknorm_rope_kv(dtype, qkv.cuda(), torch.from_numpy(pos).cuda(), seq.cuda() if use_seq else None, geom, q_out, eps=1e-5,
                           cos=cos.cuda() if rot_dim else None, sin=sin.cuda() if rot_dim else None, rot_dim=rot_dim, **nw)
        torch.cuda.synchronize()
        args = (qkv, pos, n_head, hs) + ((qw, qb, kw, kb) if norm else (None,) * 4) + (1e-5, cos, sin, rot_dim)
        rq, rk, rv = kr.qknorm_rope_ref(*args)
        fq, fk, _ = kr.qknorm_rope_ref(*args, dt=torch.float32)
        case = f"qknorm_rope_kv {dtype} hs={hs} n_head={n_head} norm={norm} rot_dim={rot_dim} row_seq={use_seq} ring={ring}"
        err, b = _report(case + " q_out", q_out.view(B, n_head, hs), rq, fq, quiet=True)
        worst["q_out"] = max(worst.get("q_out", (0.0,)), (err / b, err, b, case))
        assert err <= b, (case, err, b)
        # the addressed slots, and the sentinel everywhere else
        page = table[seq.long(), torch.from_numpy(kr.page_slot(pos, ring)).long()].long()
        slot = torch.from_numpy(pos % 64).long()
        kh, vh = kp.cpu(), vp.cpu()
        got_k, got_v = kh[page, :, slot], vh[page, :, slot]                   # [B, n_head, hs]
        untouched = torch.ones(n_pages, 64, dtype=torch.bool)
        untouched[page, slot] = False
        for pool in (kh, vh):
            assert bool((pool.permute(0, 2, 1, 3)[untouched] == SENT).all()), case + ": a slot that was not addressed changed"
        if dtype == torch.float32:
            err, b = _report(case + " K", got_k, rk, fk, quiet=True)
            worst["K"] = max(worst.get("K", (0.0,)), (err / b, err, b, case))
            assert err <= b, (case, err, b)
            _assert_same_bits(got_v, rv.float(), case + " V")
        else:
            _assert_same_bits(got_v, rv.float().to(torch.bfloat16), case + " V")
            want, ulp = _bf16_nearest(rk)
            d = (got_k.to(F64) - want).abs()
            # One bf16 ulp of the rounded reference, plus the absolute fp32 bar of the K formula: where the rotary sum cancels to
            # ~1e-6 the fp32 value carries an absolute error (~1e-7 at unit scale) far above a bf16 ulp of the tiny result — the
            # plain fp32 host formula itself misses "one ulp" there (2 of 53760 elements at hs = 64 / 256 with these seeds).
            # stored = RNE(k32), |k32 - ref| <= bar_abs  =>  |stored - want| <= ulp + bar_abs.
            _, b_rel = _report(case + " K", fk, rk, fk, quiet=True)
            bar_abs = b_rel * max(1.0, float(rk.abs().max()))
            assert bool((d <= ulp + bar_abs).all()), (case, float((d - ulp).max()), bar_abs)
            n_diff += int((d > 0).sum()); n_tot += d.numel()
            # the same share for fp32-then-bf16 rounding of the float64 reference itself (host): double rounding alone stays under 1 %
            assert float((rk.float().to(torch.bfloat16).to(F64) != want).double().mean()) < 0.01
    for what, (ratio, err, b, case) in sorted(worst.items()):
        print(f"PARITY worst of 64: {case} {what}: err {err:.3e} bar {b:.3e} (E_ref {b / 4:.3e} unless the floor holds)")
    if dtype == torch.bfloat16:
        print(f"PARITY qknorm_rope_kv bf16 hs={hs} stored K: {n_diff} of {n_tot} elements differ from the rounded reference by one ulp")
        assert n_diff < 0.01 * n_tot


def _dw_cases():
    out = []
    for K, stride, dilation in itertools.product((4, 7), (1, 2, 4), (1, 3)):
        for pad_left in (0, K - 1):
            out.append(dict(K=K, stride=stride, dilation=dilation, pad_left=pad_left, transposed=False))
    for stride in (2, 4, 6):
        for K in (2 * stride, 2 * stride + 1):
            for pad_left in (0, stride, K - stride):
                out.append(dict(K=K, stride=stride, dilation=1, pad_left=pad_left, transposed=True))
    return out


@pytest.mark.parametrize("cfg", _dw_cases(), ids=lambda c: "-".join(f"{k}{int(v)}" for k, v in c.items()))
def test_dwconv1d(cfg):
    """Forward and transposed depthwise conv, bias on / off, Tout shorter and longer than the natural length (zero-padded tail).
    The kernel is an fma chain in ascending tap order: a tolerance test."""
    from uniaudio2_amd import ops
    K, stride, dilation, pad_left, tr = cfg["K"], cfg["stride"], cfg["dilation"], cfg["pad_left"], cfg["transposed"]
    g = _gen(K * 100 + stride)
    B, Cc, Tin = 2, 5, 41
    x, w, bias = torch.randn(B, Cc, Tin, generator=g), torch.randn(Cc, K, generator=g), torch.randn(Cc, generator=g)
    natural = ((Tin - 1) * stride + K - pad_left) if tr else ((Tin + pad_left - (K - 1) * dilation - 1) // stride + 1)
    for Tout, use_bias in itertools.product((max(natural - 3, 1), natural + 9), (False, True)):
        bb = bias if use_bias else None
        y = ops.dwconv1d(x.cuda(), w.cuda(), stride=stride, dilation=dilation, pad_left=pad_left, Tout=Tout, bias=None if bb is None else bb.cuda(),
                         transposed=tr)
        kw = dict(stride=stride, dilation=dilation, pad_left=pad_left, Tout=Tout, transposed=tr)
        err, b = _report(f"dwconv1d {cfg} Tout={Tout} bias={use_bias}", y, kr.dwconv_ref(x, w, bb, **kw), kr.dwconv_ref(x, w, bb, dt=torch.float32, **kw))
        assert err <= b
