"""The order-free many-row GEMM (csrc/ua2_gemm2.hip, `sum_order = UA2_SUM_ORDER_FREE`) against float64 restatements of
include/ua2hip.h (tests/linear_refs.py): the three kernel instantiations, the K-slab combine, the tail-split combine, both halves
of the scaled-norm hand-over, the arg-max partials and the LayerNorm hand-over (y_ln_w).  tests/test_gpu_gemm2.py compares the
same family with the invariant kernels of ua2_gemm.hip only; this module is its anchor.

Tolerance: the rule of tests/test_gpu_linear_parity.py — bar = kr.bar(E_ref) = max(4 E_ref, 8 * 2^-24) of the launch's scale
max(1, max |ref|), E_ref = error of the fp32 replay lr.linear_ref(dt=F32) on the very inputs of the launch.  The replay's K sum is
one left-to-right chain over the 32-wide chunks: the order-free kernel's own order.  Every launch prints
`PARITY gemm2 <case>: err ... E_ref ... bar ...`.

Hygiene, as in that module: output buffers are pre-filled with a finite sentinel, row strides are wider than the rows, pad columns
(and rows of a packed output past M, and cache slots no row owns) must still hold the sentinel afterwards, inputs must be unchanged,
nothing non-finite is sent to a kernel (split_ws excepted: it is scratch the launch must overwrite before it reads), index inputs
are asserted in range on the host.  Every launch asserts through ua2_debug_kernel_launches(b"gemm2") that the order-free kernel took
it.

Short K.  The ring of NB slots is filled by `dma(t, t)` for t < NB - 1 and refilled by `dma(c + NB - 1, ..)` in every step; `dma`
clamps its chunk to nchunks - 1 (an address inside the operand), its slot index is < NB by construction, and the step count
(whole turns + `r = nchunks - c0` steps) depends on nchunks alone, which is uniform over the workgroup — so a launch with fewer
chunks than slots reads and writes in bounds and every wave passes the same barriers.  Those launches therefore run here
(1 and 2 chunks) instead of being refused."""
import functools
import os

import numpy as np
import pytest
import torch

import kernel_refs as kr
import linear_refs as lr
import test_gpu_linear_parity as lp
from test_gpu_rowwise import _check_handover, _decode_packed_bf16

pytestmark = pytest.mark.gpu

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
SENT = lp.SENT
EPS = lp.EPS
PAD = 4
PRO_SCALED = 4                                                     # include/ua2hip.h UA2_PRO_SCALED

# kernel form -> (knobs, ring slots).  128-row tiles take the six-slot ring when the grid has at most 256 workgroups (every grid here)
FORMS = {"bmt16_nb4": (dict(UA2_GEMM2_BMT=16), 4), "bmt8_nb6": (dict(UA2_GEMM2_BMT=8), 6), "bmt8_nb3": (dict(UA2_GEMM2_BMT=8, UA2_GEMM2_NO_DEEP=1), 3)}
MS = (257, 300)                                                    # a row block with ONE live row; a ragged last 16-row tile
N_DENSE, N_GLU, N_STORE = 320, 288, 328                            # second column block a quarter full; N % 32; 20 x 16 + 8
CHUNKS = (1, 2, 5, 7, 33, 48, 64)
KS = tuple(32 * c for c in CHUNKS)
K2 = (160, 1056)                                                   # the two K of every epilogue but RESIDUAL x CAST
SLAB_KS, SLAB_S = (3072, 3104), (2, 3, 4)
LN_NS, LN_SPLIT_KS, LN_EPS = (64, 320, 1536, 2048), (1152, 1536), 1e-6

# ---- coverage of the lists above ------------------------------------------------------------------------------------------------
assert sorted(nb for _, nb in FORMS.values()) == [3, 4, 6]
for _nb in (3, 4, 6):
    assert {c % _nb for c in CHUNKS} == set(range(_nb)), f"ring of {_nb}: a remainder is missing"
    assert any(c < _nb - 1 for c in CHUNKS), f"ring of {_nb}: no launch shorter than the prologue"
assert all(32 <= k <= 2048 and k % 32 == 0 for k in KS) and set(K2) <= set(KS)
assert any((k // 32) % s for k in SLAB_KS for s in SLAB_S) and all((3104 // 32) % s for s in SLAB_S)   # 97 chunks: every split uneven
assert all(max((m + 127) // 128, 1) * ((n + 255) // 256) * 4 <= 256 for m in MS for n in (N_DENSE, N_GLU, N_STORE, 2048))   # "deep" grids
assert all(k // 32 >= 36 for k in LN_SPLIT_KS)


@pytest.fixture
def g2env():
    """Sets UA2_GEMM2_* knobs for the launches that follow (every other key of the list is cleared) and tells the launchers to re-read
    them; the environment is restored afterwards."""
    from uniaudio2_amd._lib import lib
    keys = ("UA2_GEMM2_BMT", "UA2_GEMM2_OFF", "UA2_GEMM2_MIN_ROWS", "UA2_GEMM2_FORCE", "UA2_GEMM_NO_KSPLIT", "UA2_GEMM2_NO_TAIL", "UA2_GEMM2_R5_FORMS",
            "UA2_GEMM2_NO_DEEP", "UA2_GEMM2_TAIL_MIN_CHUNKS", "UA2_GEMM2_KSPLIT_MIN_CHUNKS")
    saved = {k: os.environ.get(k) for k in keys}

    def set_(**kw):
        assert set(kw) <= set(keys)
        for k in keys:
            os.environ.pop(k, None)
        for k, v in kw.items():
            os.environ[k] = str(v)
        lib.ua2_debug_refresh_env()
    yield set_
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    lib.ua2_debug_refresh_env()


def _judge(case, got, ref, ref32):
    """lp._judge's rule under this family's name: err, E_ref, bar of one launch relative to max(1, max |ref|)."""
    got = got.detach().cpu().to(F64)
    assert bool(torch.isfinite(got).all()), f"{case}: non-finite output"
    scale = max(1.0, float(ref.abs().max()))
    err = float((got - ref).abs().max()) / scale
    e_ref = float((ref32.to(F64) - ref).abs().max()) / scale
    b = kr.bar(e_ref)
    print(f"PARITY gemm2 {case}: err {err:.3e} E_ref {e_ref:.3e} bar {b:.3e}")
    return err, b


@functools.lru_cache(maxsize=None)
def _weight(N, K, which=0):
    g = torch.Generator().manual_seed(7919 * N + K + 104729 * which + 17)
    return torch.randn(N, K, generator=g) * K ** -0.5


@functools.lru_cache(maxsize=8)
def _packed(N, K, which=0, rope_hs=0):
    from uniaudio2_amd import ops
    return ops.pack_linear(_weight(N, K, which).cuda(), BF16, rope_head_size=rope_hs)


def _cu(t):
    return None if t is None else t.cuda()


def _launch(n_expected=1, **args):
    """One ua2_linear under the order-free contract; asserts how many gemm2_kernel launches it made."""
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import SUM_ORDER_FREE, lib
    n0 = lib.ua2_debug_kernel_launches(b"gemm2")
    ops.linear(dtype=BF16, sum_order=SUM_ORDER_FREE, **args)
    torch.cuda.synchronize()
    n = lib.ua2_debug_kernel_launches(b"gemm2") - n0
    assert n == n_expected, f"{n} launches of the order-free kernel, expected {n_expected}"


def _packed_rows_past_m(pk, M, N):
    """The rows M .. of the last 16-row tile of a packed [ceil(M/16)][N/32][64 lanes][8] output."""
    return pk.cpu().view((M + 15) // 16, N // 32, 4, 16, 8)[-1, :, :, M % 16:, :] if M % 16 else pk.cpu()[:0]


# ---- STORE / RESIDUAL / SWIGLU / GELU -----------------------------------------------------------------------------------------

def _run_dense(g2env, tag, N, K, *, epi, forms=tuple(FORMS), Ms=MS, pro=lr.PRO_CAST, norm_kind=0, bias=False, bias1=False, out_scale=False,
               act_kind=0, packed=False, slabs=0):
    """One (prologue, epilogue) configuration on every kernel form at every row count: the references once for the most rows.
    slabs > 0: split_ws (NaN-filled) sized for exactly that many K slabs (+ 3 elements that must stay NaN).  Returns worst err / bar."""
    from uniaudio2_amd import ops
    dev = torch.device("cuda")
    Mmax = max(Ms)
    if pro == lr.PRO_CAST:
        x, nw, nb = lp._rows("x", Mmax, K), None, None
    else:
        x, nw, nb, rec = lr.norm_inputs(K, norm_kind, EPS)
        assert Mmax <= x.shape[0]
        assert int(lr.flip_candidates(x, pro, norm_kind, nw, nb, EPS, rec["delta"]).sum()) == 0, "flip candidates in a NORM input"
    glu = epi == lr.EPI_SWIGLU
    W, W1 = _weight(N, K, 0), (_weight(N, K, 1) if glu else None)
    b0 = lp._vec("bias", N) if bias else None
    b1 = lp._vec("bias1", N) if bias1 else None
    osc = lp._vec("out_scale", N) if out_scale else None
    resid = lp._rows("resid", Mmax, N) if epi == lr.EPI_RESIDUAL else None
    assert all(bool(torch.isfinite(t).all()) for t in (x, W, W1, b0, b1, osc, resid, nw, nb) if t is not None)
    kw = dict(pro=pro, epi=epi, norm_kind=norm_kind, norm_w=nw, norm_b=nb, eps=EPS, W1=W1, bias=b0, bias1=b1, resid=resid, out_scale=osc,
              act_kind=act_kind)
    ref = lr.linear_ref(x[:Mmax], W, BF16, dt=F64, **kw)
    ref32 = lr.linear_ref(x[:Mmax], W, BF16, dt=F32, **kw)
    p0, p1 = _packed(N, K, 0), (_packed(N, K, 1) if glu else None)
    npart = (N + 15) // 16
    forbid = (torch.arange(Mmax, dtype=torch.int32) * 5) % 23
    assert int(forbid.min()) >= 0 and int(forbid.max()) < N
    worst = 0.0
    for form in forms:
        g2env(**FORMS[form][0])
        for M in Ms:
            xd, yd = lp._strided(x[:M], PAD), torch.full((M, N + PAD), SENT, device=dev)
            args = dict(M=M, N=N, K=K, w0=p0, w1=p1, prologue=pro, epilogue=epi, x=xd, y=yd, norm_w=_cu(nw), norm_b=_cu(nb), norm_kind=norm_kind,
                        eps=EPS, bias=_cu(b0), bias1=_cu(b1), out_scale=_cu(osc), act_kind=act_kind, workspace=ops.linear_workspace(BF16, M, K, dev))
            if epi == lr.EPI_RESIDUAL:
                rd = lp._strided(resid[:M], PAD)
                args.update(resid=rd)
            if epi == lr.EPI_STORE:
                pm = torch.full((M, npart), SENT, device=dev)
                pi = torch.full((M, npart), -7, dtype=torch.int32, device=dev)
                args.update(part_max=pm, part_idx=pi, forbid=forbid[:M].cuda())
            if packed:
                pk = torch.full(((M + 15) // 16 * 16 * N,), SENT, dtype=BF16, device=dev)
                args.update(y_packed=pk)
            if slabs:
                sw = torch.full((slabs * M * N + 3,), float("nan"), device=dev)
                args.update(split_ws=sw)
            _launch(**args)
            y = yd.cpu()
            case = f"{tag} {form} N={N} K={K} M={M}" + (f" S={slabs}" if slabs else "")
            assert lp._same_bits(y[:, N:], torch.full((M, PAD), SENT)), f"{case}: pad columns of y written"
            if epi == lr.EPI_RESIDUAL:
                assert lp._same_bits(rd.cpu(), lp._strided(resid[:M], PAD, "cpu")), f"{case}: resid changed"
            assert lp._same_bits(xd.cpu(), lp._strided(x[:M], PAD, "cpu")), f"{case}: x changed"
            err, b = _judge(case, y[:, :N], ref[:M], ref32[:M])
            assert err <= b, f"{case}: err {err:.3e} over bar {b:.3e}"
            worst = max(worst, err / b)
            if slabs:                                               # exactly S slabs ran, each wrote every partial sum, nothing beyond them
                swc = sw.cpu()
                assert bool(torch.isfinite(swc[:slabs * M * N]).all()), f"{case}: a slab's partial sums are missing"
                assert bool(torch.isnan(swc[slabs * M * N:]).all()), f"{case}: split_ws written past its slabs"
            if epi == lr.EPI_STORE:                                 # the partials of the kernel's OWN row, exactly
                pmc, pic = pm.cpu().numpy(), pi.cpu().numpy()
                for m in range(M):
                    wm, wi = kr.argmax_partials(y[m, :N].numpy(), int(forbid[m]))
                    np.testing.assert_array_equal(pmc[m], wm, err_msg=f"{case}: part_max row {m}")
                    np.testing.assert_array_equal(pic[m], wi, err_msg=f"{case}: part_idx row {m}")
            if packed:                                              # RNE to bf16 of the kernel's own fp32 y, bit for bit
                assert lp._same_bits(lr.unpack_operand(pk, BF16, M, N), y[:, :N].to(BF16)), f"{case}: y_packed"
                tail = _packed_rows_past_m(pk, M, N)
                assert lp._same_bits(tail, torch.full_like(tail, SENT)), f"{case}: y_packed rows past M written"
    return worst


@pytest.mark.parametrize("K", KS)
def test_residual_cast_every_ring_remainder(K, g2env):
    """resid + out_scale (x W^T + bias), all four bias / out_scale combinations, at every K of the list (ring remainders 0 .. NB - 1 of
    the three rings, and launches shorter than the ring's prologue) on the three kernel forms at 257 and 300 rows."""
    for osc, bias in ((False, False), (True, True), (True, False), (False, True)):
        _run_dense(g2env, f"residual cast out_scale={int(osc)} bias={int(bias)}", N_DENSE, K, epi=lr.EPI_RESIDUAL, bias=bias, out_scale=osc)


@pytest.mark.parametrize("K", K2)
def test_store_and_argmax_partials(K, g2env):
    """STORE at N = 328 (the per-lane column guard; the last arg-max group is half a tile) with part_max / part_idx / forbid."""
    for bias in (False, True):
        _run_dense(g2env, f"store cast bias={int(bias)}", N_STORE, K, epi=lr.EPI_STORE, bias=bias)


@pytest.mark.parametrize("K", K2)
def test_swiglu(K, g2env):
    """silu(s0 + b0) (s1 + b1) and (s0 + b0) sigmoid(s1 + b1) at N = 288 (N % 32 == 0 only), with and without y_packed."""
    for packed in (False, True):
        _run_dense(g2env, f"swiglu packed={int(packed)}", N_GLU, K, epi=lr.EPI_SWIGLU, packed=packed)
        _run_dense(g2env, f"swiglu sigmoid_second bias packed={int(packed)}", N_GLU, K, epi=lr.EPI_SWIGLU, bias=True, bias1=True,
                   act_kind=lr.GATE_SIGMOID_SECOND, packed=packed)


@pytest.mark.parametrize("K", K2)
def test_gelu(K, g2env):
    for act in (lr.ACT_DEFAULT, lr.GELU_TANH):
        _run_dense(g2env, f"gelu {'tanh' if act else 'erf'} bias", N_DENSE, K, epi=lr.EPI_GELU, bias=True, act_kind=act, packed=bool(act))


@pytest.mark.parametrize("name,norm_kind,K", [("rms_lit", lr.NORM_RMS_LIT, 2048), ("layernorm", lr.NORM_LAYERNORM, 1536)])
def test_norm_prologue_through_the_prep_launch(name, norm_kind, K, g2env):
    """UA2_PRO_NORM: the prep launch builds the bf16 operand from the flip-free rows of lr.norm_inputs (300 rows), into SWIGLU and STORE."""
    _run_dense(g2env, f"swiglu {name}", N_GLU, K, epi=lr.EPI_SWIGLU, pro=lr.PRO_NORM, norm_kind=norm_kind)
    _run_dense(g2env, f"store {name} bias", N_STORE, K, epi=lr.EPI_STORE, pro=lr.PRO_NORM, norm_kind=norm_kind, bias=True)


@pytest.mark.parametrize("K", SLAB_KS)
def test_k_slabs_and_their_combine(K, g2env):
    """RESIDUAL with bias and out_scale as S = 2, 3 and 4 K slabs + gemm2_combine_kernel (split_ws NaN-filled and sized for S): at
    K = 3104 (97 chunks) every split is uneven.  No NaN may reach y (the judge requires a finite y)."""
    for S in SLAB_S:
        _run_dense(g2env, "slabs residual out_scale=1 bias=1", N_DENSE, K, epi=lr.EPI_RESIDUAL, bias=True, out_scale=True, slabs=S)


# ---- q|k|v + RoPE + paged cache append ------------------------------------------------------------------------------------------

QKV_M, QKV_NSEQ, QKV_POS0, QKV_MAXPOS = 257, 3, 20, 128            # sequence s holds rows s, s + 3, ..: positions 20 .. 105 (63 | 64, 65)
QKV_FORMS = [("lm", 1, 1, 128), ("lm", 2, 1, 128), ("lm", 1, 1, 64), ("lm", 3, 1, 64), ("dit", 1, 1, 64), ("dit", 2, 2, 64)]
assert all(((nh + 2 * nkv) * hs) % 64 == 0 for _, nh, nkv, hs in QKV_FORMS)


def _qkv_geometry(hs, seed):
    """(pos, seq, table, n_pages, cos, sin, slot of every row): 257 rows over three sequences, a permuted page table, range-checked."""
    g = torch.Generator().manual_seed(seed)
    M = QKV_M
    seq = (torch.arange(M) % QKV_NSEQ).to(torch.int32)
    pos = (QKV_POS0 + torch.arange(M) // QKV_NSEQ).to(torch.int32)
    max_pages = QKV_MAXPOS // kr.PAGE
    n_pages = QKV_NSEQ * max_pages + 3
    table = torch.randperm(n_pages, generator=g)[:QKV_NSEQ * max_pages].to(torch.int32).view(QKV_NSEQ, max_pages)
    ang = torch.rand(QKV_MAXPOS, hs // 2, generator=g) * 6.28
    assert int(table.min()) >= 0 and int(table.max()) < n_pages and len(set(table.flatten().tolist())) == QKV_NSEQ * max_pages
    assert int(pos.min()) >= 0 and int(pos.max()) < QKV_MAXPOS and {63, 64, 65} <= set(pos.tolist())
    assert int(seq.min()) >= 0 and int(seq.max()) < QKV_NSEQ
    assert len({(int(s), int(p)) for s, p in zip(seq, pos)}) == M                       # no two rows share a slot
    return pos, seq, table, n_pages, ang.cos(), ang.sin()


def _check_qkv(case, q, kp, vp, ref, ref32, pos, seq, table, n_pages, nkv, hs):
    """The cache checks of lp._run_qkv: q under the bar; the k / v rows at their slots under the bar after half a bf16 ulp of the
    value (the kernel rounds its own fp32 result once); slots no row owns still hold the sentinel."""
    M = q.shape[0]
    rq, rk, rv = ref
    qc, kc_, vc = q.cpu().to(F64).view(rq.shape), kp.cpu(), vp.cpu()
    assert bool(torch.isfinite(qc).all()) and bool(torch.isfinite(kc_.float()).all()) and bool(torch.isfinite(vc.float()).all())
    scale = max(1.0, float(max(rq.abs().max(), rk.abs().max(), rv.abs().max())))
    e_ref = max(float((a.to(F64) - b).abs().max()) for a, b in zip(ref32, ref)) / scale
    b = kr.bar(e_ref)
    err_q = float((qc - rq).abs().max()) / scale
    page = table[seq.long(), pos.long() // kr.PAGE].long()
    off = pos.long() % kr.PAGE
    err_kv = 0.0
    for pool, r in ((kc_, rk), (vc, rv)):
        d = (pool[page, :, off].to(F64) - r).abs()                   # [M, nkv, hs]
        err_kv = max(err_kv, float((d - lr.half_ulp_bf16(r)).clamp_min(0.0).max()) / scale)
    print(f"PARITY gemm2 {case}: err {max(err_q, err_kv):.3e} (q {err_q:.3e} kv {err_kv:.3e}) E_ref {e_ref:.3e} bar {b:.3e}")
    assert err_q <= b and err_kv <= b, f"{case}: q {err_q:.3e} kv {err_kv:.3e} over bar {b:.3e}"
    written = torch.zeros(n_pages, kr.PAGE, dtype=torch.bool)
    written[page, off] = True
    assert int(written.sum()) == M
    untouched = ~written[:, None, :, None].expand(n_pages, nkv, kr.PAGE, hs)
    sent = torch.tensor(SENT).to(BF16)
    for pool, nm in ((kc_, "k"), (vc, "v")):
        assert bool((lp._bits(pool)[untouched] == lp._bits(sent)).all()), f"{case}: a {nm} slot no row owns was written"


@pytest.mark.parametrize("kind,nh,nkv,hs", QKV_FORMS)
def test_qkv_rope_cache_append(kind, nh, nkv, hs, g2env):
    """The LM's form (half-split rotation on a weight packed with rope_head_size, head size 128 and 64) and the DiT's (no rotation,
    bias, head size 64): 257 rows over three sequences, positions straddling a page edge, a permuted page table."""
    from uniaudio2_amd import ops
    dev = torch.device("cuda")
    M, N = QKV_M, (nh + 2 * nkv) * hs
    mode = lr.ROPE_HALF_SPLIT if kind == "lm" else lr.ROPE_NONE
    pos, seq, table, n_pages, cos, sin = _qkv_geometry(hs, 1000 * hs + N)
    b0 = lp._vec("bias", N) if kind == "dit" else None
    for K in K2:
        x, W = lp._rows("x", M, K), _weight(N, K, 0)
        qkv = dict(pos=pos, n_head=nh, n_kv=nkv, hs=hs, rope_mode=mode, cos=cos, sin=sin)
        kw = dict(epi=lr.EPI_QKV_ROPE, bias=b0, qkv=qkv)
        ref, ref32 = lr.linear_ref(x, W, BF16, dt=F64, **kw), lr.linear_ref(x, W, BF16, dt=F32, **kw)
        p0 = _packed(N, K, 0, hs if kind == "lm" else 0)
        for form in FORMS:
            g2env(**FORMS[form][0])
            xd = lp._strided(x, PAD)
            kp = torch.full((n_pages, nkv, kr.PAGE, hs), SENT, dtype=BF16, device=dev)
            vp = torch.full_like(kp, SENT)
            q = torch.full((M, nh * hs), SENT, device=dev)
            td = table.cuda()                                       # kv_geom keeps the pointer only: the tensor must outlive the launch
            _launch(M=M, N=N, K=K, w0=p0, prologue=lr.PRO_CAST, epilogue=lr.EPI_QKV_ROPE, x=xd, bias=_cu(b0), row_pos=pos.cuda(), row_seq=seq.cuda(),
                    rope_cos=cos.cuda(), rope_sin=sin.cuda(), q_out=q, rope_mode=mode, kv=ops.kv_geom(kp, vp, td, nh, nkv, hs),
                    workspace=ops.linear_workspace(BF16, M, K, dev))
            assert torch.equal(td.cpu(), table), f"{form} K={K}: the page table changed"
            case = f"qkv {kind} {form} {nh}/{nkv}/{hs} K={K} M={M}"
            assert lp._same_bits(xd.cpu(), lp._strided(x, PAD, "cpu")), f"{case}: x changed"
            _check_qkv(case, q, kp, vp, ref, ref32, pos, seq, table, n_pages, nkv, hs)


# ---- tail split -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("handover", [False, True], ids=["plain", "handover"])
def test_tail_split_and_its_combine(handover, g2env):
    """17 x 16 = 272 tiles of 256 x 256 (the launcher's own tile choice): 256 tiles whole, the last 16 as two K slabs on a second
    launch + gemm2_tail_combine_kernel.  float64 for three rows of every 256-row block over all columns (rows are independent: every
    tile is reached).  With y_norm_w the tail tiles' hand-over comes from the combine: checked over the whole output."""
    from uniaudio2_amd import ops
    dev = torch.device("cuda")
    M, N, K = 4352, 4096, 1024
    g2env(UA2_GEMM2_TAIL_MIN_CHUNKS=K // 32)
    x, resid, W = lp._rows("x", M, K), lp._rows("resid", M, N), _weight(N, K, 0)
    b0, osc = lp._vec("bias", N), lp._vec("out_scale", N)
    rows = lr.sample_rows(M, 256)
    assert len(rows) == 3 * 17 and all(any(r // 256 == blk for r in rows) for blk in range(17))
    kw = dict(epi=lr.EPI_RESIDUAL, bias=b0, out_scale=osc, resid=resid[rows])
    ref, ref32 = lr.linear_ref(x[rows], W, BF16, dt=F64, **kw), lr.linear_ref(x[rows], W, BF16, dt=F32, **kw)
    xd, rd, yd = lp._strided(x, PAD), lp._strided(resid, PAD), torch.full((M, N + PAD), SENT, device=dev)
    sw = torch.full((8 * 16 * 256 * 256,), float("nan"), device=dev)
    args = dict(M=M, N=N, K=K, w0=_packed(N, K, 0), prologue=lr.PRO_CAST, epilogue=lr.EPI_RESIDUAL, x=xd, y=yd, resid=rd, bias=b0.cuda(), out_scale=osc.cuda(),
                split_ws=sw, workspace=ops.linear_workspace(BF16, M, K, dev))
    if handover:
        nw = (1.0 + 0.1 * torch.randn(N, generator=torch.Generator().manual_seed(5))).cuda()
        yh = torch.full((M, N + 8), SENT, dtype=BF16, device=dev)
        pk = torch.full((M * N,), SENT, dtype=BF16, device=dev)
        ssq = torch.full((M, N // 16), SENT, device=dev)
        args.update(y_norm_w=nw, y_h=yh, ldh=N + 8, y_packed=pk, y_ssq=ssq)
    _launch(n_expected=2, **args)
    case = f"tail residual handover={int(handover)} N={N} K={K} M={M}"
    assert bool((~torch.isnan(sw)).any()), f"{case}: the tail slabs did not run"
    assert bool((yd[:, N:] == SENT).all()), f"{case}: pad columns of y written"
    assert torch.equal(rd, lp._strided(resid, PAD)) and torch.equal(xd, lp._strided(x, PAD)), f"{case}: an input changed"
    assert bool(torch.isfinite(yd).all()), f"{case}: non-finite y"
    err, b = _judge(case, yd[rows, :N], ref, ref32)
    assert err <= b, f"{case}: err {err:.3e} over bar {b:.3e}"
    if handover:
        assert bool((yh[:, N:].float() == torch.tensor(SENT).to(BF16).float()).all()), f"{case}: pad columns of y_h written"
        _check_handover(case, yh[:, :N], pk, ssq, yd[:, :N].contiguous(), nw)


# ---- scaled-norm hand-over: producer and consumers ------------------------------------------------------------------------------

def _produce(g2env, form, epi, C, Kp, M):
    """An order-free RESIDUAL / STORE launch Kp -> C with y_norm_w: returns (y [M, C] fp32, operand [M, C] bf16 bits, ssq [M, C / 16])
    on the host after the producer's own checks.  Row 5 is all zero (x and resid): its operand and ssq must be exactly zero."""
    from uniaudio2_amd import ops
    dev = torch.device("cuda")
    x = lp._rows("x", M, Kp).clone()
    x[5] = 0.0
    osc = lp._vec("out_scale", C) if epi == lr.EPI_RESIDUAL else None
    resid = None
    if epi == lr.EPI_RESIDUAL:
        resid = lp._rows("resid", M, C).clone()
        resid[5] = 0.0
    W = _weight(C, Kp, 2)
    nw = 1.0 + 0.1 * torch.randn(C, generator=torch.Generator().manual_seed(C))
    kw = dict(epi=epi, out_scale=osc, resid=resid)
    ref, ref32 = lr.linear_ref(x, W, BF16, dt=F64, **kw), lr.linear_ref(x, W, BF16, dt=F32, **kw)
    g2env(**FORMS[form][0])
    xd, yd = lp._strided(x, PAD), torch.full((M, C + PAD), SENT, device=dev)
    yh = torch.full((M, C + 8), SENT, dtype=BF16, device=dev)
    pk = torch.full(((M + 15) // 16 * 16 * C,), SENT, dtype=BF16, device=dev)
    ssq = torch.full((M, C // 16), SENT, device=dev)
    args = dict(M=M, N=C, K=Kp, w0=_packed(C, Kp, 2), prologue=lr.PRO_CAST, epilogue=epi, x=xd, y=yd, out_scale=_cu(osc), y_norm_w=nw.cuda(), y_h=yh,
                ldh=C + 8, y_packed=pk, y_ssq=ssq, workspace=ops.linear_workspace(BF16, M, Kp, dev))
    if resid is not None:
        args.update(resid=lp._strided(resid, PAD))
    _launch(**args)
    case = f"producer {'residual' if epi == lr.EPI_RESIDUAL else 'store'} {form} N={C} K={Kp} M={M}"
    y = yd.cpu()
    assert lp._same_bits(y[:, C:], torch.full((M, PAD), SENT)), f"{case}: pad columns of y written"
    assert lp._same_bits(yh.cpu()[:, C:], torch.full((M, 8), SENT, dtype=BF16)), f"{case}: pad columns of y_h written"
    assert lp._same_bits(xd.cpu(), lp._strided(x, PAD, "cpu")), f"{case}: x changed"
    err, b = _judge(case, y[:, :C], ref, ref32)
    assert err <= b, f"{case}: err {err:.3e} over bar {b:.3e}"
    _check_handover(case, yh[:, :C], pk, ssq, yd[:, :C].contiguous(), nw.cuda())
    tail = _packed_rows_past_m(pk, M, C)
    assert lp._same_bits(tail, torch.full_like(tail, SENT)), f"{case}: y_packed rows past M written"
    op = _decode_packed_bf16(pk.cpu(), M, C)
    assert int(lp._bits(y[5, :C]).abs().sum()) == 0 and float(op[5].float().abs().sum()) == 0.0 and float(ssq[5].abs().sum()) == 0.0, \
        f"{case}: the all-zero row"
    return pk, ssq, op, ssq.cpu()


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("C", [320, 1088])
def test_scaled_norm_handover_producer_and_consumers(C, form, g2env):
    """Producer (y_norm_w on RESIDUAL and STORE): y under the bar; y_h and y_packed = RNE_bf16(own y * w) bit for bit, y_ssq against
    float64 sums of the kernel's own y (_check_handover of test_gpu_rowwise.py); an all-zero row gives exactly zero.
    Consumers (UA2_PRO_SCALED: STORE, SWIGLU, q|k|v half-split) on the RESIDUAL producer's hand-over: the reference is built from the
    bits read back — rstd = rsqrt(sum_j ssq[m][j] / K + eps), y = epilogue(rstd[m] (operand W^T)) in float64."""
    from uniaudio2_amd import ops
    dev = torch.device("cuda")
    M, Kp = 257, 160
    _produce(g2env, form, lr.EPI_STORE, C, Kp, M)
    pk, ssq, op, ssq_h = _produce(g2env, form, lr.EPI_RESIDUAL, C, Kp, M)
    assert bool(torch.isfinite(op.float()).all()) and bool(torch.isfinite(ssq_h).all())
    pk0, ssq0 = pk.clone(), ssq.clone()
    ws = torch.full((M + 3,), SENT, device=dev)                      # the row scales go here: M floats
    base = dict(M=M, K=C, prologue=PRO_SCALED, x_packed=pk, x_ssq=ssq, eps=EPS, workspace=ws)

    def finish(case, got, ref, ref32):
        err, b = _judge(case, got, ref, ref32)
        assert err <= b, f"{case}: err {err:.3e} over bar {b:.3e}"
        assert torch.equal(pk, pk0) and torch.equal(ssq, ssq0), f"{case}: the hand-over changed"
        assert bool((ws[M:] == SENT).all()), f"{case}: the workspace was written past the row scales"

    # STORE (bias) and SWIGLU
    for tag, epi, N, extra in (("store bias", lr.EPI_STORE, N_STORE, dict(bias=lp._vec("bias", N_STORE))),
                               ("swiglu", lr.EPI_SWIGLU, N_GLU, dict(W1=_weight(N_GLU, C, 1)))):
        W = _weight(N, C, 0)
        ref = lr.scaled_linear_ref(op, ssq_h, W, eps=EPS, epi=epi, dt=F64, **extra)
        ref32 = lr.scaled_linear_ref(op, ssq_h, W, eps=EPS, epi=epi, dt=F32, **extra)
        yd = torch.full((M, N + PAD), SENT, device=dev)
        _launch(N=N, w0=_packed(N, C, 0), w1=_packed(N, C, 1) if epi == lr.EPI_SWIGLU else None, epilogue=epi, y=yd,
                bias=_cu(extra.get("bias")), **base)
        case = f"consumer {tag} {form} N={N} K={C} M={M}"
        assert bool((yd[:, N:] == SENT).all()), f"{case}: pad columns of y written"
        finish(case, yd[:, :N], ref, ref32)
    # q|k|v, half-split rotation
    for nh, nkv, hs in ((2, 1, 128), (3, 1, 64)):
        N = (nh + 2 * nkv) * hs
        pos, seq, table, n_pages, cos, sin = _qkv_geometry(hs, 7 * hs + C)
        W = _weight(N, C, 0)
        qkv = dict(pos=pos, n_head=nh, n_kv=nkv, hs=hs, rope_mode=lr.ROPE_HALF_SPLIT, cos=cos, sin=sin)
        ref = lr.scaled_linear_ref(op, ssq_h, W, eps=EPS, epi=lr.EPI_QKV_ROPE, qkv=qkv, dt=F64)
        ref32 = lr.scaled_linear_ref(op, ssq_h, W, eps=EPS, epi=lr.EPI_QKV_ROPE, qkv=qkv, dt=F32)
        kp = torch.full((n_pages, nkv, kr.PAGE, hs), SENT, dtype=BF16, device=dev)
        vp = torch.full_like(kp, SENT)
        q = torch.full((M, nh * hs), SENT, device=dev)
        td = table.cuda()                                           # kv_geom keeps the pointer only: the tensor must outlive the launch
        _launch(N=N, w0=_packed(N, C, 0, hs), epilogue=lr.EPI_QKV_ROPE, row_pos=pos.cuda(), row_seq=seq.cuda(), rope_cos=cos.cuda(), rope_sin=sin.cuda(),
                q_out=q, rope_mode=lr.ROPE_HALF_SPLIT, kv=ops.kv_geom(kp, vp, td, nh, nkv, hs), **base)
        assert torch.equal(td.cpu(), table)
        case = f"consumer qkv half_split {form} {nh}/{nkv}/{hs} K={C} M={M}"
        _check_qkv(case, q, kp, vp, ref, ref32, pos, seq, table, n_pages, nkv, hs)
        assert torch.equal(pk, pk0) and torch.equal(ssq, ssq0), f"{case}: the hand-over changed"


# ---- LayerNorm hand-over (y_ln_w) -----------------------------------------------------------------------------------------------

LN_PATHS = [("split", K) for K in LN_SPLIT_KS] + [("row_pass", LN_SPLIT_KS[0])]
assert {p for p, _ in LN_PATHS} == {"split", "row_pass"}


@pytest.mark.parametrize("N", LN_NS)
@pytest.mark.parametrize("path,K", LN_PATHS, ids=[f"{p}-K{k}" for p, k in LN_PATHS])
def test_layernorm_handover(path, K, N, g2env):
    """y_ln_w on a RESIDUAL launch, both ways gemm2_combine_ln_row_kernel runs — with the K-slab combine (split_ws given; the split
    starts at 36 chunks) and as the row pass alone (no scratch) — at N = 64 (one partly idle wave), 320 (a ragged last wave), 1536
    (the DiT) and 2048 (the launcher's maximum).  Rows 0 .. 3 are hostile: unit scale, mean 1e3 with std 1, the constant 2.5, scale
    1e-3; their x is zero and there is no GEMM bias, so y equals resid exactly.  Reference: float64 LayerNorm of the kernel's OWN fp32
    y; per element |got - ref| <= half_ulp_bf16(ref) + kr.bar(E_ref) scale, E_ref from the fp32 replay of the two-pass centred form.

    Measured on an MI355X while the kernel still formed mean(y^2) - mean^2: the mean-1e3 row off by 1.3e-2 / 5.7e-3 / 2.2e-3 /
    6.8e-3 of its scale beyond half a bf16 ulp at N = 64 / 320 / 1536 / 2048 (the launch's excess 8.8e-3 / 3.3e-3 / 1.5e-3 /
    4.9e-3 against bars of 5.3e-5 / 1.0e-4 / 9.4e-5 / 2.4e-5), on both paths; with the second pass every row is inside half an
    ulp + 4e-8 (profiles/kernel_parity_errors.txt)."""
    from uniaudio2_amd import ops
    dev = torch.device("cuda")
    M = 257
    g = torch.Generator().manual_seed(31 * N + K)
    x = lp._rows("x", M, K).clone()
    x[:4] = 0.0
    resid = lp._rows("resid", M, N).clone()
    resid[:4] = lr.hostile_rows(N, N)
    osc, W = lp._vec("out_scale", N), _weight(N, K, 0)
    lw, lb = 1.0 + 0.2 * torch.randn(N, generator=g), 0.2 * torch.randn(N, generator=g)
    kw = dict(epi=lr.EPI_RESIDUAL, out_scale=osc, resid=resid)
    ref, ref32 = lr.linear_ref(x, W, BF16, dt=F64, **kw), lr.linear_ref(x, W, BF16, dt=F32, **kw)
    for form in ("bmt8_nb6", "bmt16_nb4") if N == 1536 else ("bmt8_nb6",):
        g2env(**FORMS[form][0])
        xd, rd, yd = lp._strided(x, PAD), lp._strided(resid, PAD), torch.full((M, N + PAD), SENT, device=dev)
        pk = torch.full(((M + 15) // 16 * 16 * N,), SENT, dtype=BF16, device=dev)
        sw = torch.full((4 * M * N,), float("nan"), device=dev) if path == "split" else None
        _launch(M=M, N=N, K=K, w0=_packed(N, K, 0), prologue=lr.PRO_CAST, epilogue=lr.EPI_RESIDUAL, x=xd, y=yd, resid=rd, out_scale=osc.cuda(),
                y_ln=(lw.cuda(), lb.cuda(), LN_EPS), y_packed=pk, split_ws=sw, workspace=ops.linear_workspace(BF16, M, K, dev))
        case = f"y_ln {path} {form} N={N} K={K} M={M}"
        if path == "split":
            assert bool((~torch.isnan(sw)).any()), f"{case}: the K slabs did not run"
        y = yd.cpu()
        assert lp._same_bits(y[:, N:], torch.full((M, PAD), SENT)), f"{case}: pad columns of y written"
        assert lp._same_bits(rd.cpu(), lp._strided(resid, PAD, "cpu")) and lp._same_bits(xd.cpu(), lp._strided(x, PAD, "cpu")), f"{case}: an input changed"
        assert lp._same_bits(y[:4, :N], resid[:4]), f"{case}: the hostile rows are not resid exactly"
        err, b = _judge(case, y[4:, :N], ref[4:], ref32[4:])        # the other rows on their own: the 1e3 row must not set their scale
        assert err <= b, f"{case}: err {err:.3e} over bar {b:.3e}"
        got = _decode_packed_bf16(pk.cpu(), M, N)
        assert bool(torch.isfinite(got.float()).all()), f"{case}: non-finite hand-over"
        tail = _packed_rows_past_m(pk, M, N)
        assert lp._same_bits(tail, torch.full_like(tail, SENT)), f"{case}: y_packed rows past M written"
        worst, e_ref, bar = lr.ln_handover_excess(got, y[:, :N], lw, lb, LN_EPS)
        rowwise = [lr.ln_handover_excess(got[r:r + 1], y[r:r + 1, :N], lw, lb, LN_EPS)[0] for r in range(4)]
        print(f"PARITY gemm2 {case} hand-over: excess {worst:.3e} E_ref {e_ref:.3e} bar {bar:.3e} "
              f"(hostile rows, of their own scale: {' '.join(f'{v:.3e}' for v in rowwise)})")
        assert worst <= bar, f"{case}: hand-over {worst:.3e} over bar {bar:.3e} beyond half a bf16 ulp"
        assert lp._same_bits(got[2], lb.to(BF16)), f"{case}: the constant row is not RNE_bf16(b)"
