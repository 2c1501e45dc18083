"""ua2_linear's decode kernel (csrc/ua2_gemv.hip, forced with ua2_debug_force_general_linear(2)) and ua2_pack_linear against
float64 restatements of include/ua2hip.h (tests/linear_refs.py) — the anchor the bit-identity chains of test_gpu_invariance.py,
test_gpu_gemm2.py and test_gpu_w8*.py hang from.

Tolerance: the project's rule, bar = kr.bar(E_ref, scale) = max(4 E_ref, 8 * 2^-24 scale), scale = max(1, max |ref|) of the
launch, E_ref = error of the fp32 replay of the same formula (one pessimistic legal summation order) on the very inputs of the
launch.  Every launch prints `PARITY linear <case>: err ... E_ref ... bar ...`.

bf16 x UA2_PRO_NORM cases take their rows from lr.norm_inputs(): inputs on which the fp32 and the float64 evaluation of the
operand round to the same bf16 numbers (no element within a band of a rounding midpoint; asserted again before a launch), so
that the comparison is about the sums and not about one operand rounded to another neighbour.  The hostile rows (an offset
of 1e3, a constant row) run with UA2_F32 only, where no operand is rounded.

Every output buffer is pre-filled with a finite sentinel; row strides are wider than the rows (except in the M = 2 launches);
pad columns and cache slots no row writes must still hold the sentinel's bits afterwards.  Index-carrying inputs are asserted in
range on the host before a launch; nothing non-finite is sent to a kernel."""
import functools

import numpy as np
import pytest
import torch

import kernel_refs as kr
import linear_refs as lr

pytestmark = pytest.mark.gpu

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
SENT = 12345.0
EPS = 1e-5
DTYPES = [BF16, F32]


@pytest.fixture
def linear_mode():
    """Mode 2 (row-tiled decode kernel only) for the test; the returned setter picks another; mode 0 is restored afterwards."""
    from uniaudio2_amd._lib import lib
    lib.ua2_debug_force_general_linear(2)
    yield lib.ua2_debug_force_general_linear
    lib.ua2_debug_force_general_linear(0)


def _dn(dtype):
    return "bf16" if dtype == BF16 else "fp32"


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _row_counts(dtype, K):
    """M in {1, 2, rt, rt + 1}: the in-register single-row path, a second row, a full row tile, a second row block of one row."""
    rt = lr.rows_per_tile(dtype, K)
    return sorted({1, 2, rt, rt + 1})


def test_row_tile_sizes():
    assert lr.rows_per_tile(BF16, 8192) == 6 and lr.rows_per_tile(F32, 8192) == 3 and lr.rows_per_tile(BF16, 3072) == 16


# ---- shared inputs: drawn once per process ------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=6)
def _weight(N, K, which):
    """Source weight [N, K] fp32 on the host: randn K^-0.5."""
    g = torch.Generator().manual_seed(7919 * N + K + 104729 * which)
    return torch.randn(N, K, generator=g) * K ** -0.5


@functools.lru_cache(maxsize=6)
def _packed(dtype, N, K, which, rope_hs=0):
    from uniaudio2_amd import ops
    return ops.pack_linear(_weight(N, K, which).cuda(), dtype, rope_head_size=rope_hs)


@functools.lru_cache(maxsize=None)
def _vec(kind, n):
    g = torch.Generator().manual_seed({"bias": 1, "bias1": 2, "out_scale": 3}[kind] * 1000003 + n)
    if kind == "out_scale":
        return 0.5 + torch.rand(n, generator=g)
    return 0.1 * torch.randn(n, generator=g)


@functools.lru_cache(maxsize=None)
def _rows(kind, M, n):
    g = torch.Generator().manual_seed({"x": 11, "resid": 12}[kind] * 1000003 + 131 * M + n)
    return torch.randn(M, n, generator=g)


def _inputs(dtype, K, M, pro, norm_kind):
    """(x [M, K], norm_w, norm_b).  NORM: the flip-free rows (both dtypes take the same ones); the condition is asserted again."""
    if pro == lr.PRO_CAST:
        return _rows("x", max(M, 17), K)[:M], None, None
    x, w, b, rec = lr.norm_inputs(K, norm_kind, EPS)
    assert M <= x.shape[0]
    x = x[:M]
    if dtype == BF16:
        assert int(lr.flip_candidates(x, pro, norm_kind, w, b, EPS, rec["delta"]).sum()) == 0, "flip candidates in a NORM input"
    return x, w, b


def _strided(t, pad, dev="cuda"):
    """t [M, n] -> device buffer [M, n + pad], pad columns = sentinel."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), SENT, dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    return buf.to(dev)


def _judge(case, got, ref, ref32):
    """err, E_ref, bar of one launch (absolute, scale max(1, max |ref|)); prints the PARITY line."""
    got = got.detach().cpu().to(F64)
    assert bool(torch.isfinite(got).all()), f"{case}: non-finite output"
    scale = max(1.0, float(ref.abs().max()))
    err = float((got - ref).abs().max()) / scale
    e_ref = float((ref32.to(F64) - ref).abs().max()) / scale
    b = kr.bar(e_ref)                                               # relative to scale: kr.bar(E_ref, scale) / scale
    print(f"PARITY linear {case}: err {err:.3e} E_ref {e_ref:.3e} bar {b:.3e}")
    return err, b


# ---- STORE / RESIDUAL / SWIGLU / GELU -----------------------------------------------------------------------------------------

def _run_dense(tag, dtype, N, K, *, pro, epi, norm_kind=0, bias=False, bias1=False, out_scale=False, act_kind=0, packed=False,
               Ms=None, x_rows=None, workspace=False):
    """One (prologue, epilogue) configuration at every row count of `Ms`: reference once for the most rows (a row's value does not
    depend on the rows around it), one launch per M.  Returns the worst err / bar."""
    from uniaudio2_amd import ops
    Ms = Ms or _row_counts(dtype, K)
    Mmax = max(Ms)
    if x_rows is None:
        x, nw, nb = _inputs(dtype, K, Mmax, pro, norm_kind)
    else:
        x, nw, nb = x_rows
    W, W1 = _weight(N, K, 0), (_weight(N, K, 1) if epi == lr.EPI_SWIGLU else None)
    b0 = _vec("bias", N) if bias else None
    b1 = _vec("bias1", N) if bias1 else None
    osc = _vec("out_scale", N) if out_scale else None
    resid = _rows("resid", Mmax, N) if epi == lr.EPI_RESIDUAL else None
    kw = dict(pro=pro, epi=epi, norm_kind=norm_kind, norm_w=nw, norm_b=nb, eps=EPS, W1=W1, bias=b0, bias1=b1, resid=resid,
              out_scale=osc, act_kind=act_kind)
    ref = lr.linear_ref(x, W, dtype, dt=F64, **kw)
    ref32 = lr.linear_ref(x, W, dtype, dt=F32, **kw)
    dev = torch.device("cuda")
    p0 = _packed(dtype, N, K, 0)
    p1 = _packed(dtype, N, K, 1) if W1 is not None else None
    cu = lambda t: None if t is None else t.cuda()
    nw_d, nb_d, b0_d, b1_d, osc_d = cu(nw), cu(nb), cu(b0), cu(b1), cu(osc)
    npart = (N + 15) // 16
    forbid = (torch.arange(Mmax, dtype=torch.int32) * 5) % 23       # columns < forbid[m] are excluded from the partial arg-max
    worst = 0.0
    for M in Ms:
        pad = 0 if M == 2 else 4
        xd, yd = _strided(x[:M], pad), torch.full((M, N + pad), SENT, device=dev)
        args = dict(dtype=dtype, M=M, N=N, K=K, w0=p0, w1=p1, prologue=pro, epilogue=epi, x=xd, y=yd, norm_w=nw_d, norm_b=nb_d,
                    norm_kind=norm_kind, eps=EPS, bias=b0_d, bias1=b1_d, out_scale=osc_d, act_kind=act_kind)
        if epi == lr.EPI_RESIDUAL:
            rd = _strided(resid[:M], pad)
            args.update(resid=rd)
        if epi == lr.EPI_STORE:
            pm = torch.full((M, npart), SENT, device=dev)
            pi = torch.full((M, npart), -7, dtype=torch.int32, device=dev)
            args.update(part_max=pm, part_idx=pi, forbid=forbid[:M].cuda())
        if packed:
            pk = torch.full(((M + 15) // 16 * 16 * N,), SENT, dtype=dtype, device=dev)
            args.update(y_packed=pk)
        if workspace:
            args.update(workspace=ops.linear_workspace(dtype, M, K, dev))
        ops.linear(**args)
        torch.cuda.synchronize()
        y = yd.cpu()
        case = f"{tag} {_dn(dtype)} N={N} K={K} M={M}"
        assert _same_bits(y[:, N:], torch.full((M, pad), SENT)), f"{case}: pad columns of y written"
        if epi == lr.EPI_RESIDUAL:
            assert _same_bits(rd.cpu(), _strided(resid[:M], pad, "cpu")), f"{case}: resid changed"
        assert _same_bits(xd.cpu(), _strided(x[:M], pad, "cpu")), f"{case}: x changed"
        err, b = _judge(case, y[:, :N], ref[:M], ref32[:M])
        assert err <= b, f"{case}: err {err:.3e} over bar {b:.3e}"
        worst = max(worst, err / b)
        if epi == lr.EPI_STORE:                                     # the partials of the kernel's OWN row, exactly
            pmc, pic = pm.cpu().numpy(), pi.cpu().numpy()
            for m in range(M):
                wm, wi = kr.argmax_partials(y[m, :N].numpy(), int(forbid[m]))
                np.testing.assert_array_equal(pmc[m], wm, err_msg=f"{case}: part_max row {m}")
                np.testing.assert_array_equal(pic[m], wi, err_msg=f"{case}: part_idx row {m}")
        if packed:                                                  # RNE to the operand dtype of the kernel's own fp32 y, bit for bit
            got = lr.unpack_operand(pk, dtype, M, N)
            assert _same_bits(got, y[:, :N].to(dtype)), f"{case}: y_packed"
            rest = pk.cpu().view((M + 15) // 16, N // lr.kc(dtype), lr.kc(dtype) // lr.epl(dtype), 16, lr.epl(dtype))
            if M % 16:
                tail = rest[-1, :, :, M % 16:, :]
                assert _same_bits(tail, torch.full_like(tail, SENT)), f"{case}: y_packed rows past M written"
    return worst


PROLOGUES = [("cast", lr.PRO_CAST, 0), ("rms_lit", lr.PRO_NORM, lr.NORM_RMS_LIT), ("rms_moshi", lr.PRO_NORM, lr.NORM_RMS_MOSHI),
             ("layernorm", lr.PRO_NORM, lr.NORM_LAYERNORM)]
FULL = [(200, 72), (200, 2048), (200, 8192)]              # every prologue x epilogue combination runs at these
# (N, K) -> what the geometry choice (pick_geometry / launch_cpw of csrc/ua2_gemv.hip) does there
BRANCH = {
    (200, 72): "fewer chunks than waves, clamped loads, ragged last column tile, K not a multiple of the chunk",
    (48, 1056): "33 / 66 chunks: no exact tiling",
    (200, 2048): "exact single-burst tiling 16 x 4 (bf16)",
    (200, 3072): "exact single-burst tiling 12 x 8 (bf16) / 12 x 16 (fp32)",
    (64, 6144): "exact single-burst tiling 12 x 16 (bf16)",
    (200, 8192): "16 waves x 16 chunks (bf16); 512 chunks, multi-round fall-back (fp32)",
    (4104, 2048): "more than 256 column tiles: 8 waves, double-buffered rounds; ends in a half tile",
    (4112, 8192): "more than 256 column tiles, K = 8192: M = 1 does not take the in-register path",
}
SHAPES = [(dt, N, K) for dt in DTYPES for (N, K) in BRANCH if dt == BF16 or N < 4000]


def _subset(N, K):
    """Prologue / bias pairs at a shape: all eight at the FULL shapes, two (rotating) elsewhere."""
    allp = [(p, b) for p in PROLOGUES for b in (False, True)]
    if (N, K) in FULL:
        return allp
    i = (N + K // 8) % 4
    return [allp[2 * i + 1], allp[(2 * i + 4) % 8]]


@pytest.mark.parametrize("dtype,N,K", SHAPES, ids=lambda v: _dn(v) if isinstance(v, torch.dtype) else str(v))
def test_store_and_argmax_partials(dtype, N, K, linear_mode):
    """CAST and NORM (three flavours) into STORE, with and without bias, at the geometry branch BRANCH[(N, K)]; part_max / part_idx
    with a forbid vector equal kr.argmax_partials of the kernel's own row."""
    for (name, pro, nk), bias in _subset(N, K):
        _run_dense(f"store {name} bias={int(bias)}", dtype, N, K, pro=pro, epi=lr.EPI_STORE, norm_kind=nk, bias=bias)


@pytest.mark.parametrize("dtype,N,K", [s for s in SHAPES if (s[1], s[2]) in FULL + [(48, 1056), (64, 6144), (4104, 2048)]],
                         ids=lambda v: _dn(v) if isinstance(v, torch.dtype) else str(v))
def test_residual(dtype, N, K, linear_mode):
    """resid + out_scale (x W^T + bias), with and without out_scale and bias.  CAST only: the decode kernel builds the RESIDUAL
    epilogue for the CAST (and LOCAL_ATTN) prologue, as the models use it (o-projection, down-projection)."""
    for osc, bias in ((False, False), (True, True), (True, False), (False, True)):
        _run_dense(f"residual cast out_scale={int(osc)} bias={int(bias)}", dtype, N, K, pro=lr.PRO_CAST, epi=lr.EPI_RESIDUAL, bias=bias,
                   out_scale=osc)


SWIGLU_SHAPES = [s for s in SHAPES if (s[1], s[2]) in FULL + [(4104, 2048)]] + [(BF16, 200, 4104), (BF16, 192, 2048), (F32, 192, 2048)]


@pytest.mark.parametrize("dtype,N,K", SWIGLU_SHAPES, ids=lambda v: _dn(v) if isinstance(v, torch.dtype) else str(v))
def test_swiglu(dtype, N, K, linear_mode):
    """silu(s0 + b0) (s1 + b1) and the UA2_GATE_SIGMOID_SECOND form (s0 + b0) sigmoid(s1 + b1).  (200, 4104) bf16: 129 chunks at
    cap 8, the single-burst geometry that does not tile K exactly (the reload branch of the chunk loop).  N = 192: y_packed, the
    result rounded to the operand dtype in fragment order, must be the RNE cast of the kernel's own fp32 y."""
    packed = N == 192
    pros = PROLOGUES if (N, K) in FULL else [PROLOGUES[0], PROLOGUES[1]]
    for name, pro, nk in pros:
        _run_dense(f"swiglu {name}", dtype, N, K, pro=pro, epi=lr.EPI_SWIGLU, norm_kind=nk, packed=packed)
        _run_dense(f"swiglu sigmoid_second {name} bias", dtype, N, K, pro=pro, epi=lr.EPI_SWIGLU, norm_kind=nk, bias=True, bias1=True,
                   act_kind=lr.GATE_SIGMOID_SECOND, packed=packed)


@pytest.mark.parametrize("dtype,N,K", [s for s in SHAPES if (s[1], s[2]) in FULL] + [(BF16, 192, 2048), (F32, 192, 2048)],
                         ids=lambda v: _dn(v) if isinstance(v, torch.dtype) else str(v))
def test_gelu(dtype, N, K, linear_mode):
    """gelu(x W^T + b), erf and tanh forms; N = 192 with y_packed."""
    for name, pro, nk in PROLOGUES:
        for act in (lr.ACT_DEFAULT, lr.GELU_TANH):
            _run_dense(f"gelu {'tanh' if act else 'erf'} {name}", dtype, N, K, pro=pro, epi=lr.EPI_GELU, norm_kind=nk, bias=True,
                       act_kind=act, packed=N == 192)


# ---- hostile rows (UA2_F32: no operand rounding) ------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [72, 1536, 3072])
@pytest.mark.parametrize("name,norm_kind", [(p[0], p[2]) for p in PROLOGUES[1:]])
def test_hostile_rows_fp32(K, name, norm_kind, linear_mode):
    """The rows of test_layernorm_rows through the NORM prologue: unit scale, mean 1e3 with std 1, a constant row 2.5, scale 1e-3.
    The RMS flavours have no cancellation; LayerNorm must form its variance so that the offset row survives, and the constant
    row (variance 0) must give b W^T (+ bias), finite.
    Measured on an MI355X while the prologue still formed mean(x^2) - mean^2: LayerNorm err 7.9e-4 / 4.0e-3 / 1.0e-1 at
    K = 72 / 1536 / 3072 against bars of 1.6e-5 / 2.4e-4 / 3.2e-5; with the centred variance alone the K = 3072 row stayed at
    1.2e-4 (the fp32 sum of 3072 values near 1e3 leaves ~1e-4 in the mean, which shifts every x - mean); with the mean carried in
    two parts (norm_stat_centred) 1.2e-7 / 2.4e-7 / 3.6e-7."""
    N, M = 200, 4
    g = torch.Generator().manual_seed(K)
    x = torch.randn(M, K, generator=g)
    x[1] += 1e3
    x[2] = 2.5
    x[3] *= 1e-3
    nw = 1.0 + 0.1 * torch.randn(K, generator=g)
    nb = 0.1 * torch.randn(K, generator=g) if norm_kind == lr.NORM_LAYERNORM else None
    for bias in (False, True):
        _run_dense(f"hostile {name} bias={int(bias)}", F32, N, K, pro=lr.PRO_NORM, epi=lr.EPI_STORE, norm_kind=norm_kind, bias=bias,
                   Ms=[M], x_rows=(x, nw, nb))
    if norm_kind == lr.NORM_LAYERNORM:
        a = lr.operand_ref(x, lr.PRO_NORM, norm_kind, nw, nb, EPS, F32)
        assert torch.equal(a[2], nb.to(F64))                       # what the last launch was compared with on that row: b W^T + bias


# ---- the launcher's own choice ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("N,K", [(200, 2048), (4104, 2048)])
def test_launchers_own_choice_many_rows(dtype, N, K, linear_mode):
    """Mode 0 with a workspace at 40 and 300 rows (the many-row kernels): the same reference and bar, so that the anchor of those
    kernels does not rest on the identity chain alone."""
    linear_mode(0)
    _run_dense("mode0 swiglu rms_lit", dtype, N, K, pro=lr.PRO_NORM, epi=lr.EPI_SWIGLU, norm_kind=lr.NORM_RMS_LIT, Ms=[40, 300], workspace=True)
    x = _rows("x", 300, K)
    _run_dense("mode0 residual cast", dtype, N, K, pro=lr.PRO_CAST, epi=lr.EPI_RESIDUAL, Ms=[40, 300], workspace=True, x_rows=(x, None, None))


# ---- QKV + RoPE + paged cache append ------------------------------------------------------------------------------------------

POSITIONS = [63, 64, 65, 130]                                      # straddling a page edge
QKV_GEOMS = [(4, 2, 32, 72), (6, 2, 64, 144), (24, 8, 128, 3072)]   # n_head, n_kv, hs, K


def _run_qkv(tag, dtype, nh, nkv, hs, K, *, rope_mode, pro, norm_kind, bias, perm, ring_pages):
    from uniaudio2_amd import ops
    dev = torch.device("cuda")
    N, M = (nh + 2 * nkv) * hs, len(POSITIONS)
    rope_hs = hs if rope_mode == lr.ROPE_HALF_SPLIT else 0
    x, nw, nb = _inputs(dtype, K, M, pro, norm_kind)
    W = _weight(N, K, 0)
    b0 = _vec("bias", N) if bias else None
    g = torch.Generator().manual_seed(hs + K)
    max_pos = 160
    ang = torch.rand(max_pos, hs // 2, generator=g) * 6.28
    cos, sin = ang.cos(), ang.sin()
    pos = torch.tensor(POSITIONS, dtype=torch.int32)
    B = M
    seq = torch.tensor([2, 0, 3, 1], dtype=torch.int32) if perm else None
    max_pages = ring_pages if ring_pages else (max(POSITIONS) // kr.PAGE + 1)
    n_pages = B * max_pages + 3
    table = torch.randperm(n_pages, generator=g)[:B * max_pages].to(torch.int32).view(B, max_pages)     # scattered, every page distinct
    # host-side range checks of everything a kernel will index with
    assert int(table.min()) >= 0 and int(table.max()) < n_pages and len(set(table.flatten().tolist())) == B * max_pages
    assert int(pos.min()) >= 0 and int(pos.max()) < max_pos
    assert seq is None or sorted(seq.tolist()) == list(range(B))
    slots = [kr.page_slot(int(p), ring_pages) for p in POSITIONS]
    assert all(0 <= s < max_pages for s in slots)
    qkv = dict(pos=pos, n_head=nh, n_kv=nkv, hs=hs, rope_mode=rope_mode, cos=cos, sin=sin)
    kw = dict(pro=pro, epi=lr.EPI_QKV_ROPE, norm_kind=norm_kind, norm_w=nw, norm_b=nb, eps=EPS, bias=b0, qkv=qkv)
    ref = lr.linear_ref(x, W, dtype, dt=F64, **kw)
    ref32 = lr.linear_ref(x, W, dtype, dt=F32, **kw)
    p0 = _packed(dtype, N, K, 0, rope_hs)
    cu = lambda t: None if t is None else t.cuda()
    worst = 0.0
    for M_run in (1, M):
        xd = _strided(x[:M_run], 4)
        kp = torch.full((n_pages, nkv, kr.PAGE, hs), SENT, dtype=dtype, device=dev)
        vp = torch.full_like(kp, SENT)
        q = torch.full((M_run, nh * hs), SENT, device=dev)
        seq_run = None if seq is None else seq[:M_run].contiguous()
        table_d = table.cuda()                                      # kv_geom keeps the pointer only: the tensor must outlive the launch
        ops.linear(dtype=dtype, M=M_run, N=N, K=K, w0=p0, prologue=pro, epilogue=lr.EPI_QKV_ROPE, x=xd, norm_w=cu(nw), norm_b=cu(nb),
                   norm_kind=norm_kind, eps=EPS, bias=cu(b0), row_pos=pos[:M_run].cuda(), row_seq=cu(seq_run),
                   rope_cos=cos.cuda(), rope_sin=sin.cuda(), q_out=q, rope_mode=rope_mode,
                   kv=ops.kv_geom(kp, vp, table_d, nh, nkv, hs, ring_pages=ring_pages))
        torch.cuda.synchronize()
        case = f"{tag} {_dn(dtype)} {nh}/{nkv}/{hs} K={K} M={M_run}"
        qc, kc_, vc = q.cpu().to(F64).view(M_run, nh, hs), kp.cpu(), vp.cpu()
        assert bool(torch.isfinite(qc).all()) and bool(torch.isfinite(kc_.float()).all()) and bool(torch.isfinite(vc.float()).all())
        rq, rk, rv = (t[:M_run] for t in ref)
        scale = max(1.0, float(max(rq.abs().max(), rk.abs().max(), rv.abs().max())))
        e_ref = max(float((a[:M_run].to(F64) - b).abs().max()) for a, b in zip(ref32, (rq, rk, rv))) / scale
        b = kr.bar(e_ref)
        written = torch.zeros(n_pages, kr.PAGE, dtype=torch.bool)
        err_q = float((qc - rq).abs().max()) / scale
        err_kv = 0.0
        for m in range(M_run):
            s = m if seq is None else int(seq[m])
            page, off = int(table[s, slots[m]]), POSITIONS[m] % kr.PAGE
            assert not bool(written[page, off])
            written[page, off] = True
            for pool, r in ((kc_, rk[m]), (vc, rv[m])):
                d = (pool[page, :, off].to(F64) - r).abs()
                if dtype == BF16:                                   # the kernel rounds its own fp32 result once: half a bf16 ulp of the value on top
                    d = (d - lr.half_ulp_bf16(r)).clamp_min(0.0)
                err_kv = max(err_kv, float(d.max()) / scale)
        print(f"PARITY linear {case}: err {max(err_q, err_kv):.3e} (q {err_q:.3e} kv {err_kv:.3e}) E_ref {e_ref:.3e} bar {b:.3e}")
        assert err_q <= b and err_kv <= b, f"{case}: q {err_q:.3e} kv {err_kv:.3e} over bar {b:.3e}"
        worst = max(worst, err_q / b, err_kv / b)
        untouched = ~written[:, None, :, None].expand(n_pages, nkv, kr.PAGE, hs)
        sent = torch.tensor(SENT).to(dtype)
        for pool, nm in ((kc_, "k"), (vc, "v")):
            assert bool((_bits(pool)[untouched] == _bits(sent)).all()), f"{case}: a {nm} slot no row owns was written"
    return worst


QKV_CASES = [  # tag, rope_mode, prologue, norm_kind, bias
    ("half_split rms_lit", lr.ROPE_HALF_SPLIT, lr.PRO_NORM, lr.NORM_RMS_LIT, False),
    ("interleaved rms_moshi", lr.ROPE_INTERLEAVED, lr.PRO_NORM, lr.NORM_RMS_MOSHI, False),
    ("interleaved cast bias", lr.ROPE_INTERLEAVED, lr.PRO_CAST, 0, True),
    ("none layernorm", lr.ROPE_NONE, lr.PRO_NORM, lr.NORM_LAYERNORM, False),
    ("none cast bias", lr.ROPE_NONE, lr.PRO_CAST, 0, True),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("nh,nkv,hs,K", QKV_GEOMS)
def test_qkv_rope_cache_append(dtype, nh, nkv, hs, K, linear_mode):
    """q | k | v split, rotation of q and k (half-split on a weight packed with rope_head_size; interleaved and none on a plain
    pack, also with bias), k / v appended to a scattered paged cache at positions straddling a page edge; row_seq None and a
    permutation; one ring cache of two pages.  The reference works in source row order of W.  (24, 8, 128) at K = 3072 has 320
    column tiles: the 8-wave double-buffered geometry."""
    for i, (tag, mode, pro, nk, bias) in enumerate(QKV_CASES):
        _run_qkv(f"qkv {tag} seq=none", dtype, nh, nkv, hs, K, rope_mode=mode, pro=pro, norm_kind=nk, bias=bias, perm=False, ring_pages=0)
        _run_qkv(f"qkv {tag} seq=perm", dtype, nh, nkv, hs, K, rope_mode=mode, pro=pro, norm_kind=nk, bias=bias, perm=True, ring_pages=0)
    _run_qkv("qkv half_split rms_lit ring=2", dtype, nh, nkv, hs, K, rope_mode=lr.ROPE_HALF_SPLIT, pro=lr.PRO_NORM,
             norm_kind=lr.NORM_RMS_LIT, bias=False, perm=True, ring_pages=2)


# ---- the packer ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,K,transposed,rope_hs", [(20, 40, False, 0), (110, 128, True, 0), (384, 256, False, 32), (384, 256, False, 64),
                                                    (512, 192, False, 128)])
@pytest.mark.parametrize("src_dtype", DTYPES, ids=_dn)
@pytest.mark.parametrize("dst_dtype", DTYPES, ids=_dn)
def test_pack_linear_layout(N, K, transposed, rope_hs, src_dtype, dst_dtype):
    """unpack_linear(pack_linear(W)) is W rounded to the destination dtype, bit for bit, in source row order; padding rows and
    columns are exactly zero."""
    from uniaudio2_amd import ops
    g = torch.Generator().manual_seed(N * 31 + K)
    W = torch.randn(N, K, generator=g).to(src_dtype)
    src = (W.t().contiguous() if transposed else W).cuda()
    pk = ops.pack_linear(src, dst_dtype, transposed=transposed, rope_head_size=rope_hs)
    torch.cuda.synchronize()
    got = lr.unpack_linear(pk, dst_dtype, N, K, rope_hs)
    assert got.dtype == dst_dtype and got.shape == ((N + 15) // 16 * 16, (K + lr.kc(dst_dtype) - 1) // lr.kc(dst_dtype) * lr.kc(dst_dtype))
    assert _same_bits(got[:N, :K], W.float().to(dst_dtype)), "packed values"
    assert int(_bits(got[N:]).abs().sum()) == 0 and int(_bits(got[:, K:]).abs().sum()) == 0, "padding is not all-zero bits"


@pytest.mark.parametrize("N,K", [(200, 72), (48, 1056)])
def test_one_hot_rows_return_the_weight(N, K, linear_mode):
    """A data-path check that does not depend on the layout decoder: UA2_F32, x = the K one-hot rows (row blocks of rt rows each),
    CAST -> STORE returns W^T exactly."""
    from uniaudio2_amd import ops
    W = _weight(N, K, 0)
    y = torch.full((K, N), SENT, device="cuda")
    ops.linear(dtype=F32, M=K, N=N, K=K, w0=_packed(F32, N, K, 0), prologue=lr.PRO_CAST, epilogue=lr.EPI_STORE, x=torch.eye(K, device="cuda"), y=y)
    torch.cuda.synchronize()
    assert _same_bits(y.cpu(), W.t().contiguous())
