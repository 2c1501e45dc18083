"""The argument plumbing of the hot decode kernels (csrc/ua2_gemv.hip gemv_hot_kernel, csrc/ua2_attn.hip attn_fused_hot_kernel): what a
launch reads in front of its weight burst travels as 14 dwords of leading kernel parameters — pointers, 32-bit offsets from the first
weight pointer, 16-bit packed ints — instead of inside ua2_linear_args / ua2_attn_args.  Nothing a row computes changes, so every case
here is an identity or the project's float64 bar, at the smallest shapes where the packing can go wrong:

  * M = 1, 2, 5; K = 128 and 256 (13-bit images), K = 64 (fp8 twins), bf16 weights at all three; N = 16, 56 (a half last tile) and 48;
    K = 8192 once (the largest value the packed K field sees in the model);
  * every row stride (ldx, ldy, ldr, ldh) wider than the row, every pointer a view that starts inside its allocation at a non-zero
    16-byte-aligned offset, weights, images and side arrays in one allocation (an offset-from-base mistake then reads the wrong bytes);
  * every (prologue, epilogue) pair of the B = 1 frame: NORM and SCALED with QKV_ROPE / SWIGLU / STORE + arg-max partials, CAST and its
    bf16-row form (x_h) with RESIDUAL / STORE, LOCAL_ATTN with and without the arg-max fold (hot on bf16 weights; on an image the
    launcher keeps the by-value kernel for this prologue, which the test pins down too).

References.  (0) The by-value kernels on the same launch (UA2_GEMV_NO_HOT / UA2_ATTN_NO_HOT): torch.equal, every form; the launch
counters "gemv_hot" / "attn_hot" say which form served a launch.  (1) The many-row kernels, which this plumbing does not touch, on the
forms they serve (fp32 operands: NORM, CAST): the same row must be torch.equal — the row-invariance contract.  (2) float64
(tests/linear_refs.py, tests/kernel_refs.py) under kr.bar for the forms whose operand arrives rounded (SCALED, x_h) and for attention.
One case moves a side array to an offset the packed field cannot hold: the launcher must take the by-value kernel, same bits.
(The rider launch has no op-level entry: it keeps the by-value kernel, under the executor's tests.)"""
import contextlib
import ctypes as C
import os

import pytest
import torch

import kernel_refs as kr
import linear_refs as lr

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
PRO_SCALED, PRO_LOCAL_ATTN = 4, 3
EPS = 1e-5
SENT = 12345.0
ROWS = [1, 2, 5]
SHAPES = {"bf16": [(64, 16), (128, 56), (256, 48)], "l13": [(128, 16), (128, 56), (256, 48)], "fp8": [(64, 16), (64, 56), (64, 48)]}
KINDS = ["bf16", "l13", "fp8"]


def _launches(name):
    from uniaudio2_amd._lib import lib
    return lib.ua2_debug_kernel_launches(name.encode())


@contextlib.contextmanager
def _env(name, value):
    """A UA2_* knob for the launches inside (the library reads its environment again at ua2_debug_refresh_env)."""
    from uniaudio2_amd._lib import lib
    old = os.environ.get(name)
    os.environ[name] = value
    lib.ua2_debug_refresh_env()
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old
        lib.ua2_debug_refresh_env()


_hold = []          # buffers whose views a launch reads: kept until the process ends (tiny)


def _at(t, off_bytes=64):
    """A contiguous copy of `t` that starts off_bytes (a non-zero multiple of 16) inside its allocation."""
    assert off_bytes % 16 == 0 and off_bytes > 0
    raw = torch.zeros(off_bytes + t.numel() * t.element_size() + 64, dtype=torch.uint8, device=DEV)
    _hold.append(raw)
    v = raw[off_bytes:off_bytes + t.numel() * t.element_size()].view(t.dtype).view(t.shape)
    v.copy_(t)
    assert v.data_ptr() == raw.data_ptr() + off_bytes and v.is_contiguous()
    return v


def _wide(t, pad=8, off_bytes=32):
    """t [M, n] -> (flat view of an [M, n + pad] buffer that starts inside its allocation, ld); pad columns hold the sentinel."""
    M, n = t.shape
    buf = torch.full((M, n + pad), SENT, dtype=t.dtype)
    buf[:, :n] = t
    return _at(buf.flatten().to(DEV), off_bytes), n + pad


def _rows_of(flat, M, n, ld):
    return flat.view(M, ld)[:, :n].cpu()


_W = {}
_ARENA = {"buf": None, "pos": 0}


def _in_arena(t, misalign=0):
    """A contiguous copy of `t` inside the ONE allocation that holds every weight, image and side array of this module, 64 bytes past a
    256-byte boundary (+ misalign): a launch's second weight pointer and side arrays then lie within reach of the packed 32-bit offsets
    wherever the allocator puts things (two allocations of a long-lived process may lie more than 2^31 x 16 bytes apart)."""
    if _ARENA["buf"] is None:
        _ARENA["buf"] = torch.zeros(32 << 20, dtype=torch.uint8, device=DEV)
    n = t.numel() * t.element_size()
    start = (_ARENA["pos"] + 255) // 256 * 256 + 64 + misalign
    assert start + n <= _ARENA["buf"].numel()
    _ARENA["pos"] = start + n
    v = _ARENA["buf"][start:start + n].view(t.dtype).view(t.shape)
    v.copy_(t)
    return v


def _weights(kind, N, K, which):
    """(source weight the kernel computes with [N, K] fp32, packed bf16 view, image refs or None), packed once per process.
    Everything a launch reaches through an offset from its first weight pointer lies in one allocation (_in_arena)."""
    from uniaudio2_amd import ops
    key = (kind, N, K, which)
    if key in _W:
        return _W[key]
    g = torch.Generator().manual_seed(7919 * N + K + 104729 * which)
    W = (torch.randn(N, K, generator=g) * K ** -0.5).bfloat16().float()
    W = torch.where(W.abs() < 2.0 ** -20, torch.full_like(W, 2.0 ** -20), W)          # inside every tile's 13-bit window: no escapes
    refs = None
    if kind == "fp8":
        q, exp, twin = ops.pack_linear_w8(W.to(DEV))
        W = ops.dequant_w8(W)
        packed, parts = _in_arena(twin), (q, exp)
    else:
        packed = _in_arena(ops.pack_linear(W.to(DEV), BF16))
        parts = None
        if kind == "l13":
            image, base, esc = ops.pack_linear_l13(packed, N, K)
            assert int(esc.item()) == 0
            parts = (image, base)
    if parts is not None:
        refs = (_in_arena(parts[0]), _in_arena(parts[1]))
    _W[key] = (W, packed, refs)
    return _W[key]


def _go(kind, a, refs0, refs1=None):
    from uniaudio2_amd import _lib, ops
    if kind == "l13":
        ops.linear_l13(a, refs0, refs1)
    elif kind == "fp8":
        ops.linear_w8(a, refs0, refs1)
    else:
        _lib.check(_lib.lib.ua2_linear(C.byref(a), ops.stream()), "ua2_linear")
    torch.cuda.synchronize()


def _case(kind, pro, epi, M, N, K, *, hot=True, side_off=0, many=False):
    """One launch with every pointer a view and every stride wide.  Returns (outputs: name -> host tensor, float64 reference or None,
    its fp32 replay or None).  hot = False: UA2_GEMV_NO_HOT; many: the many-row kernels (fp32-operand forms)."""
    from uniaudio2_amd import _lib, ops
    nt = 2 if epi == lr.EPI_SWIGLU else 1
    Ws = [_weights(kind, N, K, t) for t in range(nt)]
    g = torch.Generator().manual_seed(131 * M + N + K + 17 * pro + epi)
    x = torch.randn(M, K, generator=g)
    kw = dict(dtype=BF16, M=M, N=N, K=K, w0=Ws[0][1], prologue=pro, epilogue=epi, launch=False, eps=EPS)
    if nt == 2:
        kw["w1"] = Ws[1][1]
    out, ref, ref32 = {}, None, None
    views = {}
    nw = 1 + 0.1 * torch.randn(K, generator=g)
    rowsh = pro == PRO_SCALED or (pro == lr.PRO_CAST and not many and (M == 2 or K >= 4096))   # CAST: bf16 operand rows (x_h) at M = 2 and at the large K
    if pro == lr.PRO_NORM:
        xf, ldx = _wide(x)
        kw.update(x=xf, ldx=ldx, norm_w=_at(nw.to(DEV)), norm_kind=lr.NORM_RMS_LIT)
    elif pro == PRO_SCALED:
        op = (x * nw).bfloat16()                                   # what x's producer hands over: RNE_bf16(x (.) w) and the partials of x^2
        xh, ldh = _wide(op)
        ssq = (x * x).view(M, K // 16, 16).sum(-1)
        kw.update(x_h=xh, ldh=ldh, x_ssq=_at(ssq.to(DEV).contiguous()))
    elif rowsh:
        op = x.bfloat16()
        xh, ldx = _wide(op)
        kw.update(x_h=xh, ldx=ldx)
    else:
        xf, ldx = _wide(x)
        kw.update(x=xf, ldx=ldx)
    qkv = None
    if epi == lr.EPI_QKV_ROPE:
        hs = 16
        nh = N // hs - 2
        pos = torch.tensor([5, 63, 64, 7, 70][:M], dtype=torch.int32)
        ang = torch.rand(80, hs // 2, generator=g) * 6.28
        table = torch.randperm(2 * M + 3, generator=g)[:2 * M].to(torch.int32).view(M, 2)
        kp = torch.full((2 * M + 3, 1, kr.PAGE, hs), SENT, dtype=BF16, device=DEV)
        vp = torch.full_like(kp, SENT)
        views.update(k_pool=kp, v_pool=vp, q_out=_at(torch.full((M, nh * hs), SENT, device=DEV)))
        td = _at(table.to(DEV))
        kw.update(row_pos=_at(pos.to(DEV)), rope_cos=_at(ang.cos().to(DEV)), rope_sin=_at(ang.sin().to(DEV)), q_out=views["q_out"],
                  rope_mode=lr.ROPE_INTERLEAVED, kv=ops.kv_geom(kp, vp, td, nh, 1, hs))
        qkv = dict(pos=pos, n_head=nh, n_kv=1, hs=hs, rope_mode=lr.ROPE_INTERLEAVED, cos=ang.cos(), sin=ang.sin(), table=table)
    else:
        yf, ldy = _wide(torch.full((M, N), SENT))
        views["y"] = yf
        kw.update(y=yf, ldy=ldy)
    resid = None
    if epi == lr.EPI_RESIDUAL:
        resid = torch.randn(M, N, generator=g)
        rf, ldr = _wide(resid, pad=24)
        kw.update(resid=rf, ldr=ldr)
    if epi == lr.EPI_STORE:
        nb = (N + 15) // 16
        views["part_max"] = _at(torch.zeros(M, nb, device=DEV))
        views["part_idx"] = _at(torch.zeros(M, nb, dtype=torch.int32, device=DEV))
        kw.update(part_max=views["part_max"], part_idx=views["part_idx"], forbid=_at(torch.full((M,), 3, dtype=torch.int32, device=DEV)))
    if many:
        kw["workspace"] = ops.linear_workspace(BF16, M, K, torch.device(DEV))
    a = ops.linear(**kw)
    refs = [w[2] for w in Ws]
    if side_off:                                                   # the side array of w0 at an offset no whole number of 16 bytes from the image
        img, side = refs[0]
        vs = _in_arena(side, misalign=side_off)
        assert (vs.data_ptr() - img.data_ptr()) % 16 != 0
        refs[0] = (img, vs)
    n_hot = _launches("gemv_hot")
    lib = _lib.lib
    if many:
        old = lib.ua2_debug_force_general_linear(3)
        try:
            n_g = _launches("gemv")
            _go("bf16", a, None)
            assert _launches("gemv") == n_g, "the many-row reference ran the decode kernel"
        finally:
            lib.ua2_debug_force_general_linear(old)
    elif hot:
        _go(kind, a, refs[0], refs[1] if nt == 2 else None)
        assert _launches("gemv_hot") - n_hot == (0 if side_off else 1), "which kernel form served the launch"
    else:
        with _env("UA2_GEMV_NO_HOT", "1"):
            _go(kind, a, refs[0], refs[1] if nt == 2 else None)
        assert _launches("gemv_hot") == n_hot
    for k, v in views.items():
        if k == "y":
            out[k] = _rows_of(v, M, N, ldy)
            assert bool((v.view(M, ldy)[:, N:].cpu() == SENT).all()), "pad columns of y written"
        else:
            out[k] = v.cpu().clone()
    # float64 reference for the forms whose operand arrives rounded (the rounding is then not the kernel's)
    if pro == PRO_SCALED or rowsh:
        W0, W1 = Ws[0][0], (Ws[1][0] if nt == 2 else None)
        for dt in (F64, F32):
            if pro == PRO_SCALED:
                r = lr.scaled_linear_ref(op, ssq, W0, eps=EPS, epi=epi, W1=W1, qkv=qkv, dt=dt)
            else:
                r = lr.linear_ref(op.float(), W0, BF16, pro=lr.PRO_CAST, epi=epi, W1=W1, resid=resid, dt=dt)
            if dt == F64:
                ref = r
            else:
                ref32 = r
    return out, ref, ref32, qkv


def _same(a, b, what):
    assert a.keys() == b.keys() and a
    for k in a:
        p, q = a[k], b[k]
        if p.dtype == BF16:
            p, q = p.view(torch.int16), q.view(torch.int16)
        assert torch.equal(p, q), (what, k)


def _judge(case, out, ref, ref32, qkv, M):
    if qkv is None:
        got, scale = out["y"].to(F64), max(1.0, float(ref.abs().max()))
        err = float((got - ref).abs().max()) / scale
        e_ref = float((ref32.to(F64) - ref).abs().max()) / scale
    else:
        rq, rk, rv = ref
        scale = max(1.0, float(max(rq.abs().max(), rk.abs().max(), rv.abs().max())))
        e_ref = max(float((a.to(F64) - b).abs().max()) for a, b in zip(ref32, ref)) / scale
        err = float((out["q_out"].to(F64).view(rq.shape) - rq).abs().max()) / scale
        for m in range(M):
            p = int(qkv["pos"][m])
            page, off = int(qkv["table"][m, p // kr.PAGE]), p % kr.PAGE
            for pool, r in ((out["k_pool"], rk[m]), (out["v_pool"], rv[m])):
                d = ((pool[page, :, off].to(F64) - r).abs() - lr.half_ulp_bf16(r)).clamp_min(0.0)      # the cache holds bf16: one rounding on top
                err = max(err, float(d.max()) / scale)
    b = kr.bar(e_ref)
    print(f"PARITY hot_args {case}: err {err:.3e} E_ref {e_ref:.3e} bar {b:.3e}")
    assert err <= b, f"{case}: {err:.3e} over bar {b:.3e}"


PAIRS = [(lr.PRO_NORM, lr.EPI_QKV_ROPE), (lr.PRO_NORM, lr.EPI_SWIGLU), (lr.PRO_NORM, lr.EPI_STORE),
         (PRO_SCALED, lr.EPI_QKV_ROPE), (PRO_SCALED, lr.EPI_SWIGLU), (PRO_SCALED, lr.EPI_STORE),
         (lr.PRO_CAST, lr.EPI_RESIDUAL), (lr.PRO_CAST, lr.EPI_STORE)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pro,epi", PAIRS)
def test_hot_launch_equals_the_by_value_launch_and_its_references(kind, pro, epi):
    from uniaudio2_amd import ops  # noqa: F401  (the library must be importable before the first case builds its inputs)
    for K, N in SHAPES[kind]:
        if epi == lr.EPI_QKV_ROPE and N != 48:
            continue                                               # q | k | v of 16-wide heads: N = 48
        for M in ROWS:
            case = f"{kind} pro {pro} epi {epi} K={K} N={N} M={M}"
            out, ref, ref32, qkv = _case(kind, pro, epi, M, N, K)
            by_value = _case(kind, pro, epi, M, N, K, hot=False)[0]
            _same(out, by_value, case + " (by-value kernel)")
            assert "y" not in out or float(out["y"].abs().max()) > 0, case
            if pro == lr.PRO_NORM or (pro == lr.PRO_CAST and M != 2):
                many = _case(kind, pro, epi, M, N, K, many=True)[0]          # the same rows by the many-row kernels (bf16 weights W / W')
                _same(out, many, case + " (many-row kernel)")
            if ref is not None:
                _judge(case, out, ref, ref32, qkv, M)


def test_an_offset_that_does_not_fit_takes_the_by_value_kernel():
    """The 13-bit image's base bytes 8 bytes off a 16-byte distance from the image: no packed offset; same bits from the by-value kernel."""
    for pro, epi in ((PRO_SCALED, lr.EPI_SWIGLU), (lr.PRO_CAST, lr.EPI_RESIDUAL)):
        out = _case("l13", pro, epi, 2, 56, 128)[0]
        moved = _case("l13", pro, epi, 2, 56, 128, side_off=8)[0]           # asserts that no hot launch was counted
        _same(out, moved, (pro, epi))


def test_largest_k_of_the_model_in_the_packed_field():
    """K = 8192 (the down-projection): the 16-bit K field, 16 chunks per wave, bf16 operand rows; one row, one tile."""
    out, ref, ref32, _ = _case("l13", lr.PRO_CAST, lr.EPI_RESIDUAL, 1, 16, 8192)
    _same(out, _case("l13", lr.PRO_CAST, lr.EPI_RESIDUAL, 1, 16, 8192, hot=False)[0], "K = 8192")
    assert ref is not None                                         # the x_h form
    _judge("l13 x_h residual K=8192 N=16 M=1", out, ref, ref32, None, 1)


# ---- LOCAL_ATTN, with and without the arg-max fold ---------------------------------------------------------------------------------

def _local(kind, fold, hot):
    """The O-projection with the short-context attention as its prologue (n_head 4, n_kv 2, head size 32: K = 128), N = 56, M = 1."""
    from uniaudio2_amd import ops
    n_head, n_kv, hs, N, pos = 4, 2, 32, 56, 5
    K = n_head * hs
    W, packed, refs = _weights(kind, N, K, 0)
    g = torch.Generator().manual_seed(99)
    k = _at((torch.randn(2, n_kv, 64, hs, generator=g) * 0.5).bfloat16().to(DEV))
    v = _at((torch.randn(2, n_kv, 64, hs, generator=g) * 0.5).bfloat16().to(DEV))
    pt = _at(torch.tensor([[1]], dtype=torch.int32, device=DEV))
    yf, ldy = _wide(torch.full((1, N), SENT))
    rf, ldr = _wide(torch.randn(1, N, generator=g), pad=24)
    kw = dict(dtype=BF16, M=1, N=N, K=K, w0=packed, prologue=PRO_LOCAL_ATTN, epilogue=lr.EPI_RESIDUAL, launch=False, y=yf, ldy=ldy,
              resid=rf, ldr=ldr, row_pos=_at(torch.tensor([pos], dtype=torch.int32, device=DEV)), kv=ops.kv_geom(k, v, pt, n_head, n_kv, hs))
    views = {"y": yf, "k": k, "v": v}
    if fold:
        V = 24
        views["tok"] = _at(torch.zeros(1, dtype=torch.int32, device=DEV))
        pm = torch.randn(8, generator=g)
        f = dict(part_max=_at(pm.to(DEV)), part_idx=_at((torch.arange(8, dtype=torch.int32) * 3 % V).to(DEV)), out_token=views["tok"], n_part=8,
                 limit=V, row_off=2, pos=pos, tab_y=_at(torch.randn(V + 2, N, generator=g).to(DEV)), tab_q=_at((torch.randn(V + 2, K, generator=g) * 0.5).to(DEV)),
                 tab_k=_at((torch.randn(V + 2, n_kv * hs, generator=g) * 0.5).bfloat16().to(DEV)),
                 tab_v=_at((torch.randn(V + 2, n_kv * hs, generator=g) * 0.5).bfloat16().to(DEV)))
        kw.update(fold=f)
    xf, ldx = _wide(torch.randn(1, K, generator=g) * 0.5)          # (folded: not read)
    kw.update(x=xf, ldx=ldx)
    a = ops.linear(**kw)
    n_hot = _launches("gemv_hot")
    with _env("UA2_GEMV_NO_HOT", "0" if hot else "1"):
        _go(kind, a, refs)
    assert _launches("gemv_hot") - n_hot == int(hot and kind == "bf16")      # on an image this prologue keeps the by-value kernel (profiles/hot_args.md)
    out = {n: (t.cpu().clone() if n != "y" else _rows_of(t, 1, N, ldy)) for n, t in views.items()}
    assert float(out["y"].abs().max()) > 0 and bool((out["y"] != SENT).all())
    return out


@pytest.mark.parametrize("kind,fold", [("bf16", False), ("l13", False), ("fp8", False), ("bf16", True)])
def test_local_attention_prologue_with_and_without_the_fold(kind, fold):
    _same(_local(kind, fold, True), _local(kind, fold, False), (kind, fold))


# ---- attn_fused ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("keys", [1, 17, 65])
def test_attn_fused_hot_kernel(keys):
    """One row at 1, 17 and 65 keys (one and two pages), 6 query heads on 2 kv heads of 32: the hot kernel against the by-value kernel
    bit for bit (fp32 y and the bf16 rows y_h on a wide stride), and against float64 under the bar."""
    from uniaudio2_amd import ops
    n_head, n_kv, hs = 6, 2, 32
    cache = kr.PagedCache([keys], n_kv, hs, BF16, seed=keys, extra_pages=2)
    g = torch.Generator().manual_seed(keys)
    q = torch.randn(1, n_head * hs, generator=g)
    pos = torch.tensor([keys - 1], dtype=torch.int32)
    Kst, Vst = cache.stored_seq(0)
    ref = kr.attn_ref(q, [Kst], [Vst], pos.numpy(), [0], n_head, n_kv)
    ref32 = kr.attn_ref(q, [Kst], [Vst], pos.numpy(), [0], n_head, n_kv, dt=F32)
    kp, vp, td = _at(cache.k.to(DEV)), _at(cache.v.to(DEV)), _at(cache.table.to(DEV))
    outs = []
    for hot in (True, False):
        y = _at(torch.full((1, n_head * hs), SENT, device=DEV))
        yh, ldh = _wide(torch.full((1, n_head * hs), SENT).bfloat16())
        n0 = _launches("attn_hot")
        with _env("UA2_ATTN_NO_HOT", "0" if hot else "1"):
            ops.attn(dtype=BF16, R=1, q=_at(q.to(DEV)), row_pos=_at(pos.to(DEV)), row_seq=None, kv=ops.kv_geom(kp, vp, td, n_head, n_kv, hs), y=y, y_h=yh.view(1, ldh))
            torch.cuda.synchronize()
        assert _launches("attn_hot") - n0 == int(hot)
        outs.append({"y": y.cpu().clone(), "y_h": yh.cpu().clone()})
    _same(outs[0], outs[1], keys)
    assert bool((outs[0]["y_h"].view(1, ldh)[:, n_head * hs:].float() == torch.tensor(SENT).bfloat16().float()).all()), "pad columns of y_h written"
    scale = max(1.0, float(ref.abs().max()))
    err, e_ref = float((outs[0]["y"].to(F64) - ref).abs().max()) / scale, float((ref32.to(F64) - ref).abs().max()) / scale
    print(f"PARITY hot_args attn keys={keys}: err {err:.3e} E_ref {e_ref:.3e} bar {kr.bar(e_ref):.3e}")
    assert err <= kr.bar(e_ref)
