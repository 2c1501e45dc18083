"""fp8 (OCP e4m3fn) weights in the batched decode frame: ua2_linear_w8_many, the weights-stationary kernel (csrc/ua2_skinny.hip) on the
fp8 image, 6 .. UA2_SKINNY_W8_MAX_ROWS rows.

The contract is the fp8 option's: an identity, not a tolerance.  The launch on the image gives, bit for bit, what ua2_linear gives on the
bf16 twin W' = q 2^e (same kernel family, bf16 form), and row by row what the decode kernel gives on the image (ua2_linear_w8).  No test
here compares the fp8 kernel with itself: the other side is the bf16 kernel on W', the decode kernel, or the exact value of a code.

The kernel exists only for the K geometries of the released widths, so the shapes are those Linear layers (each <= 100 MB of weights)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
FP8 = torch.float8_e4m3fn
PRO_SCALED = 4
MMAX = 64
# 6: first count past the decode kernel, a partial tile; 16: one full tile; 17: a clamped second tile; 33: three row tiles (where the
# SwiGLU ring form starts); 64: four full tiles
ROWS = [6, 16, 17, 33, 64]
COUNTERS = ("skinny2", "skinny2_w8", "gemv", "gemv_w8", "gemm", "rsplit")


def _launches(name):
    from uniaudio2_amd._lib import lib
    return lib.ua2_debug_kernel_launches(name.encode())


def _counts():
    return {k: _launches(k) for k in COUNTERS}


def _moved(before):
    return {k: _launches(k) - v for k, v in before.items() if _launches(k) != v}


_PACKS = {}


def _packs(N, K, nt, rope_hs):
    """(q, exp, twin) per matrix of the launch, packed once per shape for the whole module"""
    from uniaudio2_amd import ops
    key = (N, K, nt, rope_hs)
    if key not in _PACKS:
        g = torch.Generator(device=DEV).manual_seed(N * 31 + K + nt)
        _PACKS[key] = [ops.pack_linear_w8(torch.randn(N, K, generator=g, device=DEV) * 0.02, rope_head_size=rope_hs) for _ in range(nt)]
    return _PACKS[key]


class Case:
    """One Linear of the frame with inputs for MMAX rows; launch(kind, r0, M) runs rows [r0, r0 + M) into fresh outputs.
    kind: "twin" = ua2_linear on W', "many" = ua2_linear_w8_many, "decode" = ua2_linear_w8 (M <= 5)."""

    def __init__(self, pro, epi, N, K, heads=None, handover=False, partmax=False, seed=0):
        from uniaudio2_amd import _lib, ops
        self.pro, self.epi, self.N, self.K, self.heads, self.handover, self.partmax = pro, epi, N, K, heads, handover, partmax
        self.nt = 2 if epi == _lib.EPI_SWIGLU else 1
        self.packs = _packs(N, K, self.nt, heads[2] if epi == _lib.EPI_QKV_ROPE else 0)
        g = torch.Generator().manual_seed(seed + N + K)
        self.x = torch.randn(MMAX, K, generator=g).to(DEV)
        self.norm_w = (1 + 0.1 * torch.randn(K, generator=g)).to(DEV)
        self.resid = torch.randn(MMAX, N, generator=g).to(DEV)
        self.next_w = (1 + 0.1 * torch.randn(N, generator=g)).to(DEV)
        self.pos = ((torch.arange(MMAX) * 3) % 8).to(torch.int32).to(DEV)            # rows differ in their position
        if heads:
            ang = torch.rand(8, heads[2] // 2, generator=g)
            self.cos, self.sin = torch.cos(ang).to(DEV), torch.sin(ang).to(DEV)
        if pro == PRO_SCALED:
            # the operand as its producer hands it over (the project's own path: a RESIDUAL launch with the y_norm_w hand-over): fragment
            # order for the many-row kernels, row-major for the decode kernel, per-16-column sums of squares for both
            pk = ops.pack_linear(torch.eye(K, device=DEV) * 0.5, torch.bfloat16)
            self.xp = torch.zeros(MMAX * K, dtype=torch.bfloat16, device=DEV)
            self.xh = torch.zeros(MMAX, K, dtype=torch.bfloat16, device=DEV)
            self.xs = torch.zeros(MMAX, K // 16, device=DEV)
            ops.linear(dtype=torch.bfloat16, M=MMAX, N=K, K=K, w0=pk, prologue=_lib.PRO_CAST, epilogue=_lib.EPI_RESIDUAL, x=self.x,
                       y=torch.empty(MMAX, K, device=DEV), resid=self.x, y_norm_w=self.norm_w, y_ssq=self.xs, y_packed=self.xp, y_h=self.xh, ldh=K,
                       workspace=ops.linear_workspace(torch.bfloat16, MMAX, K, DEV))
            torch.cuda.synchronize()
            assert float(self.xs.abs().max()) > 0 and float(self.xh.float().abs().max()) > 0

    def launch(self, kind, r0, M):
        from uniaudio2_amd import _lib, ops
        N, K, epi, pro = self.N, self.K, self.epi, self.pro
        kw = dict(dtype=torch.bfloat16, M=M, N=N, K=K, w0=self.packs[0][2], prologue=pro, epilogue=epi, launch=False)
        out = {}
        if self.nt == 2:
            kw["w1"] = self.packs[1][2]
        if pro == PRO_SCALED:
            if kind == "decode":
                kw.update(x_h=self.xh[r0:r0 + M], x_ssq=self.xs[r0:r0 + M].contiguous(), ldh=K)
            else:
                assert r0 == 0                                       # fragment order: a prefix of the row tiles
                kw.update(x_packed=self.xp, x_ssq=self.xs)
        else:
            kw.update(x=self.x[r0:r0 + M])
            if pro == _lib.PRO_NORM:
                kw.update(norm_w=self.norm_w)
        if kind != "decode" and pro != PRO_SCALED:
            kw.update(workspace=ops.linear_workspace(torch.bfloat16, M, K, DEV))
        if epi == _lib.EPI_QKV_ROPE:
            n_head, n_kv, hs = self.heads
            out["k_pool"] = torch.zeros(M, n_kv, 64, hs, dtype=torch.bfloat16, device=DEV)
            out["v_pool"] = torch.zeros(M, n_kv, 64, hs, dtype=torch.bfloat16, device=DEV)
            out["q_out"] = torch.zeros(M, n_head * hs, device=DEV)
            pt = torch.arange(M, dtype=torch.int32, device=DEV).view(M, 1)
            kw.update(row_pos=self.pos[r0:r0 + M].contiguous(), kv=ops.kv_geom(out["k_pool"], out["v_pool"], pt, n_head, n_kv, hs),
                      rope_cos=self.cos, rope_sin=self.sin, q_out=out["q_out"])
            keep = pt
        else:
            out["y"] = torch.zeros(M, N, device=DEV)
            kw.update(y=out["y"])
        if epi == _lib.EPI_RESIDUAL:
            kw.update(resid=self.resid[r0:r0 + M])
        if self.handover:
            out["y_h"] = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
            out["y_ssq"] = torch.zeros(M, N // 16, device=DEV)
            kw.update(y_norm_w=self.next_w, y_h=out["y_h"], y_ssq=out["y_ssq"], ldh=N)
        if self.partmax:
            nb = (N + 15) // 16
            out["part_max"] = torch.zeros(M, nb, device=DEV)
            out["part_idx"] = torch.full((M, nb), -1, dtype=torch.int32, device=DEV)
            kw.update(part_max=out["part_max"], part_idx=out["part_idx"], forbid=torch.full((M,), 24, dtype=torch.int32, device=DEV))
        a = ops.linear(**kw)
        w0, w1 = self.packs[0][:2], (self.packs[1][:2] if self.nt == 2 else None)
        if kind == "twin":
            _lib.check(_lib.lib.ua2_linear(_lib.C.byref(a), ops.stream()), "ua2_linear")
        elif kind == "many":
            ops.linear_w8_many(a, w0, w1)
        else:
            ops.linear_w8(a, w0, w1)
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in out.items()}


def _same(ref, got, what, rows=None):
    """torch.equal on every output (bf16 as int16); `rows` = (row of ref, row of got) compares one row"""
    assert ref.keys() == got.keys() and ref
    for k in ref:
        a, b = ref[k], got[k]
        if rows is not None:
            a, b = a[rows[0]], b[rows[1]]
        if a.dtype == torch.bfloat16:
            a, b = a.view(torch.int16), b.view(torch.int16)
        assert torch.equal(a, b), (what, k)
        if ref[k].dtype != torch.int32:
            assert float(ref[k].float().abs().max()) > 0, (what, k, "output never written")


def _cases():
    from uniaudio2_amd import _lib
    L = _lib
    out = []
    for pro in (L.PRO_NORM, PRO_SCALED):                                 # as the frame pairs them
        out += [("qkv", pro, L.EPI_QKV_ROPE, 5120, 3072, dict(heads=(24, 8, 128))), ("qkv", pro, L.EPI_QKV_ROPE, 3072, 2048, dict(heads=(32, 8, 64))),
                ("swiglu", pro, L.EPI_SWIGLU, 8192, 3072, {}), ("swiglu", pro, L.EPI_SWIGLU, 8192, 2048, {}),
                ("audio_head", pro, L.EPI_STORE, 12296, 2048, dict(partmax=True))]     # N % 16 != 0: the clamped last tile
    for N, K in [(3072, 8192), (2048, 8192), (3072, 3072)]:
        out += [("down", L.PRO_CAST, L.EPI_RESIDUAL, N, K, dict(handover=True)), ("down", L.PRO_CAST, L.EPI_RESIDUAL, N, K, {})]
    out += [("projection", L.PRO_CAST, L.EPI_STORE, 2048, 3072, dict(handover=True))]
    return out


CASE_IDS = ["qkv", "swiglu", "audio_head", "down", "projection"]


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("layer", CASE_IDS)
def test_kernel_identity_with_the_bf16_kernel_on_the_twin(layer, M):
    for name, pro, epi, N, K, opt in _cases():
        if name != layer:
            continue
        c = Case(pro, epi, N, K, **opt)
        n0 = _counts()
        ref = c.launch("twin", 0, M)
        assert _moved(n0) == {"skinny2": 1}, (name, pro, N, K, _moved(n0))
        n1 = _counts()
        got = c.launch("many", 0, M)
        assert _moved(n1) == {"skinny2_w8": 1}, (name, pro, N, K, _moved(n1))
        _same(ref, got, (name, pro, N, K, M))


@pytest.mark.parametrize("layer", ["qkv", "swiglu", "audio_head", "down"])
def test_rows_of_a_17_row_launch_equal_the_decode_kernel_on_the_image(layer):
    from uniaudio2_amd import _lib
    pick = {"qkv": (_lib.PRO_NORM, _lib.EPI_QKV_ROPE, 3072, 2048, dict(heads=(32, 8, 64))),
            "swiglu": (PRO_SCALED, _lib.EPI_SWIGLU, 8192, 3072, {}),
            "audio_head": (_lib.PRO_NORM, _lib.EPI_STORE, 12296, 2048, dict(partmax=True)),
            "down": (_lib.PRO_CAST, _lib.EPI_RESIDUAL, 3072, 8192, dict(handover=True))}[layer]
    pro, epi, N, K, opt = pick
    c = Case(pro, epi, N, K, **opt)
    many = c.launch("many", 0, 17)
    for r in (0, 7, 16):                                                 # first tile, inside it, the clamped second tile's only row
        n0 = _counts()
        one = c.launch("decode", r, 1)
        assert _moved(n0) == {"gemv_w8": 1}, _moved(n0)
        _same(one, many, (layer, r), rows=(0, r))


def _forced(variant, fn):
    from uniaudio2_amd._lib import lib
    os.environ["UA2_SKINNY2"] = variant                                    # read per call
    try:
        return fn()
    finally:
        del os.environ["UA2_SKINNY2"]
        lib.ua2_debug_refresh_env()


def test_forced_variants_give_the_same_bits():
    from uniaudio2_amd import _lib
    L = _lib
    plain = [(L.PRO_NORM, L.EPI_QKV_ROPE, 5120, 3072, dict(heads=(24, 8, 128))), (L.PRO_CAST, L.EPI_RESIDUAL, 3072, 3072, dict(handover=True)),
             (L.PRO_NORM, L.EPI_STORE, 12296, 2048, dict(partmax=True))]
    for pro, epi, N, K, opt in plain:
        c = Case(pro, epi, N, K, **opt)
        ref = c.launch("twin", 0, 64)                                    # the bf16 kernel on W', its own default variant
        for v in ("1,2,2,2", "2,4,1,1"):                                 # two passes at 64 rows; two column tiles per wave
            n0 = _counts()
            got = _forced(v, lambda: c.launch("many", 0, 64))
            assert _moved(n0) == {"skinny2_w8": 1}, (v, _moved(n0))
            _same(ref, got, (epi, N, K, v))
    for pro in (L.PRO_NORM, PRO_SCALED):
        c = Case(pro, L.EPI_SWIGLU, 8192, 3072)
        ref = c.launch("twin", 0, 64)
        # + the ring forms (three bursts, two bursts) and the resident two-column-tile form, which fits the registers only as fp8 (no bf16
        # counterpart is built: the reference is the bf16 kernel's default variant, as for every forced form here)
        # (under the scaled consumer its partials do not fit beside the two column tiles: not built, NORM only)
        for v in ("1,2,2,2", "2,4,2,1,6", "2,4,1,1,4") + (("2,4,1,1",) if pro == L.PRO_NORM else ()):
            n0 = _counts()
            got = _forced(v, lambda: c.launch("many", 0, 64))
            assert _moved(n0) == {"skinny2_w8": 1}, (v, _moved(n0))
            _same(ref, got, ("swiglu", pro, v))
    c = Case(L.PRO_NORM, L.EPI_SWIGLU, 8192, 3072)
    n0 = _counts()
    with pytest.raises(L.Ua2Error, match="ua2_linear_w8_many"):         # an odd ring has no fp8 form (two chunks per load)
        _forced("2,4,1,1,3", lambda: c.launch("many", 0, 64))
    torch.cuda.synchronize()
    assert _moved(n0) == {}, _moved(n0)


def test_all_256_codes_dequantise_exactly():
    """Every e4m3fn code except the two NaNs as a weight (one 448 per row pins e = 0), 16 one-hot rows per launch at K = 2048: the output
    shows each dequantised value — subnormals, both zeros, +-448 — exactly.  The codes sit in even and odd chunks of several waves' ranges."""
    from uniaudio2_amd import ops
    N, K = 16, 2048
    vals = torch.arange(256, dtype=torch.uint8).view(FP8).float()
    vals[0x7F] = vals[0xFF] = 0.0
    cols = torch.arange(64) * 31                                          # 0 .. 1953, distinct; chunk = col // 32 takes both parities
    W = torch.zeros(N, K)
    W[:4, cols] = vals.view(4, 64)
    W[:, 2047] = 448.0
    q, exp, twin = ops.pack_linear_w8(W.to(DEV))
    assert int(exp.cpu().abs().sum()) == 0
    ks_all = cols.tolist() + [2047] + list(range(1, 16))
    n0 = _launches("skinny2_w8")
    for k0 in range(0, len(ks_all), 16):
        ks = ks_all[k0:k0 + 16]
        x = torch.zeros(16, K, device=DEV)
        x[torch.arange(16), torch.tensor(ks)] = 1.0
        y = torch.full((16, N), 7.0, device=DEV)
        a = ops.linear(dtype=torch.bfloat16, M=16, N=N, K=K, w0=twin, x=x, y=y, workspace=ops.linear_workspace(torch.bfloat16, 16, K, DEV), launch=False)
        ops.linear_w8_many(a, (q, exp))
        assert torch.equal(y.cpu(), W[:, ks].t().contiguous()), ks
    assert _launches("skinny2_w8") - n0 == len(ks_all) // 16


def test_refusals_name_the_entry_point_and_launch_nothing():
    from uniaudio2_amd import _lib, ops
    L = _lib
    g = torch.Generator(device=DEV).manual_seed(3)
    big = ops.pack_linear_w8(torch.randn(2048, 2048, generator=g, device=DEV) * 0.02)
    big1 = ops.pack_linear_w8(torch.randn(2048, 2048, generator=g, device=DEV) * 0.02)
    toy = ops.pack_linear_w8(torch.randn(64, 128, generator=g, device=DEV) * 0.02)
    f32w = ops.pack_linear(torch.randn(2048, 2048, generator=g, device=DEV) * 0.02, torch.float32)
    n0 = _counts()

    def refused(M, N, K, packs, dtype=torch.bfloat16, epi=L.EPI_STORE, w0=None, w1=None, tw1=None):
        x, y = torch.zeros(M, K, device=DEV), torch.zeros(M, N, device=DEV)
        a = ops.linear(dtype=dtype, M=M, N=N, K=K, w0=w0 if w0 is not None else packs[2], w1=w1, x=x, y=y, epilogue=epi,
                       workspace=ops.linear_workspace(dtype, M, K, DEV), launch=False)
        with pytest.raises(L.Ua2Error, match="ua2_linear_w8_many"):
            ops.linear_w8_many(a, packs[:2], tw1)

    refused(5, 2048, 2048, big)                                          # the decode kernel's rows
    refused(65, 2048, 2048, big)                                         # past the default row limit
    refused(16, 2048, 2048, big, dtype=torch.float32, w0=f32w)           # an fp32 launch
    refused(16, 2048, 2048, big, epi=L.EPI_GELU)
    refused(16, 64, 128, toy)                                            # a toy shape: outside the kernel's table
    refused(16, 2048, 2048, big, epi=L.EPI_SWIGLU, w1=big1[2])           # SwiGLU without w1's twin
    x, y = torch.zeros(6, 2048, device=DEV), torch.zeros(6, 2048, device=DEV)
    a = ops.linear(dtype=torch.bfloat16, M=6, N=2048, K=2048, w0=big[2], x=x, y=y, launch=False)
    with pytest.raises(L.Ua2Error, match="ua2_linear_w8"):                # the decode entry point still refuses more rows than it takes
        ops.linear_w8(a, big[:2])
    torch.cuda.synchronize()
    assert _moved(n0) == {}, _moved(n0)
