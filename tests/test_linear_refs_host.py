"""The float64 references of tests/linear_refs.py against the torch library functions they restate (CPU, float64, rtol 1e-12), the
layout decoder against a layout built index by index, and the flip-free input builder on every input the GPU module uses."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kernel_refs as kr
import linear_refs as lr

RTOL = 1e-12
F64 = torch.float64
BF16, F32 = torch.bfloat16, torch.float32


def _close(a, b):
    np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=RTOL, atol=1e-13)


def _g(seed):
    return torch.Generator().manual_seed(seed)


def test_rows_per_tile_restates_the_launcher():
    """The three values the LDS budget gives at the model's widths (csrc/ua2_gemv.hip ua2_gemv_rows_per_tile)."""
    assert lr.rows_per_tile(BF16, 8192) == 6 and lr.rows_per_tile(F32, 8192) == 3 and lr.rows_per_tile(BF16, 3072) == 16
    assert lr.rows_per_tile(BF16, 72) == 16 and lr.rows_per_tile(F32, 6144) == 4


def test_bf16_round64_is_rne():
    g = _g(0)
    v = torch.randn(4096, generator=g) * torch.tensor([1e-3, 1.0, 1e3, 1e-30]).repeat(1024)
    assert torch.equal(lr.bf16_round64(v.to(F64)), v.to(BF16).to(F64))            # an fp32 value: one rounding either way
    one, ulp = 1.0, 2.0 ** -7
    ties = torch.tensor([one + 0.5 * ulp, one + 1.5 * ulp, -(one + 0.5 * ulp), one + 0.5 * ulp + 2.0 ** -40, 2.0 - 0.25 * ulp], dtype=F64)
    assert lr.bf16_round64(ties).tolist() == [one, one + 2 * ulp, -one, one + ulp, 2.0]
    assert lr.midpoint_distance(ties)[:3].tolist() == [0.0, 0.0, 0.0] and float(lr.midpoint_distance(ties)[3]) == 2.0 ** -40
    assert float(lr.half_ulp_bf16(torch.tensor(1.5))) == 2.0 ** -8


@pytest.mark.parametrize("norm_kind", [lr.NORM_RMS_LIT, lr.NORM_RMS_MOSHI, lr.NORM_LAYERNORM])
def test_operand_ref_vs_torch(norm_kind):
    g = _g(norm_kind)
    x = torch.randn(5, 72, generator=g, dtype=F64) + 0.5
    w, b = 1 + 0.1 * torch.randn(72, generator=g, dtype=F64), 0.1 * torch.randn(72, generator=g, dtype=F64)
    got = lr.operand_ref(x, lr.PRO_NORM, norm_kind, w, b, 1e-5, F32)
    if norm_kind == lr.NORM_LAYERNORM:
        _close(got, F.layer_norm(x, (72,), w, b, 1e-5))
        _close(got, kr.layernorm_ref(x, w, b, 1e-5))
    else:
        _close(got, x * torch.rsqrt(torch.mean(x * x, dim=-1, keepdim=True) + 1e-5) * w)
    _close(lr.operand_ref(x, lr.PRO_CAST, 0, None, None, 0.0, F32), x)
    got16 = lr.operand_ref(x, lr.PRO_NORM, norm_kind, w, b, 1e-5, BF16)
    assert torch.equal(got16, lr.bf16_round64(got))


@pytest.mark.parametrize("dtype,K", [(BF16, 72), (BF16, 1056), (F32, 72), (F32, 1056)])
def test_ksum_and_epilogues_vs_torch(dtype, K):
    g = _g(K)
    M, N = 5, 37
    a, W, W1 = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5, torch.randn(N, K, generator=g) * K ** -0.5
    bias, bias1 = torch.randn(N, generator=g), torch.randn(N, generator=g)
    resid, osc = torch.randn(M, N, generator=g), torch.rand(N, generator=g) + 0.5
    a64 = a.to(dtype).to(F64)
    w64, w164 = W.to(dtype).to(F64), W1.to(dtype).to(F64)
    assert torch.equal(lr.weights_ref(W, dtype), w64)
    lin, lin1 = F.linear(a64, w64, bias.to(F64)), F.linear(a64, w164, bias1.to(F64))
    kw = dict(dt=F64)
    _close(lr.linear_ref(a, W, dtype, bias=bias, **kw), lin)
    _close(lr.linear_ref(a, W, dtype, **kw), F.linear(a64, w64))
    _close(lr.linear_ref(a, W, dtype, epi=lr.EPI_RESIDUAL, bias=bias, resid=resid, out_scale=osc, **kw), resid.to(F64) + osc.to(F64) * lin)
    _close(lr.linear_ref(a, W, dtype, epi=lr.EPI_RESIDUAL, resid=resid, **kw), resid.to(F64) + F.linear(a64, w64))
    _close(lr.linear_ref(a, W, dtype, epi=lr.EPI_SWIGLU, W1=W1, bias=bias, bias1=bias1, **kw), F.silu(lin) * lin1)
    _close(lr.linear_ref(a, W, dtype, epi=lr.EPI_SWIGLU, W1=W1, bias=bias, bias1=bias1, act_kind=lr.GATE_SIGMOID_SECOND, **kw),
           lin * torch.sigmoid(lin1))
    _close(lr.linear_ref(a, W, dtype, epi=lr.EPI_GELU, bias=bias, **kw), F.gelu(lin))
    _close(lr.linear_ref(a, W, dtype, epi=lr.EPI_GELU, bias=bias, act_kind=lr.GELU_TANH, **kw), F.gelu(lin, approximate="tanh"))
    # the fp32 replay is the same function to fp32 accuracy, and the deliberately wrong sum is not
    y32 = lr.linear_ref(a, W, dtype, bias=bias, dt=F32)
    assert y32.dtype == F32 and float((y32.to(F64) - lin).abs().max()) < 1e-4 * K ** 0.5
    assert float((lr.linear_ref(a, W, dtype, bias=bias, drop_last_chunk=True, **kw) - lin).abs().max()) > 1e-3


@pytest.mark.parametrize("mode", [lr.ROPE_HALF_SPLIT, lr.ROPE_INTERLEAVED, lr.ROPE_NONE])
def test_qkv_rope_ref_vs_literal_rotary(mode):
    g = _g(mode)
    M, nh, nkv, hs = 4, 3, 1, 32
    s = torch.randn(M, (nh + 2 * nkv) * hs, generator=g, dtype=F64)
    bias = torch.randn(s.shape[1], generator=g, dtype=F64)
    pos = torch.tensor([0, 5, 64, 130])
    ang = torch.arange(140, dtype=F64)[:, None] * (10000.0 ** (-torch.arange(hs // 2, dtype=F64) / (hs // 2)))[None, :]
    q, k, v = lr.qkv_rope_ref(s, pos, nh, nkv, hs, mode, ang.cos(), ang.sin(), bias)
    sb = s + bias
    q0, k0, v0 = sb[:, :nh * hs].view(M, nh, hs), sb[:, nh * hs:(nh + nkv) * hs].view(M, nkv, hs), sb[:, (nh + nkv) * hs:].view(M, nkv, hs)
    assert torch.equal(v, v0)
    a = ang[pos][:, None, :]
    for got, x in ((q, q0), (k, k0)):
        if mode == lr.ROPE_NONE:
            assert torch.equal(got, x)
        elif mode == lr.ROPE_INTERLEAVED:                  # pair (2i, 2i + 1) as the complex number x_2i + i x_2i+1, times e^(i angle_i)
            z = torch.view_as_complex(x.reshape(M, -1, hs // 2, 2).contiguous()) * torch.polar(torch.ones_like(a), a)
            _close(got, torch.view_as_real(z).reshape(M, -1, hs))
        else:                                              # pair (d, d + hs/2) likewise
            z = torch.complex(x[..., :hs // 2], x[..., hs // 2:]) * torch.polar(torch.ones_like(a), a)
            _close(got, torch.cat((z.real, z.imag), -1))


@pytest.mark.parametrize("dtype,K", [(BF16, 40), (F32, 20)])
@pytest.mark.parametrize("rope_hs", [0, 32])
def test_unpack_linear_vs_index_by_index_layout(dtype, K, rope_hs):
    """out[N/16][K/KC][64 lanes][EPL] written element by element from the header's statement of the layout (N = 20 without the
    rope permutation, N = 64 with it), decoded back."""
    N = 64 if rope_hs else 20
    KC, EPL = (32, 8) if dtype == BF16 else (16, 4)
    nt, nch = (N + 15) // 16, (K + KC - 1) // KC
    W = torch.arange(1, N * K + 1, dtype=F32).view(N, K)           # every element distinct (an fp32 container: the decoder only moves elements)
    packed = torch.zeros(nt * nch * 64 * EPL, dtype=F32)
    for tile in range(nt):
        for chunk in range(nch):
            for lane in range(64):
                for e in range(EPL):
                    n = tile * 16 + (lane & 15)
                    if rope_hs:                                    # packed column -> source row, as the header states it
                        h, within = divmod(n, rope_hs)
                        r, c = divmod(within, 16)
                        n = h * rope_hs + (r * 8 + c if c < 8 else rope_hs // 2 + r * 8 + (c - 8))
                    k = chunk * KC + (lane >> 4) * EPL + e
                    if n < N and k < K:
                        packed[((tile * nch + chunk) * 64 + lane) * EPL + e] = W[n, k]
    got = lr.unpack_linear(packed, dtype, N, K, rope_hs)
    assert got.shape == (nt * 16, nch * KC)
    assert torch.equal(got[:N, :K], W)
    assert float(got[N:].abs().sum()) == 0 and float(got[:, K:].abs().sum()) == 0
    if rope_hs:
        assert torch.equal(lr.rope_rows(64, 32)[:10], torch.tensor([0, 1, 2, 3, 4, 5, 6, 7, 16, 17]))


def test_unpack_operand_vs_index_by_index_layout():
    for dtype, KC, EPL in ((BF16, 32, 8), (F32, 16, 4)):
        M, K = 19, 2 * KC
        A = torch.arange(1, M * K + 1, dtype=F32).view(M, K)
        pk = torch.zeros(2 * (K // KC) * 64 * EPL)
        for m in range(M):
            for k in range(K):
                c, r = divmod(k, KC)
                g, e = divmod(r, EPL)
                pk[(((m >> 4) * (K // KC) + c) * 64 + g * 16 + (m & 15)) * EPL + e] = A[m, k]
        assert torch.equal(lr.unpack_operand(pk, dtype, M, K), A)


@pytest.mark.parametrize("norm_kind", [lr.NORM_RMS_LIT, lr.NORM_RMS_MOSHI, lr.NORM_LAYERNORM])
@pytest.mark.parametrize("K", lr.NORM_KS)
def test_flip_free_builder_on_every_gpu_input(K, norm_kind):
    """The builder finishes within its rounds on every UA2_PRO_NORM input of tests/test_gpu_linear_parity.py, leaves no candidate,
    and on its output the fp32 and the float64 evaluation of the operand are the same bf16 numbers bit for bit."""
    x, w, b, rec = lr.norm_inputs(K, norm_kind)
    print(f"FLIPFREE K={K} norm_kind={norm_kind} rows={x.shape[0]}: e_pro {rec['e_pro']:.2e} delta {rec['delta']:.2e} "
          f"rounds {rec['rounds']} nudged {rec['nudged']}")
    assert rec["rounds"] <= lr.MAX_ROUNDS and rec["delta"] >= 2.0 ** -20 and rec["delta"] >= 8 * rec["e_pro"]
    assert x.dtype == F32 and x.shape == (lr.norm_rows(K, norm_kind), K) and bool(torch.isfinite(x).all())
    assert int(lr.flip_candidates(x, lr.PRO_NORM, norm_kind, w, b, 1e-5, rec["delta"]).sum()) == 0
    a64 = lr.operand_ref(x, lr.PRO_NORM, norm_kind, w, b, 1e-5, BF16, F64)
    a32 = lr.operand_ref(x, lr.PRO_NORM, norm_kind, w, b, 1e-5, BF16, F32)
    assert torch.equal(a64, a32.to(F64))
    assert torch.equal(a64.to(BF16).to(F64), a64)                   # and they ARE bf16 numbers


def test_flip_free_builder_moves_a_planted_candidate():
    """An input built to sit on a midpoint is found and moved (the loop is not vacuous)."""
    K = 64
    w = torch.ones(K)
    x = torch.randn(3, K, generator=_g(5))
    for _ in range(20):                                             # fixed point: the planted element moves the row's rstd a little
        rstd = torch.rsqrt((x.to(F64) ** 2).mean(-1, keepdim=True) + 1e-5)
        x[1, 7] = float((1.0 + 2.0 ** -8) / rstd[1])                # operand = 1 + half a bf16 ulp, to fp32 accuracy
    assert bool(lr.flip_candidates(x, lr.PRO_NORM, lr.NORM_RMS_LIT, w, None, 1e-5, 2.0 ** -12)[1, 7])
    y, rec = lr.flip_free_inputs(x, lr.NORM_RMS_LIT, w, None, 1e-5)
    assert int(lr.flip_candidates(y, lr.PRO_NORM, lr.NORM_RMS_LIT, w, None, 1e-5, rec["delta"]).sum()) == 0
    assert 1 <= rec["rounds"] <= lr.MAX_ROUNDS and rec["nudged"] >= 1 and float(y[1, 7]) != float(x[1, 7])


# ---- references and judge of tests/test_gpu_gemm2_parity.py -------------------------------------------------------------------

GEMM2_KS = tuple(32 * c for c in (1, 2, 5, 7, 33, 48, 64))         # the K list of tests/test_gpu_gemm2_parity.py (restated there as CHUNKS)
LN_NS = (64, 1536, 2048)


def _ln_case(N):
    """y = the hostile rows (unit scale, mean 1e3 with std 1, the constant 2.5, scale 1e-3) and the issue's w = 1 + 0.2 randn,
    b = 0.2 randn, eps = 1e-6."""
    g = _g(N)
    return lr.hostile_rows(N, N), 1.0 + 0.2 * torch.randn(N, generator=g), 0.2 * torch.randn(N, generator=g), 1e-6


@pytest.mark.parametrize("N", LN_NS)
def test_ln_handover_ref_vs_torch(N):
    y, w, b, eps = _ln_case(N)
    _close(lr.ln_handover_ref(y, w, b, eps), F.layer_norm(y.to(F64), (N,), w.to(F64), b.to(F64), eps))
    assert torch.equal(lr.ln_handover_ref(y, w, b, eps)[2], b.to(F64))              # the constant row: exactly b
    assert lr.ln_handover_ref(y, w, b, eps, F32).dtype == F32
    assert torch.equal(y[2], torch.full((N,), 2.5)) and abs(float(y[1].mean()) - 1e3) < 1.0 and float(y[3].abs().max()) < 1e-2


def test_scaled_linear_ref_vs_torch():
    g = _g(3)
    M, K, N = 6, 64, 48
    op = torch.randn(M, K, generator=g).to(BF16)
    ssq = torch.rand(M, K // 16, generator=g) * 16
    W, W1, bias = torch.randn(N, K, generator=g) * K ** -0.5, torch.randn(N, K, generator=g) * K ** -0.5, torch.randn(N, generator=g)
    rs = torch.rsqrt(ssq.to(F64).sum(-1, keepdim=True) / K + 1e-5)
    _close(lr.scaled_rstd_ref(ssq, K, 1e-5), rs)
    lin, lin1 = rs * F.linear(op.to(F64), W.to(BF16).to(F64)), rs * F.linear(op.to(F64), W1.to(BF16).to(F64))
    _close(lr.scaled_linear_ref(op, ssq, W, eps=1e-5, bias=bias), lin + bias.to(F64))
    _close(lr.scaled_linear_ref(op, ssq, W, eps=1e-5, epi=lr.EPI_SWIGLU, W1=W1), F.silu(lin) * lin1)
    pos = torch.arange(M)
    ang = torch.rand(M, 8, generator=g, dtype=F64)
    qkv = dict(pos=pos, n_head=1, n_kv=1, hs=16, rope_mode=lr.ROPE_HALF_SPLIT, cos=ang.cos(), sin=ang.sin())
    got = lr.scaled_linear_ref(op, ssq, W, eps=1e-5, epi=lr.EPI_QKV_ROPE, qkv=qkv)
    want = lr.qkv_rope_ref(lin, pos, 1, 1, 16, lr.ROPE_HALF_SPLIT, ang.cos(), ang.sin())
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    y32 = lr.scaled_linear_ref(op, ssq, W, eps=1e-5, bias=bias, dt=F32)
    assert y32.dtype == F32 and float((y32.to(F64) - lin - bias.to(F64)).abs().max()) < 1e-5


def test_sample_rows():
    assert lr.sample_rows(4352, 256)[:4] == [0, 98, 255, 256] and len(lr.sample_rows(4352, 256)) == 51
    for M, block in ((4352, 256), (257, 256), (300, 128), (1, 256)):
        rows = lr.sample_rows(M, block)
        assert rows == sorted(set(rows)) and 0 <= rows[0] and rows[-1] == M - 1
        for r0 in range(0, M, block):                                # first, last and (where the block has three rows) one inside
            r1 = min(r0 + block, M) - 1
            inside = [r for r in rows if r0 < r < r1]
            assert r0 in rows and r1 in rows and (len(inside) == 1 or r1 - r0 < 2)


def _parity_judge(got, ref, ref32):
    """err, bar of tests/test_gpu_gemm2_parity.py's _judge (the rule of test_gpu_linear_parity.py)."""
    scale = max(1.0, float(ref.abs().max()))
    return float((got.to(F64) - ref).abs().max()) / scale, kr.bar(float((ref32.to(F64) - ref).abs().max()) / scale)


@pytest.mark.parametrize("K", GEMM2_KS)
def test_the_judge_rejects_a_dropped_chunk(K):
    """A kernel that loses the last chunk of its ring (the fault a wrong wait count or a wrong partial turn produces) is over the bar
    at every K of the GPU module's list, on that module's RESIDUAL shapes; the fp32 replay itself is under it."""
    g = _g(K)
    M, N = 300, 320
    x, W, resid = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5, torch.randn(M, N, generator=g)
    kw = dict(epi=lr.EPI_RESIDUAL, resid=resid)
    ref, ref32 = lr.linear_ref(x, W, BF16, dt=F64, **kw), lr.linear_ref(x, W, BF16, dt=F32, **kw)
    err, bar = _parity_judge(lr.linear_ref(x, W, BF16, dt=F32, drop_last_chunk=True, **kw), ref, ref32)
    assert err > bar, (K, err, bar)
    err, bar = _parity_judge(ref32, ref, ref32)
    assert err <= bar


@pytest.mark.parametrize("N", LN_NS)
def test_the_handover_condition_rejects_the_uncentred_variance(N):
    """var = mean(y^2) - mean^2 in fp32 on the hostile rows is over the LayerNorm hand-over condition (half a bf16 ulp of the value +
    the bar); the centred two-pass replay, rounded to bf16 as the kernel rounds, is under it."""
    y, w, b, eps = _ln_case(N)
    naive = kr.bf16_round(lr.ln_handover_naive32(y, w, b, eps))
    worst, e_ref, bar = lr.ln_handover_excess(naive, y, w, b, eps)
    print(f"HANDOVER N={N}: uncentred excess {worst:.3e} E_ref {e_ref:.3e} bar {bar:.3e}")
    assert worst > bar, (N, worst, bar)
    centred = kr.bf16_round(lr.ln_handover_ref(y, w, b, eps, F32))
    worst, _, bar = lr.ln_handover_excess(centred, y, w, b, eps)
    print(f"HANDOVER N={N}: centred excess {worst:.3e} bar {bar:.3e}")
    assert worst <= bar, (N, worst, bar)
    assert torch.equal(centred[2], kr.bf16_round(b))
