"""Plain restatements of ua2_linear (include/ua2hip.h) and of ua2_pack_linear's layout, used by tests/test_gpu_linear_parity.py.

Same convention as tests/kernel_refs.py: every helper takes `dt`.  torch.float64 is the reference; torch.float32 evaluates the
SAME formula in plain fp32 on the host, and its error against the float64 result is the E_ref that sizes a case's bar
(kr.bar).  tests/test_linear_refs_host.py pins each helper to the torch library function it restates.

The K sum of the float32 replay is an explicit legal order, chosen pessimistic: one partial sum per MFMA chunk (32 of K for
bf16, 16 for fp32), the chunks added left to right in ONE fp32 chain (the kernel adds at most 16 of them per chain and then the
chains), not whatever order the host BLAS happens to use.

bf16 operands and UA2_PRO_NORM.  The kernel rounds the normalised fp32 value to bf16; a float64 evaluation of the same formula
can land on the other side of a rounding midpoint, which moves one product by 2^-9 |x w| — two orders of magnitude above the
fp32 summation noise the bar is made of.  flip_free_inputs() removes the ambiguity from the INPUTS: it nudges every element
whose float64 operand lies within a band around a midpoint until none is left, so that every correct evaluation order rounds to
the same bf16 numbers and the comparison is about the sums again."""
import math

import numpy as np
import torch

import kernel_refs as kr

F64 = torch.float64
PRO_CAST, PRO_NORM = 0, 1
EPI_STORE, EPI_RESIDUAL, EPI_SWIGLU, EPI_QKV_ROPE, EPI_GELU = 0, 1, 2, 3, 4
NORM_RMS_LIT, NORM_RMS_MOSHI, NORM_LAYERNORM = 0, 1, 2
ROPE_HALF_SPLIT, ROPE_INTERLEAVED, ROPE_NONE = 0, 1, 2
ACT_DEFAULT, GELU_TANH, GATE_SIGMOID_SECOND = 0, 1, 2


def kc(dtype):
    """K per MFMA chunk."""
    return 32 if dtype == torch.bfloat16 else 16


def epl(dtype):
    """Elements per lane per chunk."""
    return 8 if dtype == torch.bfloat16 else 4


def rows_per_tile(dtype, K):
    """ua2_gemv_rows_per_tile (csrc/ua2_gemv.hip), restated: rows of the operand that fit a 112 KiB LDS tile, a row padded to
    whole chunks plus 16 bytes; 16 at the most."""
    c, b = kc(dtype), (2 if dtype == torch.bfloat16 else 4)
    row_bytes = ((K + c - 1) // c * c + 16 // b) * b
    return min(16, 112 * 1024 // row_bytes)


# ---- bf16 rounding of a float64 value ---------------------------------------------------------------------------------------

def _bf16_quantum(v):
    """Spacing of the bf16 numbers around |v| (8 significant bits; subnormal spacing 2^-133 below 2^-126)."""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -300))            # |v| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(v), (e - 8).clamp_min(-133))


def bf16_round64(v):
    """RNE to bf16 of a float64 tensor, directly (not through fp32: no double rounding), as float64."""
    v = v.to(F64)
    q = _bf16_quantum(v)
    return torch.round(v / q) * q                                  # torch.round: halves to even; v / q and the product are exact


def midpoint_distance(v):
    """|v - the midpoint of the two bf16 neighbours enclosing v|, float64."""
    v = v.to(F64)
    q = _bf16_quantum(v)
    a = v.abs()
    return (a - (torch.floor(a / q) * q + 0.5 * q)).abs()


# ---- operand ----------------------------------------------------------------------------------------------------------------

def _prologue(x, pro, norm_kind, norm_w, norm_b, eps, dt):
    """(n, mag): the operand before any rounding to the operand dtype, and the magnitude its fp32 evaluation errors scale with:
    |n| itself, except for LayerNorm, where both the difference x - mean and the sum with the bias may cancel:
    (|x| + |mean|) rstd |w| + |b|."""
    x = x.to(dt)
    if pro == PRO_CAST:
        return x, x.abs()
    w = norm_w.to(dt)
    if norm_kind == NORM_LAYERNORM:
        mean = x.mean(-1, keepdim=True)
        d = x - mean
        rstd = torch.rsqrt((d * d).mean(-1, keepdim=True) + eps)   # centred variance, as kr.layernorm_ref
        t = d * rstd * w
        b = norm_b.to(dt)
        return t + b, (x.abs() + mean.abs()) * rstd * w.abs() + b.abs()
    rstd = torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
    n = (x * rstd) * w if norm_kind == NORM_RMS_LIT else x * (w * rstd)
    return n, n.abs()


def operand_ref(x, pro, norm_kind, norm_w, norm_b, eps, dtype, dt=F64):
    """The A operand of the GEMM, [M, K] in `dt`: UA2_PRO_CAST x as is; UA2_PRO_NORM one of
    RMS_LIT (x rstd) w, RMS_MOSHI x (w rstd), rstd = rsqrt(mean(x^2) + eps); LAYERNORM (x - mean) rstd w + b with
    rstd = rsqrt(mean((x - mean)^2) + eps); then RNE to bf16 where the operand dtype is bf16."""
    n, _ = _prologue(x, pro, norm_kind, norm_w, norm_b, eps, dt)
    if dtype != torch.bfloat16:
        return n
    return bf16_round64(n) if dt == F64 else kr.bf16_round(n).to(dt)


def flip_candidates(x, pro, norm_kind, norm_w, norm_b, eps, delta):
    """Boolean [M, K]: elements whose float64 operand lies within delta * mag of a bf16 rounding midpoint."""
    n, mag = _prologue(x, pro, norm_kind, norm_w, norm_b, eps, F64)
    return midpoint_distance(n) <= delta * mag


def prologue_error(x, pro, norm_kind, norm_w, norm_b, eps):
    """e_pro: max error of the fp32 replay of the prologue against float64, relative to the element's magnitude."""
    n, mag = _prologue(x, pro, norm_kind, norm_w, norm_b, eps, F64)
    n32, _ = _prologue(x, pro, norm_kind, norm_w, norm_b, eps, torch.float32)
    return float(((n32.to(F64) - n).abs() / mag.clamp_min(1e-300)).max())


MAX_ROUNDS = 8


def flip_free_inputs(x, norm_kind, norm_w, norm_b, eps):
    """x' (fp32, a copy of x nudged in a few places) whose UA2_PRO_NORM operand has no flip candidate, and a record
    dict(delta, rounds, e_pro, nudged).  delta = max(2^-20, 8 e_pro): 8 x the measured error of one fp32 evaluation order, for
    the kernel's different but equally short one.  A candidate is moved by 4 delta of its magnitude (for the RMS flavours:
    x (1 + 4 delta)), which changes the row's rstd by about 4 delta / K — far inside the band; the loop re-evaluates everything
    and must finish within MAX_ROUNDS.  Where the bf16 spacing at the operand is itself only a few bands wide (a LayerNorm term
    and its bias cancelling to almost nothing: every value there is near a midpoint) a nudge of that size lands on the next
    midpoint, so x is set for the operand to land ON a bf16 number instead: the nearest one, or, where the spacing is below 4
    bands, the one of magnitude 2^11 delta mag (spacing 8 bands).  These moves are as small as they can be because each shifts
    the row's mean, and with it every other element of the row, by 1 / K of itself."""
    x = x.detach().clone().float()
    nudged = 0
    for rounds in range(MAX_ROUNDS + 1):
        e_pro = prologue_error(x, PRO_NORM, norm_kind, norm_w, norm_b, eps)
        delta = max(2.0 ** -20, 8.0 * e_pro)
        cand = flip_candidates(x, PRO_NORM, norm_kind, norm_w, norm_b, eps, delta)
        if not bool(cand.any()):
            return x, dict(delta=delta, rounds=rounds, e_pro=e_pro, nudged=nudged)
        assert rounds < MAX_ROUNDS, f"flip-free builder: {int(cand.sum())} candidates left after {MAX_ROUNDS} rounds"
        nudged += int(cand.sum())
        x64 = x.to(F64)
        n, mag = _prologue(x, PRO_NORM, norm_kind, norm_w, norm_b, eps, F64)
        d = x64 - x64.mean(-1, keepdim=True) if norm_kind == NORM_LAYERNORM else x64
        slope = torch.rsqrt((d * d).mean(-1, keepdim=True) + eps) * norm_w.to(F64)       # dn / dx, the row statistics held
        slope = torch.where(slope.abs() < 1e-300, torch.full_like(slope, 1e-300), slope)
        away = torch.where(n >= 0, 1.0, -1.0)
        q, band = _bf16_quantum(n), delta * mag
        target = torch.where(q >= 64.0 * band, n + away * 4.0 * band,                          # the plain nudge: 4 bands further out
                             torch.where(q >= 4.0 * band, bf16_round64(n),                     # spacing of a few bands: onto the nearest bf16 number
                                         bf16_round64(away * 2.0 ** 11 * band)))               # narrower still: out to where it is 8 bands
        x = torch.where(cand, x64 + (target - n) / slope, x64).float()
    raise AssertionError("unreachable")


# ---- weights, K sum ---------------------------------------------------------------------------------------------------------

def weights_ref(W, dtype, dt=F64):
    """The weight the kernel computes with: W.to(bfloat16) for bf16 plans, W itself for fp32."""
    return (W.to(torch.bfloat16) if dtype == torch.bfloat16 else W.float()).to(dt)


def ksum_ref(a, w, dtype, dt=F64):
    """a [M, K] w [N, K] -> a w^T [M, N].  float64: a matmul.  float32: per-chunk partial sums, one left-to-right chain."""
    if dt == F64:
        return a.to(F64) @ w.to(F64).t()
    a, w = a.float(), w.float()
    c, K = kc(dtype), a.shape[1]
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    for k0 in range(0, K, c):
        acc = acc + a[:, k0:k0 + c] @ w[:, k0:k0 + c].t()
    return acc


# ---- epilogues --------------------------------------------------------------------------------------------------------------

def silu_ref(v):
    return v / (1.0 + torch.exp(-v))


def sigmoid_ref(v):
    return 1.0 / (1.0 + torch.exp(-v))


def gelu_ref(v, tanh_form=False):
    if tanh_form:
        return 0.5 * v * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v * v * v)))
    return 0.5 * v * (1.0 + torch.erf(v * math.sqrt(0.5)))


def _opt(t, dt):
    return None if t is None else t.to(dt)


def store_ref(s, bias=None, dt=F64):
    s, bias = s.to(dt), _opt(bias, dt)
    return s if bias is None else s + bias


def residual_ref(s, resid, bias=None, out_scale=None, dt=F64):
    """resid + out_scale (s + bias)."""
    v = store_ref(s, bias, dt)
    if out_scale is not None:
        v = out_scale.to(dt) * v
    return v + resid.to(dt)


def swiglu_ref(s0, s1, bias=None, bias1=None, act_kind=ACT_DEFAULT, dt=F64):
    """default: silu(s0 + b0) (s1 + b1); UA2_GATE_SIGMOID_SECOND: (s0 + b0) sigmoid(s1 + b1)."""
    v0, v1 = store_ref(s0, bias, dt), store_ref(s1, bias1, dt)
    return v0 * sigmoid_ref(v1) if act_kind == GATE_SIGMOID_SECOND else silu_ref(v0) * v1


def gelu_epi_ref(s, bias=None, act_kind=ACT_DEFAULT, dt=F64):
    return gelu_ref(store_ref(s, bias, dt), act_kind == GELU_TANH)


def rope_interleaved(x, c, s):
    """Adjacent pairs (2i, 2i + 1) rotated by angle i: (xr c - xi s, xr s + xi c).  x [..., hs]; c, s [..., hs / 2]."""
    xr, xi = x[..., 0::2], x[..., 1::2]
    return torch.stack((xr * c - xi * s, xr * s + xi * c), dim=-1).flatten(-2)


def rope_half_split(x, c, s):
    """x cat(c, c) + rotate_half(x) cat(s, s)."""
    return x * torch.cat((c, c), -1) + kr.rotate_half(x) * torch.cat((s, s), -1)


def qkv_rope_ref(s, pos, n_head, n_kv, hs, rope_mode, cos=None, sin=None, bias=None, dt=F64):
    """s [M, (n_head + 2 n_kv) hs] = x W^T with W in SOURCE row order (q heads | k heads | v heads): bias, split, rotation of q and
    k by the row's position -> q [M, n_head, hs], k, v [M, n_kv, hs] (the k / v rows the cache must hold at the row's slot)."""
    v = store_ref(s, bias, dt)
    M = v.shape[0]
    q, k, vv = v.split((n_head * hs, n_kv * hs, n_kv * hs), dim=-1)
    q, k, vv = q.reshape(M, n_head, hs), k.reshape(M, n_kv, hs), vv.reshape(M, n_kv, hs)
    if rope_mode != ROPE_NONE:
        p = torch.as_tensor(pos).long()
        c, sn = cos[p].to(dt)[:, None, :], sin[p].to(dt)[:, None, :]
        rot = rope_half_split if rope_mode == ROPE_HALF_SPLIT else rope_interleaved
        q, k = rot(q, c, sn), rot(k, c, sn)
    return q, k, vv


def half_ulp_bf16(v):
    """Half the spacing of the bf16 numbers at |v| (float64): what one RNE rounding of a value near v may add."""
    return 0.5 * _bf16_quantum(v.to(F64))


# ---- hand-overs of the order-free kernel (include/ua2hip.h y_ln_w, y_norm_w / UA2_PRO_SCALED) -----------------------------------

def ln_handover_ref(y, w, b, eps, dt=F64):
    """The LayerNorm hand-over before its rounding to bf16: (y - mean) rstd w + b over the columns of y, the two-pass centred form
    (kr.layernorm_ref) in `dt`."""
    return kr.layernorm_ref(y, w, b, eps, dt)


def ln_handover_naive32(y, w, b, eps):
    """The formula the hand-over must NOT use, replayed in fp32: var = mean(y^2) - mean^2, which loses the variance's digits once
    |mean| >> std.  For checking that the hand-over condition notices it."""
    y, w = y.float(), w.float()
    n = y.shape[-1]
    mean = y.sum(-1, keepdim=True) / n
    var = ((y * y).sum(-1, keepdim=True) / n - mean * mean).clamp_min(0.0)
    out = (y - mean) * (1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32))) * w
    return out if b is None else out + b.float()


def ln_handover_excess(got, y, w, b, eps):
    """The hand-over's pass condition on `got` [M, N] (the bf16 values a launch wrote, or any candidate): per element
    |got - ref| <= half_ulp_bf16(ref) + B, ref = the float64 LayerNorm of y (the launch's OWN fp32 y), B = kr.bar(E_ref) scale,
    scale = max(1, max |ref|), E_ref = error of the fp32 replay of the same two-pass formula / scale.
    Returns (worst, e_ref, bar): worst = max over the elements of (|got - ref| - half_ulp_bf16(ref)) / scale, to be <= bar."""
    ref = ln_handover_ref(y, w, b, eps, F64)
    ref32 = ln_handover_ref(y, w, b, eps, torch.float32).to(F64)
    scale = max(1.0, float(ref.abs().max()))
    e_ref = float((ref32 - ref).abs().max()) / scale
    d = (got.to(F64) - ref).abs() - half_ulp_bf16(ref)
    return float(d.max()) / scale, e_ref, kr.bar(e_ref)


def hostile_rows(N, seed):
    """The four hostile rows of the LayerNorm cases [4, N] fp32: unit scale, mean 1e3 with std 1, the constant 2.5, scale 1e-3."""
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(4, N, generator=g)
    r[1] += 1e3
    r[2] = 2.5
    r[3] *= 1e-3
    return r


def scaled_rstd_ref(ssq, K, eps, dt=F64):
    """UA2_PRO_SCALED: the row scale rsqrt(sum_j ssq[m][j] / K + eps) from the producer's per-16-column sums of squares."""
    return torch.rsqrt(ssq.to(dt).sum(-1, keepdim=True) / K + eps)


def scaled_linear_ref(op, ssq, W, *, eps, epi=EPI_STORE, W1=None, bias=None, bias1=None, act_kind=0, qkv=None, dt=F64):
    """A UA2_PRO_SCALED launch: y = epilogue(rstd[m] (op W^T)), op [M, K] = the bf16 operand the producer wrote (taken as it is:
    the reference is built from the producer's bits), rstd from its ssq [M, K / 16]."""
    a = op.to(dt)
    rs = scaled_rstd_ref(ssq, a.shape[1], eps, dt)
    s = rs * ksum_ref(a, weights_ref(W, torch.bfloat16, dt), torch.bfloat16, dt)
    if epi == EPI_STORE:
        return store_ref(s, bias, dt)
    if epi == EPI_SWIGLU:
        return swiglu_ref(s, rs * ksum_ref(a, weights_ref(W1, torch.bfloat16, dt), torch.bfloat16, dt), bias, bias1, act_kind, dt)
    assert epi == EPI_QKV_ROPE
    return qkv_rope_ref(s, qkv["pos"], qkv["n_head"], qkv["n_kv"], qkv["hs"], qkv["rope_mode"], qkv.get("cos"), qkv.get("sin"), bias, dt)


def sample_rows(M, block=256):
    """Three rows of every `block`-row tile of an M-row launch — first, last and one inside — sorted, without repeats: rows are
    independent, so a reference over these rows and all columns reaches every tile of the grid."""
    rows = set()
    for r0 in range(0, M, block):
        r1 = min(r0 + block, M) - 1
        rows.update((r0, r1, r0 + (r1 - r0) * 5 // 13))
    return sorted(rows)


# ---- pack layout ------------------------------------------------------------------------------------------------------------

def rope_rows(n, hs):
    """Inverse view of the pack's row permutation: result[src_row] = packed column holding it.  Packed column p of a head holds
    source row r * 8 + c (c < 8) or hs / 2 + r * 8 + (c - 8), r = (p % hs) // 16, c = p % 16."""
    packed = torch.arange(n)
    h, within = packed // hs, packed % hs
    r, c = within // 16, within % 16
    src = h * hs + torch.where(c < 8, r * 8 + c, hs // 2 + r * 8 + (c - 8))
    inv = torch.empty(n, dtype=torch.long)
    inv[src] = packed
    return inv


def unpack_linear(packed, dtype, N, K, rope_hs=0):
    """[N/16][K/KC][64 lanes][EPL] (lane -> column lane & 15, k-group lane >> 4, k = chunk KC + g EPL + e) -> [N16, Kpad] in SOURCE
    row order (rows past N and columns past K are the pack's padding)."""
    c, e = kc(dtype), epl(dtype)
    nt, nch = (N + 15) // 16, (K + c - 1) // c
    t = packed.detach().cpu().reshape(nt, nch, 4, 16, e)            # [tile][chunk][g][col][e]
    rows = t.permute(0, 3, 1, 2, 4).reshape(nt * 16, nch * c)        # packed column order
    if rope_hs > 0:
        assert N % rope_hs == 0
        rows = rows[rope_rows(nt * 16, rope_hs)]
    return rows


def unpack_operand(pk, dtype, M, K):
    """The packed A operand [ceil(M/16)][K/KC][64 lanes][EPL] (element (m, k): chunk k // KC, lane (k % KC) // EPL * 16 + m % 16)
    -> [M, K]."""
    c, e = kc(dtype), epl(dtype)
    return pk.detach().cpu().reshape((M + 15) // 16, K // c, c // e, 16, e).permute(0, 3, 1, 2, 4).reshape(-1, K)[:M]


# ---- a whole launch ---------------------------------------------------------------------------------------------------------

def linear_ref(x, W, dtype, *, pro=PRO_CAST, epi=EPI_STORE, norm_kind=0, norm_w=None, norm_b=None, eps=1e-5, W1=None, bias=None,
               bias1=None, resid=None, out_scale=None, act_kind=0, qkv=None, dt=F64, drop_last_chunk=False):
    """ua2_linear on the host in `dt`.  qkv = dict(pos, n_head, n_kv, hs, rope_mode, cos, sin) for UA2_EPI_QKV_ROPE, which returns
    (q, k, v); every other epilogue returns y [M, N].  drop_last_chunk: a deliberately wrong K sum, for checking that the tests
    notice one."""
    a = operand_ref(x, pro, norm_kind, norm_w, norm_b, eps, dtype, dt)
    if drop_last_chunk:
        a = a.clone()
        a[:, (a.shape[1] - 1) // kc(dtype) * kc(dtype):] = 0
    s = ksum_ref(a, weights_ref(W, dtype, dt), dtype, dt)
    if epi == EPI_STORE:
        return store_ref(s, bias, dt)
    if epi == EPI_RESIDUAL:
        return residual_ref(s, resid, bias, out_scale, dt)
    if epi == EPI_SWIGLU:
        return swiglu_ref(s, ksum_ref(a, weights_ref(W1, dtype, dt), dtype, dt), bias, bias1, act_kind, dt)
    if epi == EPI_GELU:
        return gelu_epi_ref(s, bias, act_kind, dt)
    return qkv_rope_ref(s, qkv["pos"], qkv["n_head"], qkv["n_kv"], qkv["hs"], qkv["rope_mode"], qkv.get("cos"), qkv.get("sin"), bias, dt)


# ---- the inputs of the UA2_PRO_NORM cases -----------------------------------------------------------------------------------

NORM_KS = (72, 144, 1056, 1536, 2048, 3072, 4104, 6144, 8192)     # every K at which the GPU parity modules run UA2_PRO_NORM
ROW_SCALES = (1.0, 1e-3, 1e3)
_norm_cache = {}


def norm_rows(K, norm_kind):
    """Rows of the NORM input at width K: one more than the bf16 row tile (300 for RMS_LIT at K = 2048 and LayerNorm at K = 1536:
    the many-row cases)."""
    many = (K == 2048 and norm_kind == NORM_RMS_LIT) or (K == 1536 and norm_kind == NORM_LAYERNORM)
    return 300 if many else rows_per_tile(torch.bfloat16, K) + 1


def norm_inputs(K, norm_kind, eps=1e-5):
    """(x, norm_w, norm_b, record): the flip-free input rows of every UA2_PRO_NORM case at width K (rows scaled 1, 1e-3, 1e3 in
    turn), norm_w = 1 + 0.1 randn, norm_b = 0.1 randn (LayerNorm only, else None).  Deterministic; built once per process."""
    key = (K, norm_kind, eps)
    if key not in _norm_cache:
        assert K in NORM_KS and norm_kind in (NORM_RMS_LIT, NORM_RMS_MOSHI, NORM_LAYERNORM)
        g = torch.Generator().manual_seed(100003 * norm_kind + K)
        M = norm_rows(K, norm_kind)
        x = torch.randn(M, K, generator=g) * torch.tensor([ROW_SCALES[m % 3] for m in range(M)])[:, None]
        w = 1.0 + 0.1 * torch.randn(K, generator=g)
        b = 0.1 * torch.randn(K, generator=g) if norm_kind == NORM_LAYERNORM else None
        x, rec = flip_free_inputs(x, norm_kind, w, b, eps)
        _norm_cache[key] = (x, w, b, rec)
    return _norm_cache[key]
