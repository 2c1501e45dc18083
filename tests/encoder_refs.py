"""Plain restatements of the WavLM and BEST-RQ encoder kernels (csrc/ua2_wavlm.hip, ua2_conv2d.hip, ua2_bestrq.hip), used by
tests/test_encoder_refs_host.py and tests/test_gpu_encoder_parity.py, in the manner of kernel_refs.py / conv_refs.py.

Every helper takes `dt`: torch.float64 is the reference a kernel is compared with; torch.float32 evaluates the SAME formula in fp32
on the host, and its error against the float64 result (`E_ref`) sizes the bar kr.bar(E_ref, scale).  The `*_replay` helpers are
the fp32 evaluation in the kernel's documented reduction order (one partial sum per matrix-pipe step of 4 channels, all of them in
one chain; conv0: the contract of include/ua2hip.h), the pessimistic legal order conv_refs._chain uses for ua2_conv1d.  None of
the float64 helpers calls the torch library function it restates: tests/test_encoder_refs_host.py pins each to that function.

relbias_flash_model is no reference but the arithmetic contract of attn_relbias_flash_kernel on top of kr.attn_flash_model (16-bit
q and weights, one 64-key page per step, the bias added in the log2 domain); its error against relbias_attn_ref sizes the bf16 bars."""
import numpy as np
import torch

import kernel_refs as kr
import wavlm_ref as wr

F64 = torch.float64
F32 = torch.float32
LOG2E = 1.44269504088896340736
MEL_FLOOR = float(np.float32(1e-10))          # the kernel's threshold: p <= 1e-10f gives -100 exactly


# ---- ua2_attn_relbias ---------------------------------------------------------------------------------------------------------

def table_index(keys, q_pos, tab_half):
    """[r, l] index into a table row: clamp(key - q_pos + tab_half, 0, 2 tab_half)."""
    return (keys[None, :].long() - torch.as_tensor(q_pos).long()[:, None] + tab_half).clamp(0, 2 * tab_half)


def relbias_score_bias(q_pos, gate, tab, tab_half, dt, index=table_index, head_shift=0, row_shift=0):
    """score_bias hook of kr.attn_ref: gate[r, h] * tab[h][index(key, q_pos[r])] as [r, H, 1, l] in `dt`.  index, head_shift (the
    table row of head h + shift) and row_shift (the gate of row r + shift) are the hooks of the deliberately wrong models."""
    q_pos, gate, tab = torch.as_tensor(q_pos), gate.to(dt), tab.to(dt)
    H = tab.shape[0]

    def bias(rows, keys):
        rows = torch.as_tensor(rows)
        idx = index(keys, q_pos[rows], tab_half)                                       # [r, l]
        t = tab.roll(-head_shift, 0)[:, idx].permute(1, 0, 2)                          # [r, H, l]
        g = gate[(rows + row_shift) % gate.shape[0]]
        return (g[:, :, None] * t)[:, :, None, :]
    return bias


def relbias_attn_ref(q, K, V, pos, seq, q_pos, gate, tab, tab_half, n_head, dt=F64, **wrong):
    """softmax(q k^T + gate[r, h] * tab[h][clamp(key - q_pos[r] + tab_half, 0, 2 tab_half)]) v over keys 0 .. pos[r] of the row's
    sequence; q [R, n_head * hs] arrives scaled by hs^-0.5; K, V per sequence [L, n_head, hs] as stored; gate [R, n_head];
    tab [n_head, 2 tab_half + 1]."""
    assert tab.shape == (n_head, 2 * tab_half + 1)
    return kr.attn_ref(q, K, V, pos, seq, n_head, n_head, dt=dt, q_prescaled=True,
                       score_bias=relbias_score_bias(q_pos, gate, tab, tab_half, dt, **wrong))


def relbias_flash_model(q, K, V, pos, seq, q_pos, gate, tab, tab_half, n_head, mode="split", keys_per_step=64, score_dt=F32, gate_log2e=True,
                        **wrong):
    """attn_relbias_flash_kernel's contract: q RN(q log2 e) split by `mode`; g2 = RN(gate log2 e); score = RN(s + RN(g2 tab));
    blocked exp2 softmax over one page per step; weights split by `mode`.  gate_log2e = False: the wrong model whose gate stays
    in natural units."""
    g2 = gate.float() * torch.tensor(LOG2E, dtype=F32) if gate_log2e else gate.float()
    return kr.attn_flash_model(q, K, V, pos, seq, n_head, n_head, mode, keys_per_step, score_dt, q_prescaled=True,
                               score_bias=relbias_score_bias(q_pos, g2, tab.float(), tab_half, F32, **wrong)).to(F64)


# ---- ua2_relpos_gate ----------------------------------------------------------------------------------------------------------

def gate_ref(h, w, b, c, n_head, dt=F64):
    return wr.gate_ref(h.to(dt), w.to(dt), b.to(dt), c.to(dt), n_head)


# ---- ua2_wavlm_conv0 ----------------------------------------------------------------------------------------------------------

def conv0_ref(x, w, gn_w, gn_b, stride, eps=1e-5, dt=F64):
    """x [B, N], w [C, K] -> [B, T0, C]: y[b][t][c] = GELU((v - mean) / sqrt(var + eps) * gn_w[c] + gn_b[c]), v = sum_k w[c][k]
    x[b][t stride + k], mean / var (biased) over t per (clip, channel).  Taps added one by one, ascending."""
    x, w = x.to(dt), w.to(dt)
    fr = x.unfold(1, w.shape[1], stride)                                              # [B, T0, K]
    v = torch.zeros(fr.shape[0], fr.shape[1], w.shape[0], dtype=dt)
    for k in range(w.shape[1]):
        v = v + fr[:, :, k:k + 1] * w[None, None, :, k]
    mean = v.mean(1, keepdim=True)
    var = ((v - mean) ** 2).mean(1, keepdim=True)
    return wr.gelu((v - mean) / torch.sqrt(var + eps) * gn_w.to(dt) + gn_b.to(dt))


def conv0_replay(x, w, gn_w, gn_b, stride, eps=1e-5):
    """The contract of include/ua2hip.h in fp32: the conv as ONE fp32 fma chain over the taps ascending (the product is exact in
    float64, so RN32(float64(w x) + acc) is the fma up to a double rounding); sum and sum of squares of those fp32 values in
    double; mean and 1 / sqrt(var + eps) rounded to fp32; (v - mean) rstd gn_w + gn_b with single roundings; erf-GELU."""
    x, w = x.float(), w.float()
    fr = x.unfold(1, w.shape[1], stride).to(F64)
    v = torch.zeros(fr.shape[0], fr.shape[1], w.shape[0], dtype=F32)
    for k in range(w.shape[1]):
        v = (fr[:, :, k:k + 1] * w.to(F64)[None, None, :, k] + v.to(F64)).float()
    T0 = v.shape[1]
    v64 = v.to(F64)
    mean = v64.sum(1, keepdim=True) / T0
    var = ((v64 * v64).sum(1, keepdim=True) / T0 - mean * mean).clamp(min=0.0)
    mean32, rstd32 = mean.float(), (1.0 / torch.sqrt(var + float(np.float32(eps)))).float()
    n = (v - mean32) * rstd32 * gn_w.float() + gn_b.float()
    return (0.5 * n) * (1.0 + torch.erf(n * torch.tensor(0.70710678118654752440, dtype=F32)))


# ---- ua2_conv1d_grouped ---------------------------------------------------------------------------------------------------------

def _gconv(x, w, bias, groups, act, resid, dt, cb):
    B, T, C = x.shape
    Cg, K = w.shape[1], w.shape[2]
    pad = K // 2
    xg = x.to(dt).view(B, T, groups, Cg).permute(0, 2, 3, 1)                         # [B, g, Cg, T]
    wg = w.to(dt).view(groups, Cg, Cg, K)                                            # [g, n, c, K]
    t = torch.arange(T)
    acc = torch.zeros(B, groups, Cg, T, dtype=dt)
    for j in range(K):
        ti = t + j - pad
        ok = ((ti >= 0) & (ti < T)).to(dt)
        xt = xg[..., ti.clamp(0, T - 1)] * ok
        for c0 in range(0, Cg, cb or Cg):
            acc = acc + torch.einsum("gnc,bgct->bgnt", wg[:, :, c0:c0 + (cb or Cg), j], xt[:, :, c0:c0 + (cb or Cg)])
    y = acc.permute(0, 3, 1, 2).reshape(B, T, C)
    if bias is not None:
        y = y + bias.to(dt)
    if act:
        y = wr.gelu(y)
    return y + resid.to(dt) if resid is not None else y


def grouped_conv_ref(x, w, bias, groups, act, resid, dt=F64):
    """x [B, T, C], w [C, C / groups, K] -> resid + act(bias + sum_{j, ci} w[co][ci][j] x[b][t + j - K // 2][group(co) Cg + ci]), zero
    outside [0, T): an index gather per tap (not F.conv1d, which the host test compares it with)."""
    return _gconv(x, w, bias, groups, act, resid, dt, None)


def grouped_conv_replay(x, w, bias, groups, act, resid):
    """fp32 in gconv_kernel's reduction order (tap, channel in the group), one partial sum per matrix-pipe step of 4 channels, all
    of them in one chain; bias, erf-GELU and the residual with single roundings."""
    return _gconv(x, w, bias, groups, act, resid, F32, 4)


# ---- ua2_conv2d -------------------------------------------------------------------------------------------------------------

def _conv2d(x, w, bias, stride, residual, relu, dt, order):
    B, Cin, Fq, T = x.shape
    Cout = w.shape[0]
    sf, st = stride
    Fo, To = (Fq - 1) // sf + 1, (T - 1) // st + 1
    xp = torch.zeros(B, Cin, Fq + 2, T + 2, dtype=dt)
    xp[:, :, 1:-1, 1:-1] = x.to(dt)
    w = w.to(dt)
    win = lambda kf, kt: xp[:, :, kf:kf + (Fo - 1) * sf + 1:sf, kt:kt + (To - 1) * st + 1:st]   # [B, Cin, Fo, To]
    acc = torch.zeros(B, Cout, Fo, To, dtype=dt)
    if order == "plain":                                 # tap by tap, all channels at once
        steps = [(slice(0, Cin), kf, kt) for kf in range(3) for kt in range(3)]
    elif order == "small":                               # conv2d_small_kernel: (ci, kf, kt) ascending, one term per step
        steps = [(slice(ci, ci + 1), kf, kt) for ci in range(Cin) for kf in range(3) for kt in range(3)]
    else:                                                # conv2d_kernel: (group of 16 channels, tap, 4 channels of the group)
        steps = [(slice(c0 + c4, min(c0 + c4 + 4, Cin)), kf, kt) for c0 in range(0, Cin, 16) for kf in range(3) for kt in range(3)
                 for c4 in range(0, 16, 4) if c0 + c4 < Cin]
    for cs, kf, kt in steps:
        acc = acc + torch.einsum("nc,bcft->bnft", w[:, cs, kf, kt], win(kf, kt)[:, cs])
    if bias is not None:
        acc = acc + bias.to(dt)[None, :, None, None]
    if residual is not None:
        acc = acc + residual.to(dt)
    return torch.relu(acc) if relu else acc


def conv2d_ref(x, w, bias, stride, residual=None, relu=False, dt=F64):
    """relu?(bias[co] + sum_{ci, kf, kt} W[co][ci][kf][kt] x[b][ci][fo s_f + kf - 1][to s_t + kt - 1] (+ residual)), zero outside:
    strided windows of the zero-padded input, tap by tap (not F.conv2d)."""
    return _conv2d(x, w, bias, stride, residual, relu, dt, "plain")


def conv2d_replay(x, w, bias, stride, residual=None, relu=False, small_cin=4):
    """fp32 in the kernels' reduction order: Cin <= 4 the chain over (ci, kf, kt); else (group of 16 channels, tap, channel in the
    group) with one partial sum per matrix-pipe step of 4 channels, all in one chain."""
    return _conv2d(x, w, bias, stride, residual, relu, F32, "small" if x.shape[1] <= small_cin else "mfma")


# ---- ua2_layernorm_rope_rows ----------------------------------------------------------------------------------------------------

def rotate_half_wrong(x):
    """The sign on the wrong half: a deliberately wrong model."""
    x1, x2 = x[..., :x.shape[-1] // 2], x[..., x.shape[-1] // 2:]
    return torch.cat((x2, -x1), dim=-1)


def layernorm_rope_ref(x, w, b, eps, cos, sin, row_pos, hs, dt=F64, rotate=kr.rotate_half):
    """x [R, C] -> [R, 2 C] = [n cos + rotate_half(n) sin per head of hs | n], n = LayerNorm(x); cos / sin [n_pos, hs] rows picked
    by row_pos clamped into the table."""
    R, C = x.shape
    n = kr.layernorm_ref(x, w, b, eps, dt)
    p = torch.as_tensor(row_pos).long().clamp(0, cos.shape[0] - 1)
    c, s = cos.to(dt)[p][:, None, :], sin.to(dt)[p][:, None, :]
    nh = n.view(R, C // hs, hs)
    return torch.cat(((nh * c + rotate(nh) * s).reshape(R, C), n), 1)


# ---- ua2_melspec_db -------------------------------------------------------------------------------------------------------------

def melspec_db_ref(spec, fb, B, T, n_bins, mean, std, dt=F64, split=None):
    """spec [B T, ld] = (re | im | unused) -> [B, n_mels, T]: p = re^2 + im^2; the filter bank as two chains per mel split at
    n_bins // 2, low half first, bins ascending; 10 log10(max(p, 1e-10)) (the floor is -100 exactly); (db - mean) / std."""
    split = n_bins // 2 if split is None else split
    re, im = spec[:, :n_bins].to(dt), spec[:, n_bins:2 * n_bins].to(dt)
    pw = re * re + im * im
    fb = fb.to(dt)
    halves = []
    for k0, k1 in ((0, split), (split, n_bins)):
        acc = torch.zeros(spec.shape[0], fb.shape[1], dtype=dt)
        for k in range(k0, k1):
            acc = acc + pw[:, k:k + 1] * fb[k]
        halves.append(acc)
    p = halves[0] + halves[1]
    db = torch.where(p <= MEL_FLOOR, torch.full_like(p, -100.0), 10.0 * torch.log10(p.clamp(min=MEL_FLOOR)))
    out = (db - torch.tensor(mean, dtype=F32).to(dt)) / torch.tensor(std, dtype=F32).to(dt)
    return out.view(B, T, -1).transpose(1, 2).contiguous()


# ---- inputs and assertions shared by tests/test_encoder_refs_host.py (CPU) and tests/test_gpu_encoder_parity.py --------------------
LOUD = 3.0e4                                   # stale cache slots: loud, finite
RAGGED = {64: (3, [1, 7, 33, 64, 65, 130]), 128: (2, [1, 17, 70, 129])}      # head size -> (heads, sequence lengths)
DENSE = {64: (2, 1500), 128: (2, 300)}                                        # head size -> (heads, T)
HOSTILE_LENS = [3, 40, 130]
HOSTILE_KINDS = ["peaked_q", "dominant_key-k64", "wide_v", "rising_max", "bias_dominant"]


class RelbiasBatch:
    """One launch of ua2_attn_relbias on the host: a paged cache of `dtype` (scattered pages, two spare ones, stale slots 3e4), the
    values it stores, pre-scaled q, gate in (1, 2.5), an order-1 table, shuffled rows; the float64 reference, its fp32 replay and
    the flash model are evaluated once and shared.  dense: every row at pos = L - 1 with q_pos = its own position (the encoder's
    use); else row_pos = q_pos = the row's position (the causal use)."""

    def __init__(self, lens, H, hs, dtype, dense=False, kind="randn", seed=0):
        g = torch.Generator().manual_seed(1000 * hs + 10 * H + seed)
        self.lens, self.H, self.hs, self.dtype, self.dense, self.kind = list(lens), H, hs, dtype, dense, kind
        own = np.concatenate([np.arange(L) for L in lens])
        seq = np.concatenate([np.full(L, b) for b, L in enumerate(lens)])
        K = V = None
        if kind in ("randn", "bias_dominant"):
            perm = np.random.default_rng(seed + hs).permutation(len(own))
            own, seq = own[perm], seq[perm]
            q = torch.randn(len(own), H * hs, generator=g)
        else:
            K, V, q, own, seq = kr.hostile_inputs(kind, H, H, hs, lens=lens)
        self.q = q * hs ** -0.5
        self.seq, self.q_pos = seq.astype(np.int32), own.astype(np.int32)
        self.pos = (np.asarray(lens)[seq] - 1).astype(np.int32) if dense else self.q_pos.copy()
        self.cache = kr.PagedCache(lens, H, hs, dtype, seed=seed + hs, K=K, V=V, fill=LOUD, extra_pages=2)
        KV = [self.cache.stored_seq(b) for b in range(len(lens))]
        self.K, self.V = [k for k, _ in KV], [v for _, v in KV]
        self.tab_half = max(lens) - 1
        R, n = len(own), 2 * self.tab_half + 1
        if kind == "bias_dominant":                      # gate * table = +-75: the bias decides the softmax
            self.gate = torch.full((R, H), 2.5)
            self.tab = torch.where(torch.rand(H, n, generator=g) < 0.5, -30.0, 30.0)
        else:
            self.gate = 1.0 + 1.5 * torch.sigmoid(torch.randn(R, H, generator=g))
            self.tab = torch.randn(H, n, generator=g)
        self.rel = kind != "randn"                       # hostile values: errors relative to each row's max magnitude
        self._memo = {}

    def args(self):
        return (self.q, self.K, self.V, self.pos, self.seq, self.q_pos, self.gate, self.tab, self.tab_half, self.H)

    def _once(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    def ref(self):
        def make():
            r = relbias_attn_ref(*self.args())
            assert bool(torch.isfinite(r).all())
            return r
        return self._once("ref", make)

    def err(self, y):
        return kr.rel_row_err(y, self.ref()) if self.rel else kr.abs_err(y, self.ref())

    def scale(self):
        return 1.0 if self.rel else float(self.ref().abs().max())

    def e_ref(self):
        return self._once("e_ref", lambda: self.err(relbias_attn_ref(*self.args(), dt=F32)))

    def model(self):
        return self._once("model", lambda: relbias_flash_model(*self.args()))

    def e_model(self):
        return self.err(self.model())


def check_rows_fp32(y, batch):
    """The assertion of the fp32 row kernel: (passes, err, E_ref, bar)."""
    err, e = batch.err(y), batch.e_ref()
    bar = kr.bar(e, batch.scale())
    return err <= bar, err, e, bar


def check_flash_bf16(y, batch):
    """The two assertions of the bf16 flash form: against the model under kr.bar(E_model, scale), against float64 of the stored
    K / V under that bar + E_model.  (passes, err vs model, err vs float64, E_model, bar)."""
    m, e = batch.model(), batch.e_model()
    bar = kr.bar(e, batch.scale())
    err_m = kr.rel_row_err(y, m) if batch.rel else kr.abs_err(y, m)
    err_r = batch.err(y)
    return err_m <= bar and err_r <= bar + e, err_m, err_r, e, bar


def conv0_clip(B, N, seed, dc=0.0):
    """[B, N] fp32: a sine plus noise per clip (the clips of tests/test_gpu_wavlm.py), + dc."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(N, dtype=F32)
    return torch.stack([0.3 * torch.sin(0.05 * (b + 1) * t) + 0.1 * torch.randn(N, generator=g) for b in range(B)]) + dc


def conv0_weights(C, K, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(C, K, generator=g) / K ** 0.5, 1.0 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g))


def gconv_case(B, T, C, groups, K, resid, bias, seed):
    g = torch.Generator().manual_seed(seed)
    Cg = C // groups
    return (torch.randn(B, T, C, generator=g), torch.randn(C, Cg, K, generator=g) / (K * Cg) ** 0.5,
            0.3 * torch.randn(C, generator=g) if bias else None, torch.randn(B, T, C, generator=g) if resid else None)


def conv2d_case(B, Cin, Fq, T, Cout, stride, resid, bias, seed):
    g = torch.Generator().manual_seed(seed)
    Fo, To = (Fq - 1) // stride[0] + 1, (T - 1) // stride[1] + 1
    return (torch.randn(B, Cin, Fq, T, generator=g), torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5,
            0.3 * torch.randn(Cout, generator=g) if bias else None, torch.randn(B, Cout, Fo, To, generator=g) if resid else None)


def conv_check(y, ref, replay):
    """The assertion of the exact-fp32 convolutions: (passes, err, E_replay, bar), bar = kr.bar(E_replay, max |ref|)."""
    err, e = kr.abs_err(y, ref), kr.abs_err(replay, ref)
    bar = kr.bar(e, float(ref.abs().max()))
    return err <= bar, err, e, bar


def rows_check(y, ref, replay):
    """The assertion of the row-wise kernels (gate, layernorm + rope, mel): (passes, err, E_ref, bar) on absolute errors."""
    return conv_check(y, ref, replay)
