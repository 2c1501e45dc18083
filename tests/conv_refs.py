"""Plain restatements of the codec's 1-D convolutions (ua2_conv1d, ua2_conv1d_tc), used by tests/test_conv_refs_host.py and
tests/test_gpu_conv_parity.py, in the manner of kernel_refs.py / linear_refs.py.

Every helper takes `dt`: torch.float64 is the reference a kernel is compared with; torch.float32 evaluates the SAME formula in plain
fp32 on the host, and its error against the float64 result (`E_ref`) sizes the bar kr.bar(E_ref, scale).  The reduction of the float32
replay is an explicit legal order (see _chain), not the host BLAS's.  All helpers are vectorised (one gather + one matrix product per
tap), CPU only, and none calls F.conv1d: tests/test_conv_refs_host.py pins conv_ref to the torch library functions it restates.

  conv_ref       the formula at the top of csrc/ua2_conv.hip / the ua2_conv1d_args comment of include/ua2hip.h
  conv_x3_model  the arithmetic contract of precision 1 ("bf16 x 3"): what the kernels accumulate, evaluated without rounding
  split_bound    the derived per-output distance between the two

Filters are given as rows [rows, Cin, K] (rows = Cout, or out_phases * Cout phase filters: ops.convtr_phase_rows); fused2 =
(W2 [Cout, Cout] or [Cout, Cout, 1], bias2 or None, alpha2 or None) is the 1 x 1 conv of a fused residual unit."""
import torch

import kernel_refs as kr

F64 = torch.float64
ACT_NONE, ACT_PRELU, ACT_ELU, ACT_TANH, ACT_ROUND9 = 0, 1, 2, 3, 4     # enum ua2_act


def act(v, kind, alpha=None):
    """apply_act of csrc/ua2_conv.hip in v's dtype.  alpha: None (slope 0), a scalar tensor, or one value per channel of dim 1."""
    if kind == ACT_NONE:
        return v
    if kind == ACT_PRELU:
        al = torch.zeros(1, dtype=v.dtype) if alpha is None else alpha.to(v.dtype).reshape(-1)
        al = al.view(1, -1, *([1] * (v.dim() - 2))) if al.numel() > 1 else al
        return torch.where(v >= 0, v, al * v)
    if kind == ACT_ELU:
        return torch.where(v > 0, v, torch.expm1(v))                   # nn.ELU(alpha = 1)
    if kind == ACT_TANH:
        return torch.tanh(v)
    if kind == ACT_ROUND9:
        return torch.round(9 * v) / 9                                   # torch.round: halves to even, as rintf
    raise ValueError(kind)


def lipschitz(kind, alpha=None):
    """Lipschitz constant of act(., kind, alpha) per channel (a [C] or [1] float64 tensor)."""
    if kind == ACT_PRELU:
        al = torch.zeros(1, dtype=F64) if alpha is None else alpha.to(F64).reshape(-1)
        return torch.clamp(al.abs(), min=1.0)
    if kind in (ACT_NONE, ACT_ELU, ACT_TANH):
        return torch.ones(1, dtype=F64)
    raise ValueError("round(9x)/9 is not continuous: no bound passes through it")


def _tq(Tout, out_phases, out_trim_left):
    return Tout if out_phases == 1 else -(-(Tout + out_trim_left) // out_phases)


def _chain(pairs, *, K, stride, dilation, pad_left, tq, in_repeat, cb=None):
    """acc[b][n][t] = sum over the (xa, w) pairs of sum_{ci,j} w[n][ci][j] * xa[b][ci][(t * stride + j * dilation - pad_left) / in_repeat],
    zero outside [0, Tin * in_repeat): an explicit index gather per tap and one [rows, c] x [c, tq] product per (channel block, tap,
    pair), in the pairs' dtype.  cb = None: one block of all channels (float64: the order is immaterial).  cb = the channels of one
    matrix-pipe step: the float32 replay's explicit, pessimistic legal order, in the manner of linear_refs — one partial sum per step
    (exact kernel: 4 channels of a tap; bf16 x 3: 32 channels of a tap, per operand pair), all of them added left to right in ONE
    fp32 chain, channel block major and tap minor as the kernels walk them, not whatever order the host BLAS would pick."""
    B, Cin, Tin = pairs[0][0].shape
    t = torch.arange(tq)
    acc = torch.zeros(B, pairs[0][1].shape[0], tq, dtype=pairs[0][0].dtype)
    taps = []
    for j in range(K):
        pos = t * stride + j * dilation - pad_left
        ok = (pos >= 0) & (pos < Tin * in_repeat)
        taps.append((torch.div(pos.clamp(0, Tin * in_repeat - 1), in_repeat, rounding_mode="floor"), ok.to(acc.dtype)))
    cb = cb or Cin
    for c0 in range(0, Cin, cb):
        for j, (src, ok) in enumerate(taps):
            for xa, w in pairs:
                acc = acc + torch.einsum("nc,bct->bnt", w[:, c0:c0 + cb, j], xa[:, c0:c0 + cb][:, :, src] * ok)
    return acc


def _taps(xa, w, **geo):
    return _chain([(xa, w)], **geo)


def _mm_chain(pairs, cb=None):
    """sum over the (w [N, C], h [B, C, T]) pairs of w h, chained like _chain (a 1 x 1 conv)."""
    Cc = pairs[0][0].shape[1]
    cb = cb or Cc
    acc = 0
    for c0 in range(0, Cc, cb):
        for w, h in pairs:
            acc = acc + torch.einsum("nc,bct->bnt", w[:, c0:c0 + cb], h[:, c0:c0 + cb])
    return acc


def _scatter(v, Cout, Tout, out_phases, out_trim_left):
    """[B, out_phases * Cout, tq] -> [B, Cout, Tout]: row phase * Cout + co, step t goes to y[co][t * out_phases + phase - out_trim_left]."""
    if out_phases == 1:
        return v[:, :, :Tout]
    B, _, tq = v.shape
    full = v.view(B, out_phases, Cout, tq).permute(0, 2, 3, 1).reshape(B, Cout, tq * out_phases)
    return full[:, :, out_trim_left:out_trim_left + Tout]


def _per_row(vec, out_phases, dt):
    """A per-channel vector [Cout] (or [1]) as a per-row column [1, rows or 1, 1]."""
    vec = vec.to(dt).reshape(-1)
    return (vec.repeat(out_phases) if vec.numel() > 1 else vec).view(1, -1, 1)


def _w2(fused2):
    w2, b2, a2 = fused2
    return w2.reshape(w2.shape[0], w2.shape[1]), b2, a2


def conv_ref(x, w_rows, *, K, stride=1, dilation=1, pad_left=0, Tout, in_repeat=1, out_phases=1, out_trim_left=0, pre_act=ACT_NONE,
             pre_alpha=None, bias=None, post_act=ACT_NONE, post_alpha=None, residual=None, fused2=None, dt=F64):
    """y[b][co][t * P + phase - trim] = post(bias[co] + sum_{ci,j} W[phase * Cout + co][ci][j] * pre(x[b][ci][(t * stride + j * dilation
    - pad_left) / in_repeat])) + residual, zero outside [0, Tin * in_repeat); the residual is added AFTER post.  With fused2:
    y = residual + PReLU(alpha2 or 0, W2 h + bias2), h the activated conv.  Everything in `dt`."""
    assert w_rows.shape[2] == K and w_rows.shape[1] == x.shape[1] and w_rows.shape[0] % out_phases == 0
    Cout = w_rows.shape[0] // out_phases
    xa = act(x.to(dt), pre_act, pre_alpha)
    acc = _chain([(xa, w_rows.to(dt))], K=K, stride=stride, dilation=dilation, pad_left=pad_left, tq=_tq(Tout, out_phases, out_trim_left),
                 in_repeat=in_repeat, cb=None if dt == F64 else 4)
    if bias is not None:
        acc = acc + _per_row(bias, out_phases, dt)
    if post_act == ACT_PRELU:
        al = _per_row(post_alpha, out_phases, dt)
        acc = torch.where(acc >= 0, acc, al * acc)
    else:
        acc = act(acc, post_act)
    y = _scatter(acc, Cout, Tout, out_phases, out_trim_left)
    if fused2 is not None:
        w2, b2, a2 = _w2(fused2)
        v = _mm_chain([(w2.to(dt), y)], None if dt == F64 else 4)
        if b2 is not None:
            v = v + b2.to(dt).view(1, -1, 1)
        y = act(v, ACT_PRELU, a2)
    if residual is not None:
        y = y + residual.to(dt)
    return y


def split_w(w_rows):
    """ops.pack_conv_weight_x3's own split, restated: hi = RNE_bf16(w); lo = w - hi in fp32 (exact), rounded RNE to bf16 when it is
    packed.  Returns (wh, wl) as fp32."""
    w = w_rows.float()
    wh = kr.bf16_round(w)
    return wh, kr.bf16_round(w - wh)


def split_x(x32):
    """The staging split of the bf16 x 3 kernels: xh = RNE_bf16(x), xl = RNE_bf16(x - xh) (x - xh is exact in fp32).  fp32 in, fp32 out."""
    xh = kr.bf16_round(x32)
    return xh, kr.bf16_round(x32 - xh)


def conv_x3_model(x, w_rows, *, K, stride=1, dilation=1, pad_left=0, Tout, in_repeat=1, out_phases=1, out_trim_left=0, pre_act=ACT_NONE,
                  pre_alpha=None, bias=None, post_act=ACT_NONE, post_alpha=None, residual=None, fused2=None, w2_order=None, dt=F64):
    """The arithmetic contract of precision 1, evaluated in `dt`: pre(x) formed in fp32 on the host (the kernel's bits for NONE and
    PRELU: one fp32 multiply), split into xh + xl; the filter split into wh + wl as the packer does; the sum is
        sum (wl * xh + wh * xl + wh * xh)
    — in float64 the exact value of what the kernel accumulates in fp32 (every product of two bf16 values is exact in fp32 and in
    float64).  Bias, activation and residual as conv_ref.  The fused unit's h is rounded to fp32 and goes through the same split
    before W2 (itself split); w2_order (a permutation of the channels, ops.tc_w2_order's) only changes the order the 1 x 1 conv
    reduces in, which matters to the fp32 replay alone.  For the tc kernels the result is what the output planes must carry."""
    assert w_rows.shape[2] == K and w_rows.shape[1] == x.shape[1] and w_rows.shape[0] % out_phases == 0
    Cout = w_rows.shape[0] // out_phases
    xh, xl = split_x(act(x.float(), pre_act, None if pre_alpha is None else pre_alpha.float()))
    wh, wl = split_w(w_rows)
    geo = dict(K=K, stride=stride, dilation=dilation, pad_left=pad_left, tq=_tq(Tout, out_phases, out_trim_left), in_repeat=in_repeat)
    cb = None if dt == F64 else 32
    acc = _chain([(xh.to(dt), wl.to(dt)), (xl.to(dt), wh.to(dt)), (xh.to(dt), wh.to(dt))], cb=cb, **geo)   # small terms first, as the kernels
    if bias is not None:
        acc = acc + _per_row(bias, out_phases, dt)
    if post_act == ACT_PRELU:
        al = _per_row(post_alpha, out_phases, dt)
        acc = torch.where(acc >= 0, acc, al * acc)
    else:
        acc = act(acc, post_act)
    y = _scatter(acc, Cout, Tout, out_phases, out_trim_left)
    if fused2 is not None:
        w2, b2, a2 = _w2(fused2)
        hh, hl = split_x(y.float())
        w2h, w2l = split_w(w2)
        if w2_order is not None:
            hh, hl, w2h, w2l = hh[:, w2_order], hl[:, w2_order], w2h[:, w2_order], w2l[:, w2_order]
        v = _mm_chain([(w2l.to(dt), hh.to(dt)), (w2h.to(dt), hl.to(dt)), (w2h.to(dt), hh.to(dt))], cb)
        if b2 is not None:
            v = v + b2.to(dt).view(1, -1, 1)
        y = act(v, ACT_PRELU, a2)
    if residual is not None:
        y = y + residual.to(dt)
    return y


SPLIT_C = 8.0 + 2.0 ** -4                       # the a-priori form of split_bound: SPLIT_C * 2^-18 * sum |w| |pre(x)|
PRE_ULPS = {ACT_NONE: 0.0, ACT_PRELU: 0.0, ACT_ROUND9: 0.0, ACT_ELU: 4.0, ACT_TANH: 4.0}   # device vs host libm, units of 2^-24


def _abs_taps(xa, wa, geo):
    return _taps(xa.to(F64).abs(), wa.to(F64).abs(), **geo)


def split_bound(x, w_rows, *, K, stride=1, dilation=1, pad_left=0, Tout, in_repeat=1, out_phases=1, out_trim_left=0, pre_act=ACT_NONE,
                pre_alpha=None, bias=None, post_act=ACT_NONE, post_alpha=None, residual=None, fused2=None, apriori=False):
    """Per output, a bound on |conv_x3_model(float64) - conv_ref(float64)|, carried through the activations.  A bound, not a
    measurement: nothing in it comes from a kernel.

    Derivation.  bf16 keeps 8 significant bits, so RNE moves v by at most half an ulp, u |v| with u = 2^-8 (attained just above a
    power of two: 1 + 2^-8 rounds to 1).  Write p for pre(x) as the contract forms it (fp32) and
        w = wh + wl + rw,   p = xh + xl + rx        (wl = RNE(w - wh), w - wh exact in fp32; likewise xl)
    then, as an identity,
        w p - (wh xh + wh xl + wl xh) = wl xl + rw p + (wh + wl) rx.
    The bound is the sum over (ci, j) of the absolute values of the three terms with the ACTUAL split parts (abs-value convs in
    float64): sum |wl| |xl| + |rw| |p| + |wh + wl| |rx|.  A priori: |wl| <= u (1 + u) |w|; and |rw| <= 2^-17 |w|, because w - wh lies
    in a binade at least 9 below w's unless it is itself a power of two, so its 8-bit rounding moves it by at most 2^-17 |w| (hi + lo
    carry 17 bits with lo's sign) — likewise x.  Hence per product
        <= (2^-16 (1 + u)^2 + 2^-17 + 2^-17 (1 + 2^-17)) |w p| <= SPLIT_C * 2^-18 |w p|,   SPLIT_C = 8 + 2^-4
    (apriori=True returns that form, SPLIT_C * 2^-18 * sum |w| |pre(x)|; tests/test_conv_refs_host.py checks it dominates the sharp
    one.  An earlier statement of this bound took u = 2^-9 and arrived at c = 3: single-channel cases exceed that).
    (No underflow term: the operands of the tests are far above bf16's subnormals.)
    The reference forms pre(x) in float64: the difference |p - pre64| enters as sum |w| |p - pre64|, computed, not estimated; for ELU
    and tanh the device's expm1f / tanhf may differ from the host's by 2 ulp either way, PRE_ULPS * 2^-24 |pre64| more (none / PReLU /
    round9 are single correctly rounded fp32 operations — the tests keep 9x away from rint's ties — so host and device agree).
    Bias and residual add exactly.  An activation with Lipschitz constant L = max(1, |alpha|) (PReLU; 1 for ELU, tanh, none) scales
    the bound by L.  Fused unit: the contract rounds its own h_m to fp32 (hf) and splits it, hf = hh + hl + rh, W2 = w2h + w2l + rw2;
    with bound_h the bound on |h - h_m|, before the second activation
        |W2 h - contract| <= |W2| (bound_h + |h_m - hf|) + |w2l| |hl| + |rw2| |hf| + |w2h + w2l| |rh|,
    times L2 = max(1, |alpha2|) behind it."""
    Cout = w_rows.shape[0] // out_phases
    geo = dict(K=K, stride=stride, dilation=dilation, pad_left=pad_left, tq=_tq(Tout, out_phases, out_trim_left), in_repeat=in_repeat)
    p64 = act(x.to(F64), pre_act, pre_alpha)
    p32 = act(x.float(), pre_act, None if pre_alpha is None else pre_alpha.float())
    xh, xl = split_x(p32)
    wh, wl = split_w(w_rows)
    w64 = w_rows.to(F64)
    if apriori:
        s = SPLIT_C * 2.0 ** -18 * _abs_taps(p64, w64, geo)
    else:
        rx, rw = p32.to(F64) - xh.to(F64) - xl.to(F64), w64 - wh.to(F64) - wl.to(F64)
        s = _abs_taps(xl, wl, geo) + _abs_taps(p32, rw, geo) + _abs_taps(rx, wh.to(F64) + wl.to(F64), geo)
    s = s + _abs_taps((p32.to(F64) - p64).abs() + PRE_ULPS[pre_act] * 2.0 ** -24 * p64.abs(), w64, geo)
    b = _scatter(s * _per_row(lipschitz(post_act, post_alpha), out_phases, F64), Cout, Tout, out_phases, out_trim_left)
    if fused2 is not None:
        w2, _, a2 = _w2(fused2)
        hm = conv_x3_model(x, w_rows, K=K, stride=stride, dilation=dilation, pad_left=pad_left, Tout=Tout, in_repeat=in_repeat, pre_act=pre_act,
                           pre_alpha=pre_alpha, bias=bias, post_act=post_act, post_alpha=post_alpha)
        hf = hm.float()
        hh, hl = split_x(hf)
        w2h, w2l = split_w(w2)
        mm = lambda w, h: torch.einsum("nc,bct->bnt", w.to(F64).abs(), h.to(F64).abs())
        b = mm(w2, b + (hm - hf.to(F64)).abs())
        if apriori:
            b = b + SPLIT_C * 2.0 ** -18 * mm(w2, hf)
        else:
            b = b + mm(w2l, hl) + mm(w2.to(F64) - w2h.to(F64) - w2l.to(F64), hf) + mm(w2h.to(F64) + w2l.to(F64), hf.to(F64) - hh.to(F64) - hl.to(F64))
        b = b * lipschitz(ACT_PRELU, a2).view(1, -1, 1)
    return b


def representable(x):
    """An fp32 tensor rounded to the 16 significant bits the time-major planes carry (hi + lo)."""
    return kr.split16_round(x.float())


# ---- the case table -------------------------------------------------------------------------------------------------------------

class Case:
    """One conv problem.  pad: "causal" (scalar24k.py:70-74 / conv.py:239-243: left pad d(k-1) - (stride-1), right pad implied by Tout),
    "sym" (symmetric), or an int pad_left with Tout given.  P > 1: the phase form of ConvTranspose1d(k = 2P, stride P) (K = 2 taps per
    phase); causal = drop the last P samples (Tout = T P), otherwise Tout = (T + 1) P - 2 trim.  fused = (bias2?, alpha2?); w2_scale: the
    1 x 1 filter is w2_scale / sqrt(C) * randn — below 1 on the 64- and 128-channel units, whose worst-case bound compounds through
    |W2| and would otherwise pass 1e-4 * max|ref| (a condition tests/test_conv_refs_host.py puts on the table).
    env: the UA2_CONV_PIPE value the case runs under (None = unset).  plan: (kernel, ntt, rt, tpw, gpu, npg, nw) it must take."""

    def __init__(self, name, Cin, Cout, K, T, *, B=2, stride=1, dil=1, pad="causal", Tout=None, rep=1, P=1, trim=0, pre=ACT_NONE,
                 post=ACT_PRELU, pca=False, bias=True, res=False, fused=None, prec=1, env=None, hostile=False, plan=None, w2_scale=1.0):
        self.name, self.Cin, self.Cout, self.K, self.T, self.B = name, Cin, Cout, K, T, B
        self.stride, self.dil, self.rep, self.P, self.trim = stride, dil, rep, P, trim
        self.pre, self.post, self.pca, self.bias, self.res, self.fused = pre, post, pca, bias, res or fused is not None, fused
        self.prec, self.env, self.hostile, self.plan, self.w2_scale = prec, env, hostile, plan, w2_scale
        Te, span = T * rep, dil * (K - 1) + 1
        if P > 1:
            assert K == 2 and stride == 1 and dil == 1 and rep == 1
            self.pad_left = 1
            self.Tout = T * P if pad == "causal" else (T + 1) * P - 2 * trim
            assert pad != "causal" or trim == 0
        elif pad == "causal":
            self.pad_left = dil * (K - 1) - (stride - 1)
            self.Tout = -(-(Te - span + self.pad_left) // stride) + 1
        elif pad == "sym":
            self.pad_left = (K * dil - dil) // 2
            self.Tout = (Te + 2 * self.pad_left - span) // stride + 1
        else:
            self.pad_left, self.Tout = int(pad), Tout
        if fused is not None:
            assert self.Tout == T and Cin == Cout and prec == 1
        self.pad = pad

    def __repr__(self):
        return self.name

    @property
    def rows(self):
        return self.Cout * self.P

    def geo(self):
        """The geometry / activation keywords conv_ref, conv_x3_model, split_bound and ops.conv1d share."""
        return dict(K=self.K, stride=self.stride, dilation=self.dil, pad_left=self.pad_left, Tout=self.Tout, in_repeat=self.rep,
                    out_phases=self.P, out_trim_left=self.trim, pre_act=self.pre, post_act=self.post)

    def check_geometry(self):
        """The UA2_CHECKs of ua2_conv1d, restated: nothing this table holds may be rejected (or run unchecked) by the launcher."""
        assert min(self.B, self.Cin, self.Cout, self.T, self.Tout) > 0 and 1 <= self.K <= 32
        assert min(self.stride, self.dil, self.rep, self.P) >= 1 and (self.P == 1 or (self.stride == 1 and self.dil == 1))
        assert self.pad_left >= 0 and 0 <= self.trim < self.P
        tq = _tq(self.Tout, self.P, self.trim)
        last = (tq - 1) * self.stride + (self.K - 1) * self.dil - self.pad_left
        assert last < self.T * self.rep + (self.K - 1) * self.dil + self.stride, "more than a window of right padding"
        if self.fused is not None:
            assert self.Cout in (32, 64, 128) and self.stride == 1 and self.rep == 1 and self.P == 1 and self.T == self.Tout


def make_inputs(c):
    """Seeded CPU fp32 tensors of a case: x, w_rows (and w_t, the ConvTranspose1d filter, in phase mode), bias, pre_alpha, post_alpha,
    residual, fused2 = (W2, bias2, alpha2).  hostile: a channel offset by 1e3, a constant channel, a channel scaled by 1e-3."""
    import zlib
    g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
    x = torch.randn(c.B, c.Cin, c.T, generator=g)
    if c.hostile:
        x[:, 0] += 1e3
        if c.Cin > 1:
            x[:, 1] = 2.5
        if c.Cin > 2:
            x[:, 2] *= 1e-3
    d = dict(x=x)
    if c.P > 1:
        from uniaudio2_amd import ops
        d["w_t"] = torch.randn(c.Cin, c.Cout, 2 * c.P, generator=g) / (c.Cin * 2) ** 0.5
        d["w_rows"], M = ops.convtr_phase_rows(d["w_t"], c.P)
        assert M == c.K
    else:
        d["w_rows"] = torch.randn(c.Cout, c.Cin, c.K, generator=g) / (c.Cin * c.K) ** 0.5
    d["bias"] = torch.randn(c.Cout, generator=g) if c.bias else None
    d["pre_alpha"] = torch.tensor([0.1]) if c.pre == ACT_PRELU else None
    d["post_alpha"] = None
    if c.post == ACT_PRELU:
        d["post_alpha"] = torch.rand(c.Cout, generator=g) * 0.5 if c.pca else torch.tensor([0.2])
    d["residual"] = torch.randn(c.B, c.Cout, c.Tout, generator=g) if c.res else None
    d["fused2"] = None
    if c.fused is not None:
        d["residual"] = x
        d["fused2"] = (torch.randn(c.Cout, c.Cout, 1, generator=g) * c.w2_scale / c.Cout ** 0.5,
                       torch.randn(c.Cout, generator=g) * 0.1 if c.fused[0] else None, torch.tensor([0.3]) if c.fused[1] else None)
    return d


def ref_kwargs(c, d):
    return dict(c.geo(), pre_alpha=d["pre_alpha"], bias=d["bias"], post_alpha=d["post_alpha"], residual=d["residual"], fused2=d["fused2"])


OFF = "off"                    # UA2_CONV_PIPE=off: the plain bf16 x 3 kernel


def _hook(ntt, rt=0, tpw=0, gpu=0):
    return f"{ntt},{rt},{tpw},{gpu}"


# The table tests/test_conv_refs_host.py pins, bounds and plans, and tests/test_gpu_conv_parity.py runs.  plan = (kernel, ntt, rt, tpw,
# gpu, npg, nw) as ua2_debug_conv1d_plan reports it (kernel 1: gpu = RPW).  Shapes are the smallest that reach the arm named.
CASES = [
    # ---- exact fp32 kernel (precision 0) ----
    Case("exact k7 d3 causal hostile res", 33, 19, 7, 97, dil=3, res=True, prec=0, hostile=True, plan=(0, 1, 4, 1, 0, 0, 4)),
    Case("exact k5 d3 sym", 17, 19, 5, 70, dil=3, pad="sym", prec=0, hostile=True, plan=(0, 1, 4, 1, 0, 0, 4)),
    Case("exact k16 s8 streaming", 17, 33, 16, 203, stride=8, prec=0, hostile=True, plan=(0, 1, 4, 1, 0, 0, 4)),
    Case("exact elu pre k3 d2", 33, 19, 3, 150, dil=2, pre=ACT_ELU, post=ACT_NONE, prec=0, plan=(0, 1, 4, 1, 0, 0, 4)),
    Case("exact prelu pre pca", 17, 19, 7, 70, pre=ACT_PRELU, pca=True, prec=0, hostile=True, plan=(0, 1, 4, 1, 0, 0, 4)),
    Case("exact rep2 tanh res", 17, 19, 3, 75, rep=2, post=ACT_TANH, res=True, prec=0, plan=(0, 1, 4, 1, 0, 0, 4)),
    Case("exact round9 pre sym", 33, 19, 3, 150, pad="sym", pre=ACT_ROUND9, post=ACT_NONE, prec=0, plan=(0, 1, 4, 1, 0, 0, 4)),
    Case("exact P2 causal", 33, 19, 2, 50, P=2, post=ACT_NONE, prec=0, hostile=True, plan=(0, 1, 4, 1, 0, 0, 4)),
    Case("exact P5 trim1 res", 17, 19, 2, 37, P=5, trim=1, pad="sym", res=True, prec=0, plan=(0, 1, 4, 1, 0, 0, 4)),
    Case("exact B3 c1>200 nobias", 1, 200, 7, 100, B=3, bias=False, prec=0, plan=(0, 1, 4, 1, 0, 0, 4)),
    Case("exact ntt2 4 row blocks", 16, 256, 7, 2048, prec=0, hostile=True, plan=(0, 2, 4, 1, 0, 0, 4)),
    Case("exact ntt4 4 row blocks", 16, 256, 7, 4096, prec=0, hostile=True, plan=(0, 4, 4, 1, 0, 0, 4)),
    # ---- bf16 x 3, plain kernel: UA2_CONV_PIPE=off, or what the pipelined kernel does not serve (K, activations) ----
    Case("x3 plain RPW1 c33>1 nobias", 33, 1, 7, 130, env=OFF, post=ACT_NONE, bias=False, plan=(1, 1, 1, 1, 1, 0, 4)),
    Case("x3 plain rt1 c17>19 d3", 17, 19, 7, 70, dil=3, env=OFF, pre=ACT_PRELU, res=True, plan=(1, 1, 1, 1, 2, 0, 4)),
    Case("x3 plain rt2 c48>40 k1", 48, 40, 1, 333, env=OFF, pca=True, res=True, plan=(1, 1, 2, 1, 2, 0, 4)),
    Case("x3 plain rt4 ntt1 c17>200", 17, 200, 7, 100, B=3, env=OFF, plan=(1, 1, 4, 1, 2, 0, 4)),
    Case("x3 plain rt4 ntt2 c17>200", 17, 200, 7, 2800, B=3, env=OFF, plan=(1, 2, 4, 1, 2, 0, 4)),
    Case("x3 plain rt4 ntt4 c17>200", 17, 200, 7, 5500, B=3, env=OFF, plan=(1, 4, 4, 1, 2, 0, 4)),
    Case("x3 plain k5 d3 sym", 17, 19, 5, 70, dil=3, pad="sym", res=True, plan=(1, 1, 1, 1, 2, 0, 4)),
    Case("x3 plain k16 s8 streaming", 64, 128, 16, 203, stride=8, plan=(1, 1, 4, 1, 2, 0, 4)),
    Case("x3 plain k4 s2", 32, 64, 4, 301, stride=2, pre=ACT_PRELU, plan=(1, 1, 2, 1, 2, 0, 4)),
    Case("x3 plain elu pre k3 d2", 64, 64, 3, 150, dil=2, pre=ACT_ELU, post=ACT_NONE, plan=(1, 1, 2, 1, 2, 0, 4)),
    Case("x3 plain round9 pre sym", 64, 64, 3, 150, pad="sym", pre=ACT_ROUND9, post=ACT_NONE, plan=(1, 1, 2, 1, 2, 0, 4)),
    Case("x3 plain tanh pre k7", 33, 19, 7, 97, pre=ACT_TANH, plan=(1, 1, 1, 1, 2, 0, 4)),
    Case("x3 plain rep2 tanh post res", 64, 64, 3, 150, rep=2, post=ACT_TANH, res=True, plan=(1, 1, 2, 1, 2, 0, 4)),
    Case("x3 plain P5 trim1 res", 17, 19, 2, 37, P=5, trim=1, pad="sym", res=True, env=OFF, plan=(1, 1, 4, 1, 2, 0, 4)),
    Case("x3 plain fused32 d9", 32, 32, 7, 333, dil=9, fused=(True, True), env=OFF, plan=(1, 1, 1, 1, 2, 0, 4)),
    Case("x3 plain fused128 d5 auto", 128, 128, 7, 257, dil=5, fused=(True, True), w2_scale=0.25, plan=(1, 1, 4, 1, 2, 0, 4)),
    # ---- bf16 x 3, pipelined kernel: every (cpu, gpu, npg) arm, the 8-wave arm, ntt 1 / 2 / 4, UPT1 true and false ----
    Case("x3p 7,1,1 c17>19 d3", 17, 19, 7, 70, dil=3, pre=ACT_PRELU, res=True, plan=(2, 1, 2, 1, 1, 1, 4)),
    Case("x3p 7,1,1 upt>1 c136>64", 136, 64, 7, 100, plan=(2, 1, 4, 1, 1, 1, 4)),
    Case("x3p 7,1,2 fused32 d9", 32, 32, 7, 333, dil=9, fused=(True, True), plan=(2, 1, 2, 1, 1, 2, 4)),
    Case("x3p 7,1,3 fused32 d1 ntt4", 32, 32, 7, 700, fused=(True, True), env=_hook(4), plan=(2, 4, 2, 1, 1, 3, 4)),
    Case("x3p 7,1,1 fused64 d5 ntt2 tpw2", 64, 64, 7, 2500, dil=5, fused=(True, True), pca=True, w2_scale=0.5, env=_hook(2, 0, 2), plan=(2, 2, 4, 2, 1, 1, 4)),
    Case("x3p 8 waves fused128 d5", 128, 128, 7, 700, dil=5, fused=(True, True), w2_scale=0.25, env=_hook(4), plan=(2, 4, 8, 1, 1, 2, 8)),
    Case("x3p 1,1,2 c17>19 k1 nobias", 17, 19, 1, 333, res=True, bias=False, plan=(2, 1, 2, 1, 1, 2, 4)),
    Case("x3p 1,1,4 c32>16 k1 ntt4", 32, 16, 1, 1000, env=_hook(4), plan=(2, 4, 1, 1, 1, 4, 4)),
    Case("x3p 2,1,2 P2 c32>16", 32, 16, 2, 200, P=2, plan=(2, 1, 2, 1, 1, 2, 4)),
    Case("x3p 2,1,4 P2 c32>8 ntt2", 32, 8, 2, 700, P=2, env=_hook(2), plan=(2, 2, 1, 1, 1, 4, 4)),
    Case("x3p 2,2,1 c48>40 k1", 48, 40, 1, 333, pca=True, res=True, plan=(2, 1, 4, 1, 2, 1, 4)),
    Case("x3p 2,2,2 c64>32 k1 ntt4", 64, 32, 1, 1000, env=_hook(4), plan=(2, 4, 2, 1, 2, 2, 4)),
    Case("x3p 4,2,1 P4 c64>16", 64, 16, 2, 130, P=4, plan=(2, 1, 4, 1, 2, 1, 4)),
    Case("x3p 4,2,2 P4 trim1 res c64>16 ntt4", 64, 16, 2, 700, P=4, trim=1, pad="sym", res=True, env=_hook(4), plan=(2, 4, 4, 1, 2, 2, 4)),
    Case("x3p 4,4,1 c128>64 k1 res", 128, 64, 1, 333, res=True, plan=(2, 1, 4, 1, 4, 1, 4)),
    Case("x3p 8,4,1 P2 c128>64", 128, 64, 2, 257, P=2, plan=(2, 1, 4, 1, 4, 1, 4)),
    Case("x3p gpu1 forced c128>64 k1", 128, 64, 1, 333, env=_hook(0, 0, 0, 1), plan=(2, 1, 4, 1, 1, 2, 4)),
    Case("x3p rep2 res c64>32 k7", 64, 32, 7, 513, rep=2, res=True, plan=(2, 1, 2, 1, 1, 1, 4)),
    Case("x3p fused64 d3 nobias nobias2 noalpha2", 64, 64, 7, 130, dil=3, bias=False, fused=(False, False), w2_scale=0.5, plan=(2, 1, 4, 1, 1, 1, 4)),
    Case("x3 plain fused64 d3 nobias nobias2 noalpha2", 64, 64, 7, 130, dil=3, bias=False, fused=(False, False), w2_scale=0.5, env=OFF, plan=(1, 1, 2, 1, 2, 0, 4)),
    Case("x3p ntt2 tpw2 c17>200 B3", 17, 200, 7, 2049, B=3, env=_hook(2, 0, 2), plan=(2, 2, 4, 2, 1, 1, 4)),
    Case("x3p ntt4 tpw3 c64>64 d9", 64, 64, 7, 3000, dil=9, res=True, env=_hook(4, 0, 3), plan=(2, 4, 4, 3, 1, 2, 4)),
]


# ---- edge geometries, per kernel that accepts them.  plan entries that are None are not pinned. -----------------------------------

KINDS = {"exact": dict(prec=0), "x3": dict(prec=1, env=OFF), "x3p": dict(prec=1)}


def _kplan(kind, K, ntt=None):
    """exact -> kernel 0; "x3" (UA2_CONV_PIPE=off) -> 1; "x3p": 2 where the pipelined kernel has the tap count, else the plain one."""
    kernel = {"exact": 0, "x3": 1, "x3p": 2 if K in (1, 2, 7) else 1}[kind]
    return (kernel, ntt, None, None, None, None, None)


def _edge_cases():
    out = []
    for kind, kw in KINDS.items():
        def add(name, *a, ntt=None, **k):
            k = dict(kw, **k)
            out.append(Case(f"{kind} {name}", *a, plan=_kplan(kind, a[2], ntt), **k))
        for T in (1, 2, 5):                                            # a streaming decode chunk: the window is almost all padding
            add(f"Tin{T} k7 d9", 17, 19, 7, T, dil=9, res=True)
        if kind != "x3p":                                              # K = 16 has no pipelined form: "x3" already is what it takes
            add("Tin7 k16 s8 streaming", 17, 19, 16, 7, stride=8)
        add("Tin1 rep2 k7", 17, 19, 7, 1, rep=2)
        for T in (1, 2):
            for P in (2, 5):
                add(f"P{P} Tin{T} causal", 17, 19, 2, T, P=P, post=ACT_NONE)
                add(f"P{P} Tin{T} trim1", 17, 19, 2, T, P=P, trim=1, pad="sym")
        for ci in (1, 17, 33):                                         # ragged channel groups; a second row tile past the last (RPW = 2)
            for co in (1, 19, 200):
                add(f"c{ci}>{co} k7", ci, co, 7, 70, pca=True)
    # Tout one step inside, on and one step past a workgroup tile edge, for each ntt; the tile is 16 * ntt steps in all three kernels
    # with four wave row-groups.  exact / plain: the shortest lengths at which the launcher's own rule (>= 512 workgroups) picks the
    # ntt; pipelined: through the hook, two tiles per workgroup.
    for ntt, T in ((1, 32), (2, 2048), (4, 4096)):
        for dT in (-1, 0, 1):
            out.append(Case(f"exact edge ntt{ntt} T{T + dT}", 3, 256, 7, T + dT, prec=0, plan=_kplan("exact", 7, ntt)))
    for ntt, T in ((1, 32), (2, 2752), (4, 5504)):
        for dT in (-1, 0, 1):
            out.append(Case(f"x3 edge ntt{ntt} T{T + dT}", 3, 200, 7, T + dT, B=3, env=OFF, plan=_kplan("x3", 7, ntt)))
    for ntt in (1, 2, 4):
        for dT in (-1, 0, 1):
            T = 64 * ntt + dT
            out.append(Case(f"x3p edge ntt{ntt} T{T}", 3, 200, 7, T, env=_hook(ntt, 0, 2), res=True, plan=(2, ntt, 4, 2, 1, None, 4)))
    return out


EDGE_CASES = _edge_cases()


def plan_of(c):
    """ua2_debug_conv1d_plan for a case, as the tuple Case.plan is written in.  The caller sets UA2_CONV_PIPE (c.env) first."""
    from uniaudio2_amd import ops
    p = ops.conv1d_plan(c.B, c.Cin, c.Cout, c.T, c.Tout, c.K, stride=c.stride, dilation=c.dil, in_repeat=c.rep, out_phases=c.P,
                        out_trim_left=c.trim, pre_act=c.pre, post_act=c.post, precision=c.prec, fused=c.fused is not None, residual=c.res)
    return tuple(p[k] for k in ("kernel", "ntt", "rt", "tpw", "gpu", "npg", "nw"))
