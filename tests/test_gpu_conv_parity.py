"""The codec's 1-D convolutions against float64 restatements (tests/conv_refs.py; pinned and bounded on the host by
tests/test_conv_refs_host.py): ua2_conv1d — exact fp32, bf16 x 3 plain (UA2_CONV_PIPE=off) and pipelined — and ua2_conv1d_tc, variants
1, 2, 3 and automatic.  This file is the anchor of the family; tests/test_gpu_conv.py and tests/test_gpu_convtc.py hang from it by
bit-identity.

Bars (kr.bar(E_ref, scale) = max(4 E_ref, 8 * 2^-24 scale), scale = max(1, max|ref|)):
  exact kernel        |y - conv_ref(float64)| <= bar, E_ref from conv_ref(float32) on the same inputs;
  bf16 x 3 kernels    (contract) |y - conv_x3_model(float64)| <= bar, E_ref from conv_x3_model(float32): only fp32 accumulation separates
                      the kernel from the contract, so a wrong split rounding or a lost low product shows — for pre_act NONE / PRELU,
                      where the host forms the operand bit-exactly;
                      (conv) |y - conv_ref(float64)| <= split_bound + bar per output, the derived distance of the contract from the
                      conv: the only check of the ELU / tanh / round9 pre-activations;
  tc kernels          |unpack(planes) - conv_x3_model(float64)| <= bar + 2^-17 |ref| per output on representable inputs (the second
                      term is the output's own hi / lo rounding: 17 bits with lo's sign); fp32 output: bar alone.
Guards on every launch: x, residual and y live inside larger device buffers whose margins (at least a window, K * dilation + 64 steps)
hold finite sentinels — 1e30 around the inputs, so a read that should have been zero padding wrecks the result; a bit pattern around
and under the output, so a store past Tout or a skipped output shows — and after the launch the output's margins, x and the residual
must be bit-unchanged.  Every launch first asks ua2_debug_conv1d_plan (the launcher's own UA2_CHECKs and selection) and takes the
kernel the table names.  Every launch prints a `PARITY conv` line (profiles/conv_parity.txt)."""
import pytest
import torch

import conv_refs as cr
import kernel_refs as kr
from conv_refs import ACT_NONE, ACT_PRELU, CASES, EDGE_CASES, F64, Case

pytestmark = pytest.mark.gpu

ALL = CASES + EDGE_CASES
SENT_IN = 1e30                                   # finite: nothing non-finite goes to a kernel
SENT_OUT = {torch.float32: 0x7E7E7E7E, torch.bfloat16: 0x7E7E}   # finite bit patterns (8.5e37)
INT_OF = {torch.float32: torch.int32, torch.bfloat16: torch.int16}


def _ids(cases):
    return [c.name.replace(" ", "_") for c in cases]


class Guarded:
    """A tensor in the middle of a larger device buffer with `margin` elements of sentinel on each side."""

    def __init__(self, shape, dtype, margin, value=None, src=None):
        n = 1
        for s in shape:
            n *= s
        self.margin, self.n = (margin + 63) // 64 * 64, n
        self.buf = torch.empty(2 * self.margin + n, dtype=dtype, device="cuda")
        if value is None:                        # output: the bit pattern everywhere, under the view too
            self.bits = SENT_OUT[dtype]
            self.buf.view(INT_OF[dtype]).fill_(self.bits)
        else:
            self.buf.fill_(value)
        self.view = self.buf[self.margin:self.margin + n].view(shape)
        if src is not None:
            self.view.copy_(src)
        self.before = self.buf.clone()

    def assert_unchanged(self, what):
        i = INT_OF[self.buf.dtype]
        assert torch.equal(self.buf.view(i), self.before.view(i)), f"{what} was written to"

    def assert_margins(self, what):
        i = INT_OF[self.buf.dtype]
        lo, hi = self.buf[:self.margin].view(i), self.buf[self.margin + self.n:].view(i)
        assert bool((lo == self.bits).all()) and bool((hi == self.bits).all()), f"store outside {what}"
        assert bool((self.view.reshape(-1).view(i) != self.bits).all()), f"an element of {what} was never written"


def _report(name, err, e_ref, bar):
    print(f"PARITY conv {name}: err {err:.3e} E_ref {e_ref:.3e} bar {bar:.3e} err/bar {err / bar:.3f}")


def _set_env(c, monkeypatch):
    if c.env is None:
        monkeypatch.delenv("UA2_CONV_PIPE", raising=False)
    else:
        monkeypatch.setenv("UA2_CONV_PIPE", c.env)


def _launch(c, d):
    """The case through ops.conv1d with guards; returns y on the host as float64."""
    from uniaudio2_amd import ops
    c.check_geometry()
    got = cr.plan_of(c)                                                  # the launcher's own checks, before any launch
    assert all(w is None or w == g for w, g in zip(c.plan, got)), f"{c}: plan {got}, the table says {c.plan}"
    for t in d.values():
        assert not torch.is_tensor(t) or bool(torch.isfinite(t).all())
    dev = lambda t: None if t is None else t.cuda()
    w = d["w_rows"].cuda()
    w_hi, w_lo = ops.pack_conv_weight_x3(w) if c.prec == 1 else (ops.pack_conv_weight(w)[0], None)
    margin = c.K * c.dil + 64
    x = Guarded(d["x"].shape, torch.float32, margin, SENT_IN, d["x"])
    y = Guarded((c.B, c.Cout, c.Tout), torch.float32, margin)
    res, fused2 = None, None
    if c.fused is not None:                                              # the residual of the fused unit is its input
        w2, b2, a2 = d["fused2"]
        fused2 = (*ops.pack_conv_weight_x3(w2.cuda()), dev(b2), dev(a2))
    elif d["residual"] is not None:
        res = Guarded(d["residual"].shape, torch.float32, margin, SENT_IN, d["residual"])
    out = ops.conv1d(x.view, w_hi, c.K, c.Cout, stride=c.stride, dilation=c.dil, pad_left=c.pad_left, Tout=c.Tout, bias=dev(d["bias"]),
                     pre_act=c.pre, pre_alpha=dev(d["pre_alpha"]), post_act=c.post, post_alpha=dev(d["post_alpha"]),
                     residual=x.view if c.fused is not None else (None if res is None else res.view), in_repeat=c.rep, out_phases=c.P,
                     out_trim_left=c.trim, w_lo=w_lo, fused2=fused2, out=y.view)
    torch.cuda.synchronize()
    assert out.data_ptr() == y.view.data_ptr()
    y.assert_margins("y")
    x.assert_unchanged("x")
    if res is not None:
        res.assert_unchanged("residual")
    got = y.view.cpu()
    assert bool(torch.isfinite(got).all())
    return got.to(F64)


def _err(a, b):
    return float((a - b).abs().max())


@pytest.mark.parametrize("c", ALL, ids=_ids(ALL))
def test_conv1d_against_float64(c, monkeypatch):
    """Every case of the table and every edge geometry, through the kernel the table names (3b, 3c, 3e, 3f, 3g of the file's plan):
    the exact kernel against conv_ref, the bf16 x 3 kernels against their contract and against conv_ref within split_bound."""
    _set_env(c, monkeypatch)
    d = cr.make_inputs(c)
    kw = cr.ref_kwargs(c, d)
    y = _launch(c, d)
    ref = cr.conv_ref(d["x"], d["w_rows"], **kw)
    scale = max(1.0, float(ref.abs().max()))
    if c.prec == 0:
        e_ref = _err(cr.conv_ref(d["x"], d["w_rows"], dt=torch.float32, **kw).to(F64), ref)
        bar = kr.bar(e_ref, scale)
        err = _err(y, ref)
        _report(c.name, err, e_ref, bar)
        assert err <= bar
        return
    model = cr.conv_x3_model(d["x"], d["w_rows"], **kw)
    e_ref = _err(cr.conv_x3_model(d["x"], d["w_rows"], dt=torch.float32, **kw).to(F64), model)
    bar = kr.bar(e_ref, scale)
    err_conv = float(((y - ref).abs() - cr.split_bound(d["x"], d["w_rows"], **kw)).max())     # what split_bound leaves over, per output
    err_model = _err(y, model) if c.pre in (ACT_NONE, ACT_PRELU) else None
    if err_model is not None:
        _report(f"{c.name} [contract]", err_model, e_ref, bar)
    _report(f"{c.name} [conv - split_bound]", max(err_conv, 0.0), e_ref, bar)
    failed = [what for what, e in (("contract", err_model), ("conv", err_conv)) if e is not None and e > bar]
    assert not failed, f"{c}: {failed} past the bar {bar:.3e}: contract {err_model}, conv - split_bound {err_conv:.3e}"


# ---- ua2_conv1d_tc ----------------------------------------------------------------------------------------------------------------

class TcCase(Case):
    """A case of ua2_conv1d_tc: stride 1, no pre-activation, Cin (and Cout, unless the output is fp32) multiples of 32.
    variants: the kernels it runs through (1 plain, 2 pipelined, 3 big-tile, 0 automatic), all against one reference."""

    def __init__(self, name, *a, variants=(1, 2, 0), out_f32=False, **k):
        super().__init__("tc " + name, *a, **k)
        self.variants, self.out_f32 = variants, out_f32
        assert self.stride == 1 and self.pre == ACT_NONE and self.prec == 1 and self.env is None


def _tc_cases():
    out = [
        TcCase("fused32 d9", 32, 32, 7, 1000, dil=9, fused=(True, True)),
        TcCase("fused64 d5 nobias nobias2 noalpha2", 64, 64, 7, 333, dil=5, bias=False, fused=(False, False), w2_scale=0.5),
        TcCase("fused128 d3 pca", 128, 128, 7, 257, B=1, dil=3, pca=True, fused=(True, True), w2_scale=0.25),
        # the big-tile kernel takes a fused unit when its 1024- / 512-step tiles fill the device (96 workgroups): the shortest such lengths
        TcCase("fused32 d1 big", 32, 32, 7, 49152, fused=(True, True), variants=(1, 3, 0)),
        TcCase("fused64 d9 big", 64, 64, 7, 24575, dil=9, pca=True, fused=(True, True), w2_scale=0.5, variants=(1, 3, 0)),
        TcCase("k7 d3 c64>64", 64, 64, 7, 500, dil=3),
        TcCase("k7 d5 c64>96 B3", 64, 96, 7, 130, B=3, dil=5, pca=True),
        TcCase("k3 d2 c96>160 res B3", 96, 160, 3, 70, B=3, dil=2, pca=True, res=True, variants=(1, 0)),
        TcCase("k1 c128>64 res", 128, 64, 1, 333, res=True, pca=True),
        TcCase("k1 c128>64 nobias", 128, 64, 1, 130, bias=False, post=ACT_NONE),
        TcCase("P4 c128>64", 128, 64, 2, 257, P=4),
        TcCase("P2 trim1 res c64>32", 64, 32, 2, 350, P=2, trim=1, pad="sym", res=True, variants=(1, 0)),
        TcCase("P5 trim1 c64>64", 64, 64, 2, 130, P=5, trim=1, pad="sym"),
        TcCase("rep2 c64>32 k7", 64, 32, 7, 257, rep=2),
        TcCase("rep2 res c32>32 k5", 32, 32, 5, 130, rep=2, res=True, variants=(1, 0)),
        TcCase("waveform c32>1 k7 f32", 32, 1, 7, 1000, out_f32=True),
    ]
    for T in (1, 2, 5):                                                    # streaming decode chunks
        out.append(TcCase(f"Tin{T} k7 d9 c64>64", 64, 64, 7, T, dil=9))
        out.append(TcCase(f"Tin{T} fused128 d9", 128, 128, 7, T, dil=9, fused=(True, True), w2_scale=0.25))
    out.append(TcCase("Tin1 rep2 k7 c64>32", 64, 32, 7, 1, rep=2))
    for T in (1, 2):
        for P in (2, 5):
            out.append(TcCase(f"P{P} Tin{T} causal c64>64", 64, 64, 2, T, P=P, post=ACT_NONE))
            out.append(TcCase(f"P{P} Tin{T} trim1 c64>64", 64, 64, 2, T, P=P, trim=1, pad="sym"))
    for dT in (-1, 0, 1):                                                  # a 64-step workgroup tile edge of the plain and the pipelined kernel
        out.append(TcCase(f"edge T{128 + dT} k7 c64>64", 64, 64, 7, 128 + dT, res=True, variants=(1, 0)))
        out.append(TcCase(f"edge T{128 + dT} fused64", 64, 64, 7, 128 + dT, fused=(True, True), w2_scale=0.5))
    return out


TC_CASES = _tc_cases()


class Planes:
    """hi / lo bf16 planes [B, T, C], each inside its own guarded buffer; quacks like ops.TC for ops.conv1d_tc."""

    def __init__(self, B, Cc, T, margin_steps, src=None):
        value = None if src is None else SENT_IN
        hi = lo = None
        if src is not None:                                               # fp32 [B, C, T], representable: hi + lo is src exactly
            hi = src.to(torch.bfloat16)
            lo = (src - hi.float()).to(torch.bfloat16)
            assert torch.equal(hi.float() + lo.float(), src)
            hi, lo = hi.transpose(1, 2), lo.transpose(1, 2)
        self.g = [Guarded((B, T, Cc), torch.bfloat16, margin_steps * Cc, value, p) for p in (hi, lo)]
        self.hi, self.lo = self.g[0].view, self.g[1].view
        self.planes = self.hi                                             # ops.conv1d_tc reads the device from it
        self.shape = (B, Cc, T)

    def value(self):
        return (self.hi.float() + self.lo.float()).transpose(1, 2).cpu().to(F64)


def _tc_check_geometry(c):
    """The UA2_CHECKs of ua2_conv1d_tc, restated."""
    c.check_geometry()
    assert c.Cin % 32 == 0 and (c.out_f32 or c.Cout % 32 == 0) and not (c.out_f32 and (c.P > 1 or c.res))
    assert c.fused is None or (c.Cin == c.Cout and c.Cout in (32, 64, 128) and c.P == 1 and c.rep == 1 and c.T == c.Tout)


@pytest.mark.parametrize("c", TC_CASES, ids=_ids(TC_CASES))
def test_conv1d_tc_against_the_contract(c):
    """ua2_conv1d_tc, every variant the case names, on representable inputs against conv_x3_model(float64) — the fused unit with the
    model reducing the 1 x 1 conv in tc_w2_order, anchored without passing through ua2_conv1d and the 2^-14 allowance of
    tests/test_gpu_convtc.py; the fp32 (waveform) output included."""
    from uniaudio2_amd import ops
    _tc_check_geometry(c)
    d = cr.make_inputs(c)
    d["x"] = cr.representable(d["x"])
    if c.fused is not None:
        d["residual"] = d["x"]
    elif d["residual"] is not None:
        d["residual"] = cr.representable(d["residual"])
    kw = cr.ref_kwargs(c, d)
    order = None
    if c.fused is not None:
        order = ops.tc_w2_order(torch.arange(c.Cout, dtype=torch.float32).view(1, -1, 1)).view(-1).long()
        assert sorted(order.tolist()) == list(range(c.Cout))
    model = cr.conv_x3_model(d["x"], d["w_rows"], w2_order=order, **kw)
    e_ref = _err(cr.conv_x3_model(d["x"], d["w_rows"], w2_order=order, dt=torch.float32, **kw).to(F64), model)
    bar = kr.bar(e_ref, max(1.0, float(model.abs().max())))
    rounding = (0.0 if c.out_f32 else 2.0 ** -17) * model.abs()        # the planes' own hi / lo rounding, per output

    dev = lambda t: None if t is None else t.cuda()
    w_hi, w_lo = ops.pack_conv_weight_x3(d["w_rows"].cuda())
    fused2 = None
    if c.fused is not None:
        w2, b2, a2 = d["fused2"]
        fused2 = (*ops.pack_conv_weight_x3(ops.tc_w2_order(w2.cuda())), dev(b2), dev(a2))
    steps = c.K * c.dil + 64
    x = Planes(c.B, c.Cin, c.T, steps, d["x"])
    res = Planes(c.B, c.Cout, c.Tout, steps, d["residual"]) if (c.res and c.fused is None) else None
    for variant in c.variants:
        if c.out_f32:
            y = Guarded((c.B, c.Cout, c.Tout), torch.float32, steps)
            out = y.view
        else:
            y = out = Planes(c.B, c.Cout, c.Tout, steps)
        ops.conv1d_tc(x, w_hi, w_lo, c.K, c.Cout, dilation=c.dil, pad_left=c.pad_left, Tout=c.Tout, bias=dev(d["bias"]), post_act=c.post,
                      post_alpha=dev(d["post_alpha"]), in_repeat=c.rep, out_phases=c.P, out_trim_left=c.trim, fused2=fused2, residual=res,
                      out_f32=c.out_f32, variant=variant, out=out)
        torch.cuda.synchronize()
        for g in ([y] if c.out_f32 else y.g):
            g.assert_margins("y")
        for p in (x, res):
            for g in (p.g if p is not None else ()):
                g.assert_unchanged("an input plane")
        got = y.view.cpu().to(F64) if c.out_f32 else y.value()
        assert bool(torch.isfinite(got).all())
        excess = float(((got - model).abs() - rounding).max())            # what the output's own rounding leaves over
        _report(f"{c.name} v{variant}", max(excess, 0.0), e_ref, bar)
        assert excess <= bar, (c, variant)
