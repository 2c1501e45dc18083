"""Host checks behind tests/test_gpu_conv_parity.py (no GPU):
  * conv_ref(float64) against the torch library functions it restates (F.conv1d, F.conv_transpose1d, F.prelu, F.elu, torch.tanh,
    torch.round), rtol 1e-12, over the whole case table of tests/conv_refs.py;
  * split_bound really bounds |conv_x3_model(float64) - conv_ref(float64)| element-wise, and is narrower than the 1e-4 * max|ref| it
    replaces;
  * ua2_debug_conv1d_plan: every case takes the kernel and (ntt, rt, tpw, gpu, npg, nw) the table says, and the table reaches every
    instantiation arm of ua2_conv1d."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_refs as cr
from conv_refs import ACT_ELU, ACT_NONE, ACT_PRELU, ACT_ROUND9, ACT_TANH, CASES, EDGE_CASES, F64

ALL = CASES + EDGE_CASES
X3 = [c for c in ALL if c.prec == 1]


def _ids(cases):
    return [c.name.replace(" ", "_") for c in cases]


def _set_env(c, monkeypatch):
    if c.env is None:
        monkeypatch.delenv("UA2_CONV_PIPE", raising=False)
    else:
        monkeypatch.setenv("UA2_CONV_PIPE", c.env)


def _torch_act(v, kind, alpha):
    if kind == ACT_PRELU:
        return F.prelu(v, torch.zeros(1, dtype=F64) if alpha is None else alpha.to(F64))
    return {ACT_NONE: lambda t: t, ACT_ELU: F.elu, ACT_TANH: torch.tanh, ACT_ROUND9: lambda t: torch.round(9 * t) / 9}[kind](v)


def _torch_ref(c, d):
    """The case through the torch library, float64."""
    x = _torch_act(d["x"].to(F64), c.pre, d["pre_alpha"])
    bias = None if d["bias"] is None else d["bias"].to(F64)
    if c.P > 1:                                                          # scalar24k.py:76-112 / conv.py:306-329: full transposed conv, then trims
        y = F.conv_transpose1d(x, d["w_t"].to(F64), bias, stride=c.P)[:, :, c.trim:c.trim + c.Tout]
    else:
        x = x.repeat_interleave(c.rep, dim=2)                            # scalar24k.py:136-138
        right = (c.Tout - 1) * c.stride + (c.K - 1) * c.dil + 1 - c.pad_left - x.shape[2]
        y = F.conv1d(F.pad(x, (c.pad_left, right)), d["w_rows"].to(F64), bias, stride=c.stride, dilation=c.dil)
    assert y.shape[2] == c.Tout
    y = _torch_act(y, c.post, d["post_alpha"])
    if d["fused2"] is not None:
        w2, b2, a2 = d["fused2"]
        y = F.prelu(F.conv1d(y, w2.to(F64), None if b2 is None else b2.to(F64)), torch.zeros(1, dtype=F64) if a2 is None else a2.to(F64))
    return y if d["residual"] is None else y + d["residual"].to(F64)


@pytest.mark.parametrize("c", ALL, ids=_ids(ALL))
def test_conv_ref_is_the_torch_composition(c):
    c.check_geometry()
    d = cr.make_inputs(c)
    assert all(bool(torch.isfinite(t).all()) for t in d.values() if torch.is_tensor(t))
    got, want = cr.conv_ref(d["x"], d["w_rows"], **cr.ref_kwargs(c, d)), _torch_ref(c, d)
    assert got.shape == want.shape == (c.B, c.Cout, c.Tout) and got.dtype == F64
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-12, atol=1e-13 * max(1.0, float(want.abs().max())))


def test_table_holds_the_paddings_and_forms_it_promises():
    """Both causal paddings of tests/test_gpu_conv.py (stride 1: d(k-1); strided: k_eff - stride with the right pad implied by Tout),
    symmetric padding, in_repeat, and the phase form of a transposed conv with and without a trim."""
    assert any(c.pad == "causal" and c.stride == 1 and c.dil > 1 and c.P == 1 for c in CASES)
    assert any(c.pad == "causal" and c.stride > 1 and (c.Tout - 1) * c.stride + (c.K - 1) * c.dil + 1 - c.pad_left > c.T for c in CASES)
    assert any(c.pad == "sym" and c.P == 1 for c in CASES) and any(c.rep == 2 for c in CASES)
    assert any(c.P > 1 and c.trim == 0 for c in CASES) and any(c.P > 1 and c.trim > 0 for c in CASES)
    for prec in (0, 1):                                                   # the argument paths of the parity file, per precision
        sel = [c for c in CASES if c.prec == prec]
        assert any(c.pca for c in sel) and any(c.pre == ACT_PRELU for c in sel) and any(not c.bias for c in sel) and any(c.B == 3 for c in sel)
        assert any(c.res and c.P > 1 and c.trim for c in sel) and any(c.res and c.rep == 2 for c in sel)
    for kernel in (1, 2):
        assert any(c.plan[0] == kernel and c.fused == (False, False) and not c.bias for c in CASES)
    assert len({c.name for c in ALL}) == len(ALL)


def test_round9_inputs_stay_away_from_ties():
    """A condition on the inputs: rint(9x) must not depend on whether 9x was rounded to fp32 first (that rounding moves 9x by at most
    2^-24 |9x|; twice that is kept clear on either side of every tie)."""
    for c in ALL:
        if c.pre == ACT_ROUND9:
            v = 9 * cr.make_inputs(c)["x"].to(F64)
            assert bool((((v - torch.floor(v)) - 0.5).abs() > 2.0 ** -23 * v.abs()).all()), c


@pytest.mark.parametrize("c", X3, ids=_ids(X3))
def test_split_bound_holds_and_is_not_vacuous(c):
    d = cr.make_inputs(c)
    kw = cr.ref_kwargs(c, d)
    ref = cr.conv_ref(d["x"], d["w_rows"], **kw)
    model = cr.conv_x3_model(d["x"], d["w_rows"], **kw)
    bound = cr.split_bound(d["x"], d["w_rows"], **kw)
    assert bound.shape == ref.shape and bool((bound >= 0).all())
    worst = float(((model - ref).abs() - bound * (1 + 1e-9)).max())     # 1e-9: the bound itself is evaluated in float64, and is attained
    assert worst <= 0.0, f"{c}: contract is {worst:.3e} further from the conv than split_bound allows"   # where a window holds one operand
    apriori = cr.split_bound(d["x"], d["w_rows"], apriori=True, **kw)
    assert bool((bound <= apriori * (1 + 1e-9)).all())                  # the closed form SPLIT_C * 2^-18 * sum |w| |pre(x)| dominates
    assert float(bound.max()) < 1e-4 * float(ref.abs().max()), (c, float(bound.max()), float(ref.abs().max()))
    assert float((model - ref).abs().max()) > 0.0                       # the contract is not the conv: the check above is not empty


def test_contract_notices_a_truncated_split_and_a_lost_low_product():
    """The two mistakes the contract check of the parity file exists for, made on the host: lo = truncate(x - hi) instead of RNE, and
    the wl * xh product dropped.  Each moves the result by more than the bar the GPU check grants (kr.bar of the fp32 replay)."""
    import kernel_refs as kr
    c = next(c for c in CASES if c.name.startswith("x3p 7,1,1 upt>1"))
    d = cr.make_inputs(c)
    kw = cr.ref_kwargs(c, d)
    model = cr.conv_x3_model(d["x"], d["w_rows"], **kw)
    e_ref = float((cr.conv_x3_model(d["x"], d["w_rows"], dt=torch.float32, **kw).to(F64) - model).abs().max())
    bar = kr.bar(e_ref, max(1.0, float(model.abs().max())))
    geo = dict(K=c.K, stride=c.stride, dilation=c.dil, pad_left=c.pad_left, tq=c.Tout, in_repeat=c.rep)
    x32 = d["x"].float()
    xh = kr.bf16_round(x32)
    r = x32 - xh
    xl_trunc = (r.view(torch.int32) & -65536).view(torch.float32)       # the low 16 bits cut off
    wh, wl = cr.split_w(d["w_rows"])
    shift = cr._taps((xl_trunc - kr.bf16_round(r)).to(F64), wh.to(F64), **geo)
    assert float(shift.abs().max()) > bar
    assert float(cr._taps(xh.to(F64), wl.to(F64), **geo).abs().max()) > bar


# ---- plans ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", ALL, ids=_ids(ALL))
def test_case_takes_the_plan_it_names(c, monkeypatch):
    _set_env(c, monkeypatch)
    got = cr.plan_of(c)
    assert all(w is None or w == g for w, g in zip(c.plan, got)), f"{c}: plan {got}, the table says {c.plan}"
    if c in CASES:
        assert None not in c.plan


# the arms of ua2_conv1d (csrc/ua2_conv.hip): UA2_X3P_INSTANCES x ntt, the 8-wave fused-128 arm, the plain kernel's <NTT, RPW> with
# its rt, the exact kernel's <NTT>
X3P_ARMS = {(7, 1, 1), (7, 1, 2), (7, 1, 3), (1, 1, 2), (1, 1, 4), (2, 1, 2), (2, 1, 4), (2, 2, 1), (2, 2, 2), (4, 2, 1), (4, 2, 2), (4, 4, 1),
            (8, 4, 1)}
WANTED = ({("x3p arm", a) for a in X3P_ARMS} | {("x3p 8 waves",)} | {(k, "ntt", n) for k in ("exact", "x3", "x3p") for n in (1, 2, 4)} |
          {("x3 RPW", r) for r in (1, 2)} | {("x3 rt", r) for r in (1, 2, 4)} | {("x3p UPT1", u) for u in (True, False)})
UNREACHABLE = set()           # (arm, reason) pairs would go here: every arm above is reachable through the launcher's rules


def test_table_reaches_every_arm_of_the_launcher(monkeypatch):
    reached = set()
    for c in CASES:
        _set_env(c, monkeypatch)
        kernel, ntt, rt, tpw, gpu, npg, nw = cr.plan_of(c)
        reached.add((("exact", "x3", "x3p")[kernel], "ntt", ntt))
        if kernel == 1:
            reached |= {("x3 RPW", gpu), ("x3 rt", rt)}
        if kernel == 2 and nw == 8:
            assert (ntt, gpu * c.K, gpu, npg) == (4, 7, 1, 2)
            reached.add(("x3p 8 waves",))
        elif kernel == 2:
            reached |= {("x3p arm", (gpu * c.K, gpu, npg)), ("x3p UPT1", -(-c.Cin // 32) == gpu)}
    assert reached <= WANTED, reached - WANTED
    assert WANTED - reached == {arm for arm, _ in UNREACHABLE}, sorted(WANTED - reached, key=str)


def test_plan_hook_reads_the_environment_and_rejects_like_the_launcher(monkeypatch):
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import Ua2Error
    geo = dict(B=2, Cin=64, Cout=64, Tin=4097, Tout=4097, K=7, precision=1)
    monkeypatch.delenv("UA2_CONV_PIPE", raising=False)
    auto = ops.conv1d_plan(**geo)
    assert auto["kernel"] == 2
    monkeypatch.setenv("UA2_CONV_PIPE", "off")
    assert ops.conv1d_plan(**geo)["kernel"] == 1
    monkeypatch.setenv("UA2_CONV_PIPE", "2,0,3,0")
    forced = ops.conv1d_plan(**geo)
    assert (forced["kernel"], forced["ntt"], forced["tpw"]) == (2, 2, 3)
    monkeypatch.setenv("UA2_CONV_PIPE", "nonsense")
    assert ops.conv1d_plan(**geo) == auto
    monkeypatch.delenv("UA2_CONV_PIPE")
    with pytest.raises(Ua2Error, match="phase mode"):
        ops.conv1d_plan(**dict(geo, out_phases=2, stride=2))
    with pytest.raises(Ua2Error, match="fused residual unit"):
        ops.conv1d_plan(**dict(geo, Cout=96, Cin=96, fused=True))
    with pytest.raises(Ua2Error, match="precision"):
        ops.conv1d_plan(**dict(geo, precision=2))
