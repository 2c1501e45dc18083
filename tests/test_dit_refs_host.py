"""Host checks behind tests/test_gpu_dit_parity.py (no GPU), over the case table of tests/dit_refs.py:
  * the fp32 plan of dit_contract is oracle.dit_forward bit for bit (from the input and restarted from every tap), the oracle's
    float64 evaluation sits within kr.bar of it, and the restatement built from tests/linear_refs.py / tests/kernel_refs.py agrees
    with the oracle in float64 to 1e-12;
  * every wrong model lands at least 10 x over the case's fp32 bar at the stage where its defect enters (a relative RMS over the
    output lets a wrong last frame of up to 62 % through at the bf16 bar of test_dit_forward_vs_oracle);
  * the inputs are worth judging: every block changes the residual stream by at least a tenth of its RMS;
  * the bf16 bars are fair: a second fp32 evaluation in another legal summation order sits inside kr.bar(E_ref) at every stage the
    device test asserts, free-running and teacher-forced."""
import pytest
import torch

import dit_refs as dr
import kernel_refs as kr
from dit_refs import F32, F64
from oracle import codec_model_oracle as oc

CASE_NAMES = list(dr.CASES)
BF16 = [(plan, name) for plan in ("bf16_invariant", "bf16_free") for name in dr.BF16_CASES[plan]]
BF16.append(("bf16_free", "one-page"))          # the other shape of test_graph_replays_and_per_shape_caches (judged at the output)


def _hd(c):
    return c["cfg"]["heads"], c["cfg"]["head_dim"]


def _oracle(c, dt):
    taps = []
    y = oc.dit_forward(c["sd"], c["x"], torch.full((c["B"],), c["t"]), *_hd(c), dt=dt, taps=taps)
    assert taps[-1] is y and len(taps) == dr.n_stages(c["cfg"])
    return taps


def test_fp32_contract_is_the_oracle_bit_for_bit():
    c = dr.case_inputs("one-page")
    plain = oc.dit_forward(c["sd"], c["x"], torch.full((c["B"],), c["t"]), *_hd(c))
    taps = _oracle(c, F32)
    assert plain.dtype == F32 and torch.equal(plain, taps[-1])                 # taps change nothing
    got = dr.reference("one-page", "fp32", F32)
    assert all(torch.equal(a, b) for a, b in zip(got, taps))
    for s in range(c["cfg"]["layers"] + 1):                                    # restarted from tap s: the same bits from there on
        again = dr.dit_contract(c["sd"], c["x"], c["t"], *_hd(c), "fp32", F32, start=(s, taps[s]))
        assert all(a is None for a in again[:s]) and all(torch.equal(a, b) for a, b in zip(again[s:], taps[s:]))
        one = dr.dit_contract(c["sd"], c["x"], c["t"], *_hd(c), "fp32", F32, start=(s, taps[s]), stop=s + 1)
        assert torch.equal(one[s + 1], taps[s + 1]) and all(a is None for a in one[s + 2:])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_float64_sits_within_the_bar_of_the_fp32_oracle(name):
    """... and the restatement from linear_refs / kernel_refs (what the bf16 plans and the wrong models are made of) is the oracle's
    formula: 1e-12 in float64.  E_ref of the fp32 plan is a few 1e-7 of scale, so the bar is 1e-6 ... 3e-6."""
    c = dr.case_inputs(name)
    r64, r32 = dr.reference(name, "fp32", F64), dr.reference(name, "fp32", F32)
    assert all(t.dtype == F64 for t in r64) and all(torch.equal(a, b) for a, b in zip(r64, _oracle(c, F64)))
    mine = dr.dit_contract(c["sd"], c["x"], c["t"], *_hd(c), "fp32", F64, ksum=dr.lr.ksum_ref)
    for s in range(dr.n_stages(c["cfg"])):
        err, e_ref, bar = dr.judge(f"{name}/fp32/host", dr.stage_name(c["cfg"], s), r32[s], r64[s], r32[s])
        assert 0.0 < err <= bar < 4e-6, (name, s, err, bar)
        assert dr.stage_err(mine[s], r64[s])[0] < 1e-12, (name, s)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_every_block_moves_the_residual_stream(name):
    """A condition on the inputs: a block whose update vanished next to the stream could be wrong unnoticed."""
    c = dr.case_inputs(name)
    r = dr.reference(name, "fp32", F64)
    rms = lambda t: float(t.pow(2).mean().sqrt())
    for l in range(c["cfg"]["layers"]):
        assert rms(r[l + 1] - r[l]) >= 0.1 * rms(r[l]), (name, l)


@pytest.mark.parametrize("kind", dr.WRONG_KINDS)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_wrong_models_land_far_over_the_fp32_bar(name, kind):
    """The float64 formula with one planted defect, judged like a device result at the stage where the defect enters: at least
    10 x the bar.  The few case has one sequence: the two defects that need a second one are the correct formula there, which is
    asserted instead."""
    c = dr.case_inputs(name)
    r64, r32 = dr.reference(name, "fp32", F64), dr.reference(name, "fp32", F32)
    s, got = dr.wrong_model(kind, c)
    bar = kr.bar(dr.stage_err(r32[s], r64[s])[0])
    err, where = dr.stage_err(got, r64[s])
    if kind in dr.NEEDS_TWO_SEQUENCES and c["B"] < 2:
        assert err < 1e-12
        return
    assert err >= 10.0 * bar, (name, kind, err, bar)
    if kind == "window":                                   # the worst element is where the defect is: a last frame that has a successor
        assert where[1] == c["T"] - 1 and where[0] < c["B"] - 1
    if kind == "positions":
        assert where[0] >= 1


@pytest.mark.parametrize("plan,name", BF16)
def test_bf16_bar_is_fair_to_another_summation_order(plan, name):
    """The bf16 contract evaluated in fp32 a second time, K dealt to four interleaved slabs added last to first, must pass the
    judgement the device gets: free-running from the first block on against the float64 contract, and each stage teacher-forced
    from the previous stage of its own stream.
    What the two fp32 evaluations differ by is not summation noise but operand elements that round to the other bf16 neighbour
    (2^-9 of one product).  A block meets hundreds of them and its E_ref is stable (1e-3 ... 3e-3 of scale).  proj_in does not:
    its only rounded operand that depends on a sum is ffn_2's, and at one-page that is 19 000 elements, which meet zero or one flip.
    Over the input seeds 9 and 40 ... 51 its E_ref ran from 9.6e-8 to 2.2e-4 and the other order's error from 8.8e-8 to 1.2e-4,
    independently of each other (seed 9, the case's: 1.4e-5 against E_ref 4.4e-7; seed 45: 1.2e-4 against 8.7e-7): a single flip
    that both evaluations are entitled to, and a lottery no bar made of E_ref is fair to.  So stage 0 of the bf16 plans is printed
    here and on the device, not asserted; proj_in is asserted under the fp32 plan (bar ~2e-6), and the bf16 judgement starts from
    the device's own stage 0."""
    c = dr.case_inputs(name)
    r64, r32 = dr.reference(name, plan, F64), dr.reference(name, plan, F32)
    other = dr.reference(name, plan, F32, ksum=dr.ksum_slabs4)
    exact = dr.reference(name, "fp32", F64)
    assert not any(torch.equal(a, b) for a, b in zip(other, r32)), "the second order gives other bits"
    n = dr.n_stages(c["cfg"])
    for s in range(n):
        err, e_ref, bar = dr.judge(f"{name}/{plan}/other-order", dr.stage_name(c["cfg"], s), other[s], r64[s], r32[s])
        if s >= 1:
            assert err <= bar, (name, plan, s, err, bar)
            # the contract is a statement of its own: further from the formula than from its fp32 replay
            assert dr.stage_err(r64[s], exact[s])[0] > e_ref, (name, plan, s)
    for s in range(n - 1):
        f64, f32 = (dr.dit_contract(c["sd"], c["x"], c["t"], *_hd(c), plan, dt, start=(s, other[s]), stop=s + 1, ksum=k)[s + 1]
                    for dt, k in ((F64, None), (F32, dr.lr.ksum_ref)))
        err, e_ref, bar = dr.judge(f"{name}/{plan}/other-order-forced", dr.stage_name(c["cfg"], s + 1), other[s + 1], f64, f32)
        assert err <= bar, (name, plan, s + 1, err, bar)


def test_judge_names_the_worst_frame_and_rejects_non_finite(capsys):
    ref = torch.zeros(2, 5, 3, dtype=F64)
    got = ref.clone()
    got[1, 4, 2] = 1e-3
    err, e_ref, bar = dr.judge("unit", "out", got, ref, ref.float())
    assert err == 1e-3 and e_ref == 0.0 and bar == 8 * 2.0 ** -24
    assert "PARITY dit unit out:" in capsys.readouterr().out and dr.stage_err(got, ref)[1] == (1, 4, 2)
    got[0, 1, 0] = float("nan")
    assert dr.stage_err(got, ref) == (float("inf"), (0, 1, 0))
