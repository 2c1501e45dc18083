"""The flow-matching DiT step on the device against its float64 anchor, per element and per block (tests/dit_refs.py; host side:
tests/test_dit_refs_host.py).  Transformer1DModel composes ua2_linear, ua2_attn, ua2_ew_fma and ua2_layernorm_rows launches — each
anchored on its own elsewhere — through project-specific logic that lives at particular rows: ProjectLayer's flat k-tap GEMMs over
[B (T + 2), C], the position table broadcast by ua2_ew_fma's modulo, DenseKV's row tables and padded query groups over part-filled
pages, the M > 16 switch, the packed hand-offs and the LayerNorm hand-over, the per-shape plan and graph caches.  A relative RMS
over the output cannot see one wrong row; every judgement here is max |got - ref64| / max(1, max |ref64|) over the elements of a
stage against kr.bar(E_ref), E_ref from the fp32 evaluation of the same contract on the same inputs.

fp32 plan: every stage against the float64 oracle (bar ~2e-6 of scale).  bf16 plans: (a) each block and the output teacher-forced
from the device's own previous stage, so that one block's roundings separate the two sides, and (b) the output free-running from
the input.  Stage 0 of the bf16 plans is printed, not asserted: see test_bf16_bar_is_fair_to_another_summation_order.
Measured (profiles/dit_parity.txt): fp32 err 1.6e-7 ... 6.2e-7 under bars of 1.0e-6 ... 4.4e-6, worst err / bar 0.28 (released
widths, block 0); bf16_invariant worst 0.39 (three-page, block 1 teacher-forced); bf16_free worst 0.50 (released widths, output
stage teacher-forced)."""
import contextlib

import pytest
import torch

import dit_refs as dr
from attn_decode_cases import LOUD
from dit_refs import F32, F64
from weights import seeded_tensor

pytestmark = pytest.mark.gpu
BF16 = [(plan, name) for plan in ("bf16_invariant", "bf16_free") for name in dr.BF16_CASES[plan]]
_models = {}


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    yield
    _models.clear()                 # the released-width plans go back to the allocator before the next module


def _build(name, plan, monkeypatch):
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models.transformer_1d_flow import Transformer1DModel
    for k in ("UA2_DIT_SUM_ORDER", "UA2_DIT_ATTN_SPLIT", "UA2_DIT_NO_LN_HANDOVER", "UA2_GEMM_NO_KSPLIT", "UA2_GEMM2_BMT"):
        monkeypatch.delenv(k, raising=False)
    c = dr.case_inputs(name)
    cfg = c["cfg"]
    m = Transformer1DModel(num_attention_heads=cfg["heads"], attention_head_dim=cfg["head_dim"], in_channels=cfg["in_channels"],
                           out_channels=cfg["out_channels"], num_layers=cfg["layers"])
    m.load_state_dict(c["sd"])
    if plan != "fp32":
        m.sum_order = dr.SUM_ORDER[plan]
    return m.cuda().prepare(torch.float32 if plan == "fp32" else torch.bfloat16)


def _model(name, plan, monkeypatch):
    """One prepared model per (widths, plan) for the tests that leave its caches as they found them."""
    key = (id(dr.CASES[name]["cfg"]), dr.CASES[name]["seed"], plan)
    if key not in _models:
        _models[key] = _build(name, plan, monkeypatch)
    return _models[key]


@contextlib.contextmanager
def _launcher(plan, monkeypatch):
    """bf16_free: 296 rows give the order-free kernel too few tiles for the launcher's cost rule at these widths (2 x N / 256 tiles of
    256 rows, 3 x N / 256 of 128), so the tile form is pinned to 128 rows, as test_dit_order_free_plan_vs_oracle_at_640_rows does."""
    from uniaudio2_amd._lib import lib
    if plan == "bf16_free":
        monkeypatch.setenv("UA2_GEMM2_BMT", "8")
    lib.ua2_debug_refresh_env()
    try:
        yield lib
    finally:
        monkeypatch.delenv("UA2_GEMM2_BMT", raising=False)
        lib.ua2_debug_refresh_env()


def _run(m, c, x=None, t=None, taps=None):
    x = c["x"] if x is None else x
    m.ensure_plan(c["B"], c["T"], "cuda")
    dr.check_plan(m._kvs[(c["B"], c["T"])], c["B"], c["T"], c["cfg"]["heads"])       # index-carrying inputs, on the host, before the launches
    return m(x.cuda(), c["t"] if t is None else t, use_graph=False, taps=taps)


def _assert_all(results):
    bad = [(tag, err, bar) for tag, (err, _, bar) in results if not err <= bar]
    assert not bad, bad


@pytest.mark.parametrize("name", list(dr.CASES))
def test_fp32_plan_every_stage_within_the_bar_of_float64(name, monkeypatch):
    c = dr.case_inputs(name)
    m = _model(name, "fp32", monkeypatch)
    with pytest.raises(RuntimeError):
        m(c["x"].cuda(), c["t"], taps=[])                                       # taps and a recorded step do not go together
    taps = []
    with _launcher("fp32", monkeypatch):
        y = _run(m, c, taps=taps)
    assert len(taps) == dr.n_stages(c["cfg"]) and torch.equal(y, taps[-1]) and y.shape == (c["B"], c["T"], c["cfg"]["out_channels"])
    r64, r32 = dr.reference(name, "fp32", F64), dr.reference(name, "fp32", F32)
    _assert_all([(s, dr.judge(f"{name}/fp32", dr.stage_name(c["cfg"], s), taps[s], r64[s], r32[s])) for s in range(len(taps))])


@pytest.mark.parametrize("plan,name", BF16)
def test_bf16_plans_teacher_forced_per_block_and_free_running(plan, name, monkeypatch):
    c = dr.case_inputs(name)
    cfg, hd = c["cfg"], (c["cfg"]["heads"], c["cfg"]["head_dim"])
    m = _model(name, plan, monkeypatch)
    taps = []
    with _launcher(plan, monkeypatch) as lib:
        n0 = lib.ua2_debug_kernel_launches(b"gemm2")
        y = _run(m, c, taps=taps)
        n_gemm2 = lib.ua2_debug_kernel_launches(b"gemm2") - n0
    # which kernel ran: q|k|v, to_out, ff.net.0, ff.net.2 of every block and proj_in's Linear reach the order-free kernel (the conv taps
    # have K = 304 / 1040, no multiple of 32), the invariant plan never does
    if plan == "bf16_free":
        assert n_gemm2 >= 4 * cfg["layers"] + 1, n_gemm2
    else:
        assert n_gemm2 == 0, n_gemm2
    assert len(taps) == dr.n_stages(cfg) and torch.equal(y, taps[-1])
    results = []
    for s in range(cfg["layers"] + 1):                                          # (a) stage s + 1 from the device's own stage s
        f64, f32 = (dr.dit_contract(c["sd"], c["x"], c["t"], *hd, plan, dt, start=(s, taps[s]), stop=s + 1)[s + 1] for dt in (F64, F32))
        results.append((s + 1, dr.judge(f"{name}/{plan}/forced", dr.stage_name(cfg, s + 1), taps[s + 1], f64, f32)))
    r64, r32 = dr.reference(name, plan, F64), dr.reference(name, plan, F32)
    results.append(("free", dr.judge(f"{name}/{plan}/free", "out", y, r64[-1], r32[-1])))           # (b)
    dr.judge(f"{name}/{plan}/info", "proj_in", taps[0], r64[0], r32[0])
    _assert_all(results)


@pytest.mark.parametrize("plan", dr.PLANS)
def test_unused_kv_slots_are_never_read(plan, monkeypatch):
    """three-page: the third page of each sequence holds 20 frames.  Whatever the other 44 slots hold — zeros or LOUD — the step
    gives the same bits."""
    c = dr.case_inputs("three-page")
    m = _model("three-page", plan, monkeypatch)
    m.ensure_plan(c["B"], c["T"], "cuda")
    kv = m._kvs[(c["B"], c["T"])]
    outs = []
    with _launcher(plan, monkeypatch):
        for fill in (0.0, LOUD):
            kv.k.fill_(fill)
            kv.v.fill_(fill)
            outs.append(_run(m, c).clone())
    kv.k.zero_()
    kv.v.zero_()
    assert bool(torch.isfinite(outs[0]).all()) and torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("plan", ["fp32", "bf16_free"])
def test_graph_replays_and_per_shape_caches(plan, monkeypatch):
    """The recorded step equals the eager one bit for bit; a replay with another input and another timestep, a call at another
    (B, T) and a call back at the first are each judged against the contract, not against an earlier call (a stale plan, graph
    input or step embedding would still agree with that)."""
    big, small = dr.case_inputs("three-page"), dr.case_inputs("one-page")
    m = _build("three-page", plan, monkeypatch)
    x2, t2 = seeded_tensor(tuple(big["x"].shape), 35, std=1.0), 0.25
    with _launcher(plan, monkeypatch):
        eager = _run(m, big).clone()
        first = m(big["x"].cuda(), big["t"]).clone()
        second = m(x2.cuda(), t2).clone()
        other = m(small["x"].cuda(), small["t"]).clone()
        back = m(big["x"].cuda(), big["t"]).clone()
    assert torch.equal(first, eager) and torch.equal(back, first)
    assert set(m._graphs) == set(m._kvs) == {(big["B"], big["T"]), (small["B"], small["T"])}
    results = []
    for tag, name, got, kw in (("first", "three-page", first, {}), ("second", "three-page", second, dict(x=x2, t=t2, key="second")),
                               ("other-shape", "one-page", other, {}), ("back", "three-page", back, {})):
        r64, r32 = dr.reference(name, plan, F64, **kw), dr.reference(name, plan, F32, **kw)
        results.append((tag, dr.judge(f"{name}/{plan}/graph-{tag}", "out", got, r64[-1], r32[-1])))
    _assert_all(results)


def test_guided_euler_solve_with_the_real_dit(monkeypatch):
    """BASECFM.solve_euler over the DiT itself (toy widths, one utterance, 37 frames, 2 steps, 5 in-context frames, guidance 1.5,
    fp32 plan): the whole-solve recording equals the eager loop bit for bit, and both sit within the bar of the oracle's solve_euler
    with the float64 dit_forward as estimator."""
    from oracle import codec_model_oracle as oc
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models.AudioDiffusion1D import BASECFM
    monkeypatch.delenv("UA2_EULER_NO_GRAPH", raising=False)
    c = dr.case_inputs("one-page")
    cfg = c["cfg"]
    L, T, n_inc = cfg["out_channels"], 37, 5
    D = cfg["in_channels"] - 2 * L
    noise, mu = seeded_tensor((1, T, L), 61, std=1.0), seeded_tensor((1, T, D), 63, std=1.0)
    inc = seeded_tensor((1, T, L), 62, std=1.0)
    inc[:, n_inc:] = 0.0
    t_span = torch.linspace(0, 1, 3)
    cfm = BASECFM(_build("one-page", "fp32", monkeypatch))
    with _launcher("fp32", monkeypatch):
        recorded = cfm.solve_euler(noise.cuda(), inc.cuda(), n_inc, t_span, mu.cuda(), guidance_scale=1.5).clone()
        replayed = cfm.solve_euler(noise.cuda(), inc.cuda(), n_inc, t_span, mu.cuda(), guidance_scale=1.5).clone()
        eager = cfm.solve_euler(noise.cuda(), inc.cuda(), n_inc, t_span, mu.cuda(), guidance_scale=1.5, use_graph=False).clone()
    assert len(cfm._graphs) == 1 and torch.equal(recorded, eager) and torch.equal(replayed, recorded)
    ref = {}
    for dt in (F64, F32):
        est = lambda inp, t, dt=dt: oc.dit_forward(c["sd"], inp, t, cfg["heads"], cfg["head_dim"], dt=dt)
        ref[dt] = oc.solve_euler(est, noise.to(dt).clone(), inc.to(dt), n_inc, t_span.to(dt), mu.to(dt), 1.5)
    assert ref[F64].dtype == F64
    _assert_all([("euler", dr.judge("euler/fp32", "latent", recorded, ref[F64], ref[F32]))])
