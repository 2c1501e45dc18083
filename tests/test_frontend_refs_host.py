"""Host-side pins of tests/frontend_refs.py, the references tests/test_gpu_frontend_parity.py holds the device to (no GPU needed).

Resampler.  torchaudio is not installed, so the published algorithm is pinned by two independent statements instead of the package:
  * the polyphase form (fp32 bank, frames, padding, phases) equals the plain double sum over the windowed sinc to the bank's fp32
    rounding, sum|x| max|h| 2^-24, on every rate pair the product runs;
  * it carries analytic tones to the new rate within 2e-3: four times the worst ripple of the float64 reference (1.0e-3 here:
    16 -> 24 kHz at 3 kHz), two orders below what a slip of one output sample costs (>= 0.258).  A tone is used on a pair only where
    it lies in the flat part of the pass band, f <= c / 2 with c = 0.99 min(orig, new) / 2 the cut-off: the Hann-windowed sinc of
    6 zero crossings rolls off over c (1 +- 1/6), and at 8 kHz the 3 kHz tone (c = 3.96 kHz) already sits on that slope, where the
    ALGORITHM itself is 1.8e-2 below unity.
  The product's own bank (reason_tokenizer.resample_kernel) and the CPU oracle's resample are held to the same reference.
Log-mel.  Every clip of the GPU test stays within LOGMEL_MAX_E_REF in its fp32 replay (an ill-conditioned input would set its own
bar too wide), and logmel_variant at its defaults is logmel_ref bit for bit.
Wrong models.  Each must exceed the bar the GPU test applies to the case it is shown on — the proof that the inputs can see it."""
import math

import pytest
import torch

import frontend_refs as fr
import kernel_refs as kr
import whisper_ref as wr

F64, F32 = fr.F64, fr.F32
RT = "uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.reason_tokenizer"
HOST_L = {p: 2500 + 7 * i for i, p in enumerate(fr.RESAMPLE_PAIRS)}      # L ~ 2-3 k, a different residue per pair
TONE_BAR, SLIP_MIN = 2e-3, 0.25      # a slip of one output sample at 1 kHz / 24 kHz: 2 sin(pi / 24) = 0.261, 0.2588 on the sample grid


def _noise(pair):
    return fr.resample_inputs(HOST_L[pair], 7800 + fr.RESAMPLE_PAIRS.index(pair))["noise"]


def _bar(x, orig, new):
    ref = fr.resample_ref(x, orig, new, F64)
    e = float((fr.resample_ref(x, orig, new, F32).to(F64) - ref).abs().max())
    return ref, e, kr.bar(e, max(1.0, float(ref.abs().max())))


@pytest.mark.parametrize("orig,new", fr.RESAMPLE_PAIRS)
def test_polyphase_is_the_direct_double_sum(orig, new):
    inputs = fr.resample_inputs(HOST_L[(orig, new)], 7800)
    for name in ("noise", "impulse_first", "impulse_last"):
        x = inputs[name]
        ref = fr.resample_ref(x, orig, new, F64)
        direct = fr.resample_direct(x, orig, new)
        assert ref.shape == direct.shape == (1, math.ceil(new * x.shape[1] / orig))
        err, bound = float((ref - direct).abs().max()), fr.resample_direct_bound(x, orig, new)
        print(f"resample {orig}->{new} {name}: |polyphase - direct| {err:.3e} (bound {bound:.3e})")
        assert err <= bound


@pytest.mark.parametrize("orig,new", fr.RESAMPLE_PAIRS)
def test_resampler_carries_a_tone(orig, new):
    cutoff = fr.ROLLOFF * min(orig, new) / 2.0
    tones = [f for f in (1000.0, 3000.0) if f <= cutoff / 2.0]
    assert 1000.0 in tones
    L = HOST_L[(orig, new)]
    for f in tones:
        x = torch.sin(2 * math.pi * f * torch.arange(L, dtype=F64) / orig)[None]
        y = fr.resample_ref(x, orig, new, F64)
        j = torch.arange(y.shape[1], dtype=F64)
        want = torch.sin(2 * math.pi * f * j / new)[None]
        slip = torch.sin(2 * math.pi * f * (j - 1.0) / new)[None]
        s = slice(200, y.shape[1] - 200)
        err, cost = float((y - want)[:, s].abs().max()), float((slip - want)[:, s].abs().max())
        print(f"resample {orig}->{new} tone {f:.0f} Hz: ripple {err:.3e}, a one-sample slip costs {cost:.3e}")
        assert cost >= SLIP_MIN and err <= TONE_BAR


@pytest.mark.parametrize("orig,new", fr.RESAMPLE_PAIRS)
def test_product_bank_and_oracle_are_the_reference(orig, new):
    import importlib
    from oracle.codec_oracle import resample as oracle_resample
    kern, width, o, n = importlib.import_module(RT).resample_kernel(orig, new)
    assert (width, o, n) == fr.resample_geometry(orig, new)[:3]
    assert torch.equal(kern, fr.resample_bank(orig, new)), "the product's fp32 filter bank is not the reference's, bit for bit"
    x = _noise((orig, new))
    ref, e, bar = _bar(x, orig, new)
    got = oracle_resample(x, orig, new)
    assert got.shape == ref.shape and float((got.to(F64) - ref).abs().max()) <= bar
    assert fr.resample_ref(x, orig, orig) is x


@pytest.mark.parametrize("orig,new", fr.RESAMPLE_PAIRS)
def test_wrong_resamplers_exceed_the_bar(orig, new):
    x = _noise((orig, new))
    ref, e, bar = _bar(x, orig, new)
    assert bar <= 2e-6                                               # the project's rule: about 1e-6 at scale 1
    wrong = dict(delay=dict(delay=1), pad_swapped=dict(pad_swapped=True))
    if fr.resample_geometry(orig, new)[2] > 1:                        # 48 -> 24 kHz has one phase: nothing to reverse
        wrong["reverse_phases"] = dict(reverse_phases=True)
    for name, kw in wrong.items():
        err = float((fr.resample_ref(x, orig, new, F64, **kw) - ref).abs().max())
        print(f"resample {orig}->{new} wrong model {name}: {err:.3e} (bar {bar:.3e})")
        assert err > 100 * bar, name
    # the impulses see both paddings: a delayed impulse at the last sample falls off the end, swapped padding moves the first
    imp = fr.resample_inputs(HOST_L[(orig, new)], 0)
    for name, kw, which in (("delay", dict(delay=1), "impulse_last"), ("pad_swapped", dict(pad_swapped=True), "impulse_first")):
        r = fr.resample_ref(imp[which], orig, new, F64)
        assert float((fr.resample_ref(imp[which], orig, new, F64, **kw) - r).abs().max()) > 100 * kr.bar(0.0, 1.0), (name, which)


def test_resample_cases_and_prefix_rule():
    cases = fr.resample_cases()
    width, o, n, _ = fr.resample_geometry(24000, 16000)
    assert (width, o, n) == (10, 3, 2)
    frames = lambda L: (L + 2 * width + o - (2 * width + o)) // o + 1  # frames of 2 width + o taps every o samples of the padded signal
    assert [frames(L) for L in (45, 48, 381, 384)] == [16, 17, 128, 129]
    assert frames(fr.segment_len()) == fr.segment_len() // 3 + 1 == 240081
    assert cases["8k-24k L8001"][:2] == (8000, 24000) and fr.resample_bank(8000, 24000).shape == (3, 15)
    # prefix rule: the outputs it names are untouched by whatever follows the first L1 samples, the next output is not
    for orig, new in ((24000, 16000), (22050, 24000)):
        x = _noise((orig, new))
        L1 = 1201
        k = fr.prefix_outputs(L1, orig, new)
        full, head = fr.resample_ref(x, orig, new, F64), fr.resample_ref(x[:, :L1].contiguous(), orig, new, F64)
        assert 0 < k <= head.shape[1] and torch.equal(full[:, :k], head[:, :k])
        assert not torch.equal(full[:, :head.shape[1]], head)


# ---- log-mel ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", fr.LOGMEL_CASES)
def test_logmel_inputs_count_and_variant_is_the_reference(case):
    ref, emax, erms, scale = fr.logmel_refs(case)
    x = torch.from_numpy(fr.logmel_clip(case))[None]
    print(f"logmel {case}: fp32 replay max {emax:.3e} rms {erms:.3e}, scale {scale:.3f}")
    assert ref.shape == (80, 3000) and emax <= fr.LOGMEL_MAX_E_REF
    assert torch.equal(fr.logmel_variant(x)[0], ref)
    if case in ("c", "floor"):
        assert torch.equal(ref, torch.full_like(ref, -1.5))
    if case == "quiet_click":                                        # the clamp is active almost everywhere
        assert float(ref.min()) > -1.5 and float((ref[:, :625] == ref.min()).double().mean()) > 0.9      # ... of the frames that hold signal
    if case.startswith("n") and int(case[1:]) < wr.N_SAMPLES - 400:   # frames past the signal sit at the floor or the clamp
        assert float(ref[:, -1].max()) == max(-1.5, float(ref.max()) - 2.0)


CONSTANT = ("c", "floor")                                             # -1.5 everywhere: only a missing floor can show
WRONG_ON = dict(symmetric_hann=[c for c in fr.LOGMEL_CASES if c not in CONSTANT], edge_replicate=[c for c in fr.LOGMEL_CASES if c not in CONSTANT],
                last_frames=[c for c in fr.LOGMEL_CASES if c not in CONSTANT], no_floor=["c", "n1", "floor"])


@pytest.mark.parametrize("wrong", [w for w in fr.LOGMEL_WRONG if w != "batch_max"])
def test_wrong_logmels_exceed_the_bar(wrong):
    for case in WRONG_ON[wrong]:
        ref, emax, erms, scale = fr.logmel_refs(case)
        got = fr.logmel_variant(torch.from_numpy(fr.logmel_clip(case))[None], **fr.LOGMEL_WRONG[wrong])[0]
        err, rms = fr.max_rms(got, ref)
        assert err > 10 * kr.bar(emax, scale), (wrong, case, err)
    # the right-hand reflection exists only when the last sample is signal: edge-replicate shows in the LAST frame from 480 000 on
    if wrong == "edge_replicate":
        for case in ("n480000", "n480001", "n480160"):
            ref, emax, _, scale = fr.logmel_refs(case)
            got = fr.logmel_variant(torch.from_numpy(fr.logmel_clip(case))[None], pad="replicate")[0]
            assert float((got[:, -1] - ref[:, -1]).abs().max()) > 10 * kr.bar(emax, scale), case


def test_batch_rows_count_and_a_batch_wide_clamp_shows():
    x = fr.logmel_batch()
    assert x.shape == (3, wr.N_SAMPLES + 160)
    ref, emax, erms, scale = fr.logmel_stats(x)
    assert max(emax) <= fr.LOGMEL_MAX_E_REF
    tops = [float(r.max()) for r in ref]
    assert tops[0] - tops[1] > 0.5 and tops[1] - tops[2] > 0.5          # every clip's maximum is its own
    got = fr.logmel_variant(x, max_over="batch")
    for i in (1, 2):
        assert fr.max_rms(got[i], ref[i])[0] > 10 * kr.bar(emax[i], scale[i])
    for i in range(3):                                                # a row's reference does not depend on the batch
        assert torch.equal(wr.logmel_ref(x[i:i + 1], dtype=F64)[0], ref[i])


# ---- encoder ----------------------------------------------------------------------------------------------------------------

def test_rounding_hook_is_off_by_default_and_models_bf16():
    cfg, sd, mels = fr.encoder_inputs("p72")
    a, sa = wr.encoder_ref(sd, cfg, mels)
    b, sb = wr.encoder_ref(sd, cfg, mels, rnd=lambda t: t)
    assert torch.equal(a, b) and torch.equal(sa, sb)
    r = fr.encoder_refs("p72")
    assert r["e32_last"] < 1e-5 and r["e32_stem"] < 1e-5
    # bf16 operands: relative 2^-9 per operand over K = 128 .. 384 terms on values of a few units
    assert 1e-3 < r["em_stem"] < 3e-2 and 1e-3 < r["em_last"] < 1e-1


def test_odd_length_reads_the_right_zero_pad():
    """T = 149: position 74 of conv2 reads frames 147, 148 and the zero pad; torch's own conv1d agrees with the gathered-taps form."""
    cfg, sd, mels = fr.encoder_inputs("oddT")
    assert mels.shape == (3, 80, 149)
    sd64 = {k: v.double() for k, v in sd.items()}
    last, stem = wr.encoder_ref(sd64, cfg, mels.double())
    plain, pstem = wr.encoder_ref(sd64, cfg, mels.double(), plain=True)
    assert last.shape == (3, 75, 192) and float((last - plain).abs().max()) < 1e-12 and float((stem - pstem).abs().max()) < 1e-12
