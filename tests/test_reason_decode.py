"""Host logic of the reasoning-conditioned decode (ReasoningTokenizer.token2audio / detokenize / detokenize_batch) against the
REFERENCE's own token2audio: tests/golden/reason_decode.npz was produced by tests/golden/make_golden_reason_decode.py, which
runs it on the deterministic stand-ins of tests/golden/reason_decode_stub.py.  Checked here on the same stand-ins, on the CPU:
rec windows, in-context chain, random draws, cross-fade and crop bit for bit for every length; the first window's reason codes
equal the reference's; later windows follow the documented rule (reason codes [111 k, 111 k + 150)) and therefore differ from
the reference's recorded [0, 150) — the divergence is deliberate (reason_tokenizer.reason_window_plan)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from reason_decode_stub import (SEED, T_CASES, WAVE_STRIDE, NoisyStubReasonModel, StubReasonModel, make_reason_codes,  # noqa: E402
                                reason_len)
from tokenizer_stub import StubCodec, make_codes, wave_digest  # noqa: E402

from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.reason_tokenizer import (ReasoningTokenizer, reason_window_plan,  # noqa: E402
                                                                                 window_plan)

G = np.load(os.path.join(HERE, "golden", "reason_decode.npz"))


def tiled_reason(T_q, n_windows):
    """The documented rule restated independently: self-concatenate the stream until it covers every window, then window k
    is [111 k, 111 k + 150).  (Doubling a sequence repeats it with its own period, so for the lengths here this is the
    periodic extension of the reference's tiled stream.)"""
    r = make_reason_codes(T_q)[0]
    n = 150 if T_q < 150 else T_q
    if (n - 39) % 111:
        n = -(-(n - 39) // 111) * 111 + 39
    while r.shape[-1] < n:
        r = torch.cat([r, r], -1)
    r = r[:, :n]
    need = (n_windows - 1) * 111 + 150
    while r.shape[-1] < need:
        r = torch.cat([r, r], -1)
    return [r[:, 111 * k:111 * k + 150] for k in range(n_windows)]


def check_t2a(T, model, wave, exact=True):
    k = f"t2a_{T}_"
    calls = model.calls
    assert len(calls) == G[k + "windows"].shape[0] == len(model.reason_windows)
    for i, c in enumerate(calls):
        np.testing.assert_array_equal(c["codes"][0].numpy(), G[k + "windows"][i].astype(np.int64))
        assert c["incontext"] == int(G[k + "incontext"][i]) and c["latent_length"] == int(G[k + "latent_length"][i]) == 750
        assert c["steps"] == 7
        ic = c["incontext"]
        np.testing.assert_array_equal(c["true"][0, ic:ic + 3, :5].numpy(), G[k + "noise"][i])
        np.testing.assert_array_equal(c["true"][0, -2:, -5:].numpy(), G[k + "noise_tail"][i])
        if exact or ic == 0:
            np.testing.assert_array_equal(c["true"][0, :2, :5].numpy(), G[k + "ctx_head"][i])
        else:
            np.testing.assert_allclose(c["true"][0, :2, :5].numpy(), G[k + "ctx_head"][i], atol=1e-5, rtol=0)
    want = tiled_reason(reason_len(T), len(calls))
    for i, r in enumerate(model.reason_windows):
        assert tuple(r.shape) == (1, 8, 150)
        assert torch.equal(r[0], want[i])
        if i == 0:
            np.testing.assert_array_equal(r[0].numpy(), G[k + "reason_windows"][0].astype(np.int64))
        else:
            # the reference conditions every window on reason codes [0, 150) (its `cnt` never advances)
            np.testing.assert_array_equal(G[k + "reason_windows"][i], G[k + "reason_windows"][0])
            assert not np.array_equal(r[0].numpy(), G[k + "reason_windows"][i].astype(np.int64))
    assert wave.dtype == torch.float32 and wave.device.type == "cpu"
    assert tuple(wave.shape) == tuple(G[k + "wave_shape"]) == (1, int(T / 12.5 * 24000))
    if exact:
        np.testing.assert_array_equal(wave[0, ::WAVE_STRIDE].numpy(), G[k + "wave_sub"])
        np.testing.assert_array_equal(wave_digest(wave), G[k + "wave_digest"])
    else:
        np.testing.assert_allclose(wave[0, ::WAVE_STRIDE].numpy(), G[k + "wave_sub"], atol=1e-5, rtol=0)
        np.testing.assert_allclose(wave_digest(wave), G[k + "wave_digest"], rtol=1e-5)


def product_t2a(T, device):
    model = StubReasonModel()
    tok = ReasoningTokenizer(sq_codec=StubCodec(), model=model, device=device)
    torch.manual_seed(SEED)
    wave = tok.token2audio(make_reason_codes(reason_len(T)), make_codes(T), False, duration=30, guidance_scale=1.5, num_steps=7,
                           disable_progress=True)
    return model, wave


@pytest.mark.parametrize("T", T_CASES)
def test_window_plans_match_the_reference_arithmetic(T):
    p = window_plan(T, duration=30)
    n = G[f"t2a_{T}_windows"].shape[0]
    assert (p["min_codes"], p["hop_codes"], p["ovlp_codes"], p["ovlp_frames"], p["latent_length"]) == (375, 279, 96, 48, 750)
    assert (p["wav_window"], p["wav_ovlp"]) == (720000, 180000)
    assert p["starts"] == [279 * k for k in range(n)]
    assert p["target_len"] == int(G[f"t2a_{T}_wave_shape"][1])
    q = reason_window_plan(reason_len(T), n, duration=30)
    assert (q["min_codes"], q["hop_codes"], q["ovlp_codes"]) == (150, 111, 39)
    assert q["starts"] == [111 * k for k in range(n)]
    assert q["tiled_len"] >= q["starts"][-1] + 150 and q["tiled_len"] >= q["reference_tiled_len"]
    assert (q["tiled_len"] - 39) % 111 == 0


def test_reason_window_plan_extends_a_short_reason_stream():
    # 4 rec windows but a reason stream the reference's rule tiles to 150 codes only: extended to 3 * 111 + 150 = 483
    q = reason_window_plan(20, 4)
    assert q["reference_tiled_len"] == 150 and q["tiled_len"] == 483 and q["starts"] == [0, 111, 222, 333]
    # long enough already: the reference's length is kept
    q = reason_window_plan(600, 2)
    assert q["reference_tiled_len"] == q["tiled_len"] == 705          # 6 * 111 + 39
    # the 20-s shape of the same rule
    q = reason_window_plan(10, 1, duration=20)
    assert (q["min_codes"], q["hop_codes"], q["ovlp_codes"], q["tiled_len"]) == (100, 75, 25, 100)


@pytest.mark.parametrize("T", T_CASES)
def test_token2audio_host_logic_matches_reference_run(T):
    model, wave = product_t2a(T, "cpu")
    check_t2a(T, model, wave)


def test_detokenize_is_token2audio_of_one_utterance():
    model = StubReasonModel()
    tok = ReasoningTokenizer(sq_codec=StubCodec(), model=model, device="cpu")
    torch.manual_seed(SEED)
    wave = tok.detokenize(make_reason_codes(reason_len(700))[0], make_codes(700)[0], False, steps=7)
    check_t2a(700, model, wave)


def test_token2audio_refuses_reasoning_text():
    tok = ReasoningTokenizer(sq_codec=StubCodec(), model=StubReasonModel(), device="cpu")
    with pytest.raises(NotImplementedError):
        tok.token2audio(make_reason_codes(10), make_codes(20), True)


@pytest.mark.parametrize("max_batch", [1, 3])
def test_detokenize_batch_equals_the_detokenize_loop_on_the_stand_ins(max_batch):
    """One generator on the CPU: equal waves also pin the interleaving of the CPU and device draws."""
    Ts = (700, 100, 376, 1200)
    pairs = [(make_reason_codes(reason_len(T))[0], make_codes(T)[0]) for T in Ts]
    one = NoisyStubReasonModel()
    tok1 = ReasoningTokenizer(sq_codec=StubCodec(), model=one, device="cpu")
    torch.manual_seed(SEED)
    want = [tok1.detokenize(q, c, steps=7) for q, c in pairs]
    bat = NoisyStubReasonModel()
    tokb = ReasoningTokenizer(sq_codec=StubCodec(), model=bat, device="cpu")
    torch.manual_seed(SEED)
    got = tokb.detokenize_batch([q for q, _ in pairs], [c for _, c in pairs], steps=7, max_batch=max_batch)
    for T, a, b in zip(Ts, want, got):
        assert a.shape == b.shape == (1, int(T / 12.5 * 24000))
        assert torch.equal(a, b), T
    assert len(bat.calls) <= len(one.calls)
    assert max(r.shape[0] for r in bat.reason_windows) <= max_batch
    assert sorted(tuple(r.shape) for r in one.reason_windows) == [(1, 8, 150)] * len(one.reason_windows)
