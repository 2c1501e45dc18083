"""Whisper front end on the device against goldens from the reference's own code (tests/golden/make_golden_whisper.py):
ua2_logmel vs transformers.WhisperFeatureExtractor, the WhisperEncoder mirror vs the reference's WhisperEncoder, and a toy
fetch_codes_batch with the encoder inside.

Tolerances are measured, not picked (whisper_toy.json, produced on the CPU by the golden generator; max |difference|):
  log-mel       the extractor works in float64; its gap to the fp32 restatement tests/whisper_ref.py `logmel_ref` on the three
                golden clips is gap_logmel = 5.913e-05.  The kernel sums in yet another order: bound 2 x gap = 1.183e-04.  The
                all-zero clip is exact (-1.5 everywhere).
  fp32 encoder  gap between the reference encoder and `whisper_ref.encoder_ref`, both fp32, on the two golden cases (hidden state
                and stem): gap_enc_fp32 = 2.384e-06 on values up to 4.35.  Bound 2 x gap = 4.768e-06.
  bf16 encoder  the reference runs this encoder under bf16 autocast (reason_tokenizer.py:117); the gap between the reference under
                torch.autocast("cpu", dtype=torch.bfloat16) and in fp32 on the golden cases is gap_enc_bf16 = 2.443e-02.  The bf16
                kernels get 2 x gap = 4.886e-02 against the fp32 golden.
The bounds are read from the json, so regenerating the goldens moves them with the measurement.
"""
import json
import os
from functools import lru_cache

import numpy as np
import pytest
import torch

import whisper_ref as wr

pytestmark = pytest.mark.gpu
HERE = os.path.join(os.path.dirname(__file__), "golden")


@lru_cache(maxsize=None)
def _gold():
    return np.load(os.path.join(HERE, "whisper_toy.npz")), json.load(open(os.path.join(HERE, "whisper_toy.json")))


@lru_cache(maxsize=None)
def _clips():
    return wr.clips()


@lru_cache(maxsize=None)
def _logmel_single(name):
    from uniaudio2_amd import ops
    return ops.logmel(torch.from_numpy(_clips()[name])[None].cuda())[0].cpu()


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_logmel_vs_feature_extractor_golden(name):
    d, meta = _gold()
    got = _logmel_single(name)
    assert got.shape == (80, 3000) and got.dtype == torch.float32
    ref = d[f"logmel_{name}"]
    sub = got[:, meta["frame_subset"]].numpy()
    err = float(np.abs(sub - ref).max())
    emax = abs(float(got.max()) - float(d[f"logmel_{name}_max"]))
    print(f"logmel {name}: max |kernel - extractor| on the frame subset {err:.3e}, clip maximum off by {emax:.3e} (bound {2 * meta['gap_logmel']:.3e})")
    if name == "c":
        assert torch.equal(got, torch.full_like(got, -1.5))
        return
    assert float(got.min()) >= float(got.max()) - 2.0 - 1e-6          # the max - 8 clamp, after (x + 4) / 4
    assert err <= 2 * meta["gap_logmel"], err
    assert emax <= 2 * meta["gap_logmel"], emax


def test_logmel_batch_is_bitwise_the_single_clips():
    """Three clips of different lengths in one launch (zero-extended to a common length, which is what the kernel's own padding does
    to a short clip) give each clip's one-by-one bits."""
    from uniaudio2_amd import ops
    clips = _clips()
    n = max(len(c) for c in clips.values())
    batch = torch.zeros(len(clips), n)
    for i, c in enumerate(clips.values()):
        batch[i, :len(c)] = torch.from_numpy(c)
    got = ops.logmel(batch.cuda()).cpu()
    for i, name in enumerate(clips):
        assert torch.equal(got[i], _logmel_single(name)), name


def _encoder(P, dtype):
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models.modeling_whisper import WhisperEncoder
    cfg = wr.encoder_config(P)
    enc = WhisperEncoder(cfg)
    enc.load_state_dict(wr.encoder_state_dict(cfg), strict=True)
    return enc.cuda().prepare(dtype)


@pytest.mark.parametrize("name", list(wr.ENCODER_CASES))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_encoder_vs_reference_golden(name, dtype):
    d, meta = _gold()
    P = wr.ENCODER_CASES[name]
    enc = _encoder(P, dtype)
    mels = wr.encoder_mels(P).cuda()
    got = enc(mels)
    assert got.shape == (wr.ENCODER_BATCH, P, wr.TOY["d_model"])
    bound = 2 * (meta["gap_enc_fp32"] if dtype == torch.float32 else meta["gap_enc_bf16"])
    err = float((got.cpu() - torch.from_numpy(d[f"enc_{name}_last"])).abs().max())
    print(f"encoder {name} {dtype}: max |device - reference| {err:.3e} (bound {bound:.3e})")
    errs = [err]
    if f"enc_{name}_stem" in d.files:
        stem, _ = enc.stem(mels)
        errs.append(float((stem.view(wr.ENCODER_BATCH, P, -1).cpu() - torch.from_numpy(d[f"enc_{name}_stem"])).abs().max()))
        print(f"encoder {name} {dtype}: stem max |device - reference| {errs[-1]:.3e}")
    # row invariance: row 0 of the batch == the same row alone, bit for bit
    alone = enc(mels[:1].contiguous())
    assert torch.equal(alone[0], got[0]), "row 0 of B = 2 differs from the row run alone"
    assert max(errs) <= bound, errs


def test_fetch_codes_batch_with_the_encoder_inside():
    """Toy fetch_codes_batch with a Whisper encoder set and a callable that supplies WavLM / BEST-RQ only: the codes equal those of
    the same model with whisper_ref's features (computed from the same mels, cut by get_whisper_feature's length rule) injected."""
    import test_gpu_codec_model as tcm
    from codec_model_stub import CFG, fetch_inputs
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models.modeling_whisper import WhisperEncoder
    _, meta = tcm._gold()
    model, _ = tcm._toy_model(meta)
    P, B, T25 = 72, CFG["B"], CFG["T25"]
    cfg = dict(d_model=CFG["Cw"], encoder_layers=2, encoder_attention_heads=1, encoder_ffn_dim=128, num_mel_bins=80, max_source_positions=P)
    sd = wr.encoder_state_dict(cfg, seed=7300)
    enc = WhisperEncoder(cfg)
    enc.load_state_dict(sd, strict=True)
    object.__setattr__(model, "whisper_encoder", enc.cuda().prepare(torch.float32))
    f = {k: v.cuda() for k, v in fetch_inputs().items()}
    others = {k: v for k, v in f.items() if k != "whisper"}
    mels = torch.stack([wr.encoder_mels(P, seed=7400 + i)[0] for i in range(B)]).cuda()
    audios = torch.zeros(B, 1, 28800, device="cuda")                       # int(28800 / 24000 * 50) = 60 = 2 * T25 frames
    masks = torch.zeros(3, B, dtype=torch.bool)
    with pytest.raises(NotImplementedError, match="WavLM / BEST-RQ encoders"):
        model.fetch_codes_batch(audios, mels, film_masks=masks)
    model.ssl_features = lambda a, m: dict(others)
    rc, mc, _ = model.fetch_codes_batch(audios, mels, film_masks=masks)
    feat = model.get_whisper_feature(mels, audios.shape[-1], T25)
    assert feat.shape == (B, CFG["Cw"], 2 * T25)
    ref_feat = wr.encoder_ref({k: v.cuda() for k, v in sd.items()}, cfg, mels)[0][:, :2 * T25].transpose(1, 2)
    print(f"toy fetch: max |device whisper feature - whisper_ref| {float((feat - ref_feat).abs().max()):.3e}")
    model.ssl_features = lambda a, m: dict(others, whisper=ref_feat.contiguous())
    rc2, mc2, _ = model.fetch_codes_batch(audios, None, film_masks=masks)
    assert rc[0].shape == rc2[0].shape and mc[0].shape == (B, 15, 8)
    assert torch.equal(rc[0], rc2[0]) and torch.equal(mc[0], mc2[0])
