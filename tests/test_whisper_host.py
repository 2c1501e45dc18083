"""Host-side checks of the Whisper front end: the plain-torch restatement (tests/whisper_ref.py) pinned on goldens produced by the
reference's own code, get_whisper_feature's length rule, the checkpoint loader, and the C ABI additions."""
import json
import os

import numpy as np
import pytest
import torch

import whisper_ref as wr

HERE = os.path.join(os.path.dirname(__file__), "golden")
MW = "uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models.modeling_whisper"


def _gold():
    return np.load(os.path.join(HERE, "whisper_toy.npz")), json.load(open(os.path.join(HERE, "whisper_toy.json")))


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_logmel_restatement_vs_feature_extractor_golden(name):
    """whisper_ref.logmel_ref in fp32 stays within the gap the golden generator measured against the extractor (over all frames; the
    golden stores a subset)."""
    d, meta = _gold()
    clip = torch.from_numpy(wr.clips()[name])[None]
    ref = d[f"logmel_{name}"]
    got = wr.logmel_ref(clip)[0]
    assert got.shape == (wr.N_MELS, wr.N_FRAMES)
    assert float(np.abs(got[:, meta["frame_subset"]].numpy() - ref).max()) <= meta["gap_logmel"]
    assert abs(float(got.max()) - float(d[f"logmel_{name}_max"])) <= meta["gap_logmel"]
    if name == "c":
        assert torch.equal(got, torch.full_like(got, -1.5))
    if name == "a":                                                   # the max - 8 clamp is active in the silent stretch
        assert float((got == got.max() - 2.0).float().mean()) > 0.05


def test_product_tables_are_the_restatements():
    """ops.logmel_tables_host (what the kernel is handed) and whisper_ref.logmel_tables are two statements of the same tables."""
    from uniaudio2_amd import ops
    b0, f0 = ops.logmel_tables_host()
    b1, f1 = wr.logmel_tables()
    assert b0.shape == (400, 402) and f0.shape == (201, 80)
    assert float((b0 - b1).abs().max()) < 1e-14 and float((f0 - f1).abs().max()) < 1e-15
    assert int((f0 > 0).sum(0).min()) >= 1                            # no empty filter


@pytest.mark.parametrize("name", list(wr.ENCODER_CASES))
def test_encoder_restatement_vs_reference_golden(name):
    d, meta = _gold()
    P = wr.ENCODER_CASES[name]
    cfg = wr.encoder_config(P)
    sd = wr.encoder_state_dict(cfg)
    from weights import checksum
    assert np.allclose(checksum(sd), meta[f"weights_checksum_{name}"], rtol=1e-9)
    last, stem = wr.encoder_ref(sd, cfg, wr.encoder_mels(P))
    assert float((last - torch.from_numpy(d[f"enc_{name}_last"])).abs().max()) <= meta["gap_enc_fp32"]
    if f"enc_{name}_stem" in d.files:
        assert float((stem - torch.from_numpy(d[f"enc_{name}_stem"])).abs().max()) <= meta["gap_enc_fp32"]
    plain, _ = wr.encoder_ref(sd, cfg, wr.encoder_mels(P), plain=True)
    assert float((plain - last).abs().max()) <= 2 * meta["gap_enc_fp32"]


def test_get_whisper_feature_length_rule():
    """AudioDiffusion1D.py:334-343: n = max(int(n_len / 24000 * 50), 2 * len_semantic) frames, (B, T, C) -> (B, C, n)."""
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models.AudioDiffusion1D import AudioDiffusion1D
    m = AudioDiffusion1D.__new__(AudioDiffusion1D)
    torch.nn.Module.__init__(m)
    hidden = torch.arange(2 * 1500 * 4, dtype=torch.float32).view(2, 1500, 4)
    object.__setattr__(m, "whisper_encoder", lambda mels: hidden)
    for n_len, len_sem, want in ((720240, 750, 1500), (720240, 700, 1500), (480000, 400, 1000), (240000, 300, 600), (24000, 10, 50), (100, 1, 2)):
        got = m.get_whisper_feature(None, n_len, len_sem)
        assert got.shape == (2, 4, want), (n_len, len_sem, got.shape)
        assert torch.equal(got, hidden[:, :want].transpose(1, 2))
    object.__setattr__(m, "whisper_encoder", None)
    with pytest.raises(NotImplementedError):
        m.get_whisper_feature(None, 100, 1)


def test_missing_encoder_errors_keep_their_text():
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models.AudioDiffusion1D import AudioDiffusion1D
    m = AudioDiffusion1D(whisper_fea_dim=64, wavlm_fea_dim=96, codec_dim=256, encoder_depth=1)
    assert m.whisper_encoder is None and not any(k.startswith("whisper_encoder") for k in m.state_dict())
    with pytest.raises(NotImplementedError, match="frozen Whisper / WavLM / BEST-RQ encoders"):
        m.fetch_codes_batch(torch.zeros(1, 1, 10), None)
    object.__setattr__(m, "whisper_encoder", object())
    assert not any(k.startswith("whisper_encoder") for k in m.state_dict())
    with pytest.raises(NotImplementedError, match="frozen WavLM / BEST-RQ encoders"):
        m.fetch_codes_batch(torch.zeros(1, 1, 10), None)


def _write_checkpoint(tmp_path, sd, cfg, fmt):
    os.makedirs(tmp_path, exist_ok=True)
    with open(os.path.join(tmp_path, "config.json"), "w") as f:
        json.dump(dict(cfg, model_type="whisper", decoder_layers=1), f)
    if fmt == "safetensors":
        from safetensors.torch import save_file
        save_file({k: v.contiguous() for k, v in sd.items()}, os.path.join(tmp_path, "model.safetensors"))
    else:
        torch.save(dict(sd), os.path.join(tmp_path, "pytorch_model.bin"))


@pytest.mark.parametrize("fmt", ["safetensors", "bin"])
@pytest.mark.parametrize("prefix", ["", "encoder.", "model.encoder."])
def test_loader_prefixes_and_formats(tmp_path, fmt, prefix):
    import importlib
    WhisperEncoder = importlib.import_module(MW).WhisperEncoder
    cfg = wr.encoder_config(24)
    sd = wr.encoder_state_dict(cfg)
    dec = "decoder." if prefix != "model.encoder." else "model.decoder."
    on_disk = {prefix + k: v for k, v in sd.items()}
    on_disk[dec + "layers.0.fc1.weight"] = torch.zeros(3, 3)            # decoder keys are ignored
    on_disk["proj_out.weight"] = torch.zeros(2, 2)
    _write_checkpoint(str(tmp_path), on_disk, cfg, fmt)
    enc = WhisperEncoder.from_pretrained(str(tmp_path))
    assert enc.config == cfg
    got = enc.state_dict()
    assert list(got) == list(sd)
    for k in sd:
        assert torch.equal(got[k], sd[k]), k


def test_loader_names_missing_keys(tmp_path):
    import importlib
    WhisperEncoder = importlib.import_module(MW).WhisperEncoder
    cfg = wr.encoder_config(24)
    sd = {"encoder." + k: v for k, v in wr.encoder_state_dict(cfg).items()}
    del sd["encoder.layers.1.fc2.bias"], sd["encoder.conv2.weight"]
    _write_checkpoint(str(tmp_path), sd, cfg, "bin")
    with pytest.raises(RuntimeError, match=r"2 parameter\(s\) of the Whisper encoder are not in the checkpoint .*conv2\.weight.*layers\.1\.fc2\.bias"):
        WhisperEncoder.from_pretrained(str(tmp_path))
    with pytest.raises(FileNotFoundError):
        os.remove(os.path.join(str(tmp_path), "pytorch_model.bin"))
        WhisperEncoder.from_pretrained(str(tmp_path))


def test_new_symbols_and_abi_version():
    from uniaudio2_amd import _lib
    assert _lib.lib.ua2_version() == 10
    assert {"ua2_logmel", "ua2_logmel_workspace_bytes"} <= set(_lib.exported_symbols())
    assert _lib.lib.ua2_logmel_workspace_bytes(1) == 188 * 4 and _lib.lib.ua2_logmel_workspace_bytes(6) == 6 * 188 * 4
    assert _lib.lib.ua2_logmel(None, None, 1, 16000, None, None, None, 0, None) != 0          # NULL arguments are refused, nothing launched
    assert b"ua2_logmel" in _lib.lib.ua2_last_error()
    import importlib
    assert "transformers" not in open(importlib.import_module(MW).__file__).read().split('"""', 2)[2]
