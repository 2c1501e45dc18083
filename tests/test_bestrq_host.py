"""Host-side checks of the BEST-RQ (MusicFM 25 Hz) encoder: the plain-torch restatement (tests/bestrq_ref.py) pinned on goldens produced
by the reference's own modules, the checkpoint loader, fetch_codes_batch's error messages, the mirror's state-dict keys and the C ABI
additions."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

import bestrq_ref as br

HERE = os.path.join(os.path.dirname(__file__), "golden")
MM = "uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.modules.our_MERT_BESTRQ.mert_fairseq.models.musicfm.model.musicfm_25hz"


def _gold():
    return np.load(os.path.join(HERE, "bestrq_toy.npz")), json.load(open(os.path.join(HERE, "bestrq_toy.json")))


def _mirror():
    return importlib.import_module(MM)


@pytest.mark.parametrize("name", list(br.CASES))
def test_restatement_vs_reference_golden(name):
    d, meta = _gold()
    assert meta["toy"] == br.TOY and tuple(meta["taps"]) == br.TAPS
    sd = br.state_dict(br.TOY)
    from weights import checksum
    assert np.allclose(checksum({k: v for k, v in sd.items() if v.is_floating_point()}), meta["weights_checksum"], rtol=1e-9)
    x = br.stem_input(br.CASES[name])
    ref_stem = torch.from_numpy(d[f"stem_{name}"])
    assert float((br.stem_ref(sd, x) - ref_stem).abs().max()) <= meta["gap_stem_fp32"]
    taps = br.conformer_ref(sd, br.TOY, ref_stem)
    for t, got in zip(br.TAPS, taps):
        assert float((got - torch.from_numpy(d[f"tap{t}_{name}"])).abs().max()) <= meta["gap_enc_fp32"]
    # a clip alone: the restatement has no coupling across the batch either
    alone = br.conformer_ref(sd, br.TOY, ref_stem[:1])
    assert float((alone[1] - taps[1][:1]).abs().max()) <= meta["gap_enc_fp32"]


def test_mel_restatement_and_tables():
    _, meta = _gold()
    from uniaudio2_amd import ops
    b0, f0 = ops.melspec_tables_host(128)
    b1, f1 = br.mel_tables(128)
    assert b0.shape == (2048, 2050) and f0.shape == (1025, 128)
    assert float((b0 - b1).abs().max()) < 1e-14 and float((f0 - f1).abs().max()) < 1e-11
    assert int((f0 > 0).sum(0).min()) >= 1                            # no empty filter
    assert (ops.MEL_MEAN, ops.MEL_STD) == (br.MEL_MEAN, br.MEL_STD)
    gap = 0.0
    for name, clip in br.clips().items():
        w = torch.from_numpy(clip)[None]
        m32, m64 = br.mel_ref(w, br.MEL_N_MELS), br.mel_ref(w, br.MEL_N_MELS, torch.float64)
        assert m32.shape == (1, 128, 4 * (len(clip) // 960))
        gap = max(gap, float((m32.double() - m64).abs().max()))
        if name == "z":
            assert torch.equal(m32, torch.full_like(m32, float((torch.tensor(-100.0) - br.MEL_MEAN) / br.MEL_STD)))
        if name == "a":                                               # frames wholly inside the silent stretch sit on the floor
            assert float((m32 == m32.min()).float().mean()) > 0.05
    assert gap == pytest.approx(meta["gap_mel"], rel=0.5)


def test_mirror_keys_are_the_reference_keys():
    """State-dict keys of the mirror == those of the reference-built toy modules, for the parts that are used (recorded by the golden
    generator from the reference's Conv2dSubsampling and transformers' encoder layers)."""
    _, meta = _gold()
    m = _mirror().MusicFM25Hz(br.TOY, taps=(1, br.TOY["encoder_depth"]))
    assert sorted(m.state_dict()) == meta["reference_keys"]
    assert set(br.shapes(br.TOY)) == set(meta["reference_keys"])
    m = _mirror().MusicFM25Hz(br.TOY, taps=br.TAPS)                     # layers past the last tap are not built
    assert not any(k.startswith("conformer.layers.3.") for k in m.state_dict())
    m.load_state_dict(br.state_dict(br.TOY, n_layers=3), strict=True)


@pytest.mark.parametrize("wrap", ["plain", "model", "state_dict"])
@pytest.mark.parametrize("prefix", ["", "model.", "model.model."])
def test_loader_prefixes_and_ignored_keys(tmp_path, wrap, prefix):
    MusicFM25Hz = _mirror().MusicFM25Hz
    sd = br.state_dict(br.TOY)
    on_disk = {prefix + k: v for k, v in sd.items()}
    for k in ("conformer.pos_conv_embed.conv.bias", "conformer.layer_norm.weight", "conformer.embed_positions.inv_freq", "linear.weight",
              "cls_token", "quantizer_melspec_2048_0.codebook"):
        on_disk[prefix + k] = torch.zeros(3)                          # parts that never run are ignored
    path = os.path.join(str(tmp_path), "ck.pt")
    torch.save(on_disk if wrap == "plain" else {wrap: on_disk, "cfg": {"x": 1}}, path)
    m = MusicFM25Hz.from_checkpoint(path, config=br.TOY, taps=br.TAPS)
    got = m.state_dict()
    assert set(got) == {k for k in sd if not k.startswith("conformer.layers.3.")}      # layer 3 (past the last tap) is ignored too
    for k in got:
        assert torch.equal(got[k], sd[k]), k


def test_loader_names_missing_keys(tmp_path):
    MusicFM25Hz = _mirror().MusicFM25Hz
    sd = {"model." + k: v for k, v in br.state_dict(br.TOY).items()}
    del sd["model.conv.conv.1.bn3.running_var"], sd["model.conformer.layers.2.self_attn.linear_k.bias"]
    sd["model.conformer.layers.2.self_attn.k_proj.bias"] = torch.zeros(3)
    path = os.path.join(str(tmp_path), "ck.pt")
    torch.save({"model": sd}, path)
    with pytest.raises(RuntimeError, match=r"2 parameter\(s\) of the BEST-RQ encoder are not in the checkpoint .*linear_k\.bias.*bn3\.running_var"):
        MusicFM25Hz.from_checkpoint(path, config=br.TOY, taps=br.TAPS)
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models.PretrainedModel import BESTRQ_Model
    with pytest.raises(ValueError, match="never runs on random weights"):
        BESTRQ_Model()


def test_fetch_codes_batch_error_messages():
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models.AudioDiffusion1D import AudioDiffusion1D
    m = AudioDiffusion1D(whisper_fea_dim=64, wavlm_fea_dim=96, codec_dim=256, encoder_depth=1)
    assert m.bestrq_encoder is None
    with pytest.raises(NotImplementedError, match="frozen Whisper / WavLM / BEST-RQ encoders"):
        m.fetch_codes_batch(torch.zeros(1, 1, 10), None)
    object.__setattr__(m, "bestrq_encoder", object())
    assert not any(k.startswith("bestrq_encoder") for k in m.state_dict())
    with pytest.raises(NotImplementedError, match="frozen Whisper / WavLM encoders"):
        m.fetch_codes_batch(torch.zeros(1, 1, 10), None)
    object.__setattr__(m, "whisper_encoder", object())
    with pytest.raises(NotImplementedError, match=r"frozen WavLM encoder \(out of scope") as e:
        m.fetch_codes_batch(torch.zeros(1, 1, 10), None)
    assert "BEST-RQ" not in str(e.value) and "Whisper" not in str(e.value)
    object.__setattr__(m, "bestrq_encoder", None)
    with pytest.raises(NotImplementedError, match="frozen WavLM / BEST-RQ encoders"):
        m.fetch_codes_batch(torch.zeros(1, 1, 10), None)


def test_released_yaml_entry(tmp_path):
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.reason_tokenizer import ReasoningTokenizer
    path = os.path.join(str(tmp_path), "bestrq.pt")
    assert ReasoningTokenizer.bestrq_checkpoint({}) is None and ReasoningTokenizer.bestrq_checkpoint({"best_rq_ckpt": path}) is None
    open(path, "wb").close()
    assert ReasoningTokenizer.bestrq_checkpoint({"best_rq_ckpt": path}) == path


def test_released_path_builds_the_codecs_taps_in_fp32(monkeypatch, tmp_path):
    """The codec builds BESTRQ_Model(layers = [4, 11]) (reference AudioDiffusion1D.py:237-238, not the class default [3, 11]) and runs it
    with autocast disabled (:502): _load_released asks for hidden_states 4 and 11 in fp32, and those are the mirror's defaults too."""
    import inspect
    from types import SimpleNamespace
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models import PretrainedModel
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.reason_tokenizer import ReasoningTokenizer
    mod = _mirror()
    assert mod.TAPS == (4, 11)
    sig = inspect.signature(PretrainedModel.BESTRQ_Model.__init__).parameters
    assert tuple(sig["layers"].default) == (4, 11) and sig["dtype"].default == torch.float32
    assert inspect.signature(mod.MusicFM25Hz.prepare).parameters["dtype"].default == torch.float32
    cfg = br.config(encoder_depth=12)
    path = os.path.join(str(tmp_path), "bestrq.pt")
    torch.save({"model": {"model." + k: v for k, v in br.state_dict(cfg).items()}}, path)
    built = {}

    class Recorder:
        def __init__(self, **kw):
            built.update(kw)
            self.model = mod.MusicFM25Hz.from_checkpoint(kw["checkpoint_dir"], config=cfg, taps=tuple(kw["layers"]))

    monkeypatch.setattr(PretrainedModel, "BESTRQ_Model", Recorder)
    tok = ReasoningTokenizer(device="cpu")
    tok.model = SimpleNamespace()
    tok._load_bestrq({"best_rq_ckpt": path})
    assert tuple(built["layers"]) == (4, 11) and built["dtype"] == torch.float32 and tok.bestrq_dtype == torch.float32
    enc = tok.model.bestrq_encoder.model
    assert enc.taps == (4, 11) and len(enc.conformer.layers) == 11           # layers 0 .. 10 run; taps after layers 3 and 10
    tok.model = SimpleNamespace()
    tok._load_bestrq({})
    assert not hasattr(tok.model, "bestrq_encoder")


def test_new_symbols_and_abi_version():
    from uniaudio2_amd import _lib
    assert _lib.lib.ua2_version() == 10
    assert {"ua2_conv2d", "ua2_layernorm_rope_rows", "ua2_melspec_db"} <= set(_lib.exported_symbols())
    assert _lib.lib.ua2_conv2d(None, None, None, None, None, 1, 16, 16, 8, 8, 1, 1, 0, None) != 0      # NULL arguments are refused, nothing launched
    assert b"ua2_conv2d" in _lib.lib.ua2_last_error()
    assert _lib.lib.ua2_melspec_db(None, None, None, 1, 4, 1025, 128, 2064, 0.0, 1.0, None) != 0
    assert _lib.lib.ua2_layernorm_rope_rows(None, None, None, None, None, None, None, 4, 4, 64, 32, 1e-5, None) != 0
    body = open(_mirror().__file__).read().split('"""', 2)[2]
    assert "import transformers" not in body and "from transformers" not in body
