"""WavLM encoder, host side (no GPU): the restatement against transformers' goldens, the relative-position table against
transformers' compute_bias, the loader's key handling on synthetic directories, the refused configs, the frame count, the
AudioDiffusion1D / CLI wiring.  A trained WavLM checkpoint is not available: the loader is tested on synthetic files only."""
import json
import os
import types
from functools import lru_cache

import numpy as np
import pytest
import torch

import wavlm_ref as wr
from weights import seeded_tensor

HERE = os.path.join(os.path.dirname(__file__), "golden")


@lru_cache(maxsize=None)
def _gold():
    d = dict(np.load(os.path.join(HERE, "wavlm_toy.npz")))
    d.update(np.load(os.path.join(HERE, "wavlm_toy_a.npz")))
    return d, json.load(open(os.path.join(HERE, "wavlm_toy.json")))


def _mod():
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models import modeling_wavlm
    return modeling_wavlm


@pytest.mark.parametrize("name", list(wr.CASES))
def test_restatement_vs_transformers_golden(name):
    d, meta = _gold()
    front, hs = wr.encoder_ref(wr.state_dict(wr.TOY), wr.TOY, wr.clips(name))
    assert float((front - torch.from_numpy(d[f"front_{name}"])).abs().max()) <= meta["gap_front_fp32"]
    errs = [float((hs[i] - torch.from_numpy(d[f"hs{i}_{name}"])).abs().max()) for i in (0,) + wr.TAPS]
    errs.append(float((wr.tap_mean(hs) - torch.from_numpy(d[f"mean_{name}"])).abs().max()))
    assert hs[0].shape == (wr.BATCH, _mod().frame_count(wr.CASES[name], wr.TOY["conv_kernel"], wr.TOY["conv_stride"]), wr.TOY["hidden_size"])
    assert max(errs) <= meta["gap_enc_fp32"], errs


@pytest.mark.parametrize("T", wr.BIAS_T)
def test_bias_table_is_transformers_compute_bias(T):
    """The product's [n_head, 2 T - 1] table and the restatement's dense form against WavLMAttention.compute_bias at the released
    320 buckets / 800 distance (T = 130 reaches the log-spaced buckets): exact."""
    d, _ = _gold()
    gold = torch.from_numpy(d[f"bias_{T}"])
    embed = seeded_tensor((320, 2), 6300, std=1.0)
    tab = _mod().bias_table(embed, T, 320, 800)
    assert tab.shape == (2, 2 * T - 1) and tab.dtype == torch.float32
    pos = torch.arange(T)
    idx = pos[None, :] - pos[:, None] + T - 1                         # [q][k] -> entry k - q + T - 1
    assert torch.equal(tab[:, idx], gold)
    assert torch.equal(wr.bias_table(embed, T, 320, 800), gold)
    far = torch.arange(-2000, 2001)
    assert torch.equal(_mod().relative_buckets(far, 320, 800), wr.buckets(far, 320, 800))        # the saturated buckets too


def test_frame_count():
    m = _mod()
    n, seen = 480160, []
    for k, s in zip(m.RELEASED_CONFIG["conv_kernel"], m.RELEASED_CONFIG["conv_stride"]):
        n = (n - k) // s + 1
        seen.append(n)
    assert seen == [96031, 48015, 24007, 12003, 6001, 3000, 1500]
    assert m.frame_count(480160) == 1500 and m.frame_count(4000, (10, 3, 2), (5, 2, 2)) == 199


def test_mirror_keys_are_transformers_keys():
    _, meta = _gold()
    m = _mod()
    enc = m.WavLMEncoder(wr.TOY, taps=wr.TAPS)
    assert sorted(enc.state_dict()) == sorted(k for k in meta["reference_keys"] if k != "masked_spec_embed")
    enc.load_state_dict(wr.state_dict(wr.TOY), strict=True)
    assert len(m.WavLMEncoder(wr.TOY, taps=(1, 2)).encoder.layers) == 2                    # layers past the last tap are not built


def _write_dir(path, cfg, sd, fmt):
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump({k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()} | {"model_type": "wavlm", "vocab_size": 32}, f)
    if fmt == "safetensors":
        from safetensors.torch import save_file
        save_file({k: v.contiguous() for k, v in sd.items()}, os.path.join(path, "model.safetensors"))
    else:
        torch.save(dict(sd), os.path.join(path, "pytorch_model.bin"))


@pytest.mark.parametrize("fmt,old_names,prefix", [("safetensors", False, ""), ("bin", True, ""), ("bin", False, "wavlm.")])
def test_loader_filters_and_renames(tmp_path, fmt, old_names, prefix):
    """A 12-layer-style file (here: the toy's 3 layers, taps (1, 2) -> layer 2 dropped) with masked_spec_embed, optionally the old
    weight_g / weight_v spelling and a `wavlm.` prefix, loads strict=True."""
    m = _mod()
    sd = dict(wr.state_dict(wr.TOY))
    sd["masked_spec_embed"] = torch.zeros(wr.TOY["hidden_size"])
    if old_names:
        sd["encoder.pos_conv_embed.conv.weight_g"] = sd.pop("encoder.pos_conv_embed.conv.parametrizations.weight.original0")
        sd["encoder.pos_conv_embed.conv.weight_v"] = sd.pop("encoder.pos_conv_embed.conv.parametrizations.weight.original1")
    _write_dir(str(tmp_path), wr.TOY, {prefix + k: v for k, v in sd.items()}, fmt)
    enc = m.WavLMEncoder.from_pretrained(str(tmp_path), taps=(1, 2))
    assert len(enc.encoder.layers) == 2 and enc.config["num_buckets"] == 32
    own = enc.state_dict()
    ref = wr.state_dict(wr.TOY)
    assert not [k for k in own if k.startswith("encoder.layers.2.")]
    for k, v in own.items():
        assert torch.equal(v, ref[k]), k
    folded = torch._weight_norm(own["encoder.pos_conv_embed.conv.parametrizations.weight.original1"],
                                own["encoder.pos_conv_embed.conv.parametrizations.weight.original0"], 2)
    assert torch.allclose(folded, wr.pos_weight(ref), atol=1e-7)                             # weight norm over (out, in) per tap


def test_loader_names_missing_and_unexpected_keys(tmp_path):
    m = _mod()
    sd = dict(wr.state_dict(wr.TOY))
    del sd["encoder.layers.0.attention.rel_attn_embed.weight"]
    _write_dir(str(tmp_path), wr.TOY, sd, "bin")
    with pytest.raises(RuntimeError, match="rel_attn_embed"):
        m.WavLMEncoder.from_pretrained(str(tmp_path), taps=wr.TAPS)
    with pytest.raises(FileNotFoundError):
        m.WavLMEncoder.read_checkpoint(str(tmp_path / "nothing"))


@pytest.mark.parametrize("override,word", [(dict(feat_extract_norm="layer"), "feat_extract_norm"), (dict(do_stable_layer_norm=True), "stable"),
                                           (dict(conv_bias=True), "conv_bias"), (dict(hidden_size=120, num_attention_heads=3), "head size"),
                                           (dict(hidden_size=192, num_attention_heads=3, num_conv_pos_embedding_groups=8), "groups")])
def test_refused_configs(override, word):
    with pytest.raises(NotImplementedError, match=word):
        _mod().WavLMEncoder({**wr.TOY, **override}, taps=wr.TAPS)


def test_released_config_is_wavlm_base():
    c = _mod().RELEASED_CONFIG
    assert (c["hidden_size"], c["num_attention_heads"], c["intermediate_size"], c["num_hidden_layers"]) == (768, 12, 3072, 12)
    assert (c["num_conv_pos_embeddings"], c["num_conv_pos_embedding_groups"], c["num_buckets"], c["max_bucket_distance"]) == (128, 16, 320, 800)
    enc = _mod().WavLMEncoder()
    assert enc.taps == (6, 7, 8, 9) and len(enc.encoder.layers) == 9                         # layers 10 .. 12 are never computed


# ---- wiring ----------------------------------------------------------------------------------------------------------------
def test_audio_diffusion_takes_the_encoder_and_keeps_its_messages():
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models.AudioDiffusion1D import AudioDiffusion1D
    marker = object()
    m = AudioDiffusion1D(use_detokenizer=False, whisper_fea_dim=32, wavlm_fea_dim=32, codec_dim=32, encoder_depth=1, wavlm_encoder=marker)
    assert m.wavlm_encoder is marker and "wavlm_encoder" not in dict(m.named_modules())
    with pytest.raises(NotImplementedError, match=r"frozen Whisper / BEST-RQ encoder\(s\) next to the WavLM encoder"):
        m.fetch_codes_batch(torch.zeros(1, 1, 8), None)
    object.__setattr__(m, "wavlm_encoder", None)
    with pytest.raises(NotImplementedError, match=r"frozen Whisper / WavLM / BEST-RQ encoders \(out of scope"):
        m.fetch_codes_batch(torch.zeros(1, 1, 8), None)
    with pytest.raises(NotImplementedError, match="needs a WavLMEncoder"):
        m.get_wavlm_feature(torch.zeros(1, 1, 8), 4)


def test_released_yaml_loads_wavlm_when_the_directory_exists(monkeypatch, tmp_path):
    """_load_released -> _load_wavlm: `wav_lm_path` naming an existing directory -> from_pretrained(dir, taps 6 .. 9) -> .to(device) ->
    prepare(wavlm_dtype), set on the model; no entry or no directory: nothing is set.  The real loader reads the synthetic directory."""
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models import modeling_wavlm
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.reason_tokenizer import ReasoningTokenizer
    _write_dir(str(tmp_path / "wavlm"), wr.TOY, wr.state_dict(wr.TOY), "bin")
    seen = {}
    real = modeling_wavlm.WavLMEncoder.from_pretrained.__func__

    def from_pretrained(cls, path, taps=(6, 7, 8, 9)):
        seen.update(path=path, taps=tuple(taps))
        return real(cls, path, taps=(1, 2, 3))                       # the toy has three layers

    monkeypatch.setattr(modeling_wavlm.WavLMEncoder, "from_pretrained", classmethod(from_pretrained))
    monkeypatch.setattr(modeling_wavlm.WavLMEncoder, "prepare", lambda self, dtype=None: (seen.update(dtype=dtype), self)[1])
    tok = ReasoningTokenizer(device="cpu")
    assert tok.wavlm_dtype == torch.float32
    tok.model = types.SimpleNamespace()
    tok._load_wavlm({"wav_lm_path": str(tmp_path / "wavlm")})
    assert seen == dict(path=str(tmp_path / "wavlm"), taps=(6, 7, 8, 9), dtype=torch.float32)
    assert isinstance(tok.model.wavlm_encoder, modeling_wavlm.WavLMEncoder)
    for ta in ({}, {"wav_lm_path": str(tmp_path / "absent")}):
        tok.model = types.SimpleNamespace()
        tok._load_wavlm(ta)
        assert not hasattr(tok.model, "wavlm_encoder")


class _FakeTokenizer:
    def __init__(self, have):
        self.model = types.SimpleNamespace(whisper_encoder=object(), bestrq_encoder=object(), wavlm_encoder=object() if have else None,
                                           ssl_features=None)
        self.paths = []

    def tokenize(self, path, return_reasoning_text=False):
        self.paths.append(path)
        return torch.arange(8 * 3, dtype=torch.int32).view(8, 3), torch.arange(8 * 7, dtype=torch.int32).view(8, 7) + 100


def _cli(monkeypatch, tmp_path, have_wavlm):
    from uniaudio2_amd import multi_task_inference as cli
    calls = []

    class Gen:
        def __init__(self, model, train_args, **kw):
            self._text_tokenizer = types.SimpleNamespace(tokenize=lambda t: [1, 2, 3])
            self._audio_tokenizer = _FakeTokenizer(have_wavlm)
            self.device = "cpu"
            Gen.last = self

        def generate_asr(self, task_prompt, task_name, reason_token, semantic_token, **kw):
            calls.append((task_name, reason_token.clone(), semantic_token.clone()))
            return "hello world"

    monkeypatch.setattr(cli, "_load_config_and_llm", lambda args: (types.SimpleNamespace(), object(), "cpu"))
    monkeypatch.setattr(cli, "_get_generator_class", lambda task: Gen)
    monkeypatch.setattr(cli, "_get_prompt_tensor", lambda args, tok, task: torch.zeros(1, dtype=torch.long))
    wav = tmp_path / "clip.wav"
    wav.write_bytes(b"RIFF")                                      # only its existence matters: the tokenizer is a stand-in
    argv = ["--task", "ASR", "--audio", str(wav), "--output_dir", str(tmp_path / "out"), "--llm_train_config", "x.yaml", "--text_tokenizer_path", "tok"]
    return cli, argv, calls, Gen, wav


def test_cli_audio_without_wavlm_names_the_missing_encoder(monkeypatch, tmp_path):
    cli, argv, calls, _, _ = _cli(monkeypatch, tmp_path, have_wavlm=False)
    with pytest.raises(NotImplementedError, match=r"encoding raw audio needs the codec's frozen SSL encoders .*WavLM \(yaml key wav_lm_path\)") as e:
        cli.run_understanding(cli.get_parser().parse_args(argv))
    assert "Whisper" not in str(e.value).split("not provided")[1] and not calls


def test_cli_audio_reaches_the_generator_with_the_tokenised_codes(monkeypatch, tmp_path):
    cli, argv, calls, Gen, wav = _cli(monkeypatch, tmp_path, have_wavlm=True)
    cli.run_understanding(cli.get_parser().parse_args(argv))
    assert Gen.last._audio_tokenizer.paths == [str(wav)]
    (task, reason, semantic), = calls
    assert task == "asr"
    assert torch.equal(reason, torch.arange(24).view(8, 3).t()) and torch.equal(semantic, (torch.arange(56).view(8, 7) + 100).t())
    out = tmp_path / "out"
    assert torch.equal(torch.load(out / "clip_reason.pt"), torch.arange(24, dtype=torch.int32).view(8, 3))
    assert (out / "clip_semantic.pt").exists() and "clip\thello world" in (out / "asr_results.txt").read_text()


def test_new_symbols_and_abi_version():
    from uniaudio2_amd import _lib
    for name in ("ua2_wavlm_conv0", "ua2_wavlm_conv0_workspace_bytes", "ua2_conv1d_grouped", "ua2_relpos_gate", "ua2_attn_relbias"):
        assert name in _lib.exported_symbols() and hasattr(_lib.lib, name)
    assert _lib.lib.ua2_version() == 10
    # 96 031 frames of the released first layer: 376 chunks of 256 frames x 512 channels x (sum, sum of squares) in double + (mean, rstd)
    assert _lib.lib.ua2_wavlm_conv0_workspace_bytes(1, 480160, 512, 10, 5) == 376 * 512 * 16 + 512 * 8
    assert _lib.lib.ua2_conv1d_grouped(None, None, None, None, None, 1, 1, 64, 4, 16, 0, None) != 0 and b"NULL" in _lib.lib.ua2_last_error()
