#!/usr/bin/env python3
"""Golden vectors for the reasoning-conditioned decode, produced by RUNNING THE REFERENCE's own code:

  t2a_*     ReasoningTokenizer.token2audio (tools/tokenizer/ReasoningCodec_film/reason_tokenizer.py:132-226) — unbound, on a
            SimpleNamespace `self` — with model.inference_codes / SQCodec.decode replaced by the stand-ins of
            reason_decode_stub.py / tokenizer_stub.py: the 30-s rec windows (375 codes, hop 279), the reason windows the
            reference hands to inference_codes, the in-context chain, the randn draw order, the float64 cross-fade and crop.
            The stand-in takes **kw, so the reference's second-window TypeError (:201 `return_reasoning_text=`) does not stop
            the record; the recorded reason windows show its other defect (every window gets reason codes [0, 150)).
  infer2_*  AudioDiffusion1D.inference_codes (models/AudioDiffusion1D.py:554-624) with codes = [reason, rec]:
            feature_combine (:440-456: reason_adaptor, x2.5 nearest interpolation, crop to T, add) on the reasoning_vq
            look-up, then the one-stream path (cond_feature_emb, x2 nearest, masks, zero_cond, guided Euler, in-context
            overwrite), at toy size with T_q = 11, T = 25 (27 up-sampled rows cropped to 25).  Look-ups: table stand-ins for
            the four ResidualVQs; estimator: codec_model_stub.StubEstimator.
  up_*      the x2.5 nearest index tables of F.interpolate for T_q = 11 and 150.

Absent third-party imports are MagicMock'ed as in make_golden_tokenizer.py / make_golden_codec_model.py.
Container-only (needs /root/reference).  Usage: python tests/golden/make_golden_reason_decode.py
"""
import importlib
import json
import os
import sys
import types
from unittest.mock import MagicMock

os.environ.setdefault("NO_TORCH_COMPILE", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, "/root/reference")

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from codec_model_stub import CFG, StubEstimator, module_state_dict
from reason_decode_stub import INFER, SEED, T_CASES, WAVE_STRIDE, StubReasonModel, infer_reason_inputs, make_reason_codes, reason_len
from tokenizer_stub import StubCodec, make_codes, wave_digest

P = "tools.tokenizer.ReasoningCodec_film."
TOK_STUBBED = ["omegaconf", "torchaudio", "torchaudio.transforms", "transformers", "huggingface_hub", "safetensors", "safetensors.torch",
               P + "models.AudioDiffusion1D", P + "models.model_utils", P + "models.scalar24k", "tools.tokenizer.common"]
MODEL_STUBBED = ["torchaudio", "diffusers", "diffusers.utils", "diffusers.utils.torch_utils", "whisper", "whisper.audio", "peft",
                 "vector_quantize_pytorch", "soft_moe_pytorch", "transformers", P + "models.processor", P + "models.transformer_1d_flow",
                 P + "modules.our_MERT_BESTRQ.test", P + "models.PretrainedModel", P + "models.modeling_whisper", P + "models.vocos",
                 P + "models.model_utils"]


class TableVQ(nn.Module):
    """Stand-in for ResidualVQ.get_output_from_indices: sum of per-level table rows."""

    def __init__(self, tables):
        super().__init__()
        self.tables = tables                               # [L, C, D]

    def get_output_from_indices(self, idx):                # (B, T, L) -> (B, T, D)
        return sum(self.tables[l][idx[..., l]] for l in range(idx.shape[-1]))


def record_token2audio(out):
    for name in TOK_STUBBED:
        sys.modules[name] = MagicMock()
    rt = importlib.import_module(P + "reason_tokenizer")
    RT = rt.ReasoningTokenizer
    for T in T_CASES:
        model, codec = StubReasonModel(), StubCodec()
        fake = types.SimpleNamespace(device=torch.device("cpu"), sample_rate=24000, rec_frame_rate=12.5, reason_frame_rate=5,
                                     sq_codec_hz=25, model=model, SQCodec=codec)
        torch.manual_seed(SEED)
        wave = RT.token2audio(fake, make_reason_codes(reason_len(T)), make_codes(T), False, duration=30, guidance_scale=1.5, num_steps=7,
                              disable_progress=True)
        k = f"t2a_{T}_"
        out[k + "windows"] = torch.stack([c["codes"][0] for c in model.calls]).numpy().astype(np.int16)           # (n_win, 8, 375)
        out[k + "reason_windows"] = torch.stack([r[0] for r in model.reason_windows]).numpy().astype(np.int16)    # (n_win, 8, 150)
        out[k + "incontext"] = np.array([c["incontext"] for c in model.calls], dtype=np.int32)
        out[k + "latent_length"] = np.array([c["latent_length"] for c in model.calls], dtype=np.int32)
        out[k + "noise"] = np.stack([c["true"][0, c["incontext"]:c["incontext"] + 3, :5].numpy() for c in model.calls])
        out[k + "noise_tail"] = np.stack([c["true"][0, -2:, -5:].numpy() for c in model.calls])
        out[k + "ctx_head"] = np.stack([c["true"][0, :2, :5].numpy() for c in model.calls])
        out[k + "wave_shape"] = np.array(wave.shape, dtype=np.int64)
        out[k + "wave_sub"] = wave[0, ::WAVE_STRIDE].numpy().astype(np.float32)
        out[k + "wave_digest"] = wave_digest(wave)
        assert wave.dtype == torch.float32
        print("token2audio T =", T, "reason", reason_len(T), "windows", len(model.calls), "wave", tuple(wave.shape),
              "incontext", out[k + "incontext"].tolist())
    for name in TOK_STUBBED:
        sys.modules.pop(name, None)
    for name in list(sys.modules):
        if name.startswith("tools"):
            sys.modules.pop(name)


def record_inference_codes(out, meta):
    for name in MODEL_STUBBED:
        sys.modules[name] = MagicMock()
    ad = importlib.import_module(P + "models.AudioDiffusion1D")
    c, i = CFG, infer_reason_inputs()
    holder = nn.ModuleDict(dict(cond_feature_emb=nn.Linear(c["D"], c["D"]), reason_adaptor=nn.Linear(c["D"], c["D"])))
    shapes = {k: tuple(v.shape) for k, v in holder.state_dict().items()}
    meta["keys"] = [[k, list(s)] for k, s in shapes.items()]
    holder.load_state_dict(module_state_dict(shapes, 503))
    fake = types.SimpleNamespace(device=torch.device("cpu"), dtype=torch.float32, max_t_len=30 * 50, sq_codec_latent=c["latent"],
                                 cond_feature_emb=holder["cond_feature_emb"], reason_adaptor=holder["reason_adaptor"],
                                 zero_cond_embedding1=i["zero_cond"], audio_thinking=types.SimpleNamespace(reasoning_vq=TableVQ(i["tab_reason"])),
                                 vq_pronunciation_semantic=TableVQ(i["tab_phone"]), vq_structure_semantic=TableVQ(i["tab_sem"]),
                                 vq_acoustic=TableVQ(i["tab_ac"]), cfm_wrapper=ad.BASECFM(StubEstimator()))
    fake.feature_combine = types.MethodType(ad.AudioDiffusion1D.feature_combine, fake)
    fake.prepare_latents = lambda bsz, nf, dtype, device: i["noise"].clone()
    ad.tqdm = lambda it: it
    with torch.no_grad():
        for tag, kw in (("infer2_first", dict(true_latents=i["first_latent"].clone(), incontext_length=0)),
                        ("infer2_other", dict(true_latents=i["true_latent"].clone(), incontext_length=i["incontext"]))):
            lat = ad.AudioDiffusion1D.inference_codes(fake, [i["reason"], i["codes"]], None, kw["true_latents"], i["latent_length"],
                                                      kw["incontext_length"], additional_feats=[], guidance_scale=1.5, num_steps=c["steps"],
                                                      disable_progress=True, scenario="other_seg")
            out[tag] = lat.numpy()
    for tq in (INFER["T_q"], 150):
        ramp = torch.arange(tq, dtype=torch.float32).view(1, 1, tq)
        out[f"up_{tq}"] = F.interpolate(ramp, scale_factor=2.5, mode="nearest").view(-1).numpy().astype(np.int32)


def main():
    torch.set_num_threads(4)
    out, meta = {}, {}
    record_token2audio(out)
    record_inference_codes(out, meta)
    np.savez_compressed(os.path.join(HERE, "reason_decode.npz"), **out)
    with open(os.path.join(HERE, "reason_decode.json"), "w") as f:
        json.dump(meta, f)
    print("wrote", os.path.join(HERE, "reason_decode.npz"), os.path.getsize(os.path.join(HERE, "reason_decode.npz")), "bytes")


if __name__ == "__main__":
    main()
