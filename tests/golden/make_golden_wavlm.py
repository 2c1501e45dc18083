#!/usr/bin/env python3
"""Golden vectors for the WavLM encoder, produced by RUNNING transformers' `WavLMModel` on the CPU at the toy size of
tests/wavlm_ref.py with its seeded weights (the reference loads the same class: AutoModel.from_pretrained(wav_lm_path),
AudioDiffusion1D.py:233), B = 2, clips of 4 000 and 1 365 samples:

  front_*    feature_extractor output, [B, T, 32]
  hs{i}_*    hidden_states[i], i = 0 .. 3 (0 = after encoder.layer_norm)
  mean_*     torch.stack(hidden_states, 1)[:, 1:4].mean(1), the codec's tap mean at the toy taps (1, 2, 3)
  bias_T     WavLMAttention.compute_bias(T, T) at the released num_buckets 320 / max_distance 800 with a seeded [320, 2] embedding,
             T = 50 and 130

and, in wavlm_toy.json, the measured gaps the GPU tests derive their tolerances from (max |difference|):
  gap_front_fp32  transformers feature extractor vs wavlm_ref.frontend_ref, both fp32
  gap_enc_fp32    transformers hidden_states[0], the taps and their mean vs wavlm_ref.encoder_ref, both fp32
  gap_enc_bf16    transformers under torch.autocast("cpu", dtype=torch.bfloat16) vs itself in fp32, the same outputs
  gap_gate        wavlm_ref.gate_ref in fp32 vs float64 on wavlm_ref.GATE_CASES
  gap_attn_fp32   wavlm_ref.attn_ref in fp32 vs float64 on wavlm_ref.ATTN_CASES
The outputs of clip "a" go to wavlm_toy_a.npz, everything else to wavlm_toy.npz (a committed file stays below 1 MiB).  The npz files
hold expected outputs only; inputs and weights are regenerated from seeds by wavlm_ref.

Container-only (needs transformers).  Usage: python tests/golden/make_golden_wavlm.py
"""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np
import torch

import wavlm_ref as wr
from weights import checksum, seeded_tensor


def reference_model(cfg):
    from transformers import WavLMConfig, WavLMModel
    vals = {k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}
    return WavLMModel(WavLMConfig(**vals, hidden_dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, feat_proj_dropout=0.0,
                                  layerdrop=0.0, apply_spec_augment=False)).eval()


def main():
    torch.manual_seed(0)
    cfg = wr.TOY
    out, meta = {}, {"toy": {k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}, "taps": list(wr.TAPS), "cases": dict(wr.CASES),
                     "batch": wr.BATCH}
    sd = wr.state_dict(cfg)
    meta["weights_checksum"] = checksum(sd)
    model = reference_model(cfg)
    ref_sd = dict(sd)
    ref_sd["masked_spec_embed"] = model.state_dict()["masked_spec_embed"]
    model.load_state_dict(ref_sd, strict=True)
    meta["reference_keys"] = sorted(model.state_dict())
    g_front = g32 = g16 = 0.0
    L = cfg["num_hidden_layers"]
    for name in wr.CASES:
        wav = wr.clips(name)
        with torch.no_grad():
            front = model.feature_extractor(wav).transpose(1, 2)
            hs = model(wav, output_hidden_states=True).hidden_states
            mean = torch.stack(hs, dim=1)[:, wr.TAPS[0]:wr.TAPS[-1] + 1].mean(1)
            with torch.autocast("cpu", dtype=torch.bfloat16):
                hs16 = model(wav, output_hidden_states=True).hidden_states
            mean16 = torch.stack([h.float() for h in hs16], dim=1)[:, wr.TAPS[0]:wr.TAPS[-1] + 1].mean(1)
            my_front, mine = wr.encoder_ref(sd, cfg, wav)
        assert len(hs) == L + 1 and hs[0].shape == (wr.BATCH, front.shape[1], cfg["hidden_size"])
        idx = (0,) + wr.TAPS
        gf = float((front - my_front).abs().max())
        ge = max(max(float((hs[i] - mine[i]).abs().max()) for i in idx), float((mean - wr.tap_mean(mine)).abs().max()))
        gb = max(max(float((hs16[i].float() - hs[i]).abs().max()) for i in idx), float((mean16 - mean).abs().max()))
        print(f"{name}: T {front.shape[1]}, |front| max {float(front.abs().max()):.3f}, |ref - wavlm_ref| front {gf:.3e}; |hs| max "
              f"{max(float(hs[i].abs().max()) for i in idx):.3f}, |ref - wavlm_ref| {ge:.3e}; |ref bf16 autocast - ref| {gb:.3e}")
        g_front, g32, g16 = max(g_front, gf), max(g32, ge), max(g16, gb)
        out[f"front_{name}"] = front.numpy()
        for i in range(L + 1):
            out[f"hs{i}_{name}"] = hs[i].numpy()
        out[f"mean_{name}"] = mean.numpy()
    meta["gap_front_fp32"], meta["gap_enc_fp32"], meta["gap_enc_bf16"] = g_front, g32, g16

    from transformers.models.wavlm.modeling_wavlm import WavLMAttention
    att = WavLMAttention(embed_dim=128, num_heads=2, num_buckets=320, max_distance=800, has_relative_position_bias=True)
    embed = seeded_tensor((320, 2), 6300, std=1.0)
    with torch.no_grad():
        att.rel_attn_embed.weight.copy_(embed)
        for T in wr.BIAS_T:
            out[f"bias_{T}"] = att.compute_bias(T, T).numpy()

    gg = ga = 0.0
    for R, H, hs_ in wr.GATE_CASES:
        h, w, b, c = wr.gate_case(R, H, hs_)
        gg = max(gg, float((wr.gate_ref(h, w, b, c, H).double() - wr.gate_ref(h.double(), w.double(), b.double(), c.double(), H)).abs().max()))
    for B, H, hs_, T in wr.ATTN_CASES:
        q, k, v, gate, embed = wr.attn_case(B, H, hs_, T)
        bias = wr.bias_table(embed, T, 320, 800)
        a32 = wr.attn_ref(q, k, v, gate, bias)
        a64 = wr.attn_ref(q.double(), k.double(), v.double(), gate.double(), bias.double())
        ga = max(ga, float((a32.double() - a64).abs().max()))
    meta["gap_gate"], meta["gap_attn_fp32"] = gg, ga
    # two files: the 4 000-sample clip alone fills most of the 1 MiB a committed file may have
    np.savez_compressed(os.path.join(HERE, "wavlm_toy_a.npz"), **{k: v for k, v in out.items() if k.endswith("_a")})
    np.savez_compressed(os.path.join(HERE, "wavlm_toy.npz"), **{k: v for k, v in out.items() if not k.endswith("_a")})
    with open(os.path.join(HERE, "wavlm_toy.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print({k: meta[k] for k in meta if k.startswith("gap_")}, [os.path.getsize(os.path.join(HERE, n)) for n in ("wavlm_toy.npz", "wavlm_toy_a.npz")], "bytes")


if __name__ == "__main__":
    main()
