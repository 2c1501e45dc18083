#!/usr/bin/env python3
"""Golden vectors for the Whisper front end, produced by RUNNING THE REFERENCE's own code on the CPU:

  logmel_*   transformers.WhisperFeatureExtractor(feature_size=80) — the reference's log-mel (reason_tokenizer.py:36, 67-72) — on
             the three seeded clips of tests/whisper_ref.py `clips()`: the values of a fixed frame subset (FRAME_SUBSET: the
             first 8, the last 8, every 37th) and each clip's maximum
  enc_*      tools/tokenizer/ReasoningCodec_film/models/modeling_whisper.py `WhisperEncoder` in fp32 at the toy size of
             whisper_ref.TOY with max_source_positions = 72 and 200, B = 2, seeded weights and inputs: the full
             last_hidden_state, and for P = 72 the stem's output (conv1 / conv2 / GELU / + embed_positions, captured as the input
             of layer 0)

and, in whisper_toy.json, the three measured gaps the GPU tests derive their tolerances from (max |difference|):
  gap_logmel     reference extractor (float64) vs whisper_ref.logmel_ref (fp32), all 3000 frames of the three clips
  gap_enc_fp32   reference encoder (fp32) vs whisper_ref.encoder_ref (fp32), both cases, last_hidden_state and stem
  gap_enc_bf16   reference encoder under torch.autocast("cpu", dtype=torch.bfloat16) vs the same in fp32, both cases

Container-only (needs /root/reference and transformers).  Usage: python tests/golden/make_golden_whisper.py
"""
import importlib.util
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np
import torch

import whisper_ref as wr
from weights import checksum


def reference_encoder_class():
    path = "/root/reference/tools/tokenizer/ReasoningCodec_film/models/modeling_whisper.py"
    spec = importlib.util.spec_from_file_location("ref_modeling_whisper", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.WhisperEncoder


def main():
    from transformers import WhisperConfig, WhisperFeatureExtractor
    torch.manual_seed(0)
    out, meta = {}, {"frame_subset": wr.FRAME_SUBSET, "toy": wr.TOY, "cases": dict(wr.ENCODER_CASES), "batch": wr.ENCODER_BATCH}
    fe = WhisperFeatureExtractor(feature_size=80)
    gap = 0.0
    for name, clip in wr.clips().items():
        ref = fe(clip, sampling_rate=16000, return_tensors="np")["input_features"][0]             # [80, 3000] fp32
        assert ref.shape == (wr.N_MELS, wr.N_FRAMES), ref.shape
        mine = wr.logmel_ref(torch.from_numpy(clip)[None])[0].numpy()
        g = float(np.abs(ref.astype(np.float64) - mine).max())
        print(f"logmel {name}: {len(clip)} samples, max {ref.max():.6f} min {ref.min():.6f}, |extractor - whisper_ref fp32| {g:.3e}")
        gap = max(gap, g)
        out[f"logmel_{name}"] = ref[:, wr.FRAME_SUBSET].astype(np.float32)
        out[f"logmel_{name}_max"] = np.float32(ref.max())
    meta["gap_logmel"] = gap
    Enc = reference_encoder_class()
    gap32 = gap16 = 0.0
    for name, P in wr.ENCODER_CASES.items():
        cfg = wr.encoder_config(P)
        sd = wr.encoder_state_dict(cfg)
        enc = Enc(WhisperConfig(**cfg, decoder_layers=1, decoder_attention_heads=2, decoder_ffn_dim=32, vocab_size=64)).eval()
        enc.load_state_dict(sd, strict=True)
        mels = wr.encoder_mels(P)
        stem = {}

        def grab(module, args, kwargs):
            stem.setdefault("x", (args[0] if args else kwargs["hidden_states"]).detach().clone())

        hook = enc.layers[0].register_forward_pre_hook(grab, with_kwargs=True)
        with torch.no_grad():
            ref = enc(mels, return_dict=True).last_hidden_state
            hook.remove()
            with torch.autocast("cpu", dtype=torch.bfloat16):
                ref16 = enc(mels, return_dict=True).last_hidden_state.float()
            mine, mine_stem = wr.encoder_ref(sd, cfg, mels)
            plain, _ = wr.encoder_ref(sd, cfg, mels, plain=True)
        g32 = max(float((ref - mine).abs().max()), float((stem["x"] - mine_stem).abs().max()))
        g16 = float((ref16 - ref).abs().max())
        print(f"encoder {name}: |ref| max {float(ref.abs().max()):.3f}; |ref - whisper_ref| {g32:.3e}; |ref - whisper_ref plain| "
              f"{float((ref - plain).abs().max()):.3e}; |ref bf16 autocast - ref| {g16:.3e}")
        gap32, gap16 = max(gap32, g32), max(gap16, g16)
        out[f"enc_{name}_last"] = ref.numpy()
        if P == 72:
            out[f"enc_{name}_stem"] = stem["x"].numpy()
        meta[f"weights_checksum_{name}"] = checksum(sd)
    meta["gap_enc_fp32"], meta["gap_enc_bf16"] = gap32, gap16
    np.savez_compressed(os.path.join(HERE, "whisper_toy.npz"), **out)
    with open(os.path.join(HERE, "whisper_toy.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print({k: meta[k] for k in ("gap_logmel", "gap_enc_fp32", "gap_enc_bf16")}, os.path.getsize(os.path.join(HERE, "whisper_toy.npz")), "bytes")


if __name__ == "__main__":
    main()
