#!/usr/bin/env python3
"""Golden vectors for the BEST-RQ (MusicFM 25 Hz) encoder, produced by RUNNING THE REFERENCE's own code on the CPU:

  stem_*     modules/our_MERT_BESTRQ/mert_fairseq/models/musicfm/modules/conv.py `Conv2dSubsampling` (loaded by path, eval mode: the
             BatchNorms use their running statistics) at the toy size of tests/bestrq_ref.py, B = 2, T25 = 12 and 37
  tap*_*     transformers' `Wav2Vec2ConformerEncoder` built from the VALUES of the reference's w2v2_config.json overridden to the toy
             size (as musicfm_25hz.py:144-150 builds it), run on the reference stem's output with output_hidden_states=True:
             hidden_states[1] and hidden_states[3]

and, in bestrq_toy.json, the measured gaps the GPU tests derive their tolerances from (max |difference|):
  gap_stem_fp32  reference Conv2dSubsampling vs bestrq_ref.stem_ref, both fp32
  gap_enc_fp32   reference conformer taps vs bestrq_ref.conformer_ref, both fp32, on the reference stem's output
  gap_enc_bf16   reference conformer under torch.autocast("cpu", dtype=torch.bfloat16) vs the same in fp32
  gap_mel        bestrq_ref.mel_ref in fp32 vs in float64 on the seeded clips (torchaudio is not installed here: the front end is
                 NOT pinned on the reference's own output)
The npz holds expected outputs only; inputs and weights are regenerated from seeds by bestrq_ref.

Container-only (needs /root/reference, transformers and einops).  Usage: python tests/golden/make_golden_bestrq.py
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

import bestrq_ref as br
from weights import checksum

REF = "/root/reference/tools/tokenizer/ReasoningCodec_film/modules/our_MERT_BESTRQ/mert_fairseq/models/musicfm"


def reference_stem_class():
    spec = importlib.util.spec_from_file_location("ref_musicfm_conv", os.path.join(REF, "modules", "conv.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Conv2dSubsampling


def reference_conformer(cfg):
    from transformers.models.wav2vec2_conformer.modeling_wav2vec2_conformer import Wav2Vec2ConformerConfig, Wav2Vec2ConformerEncoder
    with open(os.path.join(REF, "model", "w2v2_config.json"), "r", encoding="utf-8") as f:
        vals = json.load(f)
    vals.update(num_hidden_layers=cfg["encoder_depth"], hidden_size=cfg["encoder_dim"], num_attention_heads=cfg["num_attention_heads"],
                intermediate_size=cfg["intermediate_size"], conv_depthwise_kernel_size=cfg["conv_depthwise_kernel_size"],
                num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=2)
    for k in ("architectures", "model_type", "transformers_version", "torch_dtype"):
        vals.pop(k, None)
    return Wav2Vec2ConformerEncoder(Wav2Vec2ConformerConfig(**vals)).eval()


def main():
    torch.manual_seed(0)
    cfg = br.TOY
    out, meta = {}, {"toy": cfg, "taps": list(br.TAPS), "cases": dict(br.CASES), "batch": br.BATCH}
    sd = br.state_dict(cfg)
    meta["weights_checksum"] = checksum({k: v for k, v in sd.items() if v.is_floating_point()})
    stem = reference_stem_class()(1, cfg["conv_dim"], cfg["encoder_dim"], strides=[2, 2], n_bands=cfg["n_mels"]).eval()
    stem.load_state_dict({k[len("conv."):]: v for k, v in sd.items() if k.startswith("conv.")}, strict=True)
    enc = reference_conformer(cfg)
    missing, unexpected = enc.load_state_dict({k[len("conformer."):]: v for k, v in sd.items() if k.startswith("conformer.")}, strict=False)
    assert not unexpected, unexpected
    used = ("layers.",)
    assert not [k for k in missing if k.startswith(used)], missing          # only pos_conv_embed / layer_norm / inv_freq may be absent
    meta["reference_keys"] = sorted(["conv." + k for k in stem.state_dict()] + ["conformer." + k for k in enc.state_dict() if k.startswith("layers.")])
    g_stem = g32 = g16 = 0.0
    for name, T25 in br.CASES.items():
        x = br.stem_input(T25)
        with torch.no_grad():
            ref_stem = stem(x)
            hs = enc(ref_stem.clone(), output_hidden_states=True).hidden_states
            with torch.autocast("cpu", dtype=torch.bfloat16):
                hs16 = enc(ref_stem.clone(), output_hidden_states=True).hidden_states
            mine_stem = br.stem_ref(sd, x)
            mine = br.conformer_ref(sd, cfg, ref_stem)
        assert ref_stem.shape == (br.BATCH, T25, cfg["encoder_dim"]), ref_stem.shape
        gs = float((ref_stem - mine_stem).abs().max())
        ge = max(float((hs[t] - m).abs().max()) for t, m in zip(br.TAPS, mine))
        gb = max(float((hs16[t].float() - hs[t]).abs().max()) for t in br.TAPS)
        print(f"{name}: |stem| max {float(ref_stem.abs().max()):.3f}, |ref - bestrq_ref| stem {gs:.3e}; taps max "
              f"{max(float(hs[t].abs().max()) for t in br.TAPS):.3f}, |ref - bestrq_ref| {ge:.3e}; |ref bf16 autocast - ref| {gb:.3e}")
        g_stem, g32, g16 = max(g_stem, gs), max(g32, ge), max(g16, gb)
        out[f"stem_{name}"] = ref_stem.numpy()
        for t in br.TAPS:
            out[f"tap{t}_{name}"] = hs[t].numpy()
    meta["gap_stem_fp32"], meta["gap_enc_fp32"], meta["gap_enc_bf16"] = g_stem, g32, g16
    gm = 0.0
    for name, clip in br.clips().items():
        w = torch.from_numpy(clip)[None]
        m32, m64 = br.mel_ref(w, br.MEL_N_MELS), br.mel_ref(w, br.MEL_N_MELS, torch.float64)
        g = float((m32.double() - m64).abs().max())
        print(f"mel {name}: {len(clip)} samples -> {tuple(m32.shape)}, range [{float(m64.min()):.3f}, {float(m64.max()):.3f}], |fp32 - float64| {g:.3e}")
        gm = max(gm, g)
    meta["gap_mel"] = gm
    np.savez_compressed(os.path.join(HERE, "bestrq_toy.npz"), **out)
    with open(os.path.join(HERE, "bestrq_toy.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print({k: meta[k] for k in ("gap_stem_fp32", "gap_enc_fp32", "gap_enc_bf16", "gap_mel")}, os.path.getsize(os.path.join(HERE, "bestrq_toy.npz")), "bytes")


if __name__ == "__main__":
    main()
