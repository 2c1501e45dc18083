#!/usr/bin/env python3
"""Whisper front end at the released size (80 mels, 24 layers x 1024-d x 16 heads, ffn 4096, P = 1500) on seeded random weights:
device-event time of the log-mel (ua2_logmel on [B, 480160] samples), of the stem (conv1 / conv2 as GEMMs + GELU + positional add)
and of the 24 layers + final LayerNorm, for 1 and 6 segments (6 = the reference's batch_size), in bf16 and in fp32; and, as the
comparison, the plain PyTorch restatement of tests/whisper_ref.py (`encoder_ref(plain=True)`: F.conv1d, F.layer_norm, F.gelu, SDPA)
on the same card in bf16, with the max |difference| between the two bf16 results.  The layers' FLOP count comes from the shapes
(below), their share of the bf16 dense peak from it and the measured time.
python tools/ubench/whisper_frontend.py [--out profiles/whisper_frontend.txt] [--iters 10] [--no-fp32]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch

import whisper_ref as wr
from uniaudio2_amd import ops
from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models.modeling_whisper import RELEASED_CONFIG, WhisperEncoder

BF16_DENSE_PEAK = 2.5e15           # FLOP/s, MI355X spec


def layer_flops(cfg, B, P):
    """Multiply-adds x 2 of the layers: q|k|v, out_proj, fc1, fc2 GEMMs and the two attention products, per segment batch."""
    d, f, L = cfg["d_model"], cfg["encoder_ffn_dim"], cfg["encoder_layers"]
    return L * B * (2 * P * d * (4 * d + 2 * f) + 4 * P * P * d)


def stem_flops(cfg, B, P):
    d = cfg["d_model"]
    return B * (2 * (2 * P) * d * 3 * cfg["num_mel_bins"] + 2 * P * d * 3 * d)


def event_ms(fn, iters, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-fp32", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("whisper_frontend.py measures on the GPU; none found")
    cfg = dict(RELEASED_CONFIG)
    P = cfg["max_source_positions"]
    sd = wr.encoder_state_dict(cfg, seed=7500)
    enc = WhisperEncoder(cfg)
    enc.load_state_dict(sd, strict=True)
    enc = enc.cuda()
    lines = [f"Whisper front end, released size {cfg}, seeded random weights; device-event ms per call, mean of {a.iters} after 2 warm-up calls"]
    say = lambda s: (lines.append(s), print(s, flush=True))
    g = torch.Generator().manual_seed(3)
    wav = (0.1 * torch.randn(6, 480160, generator=g)).cuda()
    mel6 = ops.logmel(wav)
    for B in (1, 6):
        say(f"log-mel  B={B}: {event_ms(lambda: ops.logmel(wav[:B]), a.iters * 5):8.3f} ms   (ua2_logmel, fp32)")
    results = {}
    for dtype in ([torch.bfloat16] if a.no_fp32 else [torch.bfloat16, torch.float32]):
        enc.prepare(dtype)
        for B in (1, 6):
            mels = mel6[:B].contiguous()
            iters = a.iters if dtype == torch.bfloat16 else max(a.iters // 5, 1)
            t_stem = event_ms(lambda: enc.stem(mels), iters)
            t_all = event_ms(lambda: enc(mels), iters)
            t_layers = t_all - t_stem
            fl = layer_flops(cfg, B, P)
            say(f"{str(dtype):15s} B={B}: stem {t_stem:8.3f} ms ({stem_flops(cfg, B, P) / t_stem / 1e9:7.1f} TFLOP/s)   24 layers + final LN {t_layers:8.3f} ms "
                f"({fl / t_layers / 1e9:7.1f} TFLOP/s" + (f", {100 * fl / (t_layers * 1e-3) / BF16_DENSE_PEAK:.1f} % of the 2.5 PFLOP/s bf16 dense peak" if dtype == torch.bfloat16 else "")
                + f")   whole forward {t_all:8.3f} ms")
            if dtype == torch.bfloat16:
                results[B] = enc(mels)
    sdb = {k: v.cuda().to(torch.bfloat16) for k, v in sd.items()}
    with torch.inference_mode():
        for B in (1, 6):
            mels = mel6[:B].to(torch.bfloat16)
            t = event_ms(lambda: wr.encoder_ref(sdb, cfg, mels, plain=True), a.iters)
            ref = wr.encoder_ref(sdb, cfg, mels, plain=True)[0].float()
            say(f"plain PyTorch bf16 B={B}: whole forward {t:8.3f} ms   max |ours bf16 - plain bf16| {float((results[B] - ref).abs().max()):.3e} "
                f"(|ref| max {float(ref.abs().max()):.2f})")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
