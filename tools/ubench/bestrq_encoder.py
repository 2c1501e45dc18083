#!/usr/bin/env python3
"""BEST-RQ (MusicFM 25 Hz) encoder at the released size (128 mels, conv_dim 512, encoder_dim 1024, 16 heads, ffn 4096, 11 conformer
layers run) on seeded random weights, one 30-s clip (720 000 samples at 24 kHz) and six (the reference's audio2token batch size):
device-event time of the mel front end, of each of the stem's six ua2_conv2d launches, of the stem's copy + linear, of the conformer
(fp32, the default plan, and the opt-in bf16 plan) and of the whole forward; the achieved TFLOP/s of the five 512 -> 512 convolutions against the
157 TFLOP/s f32 matrix peak.

Yardstick, timed in the same run: the existing exact ua2_conv1d (precision 0) on the equivalent formulation of the first block's
conv2 — Cin = 3 x 512 = 1536, k = 3, Cout = 512 over B x 64 rows of 1500 steps (the gather that would build that operand is NOT
timed).  The 2-D kernel has to be no slower than that.

Every figure is the median of --iters timed calls after 2 warm-up calls.
python tools/ubench/bestrq_encoder.py [--out profiles/bestrq_encoder.txt] [--iters 7] [--batches 1,6]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch

import bestrq_ref as br
from uniaudio2_amd import ops
from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.modules.our_MERT_BESTRQ.mert_fairseq.models.musicfm.model.musicfm_25hz import (
    RELEASED_CONFIG, TAPS, MusicFM25Hz)

F32_MATRIX_PEAK = 157e12            # FLOP/s, MI355X spec


def median_ms(fn, iters, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--batches", default="1,6")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bestrq_encoder.py measures on the GPU; none found")
    cfg = dict(RELEASED_CONFIG)
    enc = MusicFM25Hz(cfg, taps=TAPS)
    enc.load_state_dict(br.state_dict(cfg, seed=8500, n_layers=max(TAPS)), strict=True)
    enc = enc.cuda()
    lines = [f"BEST-RQ encoder, released size {cfg}, taps {TAPS} ({max(TAPS)} layers run), seeded random weights; device-event ms per call, "
             f"median of {a.iters} after 2 warm-up calls"]
    say = lambda s: (lines.append(s), print(s, flush=True))
    g = torch.Generator().manual_seed(5)
    batches = [int(b) for b in a.batches.split(",")]
    wav = (0.1 * torch.randn(max(batches), 720000, generator=g)).cuda()
    C = cfg["conv_dim"]
    for B in batches:
        enc.prepare(torch.float32)
        w = wav[:B].contiguous()
        t_mel = median_ms(lambda: enc.preprocess(w), a.iters)
        mel = enc.preprocess(w)
        say(f"B={B}: mel front end {t_mel:8.3f} ms   (frames gather + exact-fp32 DFT GEMM + ua2_melspec_db; {tuple(mel.shape)})")
        # the stem, launch by launch
        x = mel.unsqueeze(1).contiguous()
        t_convs, flops_512 = 0.0, 0.0
        t_512 = 0.0
        for bi, blk in enumerate(enc.conv.conv):
            p = blk._p
            h = ops.conv2d(x, p[1][0], C, stride=blk.stride, bias=p[1][1], relu=True)
            sc = ops.conv2d(x, p[3][0], C, stride=blk.stride, bias=p[3][1])
            for name, fn, src, cin, stride in (("conv1", lambda: ops.conv2d(x, p[1][0], C, stride=blk.stride, bias=p[1][1], relu=True), x, x.shape[1], blk.stride),
                                               ("conv3", lambda: ops.conv2d(x, p[3][0], C, stride=blk.stride, bias=p[3][1]), x, x.shape[1], blk.stride),
                                               ("conv2", lambda: ops.conv2d(h, p[2][0], C, bias=p[2][1], residual=sc, relu=True), h, C, (1, 1))):
                t = median_ms(fn, a.iters)
                Fo, To = (src.shape[2] - 1) // stride[0] + 1, (src.shape[3] - 1) // stride[1] + 1
                fl = 2.0 * B * C * cin * 9 * Fo * To
                t_convs += t
                if cin == C:
                    flops_512, t_512 = flops_512 + fl, t_512 + t
                say(f"B={B}: block {bi} {name} [{cin} -> {C}, {tuple(src.shape[2:])} -> ({Fo}, {To}), stride {tuple(stride)}] {t:8.3f} ms   "
                    f"{fl / 1e9:8.1f} GFLOP   {fl / t / 1e9:6.1f} TFLOP/s" + (f" ({100 * fl / (t * 1e-3) / F32_MATRIX_PEAK:.1f} % of the f32 matrix peak)" if cin > 4 else ""))
                if bi == 0 and name == "conv2":
                    t_c2 = t
            x = ops.conv2d(h, p[2][0], C, bias=p[2][1], residual=sc, relu=True)
            del h, sc
        say(f"B={B}: the five 512 -> 512 convolutions {t_512:8.3f} ms, {flops_512 / 1e12:.3f} TFLOP: {flops_512 / t_512 / 1e9:6.1f} TFLOP/s "
            f"({100 * flops_512 / (t_512 * 1e-3) / F32_MATRIX_PEAK:.1f} % of the 157 TFLOP/s f32 matrix peak)")
        del x
        t_stem = median_ms(lambda: enc.stem(mel), a.iters)
        say(f"B={B}: stem {t_stem:8.3f} ms   (six convolutions {t_convs:.3f} ms + 'b c f t -> b t (c f)' copy + linear K = {C * cfg['n_mels'] // 4})")
        # yardstick: ua2_conv1d precision 0 on the equivalent formulation of block 0's conv2
        rows = B * cfg["n_mels"] // 2
        xw = torch.randn(rows, 3 * C, 1500, device="cuda")
        wp, K = ops.pack_conv_weight(torch.randn(C, 3 * C, 3, device="cuda") / (9 * C) ** 0.5)
        bias = torch.zeros(C, device="cuda")
        t_1d = median_ms(lambda: ops.conv1d(xw, wp, K, C, pad_left=1, Tout=1500, bias=bias), a.iters)
        fl = 2.0 * rows * C * 3 * C * 3 * 1500
        say(f"B={B}: yardstick ua2_conv1d precision 0 [1536 -> 512, k 3, {rows} rows x 1500 steps, gather not timed] {t_1d:8.3f} ms   {fl / t_1d / 1e9:6.1f} TFLOP/s"
            f"   ->  block 0 conv2 on ua2_conv2d is {t_1d / t_c2:.2f} x the yardstick's speed ({'not slower' if t_c2 <= t_1d else 'SLOWER'})")
        del xw
        for dtype in (torch.float32, torch.bfloat16):
            enc.prepare(dtype)
            t_all = median_ms(lambda: enc.encode(mel), a.iters)
            say(f"B={B}: {str(dtype):15s} stem + {max(TAPS)} conformer layers {t_all:8.3f} ms   (conformer {t_all - t_stem:8.3f} ms)   "
                f"whole forward with the mel front end {t_all + t_mel:8.3f} ms")
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
