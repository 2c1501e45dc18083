#!/usr/bin/env python3
"""Reasoning-conditioned decode (ReasoningTokenizer.detokenize, 30-s windows) at the released DiT size with seeded weights and
the bench's ScalarModel: ms per 30-s window at 50 guided Euler steps, the conditioning merge (ua2_reason_merge) against the
gather + add it replaces, the device cross-fade (ua2_crossfade) against the host crossfade_concat, detokenize_batch at 8
utterances, and the 20-s detokenize_no_reason window beside them for scale.
python tools/ubench/reason_decode.py [--steps 50] [--profile]   (--profile: one detokenize call of one window, for rocprofv3)"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch

from uniaudio2_amd import ops


def tokenizer():
    import bench
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models.AudioDiffusion1D import AudioDiffusion1D
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models.scalar24k import ScalarModel
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models.transformer_1d_flow import RELEASED_CONFIG
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.reason_tokenizer import ReasoningTokenizer
    torch.manual_seed(0)
    model = AudioDiffusion1D(unet_model_config_path=dict(RELEASED_CONFIG), encoder_depth=1, device="cuda")
    with torch.no_grad():
        for _, p_ in model.named_parameters():
            if p_.dim() > 1:
                p_.normal_(0, 0.02)
        for n_, b_ in model.named_buffers():
            if n_.endswith("_codebook.embed"):
                b_.normal_(0, 0.5)
    model = model.cuda().prepare()
    sq = ScalarModel(**bench.SCALAR_CFG).cuda().prepare()
    return ReasoningTokenizer(sq_codec=sq, model=model, device="cuda")


def codes(T, g):
    return torch.randint(0, 4096, (8, int(T * 0.4) + 1), generator=g), torch.randint(0, 8192, (8, T), generator=g)


def wall(fn, n=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3, out


def event_us(fn, n=200):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    tok = tokenizer()
    g = torch.Generator().manual_seed(1)
    if a.profile:
        q, c = codes(375, g)
        ms, wav = wall(lambda: tok.detokenize(q, c, steps=a.steps))
        print(f"profile: one detokenize call, one 30-s window, {a.steps} steps (solve recorded and replayed): {ms:.1f} ms, {tuple(wav.shape)}")
        return

    # conditioning: the merge kernel against gather + add
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models._dense import nearest_indices
    rec, reason = torch.randn(375, 768, device="cuda"), torch.randn(150, 768, device="cuda")
    src = nearest_indices(150, 2.5, "cuda")[:375].contiguous()
    out = torch.empty_like(rec)
    us_merge = event_us(lambda: ops.reason_merge(rec, reason, src, out=out, src_checked=True))
    us_gather = event_us(lambda: ops.ew_fma(ops.gather_rows(reason, src), c=rec, out=out))
    print(f"conditioning merge (375 x 768): ua2_reason_merge {us_merge:.2f} us, gather_rows + ew_fma {us_gather:.2f} us")

    # cross-fade of 3 decoded 30-s windows (T = 700 codes)
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.reason_tokenizer import crossfade_concat
    seg = torch.rand(3, 720000, device="cuda") - 0.5
    target = int(700 / 12.5 * 24000)
    us_xf = event_us(lambda: ops.crossfade(seg, 720000, 180000, target), 50)
    host = seg.cpu()
    ms_host, _ = wall(lambda: crossfade_concat([host[k:k + 1].clone() for k in range(3)], 720000, 180000, target), 5)
    ms_dev_copy, _ = wall(lambda: ops.crossfade(seg, 720000, 180000, target).cpu(), 5)
    ms_copy3, _ = wall(lambda: seg.cpu(), 5)
    print(f"cross-fade of 3 x 720000 -> {target}: ua2_crossfade {us_xf:.1f} us (+ copy to host: {ms_dev_copy:.2f} ms); host crossfade_concat "
          f"{ms_host:.2f} ms after copying the 3 windows ({ms_copy3:.2f} ms)")

    # one 30-s window at `steps` guided steps, and three
    for T in (375, 700):
        q, c = codes(T, g)
        tok.detokenize(q, c, steps=a.steps)                       # records the solves
        ms, _ = wall(lambda: tok.detokenize(q, c, steps=a.steps), 3)
        n = 1 if T == 375 else 3
        print(f"detokenize T = {T} ({n} window{'s' if n > 1 else ''} of 30 s), {a.steps} steps: {ms:.1f} ms = {ms / n:.1f} ms per window")
    # the 20-s reason-free window for scale
    c20 = torch.randint(0, 8192, (8, 250), generator=g)
    tok.detokenize_no_reason(c20, steps=a.steps)
    ms, _ = wall(lambda: tok.detokenize_no_reason(c20, steps=a.steps), 3)
    print(f"detokenize_no_reason T = 250 (one 20-s window), {a.steps} steps: {ms:.1f} ms")
    # detokenize_batch: 8 one-window utterances in one solve
    pairs = [codes(375, g) for _ in range(8)]
    qs, cs = [p[0] for p in pairs], [p[1] for p in pairs]
    tok.detokenize_batch(qs, cs, steps=a.steps, max_batch=8)
    ms, _ = wall(lambda: tok.detokenize_batch(qs, cs, steps=a.steps, max_batch=8), 2)
    print(f"detokenize_batch of 8 x 30 s (one solve of 2 x 8 x 750 rows), {a.steps} steps: {ms:.1f} ms = {ms / 8:.1f} ms per utterance")


if __name__ == "__main__":
    main()
