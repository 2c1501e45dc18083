#!/usr/bin/env python3
"""Cost of the n-gram filter in the on-device text loop (Model_stage3.set_ngram; --decode_type ngram): ms per text frame with the
filter off and on (n = 3), alternating, 3 repeats each, at B = 1 and at BASELINE config 3's 32 rows.  Set-up as bench.py's ASR leg
(config3_leg): released sizes, seeded random weights, bf16, 32 prompts of 15 text + 53 reason + 128 semantic frames, one ragged
prefill, then 32 text frames with the experts skipped after the first (what the generators run).  The prefill is not timed.
python tools/ubench/ngram_text_loop.py [--frames 32] [--profile]   (--profile: one off and one on run per batch, for rocprofv3)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch


def prompts(dev, B=32, n_text=15, n_reason=53, n_sem=128):
    import bench
    g = torch.Generator().manual_seed(303)                 # bench.config3_leg's prompts
    L = n_text + n_reason + n_sem
    out = []
    for _ in range(B):
        t = torch.zeros(L, 9, dtype=torch.long)
        m = torch.zeros(L, 9, dtype=torch.bool)
        t[:n_text, -1] = torch.randint(0, 128000, (n_text,), generator=g); m[:n_text, -1] = True
        t[n_text:n_text + n_reason, :8] = torch.randint(0, bench.REASON_CARD, (n_reason, 8), generator=g)
        t[n_text + n_reason:, :8] = bench.REASON_CARD + torch.randint(0, bench.SEM_CARD, (n_sem, 8), generator=g)
        m[n_text:, :8] = True
        out.append((t.to(dev), m.to(dev)))
    return out


def run(model, ps, frames, n):
    """ms per frame of `frames` text frames after a ragged prefill of `ps`, and the (frames, B) text ids."""
    model.begin_ragged(ps)
    model.set_ngram(n, 128000, capacity=frames)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    log = model.generate_frames(frames, len(ps), 1, skip_audio_experts=True)
    e1.record()
    torch.cuda.synchronize()
    model.set_ngram(0)
    return e0.elapsed_time(e1) / frames, log[:, :, 0].clone()


def main():
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda")
    model = bench.build_model(dev, seed=0)
    allp = prompts(dev)
    rows = len(allp) * (allp[0][0].shape[0] - 1)
    model.setup_caches(len(allp), dtype=torch.bfloat16, max_seq_length=2048, max_rows=rows, log_frames=a.frames + 8)
    for B in (1, 32):
        ps = allp[:B]
        for n in (0, 3):                                   # first pass per setting captures the frame graphs
            run(model, ps, a.frames, n)
        if a.profile:
            continue
        t = {0: [], 3: []}
        ids = {}
        for _ in range(a.repeats):
            for n in (0, 3):
                ms, ids[n] = run(model, ps, a.frames, n)
                t[n].append(ms)
        fb = int((ids[3] == 128000).sum())
        off, on = min(t[0]), min(t[3])
        print(f"B = {B:2d}: {a.frames} text frames, ms/frame off {' '.join(f'{x:.4f}' for x in t[0])} | "
              f"n = 3 {' '.join(f'{x:.4f}' for x in t[3])}; best {off:.4f} -> {on:.4f} ({(on - off) * 1e3:+.1f} us/frame, "
              f"{(on - off) / off * 100:+.2f} %); {fb} fallback ids in {B} x {a.frames}")


if __name__ == "__main__":
    main()
