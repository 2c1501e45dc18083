"""Admission against consecutive chunks on bench config 4's workload (256 prompts, 64 rows, bf16 plan, random weights at the
released sizes), and the per-frame cost of the row-form sampler against the shared form at 64 rows.

    python tools/ubench/row_streams_admission.py [--sampler-only] [--out profiles/row_streams_admission.txt]
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

N, ROWS, REPS = 256, 64, 3
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "row_streams_admission.txt")
dev = torch.device("cuda:0")
out_lines = []


def say(s):
    print(s, flush=True)
    out_lines.append(s)
    open(OUT, "w").write("\n".join(out_lines) + "\n")


model = bench.build_model(dev).to(torch.bfloat16)
rs = np.random.RandomState(0)
lens = rs.randint(24, 49, size=N)
nfr = rs.randint(60, 301, size=N)
items = []
for i in range(N):
    g = torch.Generator().manual_seed(4000 + i)
    t = torch.zeros(int(lens[i]), 9, dtype=torch.long)
    t[:, -1] = torch.randint(0, 128000, (int(lens[i]),), generator=g)
    m = torch.zeros(int(lens[i]), 9, dtype=torch.bool)
    m[:, -1] = True
    items.append((t.to(dev), m.to(dev)))
model.setup_caches(ROWS, dtype=torch.bfloat16, max_seq_length=512, max_rows=4096, log_frames=320)
frames_total = int(nfr.sum())
say(f"workload: {N} prompts, lengths U[24,48], frames U[60,300] (seed 0), {frames_total} frames in all, {ROWS} rows, bf16 plan, skip_text_head")
seeds = [1000 + i for i in range(N)]
kw = dict(mode=0, reason_eos=-1, reason_card=bench.REASON_CARD, skip_text_head=True)


def chunked(order):
    for s0 in range(0, N, ROWS):
        idx = order[s0:s0 + ROWS]
        model.generate_ragged([items[i] for i in idx], [int(nfr[i]) for i in idx], **kw)


def admitting(order, with_seeds):
    model.generate_ragged([items[i] for i in order], [int(nfr[i]) for i in order], batch_size=ROWS,
                          seeds=[seeds[i] for i in order] if with_seeds else None, **kw)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


inp = list(range(N))
longest = sorted(inp, key=lambda i: (-int(nfr[i]), i))
for topk in (() if "--sampler-only" in sys.argv else (1, 50)):
    model.set_sampling(topk, 0.9 if topk > 1 else 1.0, seed=888)
    forms = [("chunked, input order", lambda: chunked(inp)), ("admission, input order", lambda: admitting(inp, topk > 1)),
             ("chunked, longest first", lambda: chunked(longest)), ("admission, longest first", lambda: admitting(longest, topk > 1))]
    res = {name: [] for name, _ in forms}
    for rep in range(REPS + 1):                     # the first pass (graph captures) is untimed
        for name, fn in forms:
            dt = timed(fn)
            if rep:
                res[name].append(dt)
    for name, _ in forms:
        ts = res[name]
        tps = [8 * frames_total / t for t in ts]
        say(f"topk {topk:2d}  {name:26s} seconds {' '.join(f'{t:.3f}' for t in ts)}  audio tokens/s {' '.join(f'{v:.0f}' for v in tps)}  "
            f"median {sorted(tps)[len(tps) // 2]:.0f}  spread {(max(tps) - min(tps)) / sorted(tps)[len(tps) // 2] * 100:.1f} %")

# per-frame cost of the sampler forms at 64 rows: 100 frames of a 64-row batch under top-k 50
model.set_sampling(50, 0.9, seed=888)
for name, on in (("shared stream", False), ("row streams", True), ("shared stream", False), ("row streams", True)):
    ms = []
    for rep in range(REPS + 1):
        model.begin_ragged(items[:ROWS])
        model.set_row_seeds(seeds[:ROWS] if on else None)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        model.generate_frames(100, ROWS, 0, reason_eos=-1, reason_card=bench.REASON_CARD, skip_text_head=True)
        e1.record()
        torch.cuda.synchronize()
        if rep:
            ms.append(e0.elapsed_time(e1) / 100)
    model.set_row_seeds(None)
    say(f"top-k 50 frame of {ROWS} rows, {name:13s}: ms per frame {' '.join(f'{v:.4f}' for v in ms)}")
say("done")
