#!/usr/bin/env python3
"""Cost of the repetition penalty (ua2_sample_penalized; Model_stage3.set_repetition_penalty; --repetition_penalty).

Part 1, the tail alone: us per launch of the sampling tail at the released head widths (audio va, text vt), M = 1 row of seeded N(0, 2)
logits at T = 0.9, top-k 50 — the existing launch (ua2_sample_topk) against ua2_sample_penalized with theta 1.1 and a FULL window of
W = 16 / 64 / 512 distinct ids (the ring is rewound to a full one before every window: each launch appends).  Each figure: 20 warm-up
launches, then 7 windows of 200 back-to-back launches between device events; min / median / max of the windows.

Part 2, the frame: ms per sampled frame (topk 50, T 0.9, audio feedback, graph replay) at released sizes with seeded random weights,
bf16, at B = 1 (shared stream) and at 64 rows with row streams — this checkout with the penalty off, the checkout given by
--baseline-root (the parent commit, built) and this checkout with theta 1.1, W 64.  One fresh process per figure, in the order baseline,
off, on, baseline, off, on: this process never opens the device, and the repeats bracket each other and show the drift of the box.
Each process: prefill of 33 frames, 8 warm-up frames, then 7 windows of 64 frames.

python tools/ubench/rep_penalty.py --baseline-root ../parent > profiles/rep_penalty.txt"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if "--root" in sys.argv:                               # a child process: measure the checkout it was pointed at
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)

WINDOWS, LAUNCHES, FRAMES = 7, 200, 64
THETA, WINDOW = 1.1, 64


def timed(fn):
    import torch
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def spread(xs):
    return f"min {min(xs):.2f} median {statistics.median(xs):.2f} max {max(xs):.2f}"


def tail_child(a):
    """Part 1 in one process: prints the table."""
    import torch
    import bench
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import SampleArgs, check, lib
    va, vt = bench.SEM_CARD + bench.REASON_CARD, 128256
    counter = torch.zeros(3, dtype=torch.int32, device="cuda")
    print(f"tail alone, us per launch ({WINDOWS} windows of {LAUNCHES} launches): M 1, top-k 50, T 0.9, fp32 logits N(0, 2), no gather")
    for name, V in (("audio va", va), ("text vt", vt)):
        g = torch.Generator().manual_seed(V + 1)
        lg = (torch.randn(1, V, generator=g) * 2).cuda()
        out = torch.zeros(1, dtype=torch.int32, device="cuda")

        def measure(label, fn, before=lambda: None):
            for _ in range(20):
                fn()
            us = []
            for _ in range(WINDOWS):
                before()
                us.append(timed(lambda: [fn() for _ in range(LAUNCHES)]) * 1e3 / LAUNCHES)
            print(f"  {name} = {V}, {label}: {spread(us)}", flush=True)

        measure("existing launch", lambda: check(lib.ua2_sample_topk(1, 1, lg.data_ptr(), V, V, 50, C.c_float(0.9), None, 1, counter.data_ptr(), 0,
                                                                      out.data_ptr(), 1, 0, None, 0, 0, None, 0, ops.stream()), "ua2_sample_topk"))
        for W in (16, 64, 512):
            full = torch.randperm(V, generator=g)[:W].int().cuda()         # W distinct ids: the largest set a window holds
            hist, length = full.clone(), torch.full((1,), W, dtype=torch.int32, device="cuda")
            s = SampleArgs()
            s.dtype, s.M, s.logits, s.ld, s.V, s.topk, s.temperature = 1, 1, lg.data_ptr(), V, V, 50, 0.9
            s.seed, s.counter, s.out_tokens, s.out_ld = 1, counter.data_ptr(), out.data_ptr(), 1
            s.rep_penalty, s.rep_window, s.rep_cap, s.rep_hist_ld, s.rep_len_ld = THETA, W, W, W, 1
            s.rep_hist, s.rep_len = hist.data_ptr(), length.data_ptr()

            def rewind():
                hist.copy_(full)
                length.fill_(W)

            measure(f"penalised, theta {THETA}, W {W:3d}", lambda: check(lib.ua2_sample_penalized(C.byref(s), ops.stream()), "ua2_sample_penalized"),
                    rewind)


def frame_child(a):
    """One figure of part 2 in one process: prints one RESULT line (ms per frame of each window)."""
    import torch
    import bench
    dev = torch.device("cuda")
    B = a.rows
    model = bench.build_model(dev, seed=0)
    tokens, mask = bench.make_prompt(dev, 7)
    # (64 rows: 33 + 8 + 7 * 64 = 489 positions per row, planned at 512 as tools/ubench/row_streams_admission.py plans its rows)
    model.setup_caches(B, dtype=torch.bfloat16, max_seq_length=2048 if B == 1 else 512, log_frames=8 + WINDOWS * FRAMES)
    model.set_sampling(50, 0.9, seed=1)
    if a.penalty != 1.0:
        model.set_repetition_penalty(a.penalty, WINDOW)
    model.begin_ragged([(tokens[0], mask[0])] * B)
    if B > 1:
        model.set_row_seeds(list(range(1, B + 1)))
    model.generate_frames(8, B, 0)
    ms = [timed(lambda: model.generate_frames(FRAMES, B, 0)) / FRAMES for _ in range(WINDOWS)]
    print("RESULT " + json.dumps(ms), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-root", default=None, help="a built checkout of the parent commit (part 2); without it part 2 has no baseline")
    ap.add_argument("--child-timeout", type=int, default=300, help="seconds one measuring process may take")
    ap.add_argument("--parts", default="tail,1,64", help="which parts to measure: tail, 1 (the B = 1 frame), 64 (the 64-row frame)")
    ap.add_argument("--child", choices=["tail", "frame"], default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--penalty", type=float, default=1.0, help=argparse.SUPPRESS)
    ap.add_argument("--rows", type=int, default=1, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child == "tail":
        return tail_child(a)
    if a.child == "frame":
        return frame_child(a)

    def spawn(mode, root, penalty=1.0, rows=1):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--root", root, "--penalty", str(penalty), "--rows", str(rows)]
        print(f"[rep_penalty] measuring: {mode} {root} penalty {penalty} rows {rows} ...", file=sys.stderr, flush=True)
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.child_timeout, cwd=root)
        if r.returncode != 0:
            sys.exit(f"the {mode} process ended with {r.returncode}: nothing further is started")
        return r.stdout

    parts = a.parts.split(",")
    if "tail" in parts:
        sys.stdout.write(spawn("tail", ROOT))
        sys.stdout.flush()
    on = f"this commit, theta {THETA}, W {WINDOW}"
    legs = [("this commit, penalty off", ROOT, 1.0), (on, ROOT, THETA)]
    if a.baseline_root:
        if not os.path.isdir(os.path.join(a.baseline_root, "uniaudio2_amd")):
            sys.exit("--baseline-root: not a checkout of this repository")
        legs.insert(0, ("parent commit", os.path.abspath(a.baseline_root), 1.0))
    for rows, what in ((1, "B = 1, shared stream"), (64, "64 rows, row streams")):
        if str(rows) not in parts:
            continue
        res = {label: [] for label, _, _ in legs}
        for _ in range(2):
            for label, root, p in legs:
                out = spawn("frame", root, p, rows)
                res[label] += json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][7:])
        print(f"{what}: sampled frame (topk 50, T 0.9, audio feedback, graph replay), released sizes, bf16: us per frame, 2 processes x {WINDOWS} "
              f"windows of {FRAMES} frames each")
        for label, _, _ in legs:
            xs = res[label]
            print(f"  {label}: {spread([x * 1e3 for x in xs])} us; the two processes' medians "
                  f"{statistics.median(xs[:WINDOWS]) * 1e3:.2f} / {statistics.median(xs[WINDOWS:]) * 1e3:.2f} us")
        med = {label: statistics.median(xs) * 1e3 for label, xs in res.items()}
        if a.baseline_root:
            print(f"  off against the parent: {med['this commit, penalty off'] - med['parent commit']:+.2f} us per frame (medians)")
        print(f"  penalty on against off: {med[on] - med['this commit, penalty off']:+.2f} us per frame (medians; 9 samplers per frame)", flush=True)


if __name__ == "__main__":
    main()
