#!/usr/bin/env python3
"""Cost of nucleus (top-p) sampling (ua2_sample_topp; Model_stage3.set_top_p; --top_p).

Part 1, the tail alone: us per launch of the sampling tail at the released head widths (audio va, text vt), M = 1 and 64 rows of seeded
N(0, 2) logits at T = 0.9 — the top-k launch (ua2_sample_topk) against ua2_sample_topp with top_p = 0.9, at topk = 50 and at full
width, and the nucleus on a FLAT row (all logits equal: every column of every pass in one bucket, the worst case of the mass
histogram).  Each figure: 20 warm-up launches, then 7 windows of 200 back-to-back launches between device events; min / median / max of
the windows.

Part 2, the frame: ms per B = 1 sampled frame (topk 50, T 0.9, audio feedback, graph replay) at released sizes with seeded random
weights — this checkout with top_p off, the checkout given by --baseline-root (the parent commit, built) and this checkout with
top_p = 0.9.  One fresh process per figure, in the order baseline, off, 0.9, baseline, off, 0.9: this process never opens the device,
and the repeats bracket each other and show the drift of the box.  Each process: prefill of 33 frames, 8 warm-up frames, then 7
windows of 64 frames.

python tools/ubench/top_p_sampling.py --baseline-root ../parent > profiles/top_p_sampling.txt"""
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
    from uniaudio2_amd._lib import check, lib
    va, vt = bench.SEM_CARD + bench.REASON_CARD, 128256
    counter = torch.zeros(3, dtype=torch.int32, device="cuda")
    print(f"tail alone, us per launch ({WINDOWS} windows of {LAUNCHES} launches): T 0.9, fp32 logits N(0, 2), no gather")
    for name, V in (("audio va", va), ("text vt", vt)):
        for M in (1, 64):
            g = torch.Generator().manual_seed(V + M)
            rnd = (torch.randn(M, V, generator=g) * 2).cuda()
            flat = torch.full((M, V), 0.5, device="cuda")
            out = torch.zeros(M, dtype=torch.int32, device="cuda")
            kc = torch.zeros(M, dtype=torch.int32, device="cuda")

            def launch(lg, topk, p):
                if p is None:
                    return lambda: check(lib.ua2_sample_topk(1, M, lg.data_ptr(), V, V, topk, C.c_float(0.9), None, 1, counter.data_ptr(), 0,
                                                             out.data_ptr(), 1, 0, None, 0, 0, None, 0, ops.stream()), "ua2_sample_topk")
                return lambda: check(lib.ua2_sample_topp(1, M, lg.data_ptr(), V, V, topk, C.c_float(0.9), None, 1, counter.data_ptr(), 0,
                                                         out.data_ptr(), 1, 0, None, 0, 0, None, 0, C.c_float(p), kc.data_ptr(), ops.stream()),
                                     "ua2_sample_topp")

            for label, lg, topk, p in (("top-k 50, off", rnd, 50, None), ("top-k 50, top_p 0.9", rnd, 50, 0.9), ("full width, off", rnd, V, None),
                                       ("full width, top_p 0.9", rnd, V, 0.9), ("flat row, full width, off", flat, V, None),
                                       ("flat row, full width, top_p 0.9", flat, V, 0.9)):
                fn = launch(lg, topk, p)
                for _ in range(20):
                    fn()
                us = [timed(lambda: [fn() for _ in range(LAUNCHES)]) * 1e3 / LAUNCHES for _ in range(WINDOWS)]
                kept = f", nucleus of row 0: {int(kc[0])} columns" if p is not None else ""
                print(f"  {name} = {V}, M = {M:2d}, {label}: {spread(us)}{kept}", flush=True)


def frame_child(a):
    """One figure of part 2 in one process: prints one RESULT line (ms per frame of each window)."""
    import torch
    import bench
    dev = torch.device("cuda")
    model = bench.build_model(dev, seed=0)
    tokens, mask = bench.make_prompt(dev, 7)
    model.setup_caches(1, dtype=torch.bfloat16, max_seq_length=2048, log_frames=8 + WINDOWS * FRAMES)
    model.set_sampling(50, 0.9, seed=1)
    if a.top_p > 0:
        model.set_top_p(a.top_p)
    L = tokens.size(1)
    model.reset_caches()
    pos = torch.arange(L, device=dev).unsqueeze(0)
    model.forward_prefix(tokens[:, :-1], tokens_mask=mask, input_pos=pos[:, :-1])
    model.begin_decode(tokens[:, -1:], mask[:, -1:], torch.tensor([L - 1], device=dev))
    model.generate_frames(8, 1, 0)
    ms = [timed(lambda: model.generate_frames(FRAMES, 1, 0)) / FRAMES for _ in range(WINDOWS)]
    print("RESULT " + json.dumps(ms), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-root", default=None, help="a built checkout of the parent commit (part 2); without it part 2 has no baseline")
    ap.add_argument("--child-timeout", type=int, default=300, help="seconds one measuring process may take")
    ap.add_argument("--child", choices=["tail", "frame"], default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--top_p", type=float, default=0.0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child == "tail":
        return tail_child(a)
    if a.child == "frame":
        return frame_child(a)

    def spawn(mode, root, top_p=0.0):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--root", root, "--top_p", str(top_p)]
        print(f"[top_p_sampling] measuring: {mode} {root} top_p {top_p} ...", file=sys.stderr, flush=True)
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.child_timeout, cwd=root)
        if r.returncode != 0:
            sys.exit(f"the {mode} process ended with {r.returncode}: nothing further is started")
        return r.stdout

    sys.stdout.write(spawn("tail", ROOT))
    sys.stdout.flush()
    legs = [("this commit, top_p off", ROOT, 0.0), ("this commit, top_p 0.9", ROOT, 0.9)]
    if a.baseline_root:
        if not os.path.isdir(os.path.join(a.baseline_root, "uniaudio2_amd")):
            sys.exit("--baseline-root: not a checkout of this repository")
        legs.insert(0, ("parent commit (top-k only)", os.path.abspath(a.baseline_root), 0.0))
    res = {label: [] for label, _, _ in legs}
    for _ in range(2):
        for label, root, p in legs:
            out = spawn("frame", root, p)
            res[label] += json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][7:])
    print(f"B = 1 sampled frame (topk 50, T 0.9, audio feedback, graph replay), released sizes, bf16: ms per frame, 2 processes x {WINDOWS} windows of "
          f"{FRAMES} frames each")
    for label, _, _ in legs:
        xs = res[label]
        print(f"  {label}: {spread([x * 1e3 for x in xs])} us; the two processes' medians "
              f"{statistics.median(xs[:WINDOWS]) * 1e3:.2f} / {statistics.median(xs[WINDOWS:]) * 1e3:.2f} us")
    med = {label: statistics.median(xs) * 1e3 for label, xs in res.items()}
    if a.baseline_root:
        print(f"  off against the parent: {med['this commit, top_p off'] - med['parent commit (top-k only)']:+.2f} us per frame (medians)")
    print(f"  top_p 0.9 against off: {med['this commit, top_p 0.9'] - med['this commit, top_p off']:+.2f} us per frame (medians; 9 samplers per frame)")


if __name__ == "__main__":
    main()
