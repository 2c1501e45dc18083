#!/usr/bin/env python3
"""Cost of the on-device beam search (Model_stage3.beam_search; --beam_width): ms per beam frame (feedback mode 3) at W = 1, 3, 5, 8
next to the existing text frame (mode 1) at the same row count in the same run, alternating, 3 repeats each; then the two entry
points of a step on their own — ua2_beam_step over the plan's logits, ua2_beam_reorder at partial-page fills 1-2 and 62-63 (the
largest a 64-position page can carry over) — as us per call over a run of back-to-back calls.  Set-up as bench.py's ASR leg: released
sizes, seeded random weights, bf16, a prompt of 15 text + 53 reason + 128 semantic frames, experts skipped after the first frame (what
the generators run).  The EOS id is -1 (never matches), so every slot stays live.  Prefill and graph capture are not timed.
python tools/ubench/beam_search.py [--frames 32] > profiles/beam_search.txt

--groups --baseline-root DIR: the batched search (Model_stage3.beam_search_batch: G utterances' beams as row groups of one frame) at
(G, W) = (1, 8), (2, 8), (4, 8), (8, 8), (4, 4), (16, 4), 3 repeats each, every group on the same prompt, a plan of 2 G W sequences;
then ua2_beam_step_groups and ua2_beam_reorder_groups alone.  The baseline is the single search of ANOTHER checkout of this
repository (DIR: the commit before the groups, built) — G x its ms per frame — measured in the same session: this process never
opens the device; it starts one fresh process per checkout (baseline, groups, baseline again: the two baseline runs bracket the
grouped one and show the drift of the box), and a baseline process uses only the single-search API (begin_beams, generate_frames,
end_beams).
python tools/ubench/beam_search.py --groups --baseline-root ../parent > profiles/beam_search_groups.txt

--ngram --baseline-root DIR: the no-repeat-n-gram ban inside the beam (beam_search(no_repeat_ngram_size=3)) at (G, W) = (1, 5) and (8, 5):
ms per mode-3 frame over 32 frames that start at step 34 and at step 468 (histories of about 50 and about 500 ids; the K/V is that much
longer too, so every column is compared at the same step), 3 repeats each, for the baseline checkout (DIR: the commit before the ban,
built), this checkout with the ban off, and with the ban on.  Processes as under --groups: baseline, this checkout, baseline again.
python tools/ubench/beam_search.py --ngram --baseline-root ../parent > profiles/beam_ngram.txt"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if "--root" in sys.argv:                               # a child process of --groups: measure the checkout it was pointed at
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
import torch

GROUPS = ((1, 8), (2, 8), (4, 8), (8, 8), (4, 4), (16, 4))
NGRAM_GROUPS = ((1, 5), (8, 5))
NGRAM_STARTS = (34, 468)                               # the timed frames start here: texts of 34 .. 66 and of 468 .. 500 ids


def prompt(dev, n_text=15, n_reason=53, n_sem=128):
    import bench
    g = torch.Generator().manual_seed(303)
    L = n_text + n_reason + n_sem
    t = torch.zeros(L, 9, dtype=torch.long)
    m = torch.zeros(L, 9, dtype=torch.bool)
    t[:n_text, -1] = torch.randint(0, 128000, (n_text,), generator=g); m[:n_text, -1] = True
    t[n_text:n_text + n_reason, :8] = torch.randint(0, bench.REASON_CARD, (n_reason, 8), generator=g)
    t[n_text + n_reason:, :8] = bench.REASON_CARD + torch.randint(0, bench.SEM_CARD, (n_sem, 8), generator=g)
    m[n_text:, :8] = True
    return t.to(dev), m.to(dev)


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def text_frames(model, p, W, frames):
    model.begin_ragged([p] * W)
    model.generate_frames(1, W, 1, skip_audio_experts=True)              # the first frame runs the experts: not the steady state
    return timed(lambda: model.generate_frames(frames, W, 1, skip_audio_experts=True)) / frames


def beam_frames(model, p, W, frames):
    model.begin_beams(p[0], p[1], beam_width=W, max_length=frames + 1, eos_id=-1)
    try:
        model.generate_frames(1, W, 3, skip_audio_experts=True)
        return timed(lambda: model.generate_frames(frames, W, 3, skip_audio_experts=True)) / frames
    finally:
        model.end_beams()


def entry_points(model, p, W, calls=200):
    """us per ua2_beam_step and per ua2_beam_reorder (fills 1-2 and 62-63) inside a started search; the search is discarded."""
    import ctypes as C
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import check, lib, vp
    st = model._st
    model.begin_beams(p[0], p[1], beam_width=W, max_length=calls + 2, eos_id=-1)
    try:
        model.generate_frames(2, W, 3, skip_audio_experts=True)           # every slot live, logits of a real frame in the buffer
        bm = model._beam
        logits = model.buffer("text_logits", W)
        vt = logits.shape[1]
        # ua2_stage3_set_beam copied the state by value: the same buffers serve the direct calls (the log has room for `calls` more steps)
        step = lambda: [check(lib.ua2_beam_step(logits.data_ptr(), vt, vt, W, -1, C.byref(bm["state"]), st["out_tokens"].data_ptr(), 9,
                                                ops.stream()), "ua2_beam_step") for _ in range(calls)]
        us_step = timed(step) * 1e3 / calls
        tabs = (vp * 3)(*[g.kv_cache.page_table.data_ptr() for g in (model.audio_understanding_expert, model.backbone, model.audio_generation_expert)])
        n_pools = bm["pools"].numel() // 24
        ident = torch.arange(W, dtype=torch.int32, device=st["device"])
        out = [us_step]
        for fill in (1, 62):                                               # alternating n, n + 1: the page sets alternate, every call copies
            rp = [torch.full((W,), 64 * 3 + fill + k, dtype=torch.int32, device=st["device"]) for k in (0, 1)]
            reorder = lambda: [check(lib.ua2_beam_reorder(W, ident.data_ptr(), rp[i & 1].data_ptr(), 0, bm["pools"].data_ptr(), n_pools, tabs, 3,
                                                          st["B"], model.backbone.kv_cache.max_pages, ops.stream()), "ua2_beam_reorder")
                               for i in range(calls)]
            reorder()
            out.append(timed(reorder) * 1e3 / calls)
        return out
    finally:
        model.end_beams()


def group_frames(model, p, G, W, frames):
    model.begin_beams_groups([p] * G, beam_width=W, max_length=frames + 1, eos_id=-1)
    try:
        model.generate_frames(1, G * W, 3, skip_audio_experts=True)
        return timed(lambda: model.generate_frames(frames, G * W, 3, skip_audio_experts=True)) / frames
    finally:
        model.end_beams_groups()


def group_frames_at(model, p, G, W, frames, start, ngram=0):
    """ms per frame over `frames` frames behind `start` untimed ones; ngram = 0 passes nothing (a baseline checkout has no such argument)."""
    kw = dict(no_repeat_ngram_size=ngram) if ngram else {}
    model.begin_beams_groups([p] * G, beam_width=W, max_length=start + frames + 1, eos_id=-1, **kw)
    try:
        done = 0
        while done < start:
            n = min(frames, start - done)
            model.generate_frames(n, G * W, 3, skip_audio_experts=True)
            done += n
        return timed(lambda: model.generate_frames(frames, G * W, 3, skip_audio_experts=True)) / frames
    finally:
        model.end_beams_groups()


def group_entry_points(model, p, G, W, calls=200):
    """us per ua2_beam_step_groups and per ua2_beam_reorder_groups (fills 1-2 and 62-63) inside a started search; the search is discarded."""
    import ctypes as C
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import check, lib, vp
    st = model._st
    R = G * W
    model.begin_beams_groups([p] * G, beam_width=W, max_length=calls + 2, eos_id=-1)
    try:
        model.generate_frames(2, R, 3, skip_audio_experts=True)
        bm = model._beam
        logits = model.buffer("text_logits", R)
        vt = logits.shape[1]
        step = lambda: [check(lib.ua2_beam_step_groups(logits.data_ptr(), vt, vt, W, G, -1, C.byref(bm["state"]), st["out_tokens"].data_ptr(), 9,
                                                       ops.stream()), "ua2_beam_step_groups") for _ in range(calls)]
        out = [timed(step) * 1e3 / calls]
        tabs = (vp * 3)(*[g.kv_cache.page_table.data_ptr() for g in (model.audio_understanding_expert, model.backbone, model.audio_generation_expert)])
        n_pools = bm["pools"].numel() // 24
        ident = torch.arange(8, dtype=torch.int32, device=st["device"]).repeat(G)       # strided 8 per group, local slot numbers
        for fill in (1, 62):
            rp = [torch.full((R,), 64 * 3 + fill + k, dtype=torch.int32, device=st["device"]) for k in (0, 1)]
            reorder = lambda: [check(lib.ua2_beam_reorder_groups(W, G, ident.data_ptr(), rp[i & 1].data_ptr(), 0, bm["pools"].data_ptr(), n_pools,
                                                                 tabs, 3, st["B"], model.backbone.kv_cache.max_pages, ops.stream()),
                                     "ua2_beam_reorder_groups") for i in range(calls)]
            reorder()
            out.append(timed(reorder) * 1e3 / calls)
        return out
    finally:
        model.end_beams_groups()


def child(a):
    """One checkout, one process: prints one JSON line.  --child single: the single search at W = 8 and 4 on a plan of 2 W sequences (what
    a search over one utterance runs on); --child groups: every (G, W) on a plan of 2 G W sequences."""
    import bench
    dev = torch.device("cuda")
    model = bench.build_model(dev, seed=0)
    p = prompt(dev)
    out = {}
    if a.child in ("ngram-base", "ngram"):
        for G, W in NGRAM_GROUPS:
            model.setup_caches(2 * G * W, dtype=torch.bfloat16, max_seq_length=2048, max_rows=max(64, p[0].shape[0]),
                               log_frames=max(NGRAM_STARTS) + a.frames + 8)     # the frame log counts on through a search
            for n in ((0,) if a.child == "ngram-base" else (0, 3)):
                for start in NGRAM_STARTS:
                    run = lambda: group_frames_at(model, p, G, W, a.frames, start, n)
                    run()                                                  # capture the graphs
                    out[f"{G}x{W} n{n} @{start}"] = [run() for _ in range(a.repeats)]
        print("RESULT " + json.dumps(out), flush=True)
        return
    for G, W in ([(1, 8), (1, 4)] if a.child == "single" else GROUPS):
        model.setup_caches(2 * G * W, dtype=torch.bfloat16, max_seq_length=2048, max_rows=max(64, p[0].shape[0]), log_frames=a.frames + 8)
        run = (lambda: beam_frames(model, p, W, a.frames)) if a.child == "single" else (lambda: group_frames(model, p, G, W, a.frames))
        run()                                                              # capture the graph
        ms = [run() for _ in range(a.repeats)]
        out[f"{G}x{W}"] = dict(ms=ms, us=group_entry_points(model, p, G, W) if a.child == "groups" else None)
    print("RESULT " + json.dumps(out), flush=True)


def _spawn(a, mode, root):
    root = os.path.abspath(root)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--root", root, "--frames", str(a.frames), "--repeats", str(a.repeats)]
    print(f"[beam_search] measuring: {mode} ...", file=sys.stderr, flush=True)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.child_timeout, cwd=root)
    if r.returncode != 0:
        sys.exit(f"the {mode} process ended with {r.returncode}: nothing further is started")
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def ngram_report(a):
    if not a.baseline_root or not os.path.isdir(os.path.join(a.baseline_root, "uniaudio2_amd")):
        sys.exit("--ngram needs --baseline-root DIR: a built checkout of the commit to compare against")
    base_a = _spawn(a, "ngram-base", a.baseline_root)
    new = _spawn(a, "ngram", ROOT)
    base_b = _spawn(a, "ngram-base", a.baseline_root)
    fmt = lambda xs: " ".join(f"{x:.4f}" for x in xs)
    print(f"released sizes, bf16, prompt of 196 frames per utterance, {a.frames} timed frames per run behind 34 / 468 untimed ones, {a.repeats} runs; "
          "one process per checkout, in the order baseline, this checkout, baseline; ms per mode-3 frame")
    for G, W in NGRAM_GROUPS:
        for start in NGRAM_STARTS:
            k = f"{G}x{W} n0 @{start}"
            xa, xb, off, on = base_a[k], base_b[k], new[k], new[f"{G}x{W} n3 @{start}"]
            base = min(xa + xb)
            print(f"G = {G}, W = {W}, steps {start}..{start + a.frames}: baseline before {fmt(xa)} | after {fmt(xb)}; best {base:.4f}, spread of the six runs "
                  f"{(max(xa + xb) - base) * 1e3:.1f} us ({(max(xa + xb) / base - 1) * 100:.2f} %)")
            print(f"    ban off {fmt(off)}; best {min(off):.4f} ({(min(off) - base) * 1e3:+.1f} us, {(min(off) / base - 1) * 100:+.2f} % of the baseline's best)")
            print(f"    ban on, n = 3 {fmt(on)}; best {min(on):.4f} ({(min(on) - min(off)) * 1e3:+.1f} us, {(min(on) / min(off) - 1) * 100:+.2f} % over the ban off)")


def groups_report(a):
    if not a.baseline_root or not os.path.isdir(os.path.join(a.baseline_root, "uniaudio2_amd")):
        sys.exit("--groups needs --baseline-root DIR: a built checkout of the commit to compare against")

    spawn = lambda mode, root: _spawn(a, mode, root)
    base_a = spawn("single", a.baseline_root)
    new = spawn("groups", ROOT)
    base_b = spawn("single", a.baseline_root)
    fmt = lambda xs: " ".join(f"{x:.4f}" for x in xs)
    print(f"released sizes, bf16, prompt of 196 frames per utterance, {a.frames} frames per run, {a.repeats} runs; one process per checkout, in the order "
          "baseline, groups, baseline")
    best = {}
    for W in (8, 4):
        xa, xb = base_a[f"1x{W}"]["ms"], base_b[f"1x{W}"]["ms"]
        best[W] = min(xa + xb)
        print(f"baseline (the commit before the groups), single search W = {W}, plan of {2 * W} sequences: ms/frame before {fmt(xa)} | after {fmt(xb)}; "
              f"best {best[W]:.4f}, spread of the six runs {(max(xa + xb) - min(xa + xb)) * 1e3:.1f} us ({(max(xa + xb) / min(xa + xb) - 1) * 100:.2f} %)")
    for G, W in GROUPS:
        r = new[f"{G}x{W}"]
        b, base = min(r["ms"]), G * best[W]
        us = r["us"]
        print(f"G = {G}, W = {W} ({G * W} rows, plan of {2 * G * W} sequences): ms/frame {fmt(r['ms'])}; best {b:.4f}, spread {(max(r['ms']) - b) * 1e3:.1f} us; "
              f"baseline {G} x {best[W]:.4f} = {base:.4f} ms -> ratio {b / base:.3f} ({base / b:.2f} x the baseline's utterances per second); "
              f"alone, us/call: beam_step_groups (2 launches) {us[0]:.1f}, beam_reorder_groups (2 launches) fill 1-2 {us[1]:.1f}, fill 62-63 {us[2]:.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--groups", action="store_true", help="the batched search against the single search of --baseline-root")
    ap.add_argument("--baseline-root", default=None, help="--groups: a built checkout of the commit to compare against")
    ap.add_argument("--child-timeout", type=int, default=420, help="--groups: seconds one measuring process may take")
    ap.add_argument("--ngram", action="store_true", help="the no-repeat-n-gram ban inside the beam against the search of --baseline-root")
    ap.add_argument("--child", choices=["single", "groups", "ngram-base", "ngram"], default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.groups:
        return groups_report(a)
    if a.ngram:
        return ngram_report(a)
    import bench
    dev = torch.device("cuda")
    model = bench.build_model(dev, seed=0)
    p = prompt(dev)
    model.setup_caches(16, dtype=torch.bfloat16, max_seq_length=2048, max_rows=max(64, p[0].shape[0]), log_frames=a.frames + 8)
    kv = sum(2 * g.config.n_layer * g.config.n_query_groups * g.config.head_size * 2
             for g in (model.audio_understanding_expert, model.backbone, model.audio_generation_expert))
    print(f"released sizes, bf16, prompt of {p[0].shape[0]} frames, {a.frames} frames per run; K/V of one position, three trunk GPTs: {kv / 1e3:.0f} kB")
    for W in (1, 3, 5, 8):
        text_frames(model, p, W, a.frames); beam_frames(model, p, W, a.frames)      # capture the graphs
        t, b = [], []
        for _ in range(a.repeats):
            t.append(text_frames(model, p, W, a.frames))
            b.append(beam_frames(model, p, W, a.frames))
        us = entry_points(model, p, W)
        print(f"W = {W}: ms/frame text (mode 1, {W} rows) {' '.join(f'{x:.4f}' for x in t)} | beam (mode 3) {' '.join(f'{x:.4f}' for x in b)}; "
              f"best {min(t):.4f} -> {min(b):.4f} ({(min(b) - min(t)) * 1e3:+.1f} us/frame, {(min(b) - min(t)) / min(t) * 100:+.2f} %); "
              f"alone, us/call: beam_step (2 launches) {us[0]:.1f}, beam_reorder (2 launches) fill 1-2 {us[1]:.1f}, fill 62-63 {us[2]:.1f}")


if __name__ == "__main__":
    main()
