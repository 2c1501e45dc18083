#!/usr/bin/env python3
"""Cost of the on-device beam search (Model_stage3.beam_search; --beam_width): ms per beam frame (feedback mode 3) at W = 1, 3, 5, 8
next to the existing text frame (mode 1) at the same row count in the same run, alternating, 3 repeats each; then the two entry
points of a step on their own — ua2_beam_step over the plan's logits, ua2_beam_reorder at partial-page fills 1-2 and 62-63 (the
largest a 64-position page can carry over) — as us per call over a run of back-to-back calls.  Set-up as bench.py's ASR leg: released
sizes, seeded random weights, bf16, a prompt of 15 text + 53 reason + 128 semantic frames, experts skipped after the first frame (what
the generators run).  The EOS id is -1 (never matches), so every slot stays live.  Prefill and graph capture are not timed.
python tools/ubench/beam_search.py [--frames 32] > profiles/beam_search.txt"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch


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


def main():
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
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
