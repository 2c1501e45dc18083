#!/usr/bin/env python3
"""Throughput of the batched text loop (GeneratorBase._generate_text_batch; --batch_size N for the understanding tasks) against the
one-by-one loop (_generate_text per utterance, what --batch_size 1 runs): utterances/s and text tokens/s over 256 ASR-shaped
prompts at batch_size 1, 8, 32 and 64, and the share of a session's time spent in admission prefills.
Set-up: released sizes, seeded random weights (they never emit EOS: every utterance runs its max_frames), bf16 default plan, greedy,
chunk_frames 16, one plan of 64 sequences for every leg.  Workload (seed 0): a prompt is 15 text frames, then A audio frames with
A ~ U[64, 320] (the first third reason ids, the rest semantic ids + offset), prepare_asr_task's layout; max_frames ~ U[8, 64].
Every leg runs once untimed (graph captures), then `--repeats` timed passes with the legs alternating; a pass is timed on the host
clock around the call, which ends in the loop's last device-to-host read.  The admission share comes from one more pass per
batch size with a device synchronise and a host clock around every admit_rows call — a pass of its own, not one of the timed ones.
python tools/ubench/text_batch_admission.py [--utterances 256] [--repeats 3]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch

N_TEXT = 15


def workload(n, seed=0):
    import bench
    g = torch.Generator().manual_seed(seed)
    n_audio = torch.randint(64, 321, (n,), generator=g).tolist()
    frames = torch.randint(8, 65, (n,), generator=g).tolist()
    prompts = []
    for a in n_audio:
        L, r = N_TEXT + a, a // 3
        t = torch.zeros(L, 9, dtype=torch.long)
        m = torch.zeros(L, 9, dtype=torch.bool)
        t[:N_TEXT, -1] = torch.randint(0, 128000, (N_TEXT,), generator=g); m[:N_TEXT, -1] = True
        t[N_TEXT:N_TEXT + r, :8] = torch.randint(0, bench.REASON_CARD, (r, 8), generator=g)
        t[N_TEXT + r:, :8] = bench.REASON_CARD + torch.randint(0, bench.SEM_CARD, (a - r, 8), generator=g)
        m[N_TEXT:, :8] = True
        prompts.append((t, m))
    return prompts, frames, n_audio


def generator(model):
    """A Generator around `model` without the constructor's own plan (setup_caches(1) at these sizes costs seconds)."""
    from uniaudio2_amd.evaluation.asr_task import Generator
    from uniaudio2_amd.tools.tokenizer.Text2ID.text_tokenizer import load_text_tokenizer
    gen = Generator.__new__(Generator)
    gen._model, gen.device, gen.is_cfg = model, next(model.parameters()).device, False
    gen._text_tokenizer = load_text_tokenizer("ids")
    return gen


def one_by_one(gen, prompts, frames):
    return [gen._generate_text(t, m, topk=1, max_frames=f) for (t, m), f in zip(prompts, frames)]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda")
    model = bench.build_model(dev, seed=0).to(torch.bfloat16)
    gen = generator(model)
    prompts, frames, n_audio = workload(a.utterances)
    sizes = [1, 8, 32, 64]
    model.setup_caches(max(sizes), max_rows=8192, log_frames=512)        # one plan for every leg: no leg re-plans
    legs = [("one by one (_generate_text)", lambda: one_by_one(gen, prompts, frames))]
    legs += [(f"_generate_text_batch, batch_size {n:2d}", (lambda n=n: gen._generate_text_batch(prompts, topk=1, max_frames=frames, batch_size=n)))
             for n in sizes]
    print(f"workload: {a.utterances} prompts, {N_TEXT} text + U[64,320] audio frames (mean {statistics.mean(n_audio):.0f}), max_frames U[8,64] "
          f"(seed 0), {sum(frames)} text frames in all, bf16 plan of {max(sizes)} sequences, greedy, chunk_frames {gen.chunk_frames}")
    ref = None
    for name, fn in legs:                                                # untimed: graph captures of every live row count
        out = fn()
        ref = out if ref is None else ref
        tokens = sum(len(t.split()) for t in out)
        print(f"{name:40s} untimed pass: {tokens} text tokens, texts equal the one-by-one texts: {out == ref}")
    secs, same = {name: [] for name, _ in legs}, {name: True for name, _ in legs}
    for _ in range(a.repeats):
        for name, fn in legs:
            s, out = timed(fn)
            same[name] = same[name] and out == ref
            secs[name].append(s)
    tokens = sum(len(t.split()) for t in ref)
    for name, _ in legs:
        s = secs[name]
        med = statistics.median(s)
        print(f"{name:40s} seconds {' '.join(f'{x:.3f}' for x in s)}  utterances/s {a.utterances / med:7.1f}  text tokens/s {tokens / med:8.0f}  "
              f"spread {(max(s) - min(s)) / med * 100:.1f} %  texts equal: {same[name]}")
    base, new = statistics.median(secs[legs[0][0]]), statistics.median(secs[legs[1][0]])
    print(f"batch_size 1 through the new loop against the one-by-one loop: {new / base:.3f} x the time (medians)")
    real = model.admit_rows
    for n in sizes:                                                      # the admission share: a pass of its own
        spent = []

        def admit(*args, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = real(*args, **kw)
            torch.cuda.synchronize()
            spent.append(time.perf_counter() - t0)
            return r
        model.admit_rows = admit
        try:
            s, _ = timed(lambda: gen._generate_text_batch(prompts, topk=1, max_frames=frames, batch_size=n))
        finally:
            del model.admit_rows
        print(f"batch_size {n:2d}: {len(spent)} admit_rows calls, {sum(spent):.3f} s of {s:.3f} s in admission prefills = {sum(spent) / s * 100:.1f} %")


if __name__ == "__main__":
    main()
