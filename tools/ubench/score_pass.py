"""Teacher-forced scoring pass (Model_stage3.score: ua2_stage3_trunk + ua2_stage3_score per chunk) at the released sizes, random
init, bf16 plan and fp8 plan, plans of 64 sequences.

  python tools/ubench/score_pass.py [--positions 2048] [--frames 100] > profiles/score_pass.txt

One sequence of --positions frames (text, then audio, then text thirds) is scored in chunks of 64 consecutive positions.  Per plan:
ms per 64-row chunk (mean over the chunks, and the first / last chunk: the attention context grows along the sequence), split by
HIP events into trunk | ua2_stage3_score, the latter into heads (lm_head, 8 x projection + depth decoder + audio head) | cross-entropy
tails (the nine ua2_xent_embed launches timed alone on the plan's logits buffers); tokens scored per second of the whole pass through
Model_stage3.score (host work included); and, for orientation, the same plan's 64-row decode frame (graph replay, p50).
Records, not assertions."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

import bench

FP8 = torch.float8_e4m3fn
ROWS = 64


def sequence(L, va, seed=5):
    g = torch.Generator().manual_seed(seed)
    t = torch.zeros(1, L, 9, dtype=torch.long)
    m = torch.zeros(1, L, 9, dtype=torch.bool)
    a, b = L // 3, 2 * L // 3
    for lo, hi, audio in ((0, a, False), (a, b, True), (b, L, False)):
        if audio:
            t[0, lo:hi, :-1] = torch.randint(0, va, (hi - lo, 8), generator=g)
            m[0, lo:hi, :-1] = True
        else:
            t[0, lo:hi, -1] = torch.randint(0, 128000, (hi - lo,), generator=g)
            m[0, lo:hi, -1] = True
    return t, m


def chunk_times(model, tokens, mask):
    """The chunk loop of Model_stage3._teacher_forced for one sequence with events around its two C calls -> (trunk ms, score ms) per chunk."""
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import check, lib
    dev = tokens.device
    S = tokens.shape[1] - 1
    tk, mk = tokens[0, :-1], mask[0, :-1]
    lab = tokens[0, 1:].clone()
    lab[:, -1] = torch.where(mask[0, 1:, -1], lab[:, -1], torch.full_like(lab[:, -1], -1))
    lab[:, :-1] = torch.where(mask[0, 1:, :1], lab[:, :-1], torch.full_like(lab[:, :-1], -1))
    lab = lab.to(torch.int32).contiguous()
    nll = torch.zeros(S, 9, device=dev)
    pred = torch.zeros(S, 9, dtype=torch.int32, device=dev)
    pos, seq = torch.arange(S, device=dev), torch.zeros(S, dtype=torch.long, device=dev)
    s = ops.stream()
    out = []
    for s0 in range(0, S - S % ROWS, ROWS):
        n = model._load_rows(tk[s0:s0 + ROWS], mk[s0:s0 + ROWS], pos[s0:s0 + ROWS], seq[s0:s0 + ROWS])
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        check(lib.ua2_stage3_trunk(model._h, n, s), "ua2_stage3_trunk")
        ev[1].record()
        check(lib.ua2_stage3_score(model._h, n, lab[s0:].data_ptr(), nll[s0:].data_ptr(), pred[s0:].data_ptr(), s), "ua2_stage3_score")
        ev[2].record()
        out.append(ev)
    torch.cuda.synchronize()
    return np.array([[e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])] for e in out]), lab


def tails_ms(model, lab, iters=20):
    """The nine cross-entropy launches of one 64-row chunk, alone, on the logits the last chunk left in the plan's buffers."""
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import check, lib
    st = model._st
    dev, va, vt, Cb = st["device"], st["va"], model.backbone.config.padded_vocab_size, model.backbone.config.n_embd
    text, audio = model.buffer("text_logits", ROWS), model.buffer("audio_logits", ROWS)
    nll = torch.zeros(ROWS, 9, device=dev)
    pred = torch.zeros(ROWS, 9, dtype=torch.int32, device=dev)
    emb_out = torch.zeros(ROWS, Cb, device=dev)
    dt, s = ops.dtype_code(st["dtype"]), ops.stream()

    def once():
        check(lib.ua2_xent_embed(dt, ROWS, text.data_ptr(), vt, vt, lab.data_ptr(), 9, 8, nll.data_ptr(), pred.data_ptr(), 9, 8, None, 0, Cb, None, s), "xent")
        for i in range(8):
            check(lib.ua2_xent_embed(dt, ROWS, audio[:, i].data_ptr(), 8 * va, va, lab.data_ptr(), 9, i, nll.data_ptr(), pred.data_ptr(), 9, i,
                                     st["audio_emb"].data_ptr() if i < 7 else None, i * va, Cb, emb_out.data_ptr() if i < 7 else None, s), "xent")
    once()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        once()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def decode_frame_p50(model, dev, frames):
    prompts = [bench.make_prompt(dev, seed=900 + b) for b in range(ROWS)]
    tokens, mask = torch.cat([t for t, _ in prompts]), torch.cat([k for _, k in prompts])
    L = tokens.size(1)
    model.reset_caches()
    pos = torch.arange(L, device=dev).unsqueeze(0).repeat(ROWS, 1)
    model.forward_prefix(tokens[:, :-1], tokens_mask=mask, input_pos=pos[:, :-1])
    model.begin_decode(tokens[:, -1:], mask[:, -1:], torch.tensor([L - 1], device=dev))
    model.generate_frames(10, ROWS, 0, reason_eos=-1, reason_card=bench.REASON_CARD)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(frames + 1)]
    torch.cuda.synchronize()
    ev[0].record()
    model.generate_frames(frames, ROWS, 0, reason_eos=-1, reason_card=bench.REASON_CARD, frame_events=ev[1:])
    torch.cuda.synchronize()
    return float(np.percentile([ev[i].elapsed_time(ev[i + 1]) for i in range(frames)], 50))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=100)
    a = ap.parse_args()
    import time
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    model = bench.build_model(dev).to(torch.bfloat16)
    va = bench.SEM_CARD + bench.REASON_CARD
    tokens, mask = sequence(a.positions, va)
    tokens, mask = tokens.to(dev), mask.to(dev)
    print(f"# teacher-forced scoring, released sizes (V_t = 128256, V_a = {va}), random init, one sequence of {a.positions} positions in chunks of "
          f"{ROWS} consecutive positions, plans of {ROWS} sequences x 2048 positions; times in ms (HIP events)", flush=True)
    for name, wd in (("bf16", None), ("fp8_e4m3", FP8)):
        model.setup_caches(ROWS, dtype=torch.bfloat16, max_seq_length=2048, max_rows=ROWS, log_frames=a.frames + 16, weight_dtype=wd)
        chunk_times(model, tokens, mask)                                 # warm-up pass
        ms, lab = chunk_times(model, tokens, mask)
        tails = tails_ms(model, lab[-ROWS:].contiguous())
        trunk, score = ms[:, 0], ms[:, 1]
        print(f"{name:9s} per {ROWS}-row chunk, mean of {len(ms)} chunks: total {trunk.mean() + score.mean():.3f} | trunk {trunk.mean():.3f} | heads "
              f"{score.mean() - tails:.3f} | cross-entropy tails {tails:.3f}   (first chunk: trunk {trunk[0]:.3f} score {score[0]:.3f}; last chunk: trunk "
              f"{trunk[-1]:.3f} score {score[-1]:.3f})", flush=True)
        model.score_sequence(tokens, mask)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.score_sequence(tokens, mask)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        n_tok = int(mask[0, 1:].sum())
        print(f"{name:9s} Model_stage3.score_sequence of the {a.positions}-position sequence: {dt * 1e3:.1f} ms wall, {a.positions - 1} positions / "
              f"{n_tok} tokens scored: {(a.positions - 1) / dt:.0f} positions/s, {n_tok / dt:.0f} tokens/s; loss_text {float(out['metrics']['loss_text']):.4f} "
              f"loss_1 {float(out['metrics']['loss_1']):.4f}", flush=True)
        print(f"{name:9s} for orientation, the same plan's {ROWS}-row decode frame (graph replay, p50 of {a.frames}): "
              f"{decode_frame_p50(model, dev, a.frames):.3f} ms", flush=True)


if __name__ == "__main__":
    main()
