"""Decode frame of the fp8 weight-only plan (setup_caches(weight_dtype=torch.float8_e4m3fn)) against the bf16 plan on the original
weights, released sizes, random init, graph replay.

  python tools/ubench/w8_frame.py [--frames 200] [--batches 1 2 5]   ms per frame p50 / p99 per batch, three configurations interleaved in one
                                                                      process (on off bf16 bf16 off on): the fp8 plan, the fp8 plan with
                                                                      UA2_SKINNY_W8_MAX_ROWS=0 (frames of more than 5 rows read the bf16 twin: the
                                                                      behaviour before the fp8 weights-stationary kernel) and the bf16 plan; the two
                                                                      runs of a configuration give the run-to-run spread
  python tools/ubench/w8_frame.py --quality                           logit distance of the first 8 teacher-forced frames (fp8 vs bf16 plan)
  rocprofv3 --kernel-trace --stats -d DIR -o w8 -- python tools/ubench/w8_frame.py --profile
                                                                      20 frames of each plan at B = 1, un-graphed, for tools/rocpd_stats.py --by-grid
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

import bench

FP8 = torch.float8_e4m3fn


def plan(model, B, fp8, log_frames=512):
    model.setup_caches(max(B, 2), dtype=torch.bfloat16, max_seq_length=1024, max_rows=64, log_frames=log_frames,
                       weight_dtype=FP8 if fp8 else None)


def start(model, dev, B):
    prompts = [bench.make_prompt(dev, seed=900 + b) for b in range(B)]
    tokens, mask = torch.cat([t for t, _ in prompts]), torch.cat([k for _, k in prompts])
    L = tokens.size(1)
    model.reset_caches()
    pos = torch.arange(L, device=dev).unsqueeze(0).repeat(B, 1)
    model.forward_prefix(tokens[:, :-1], tokens_mask=mask, input_pos=pos[:, :-1])
    model.begin_decode(tokens[:, -1:], mask[:, -1:], torch.tensor([L - 1], device=dev))
    return tokens, mask


def time_frames(model, dev, B, frames, warmup=20, use_graph=True):
    start(model, dev, B)
    model.generate_frames(warmup, B, 0, reason_eos=-1, reason_card=bench.REASON_CARD, use_graph=use_graph)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(frames + 1)]
    torch.cuda.synchronize()
    ev[0].record()
    model.generate_frames(frames, B, 0, reason_eos=-1, reason_card=bench.REASON_CARD, use_graph=use_graph, frame_events=ev[1:])
    torch.cuda.synchronize()
    ms = np.array([ev[i].elapsed_time(ev[i + 1]) for i in range(frames)])
    return float(np.percentile(ms, 50)), float(np.percentile(ms, 99)), float(ms.mean())


def teacher_forced(model, dev, tokens, mask, frames, forced=None):
    """frames of the reference-shaped API from one prompt; forced = the id frames to feed back (None: the plan's own)."""
    L = tokens.size(1)
    model.reset_caches()
    model.forward_prefix(tokens[:, :-1], tokens_mask=mask, input_pos=torch.arange(L - 1, device=dev).unsqueeze(0))
    ct, cm = tokens[:, -1:], mask[:, -1:]
    ids, tl, al = [], [], []
    for f in range(frames):
        s = model.generate_frame(ct, cm, input_pos=torch.tensor([L - 1 + f], device=dev), input_pos_maxp1=L + f)
        ids.append(s.cpu())
        tl.append(model.buffer("text_logits", 1).float().cpu().clone())
        al.append(model.buffer("audio_logits", 1).float().cpu().clone())
        nxt = (forced[f] if forced is not None else s.cpu()).to(dev)
        audio, text_tok = nxt[:, 1:].long(), nxt[:, 0:1].long()
        ct = torch.cat([audio, text_tok], dim=-1).unsqueeze(1)
        cm = torch.cat([torch.ones_like(audio).bool(), torch.zeros(1, 1, device=dev).bool()], dim=1).unsqueeze(1)
    return ids, torch.stack(tl), torch.stack(al)


def toy_quality(dev):
    """the same distance at the toy sizes of the test-suite (seeded weights, golden prompt tts1)"""
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for p in (os.path.join(root, "tests"), os.path.join(root, "tests", "golden")):
        sys.path.insert(0, p)
    from helpers import build_product_model, load_golden_lm, toy_state_dict
    d, meta = load_golden_lm()
    sd = toy_state_dict(meta)
    tokens = torch.from_numpy(d["tts1_tokens"]).long()[None].to(dev)
    mask = torch.from_numpy(d["tts1_mask"]).bool()[None].to(dev)
    ids_b, tl_b, al_b = teacher_forced(build_product_model(sd, torch.bfloat16, batch=1), dev, tokens, mask, 8)
    ids_q, tl_q, al_q = teacher_forced(build_product_model(sd, torch.bfloat16, batch=1, weight_dtype=FP8), dev, tokens, mask, 8, forced=ids_b)
    rms = lambda x: float(x.double().pow(2).mean().sqrt())
    same = sum(int((p == q).sum()) for p, q in zip(ids_b, ids_q))
    print(f"quality, toy sizes, seeded weights, 8 teacher-forced frames (fp8 plan fed the bf16 plan's ids): "
          f"text logits rms diff {rms(tl_q - tl_b):.3e} max {float((tl_q - tl_b).abs().max()):.3e} (logit rms {rms(tl_b):.3f}); "
          f"audio logits rms diff {rms(al_q - al_b):.3e} max {float((al_q - al_b).abs().max()):.3e} (logit rms {rms(al_b):.3f}); "
          f"ids equal {same}/{8 * 9}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 2, 5])
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    model = bench.build_model(dev).to(torch.bfloat16)
    if a.profile:
        for fp8 in (False, True):
            plan(model, 1, fp8)
            time_frames(model, dev, 1, 20, warmup=2, use_graph=False)
        return
    if a.quality:
        toy_quality(dev)
        tokens, mask = bench.make_prompt(dev, seed=4242)
        plan(model, 1, False)
        ids_b, tl_b, al_b = teacher_forced(model, dev, tokens, mask, 8)
        plan(model, 1, True)
        ids_q, tl_q, al_q = teacher_forced(model, dev, tokens, mask, 8, forced=ids_b)
        rms = lambda x: float(x.double().pow(2).mean().sqrt())
        same = sum(int((p == q).sum()) for p, q in zip(ids_b, ids_q))
        print(f"quality, released sizes, random init, 8 teacher-forced frames (fp8 plan fed the bf16 plan's ids): "
              f"text logits rms diff {rms(tl_q - tl_b):.3e} max {float((tl_q - tl_b).abs().max()):.3e} (logit rms {rms(tl_b):.3f}); "
              f"audio logits rms diff {rms(al_q - al_b):.3e} max {float((al_q - al_b).abs().max()):.3e} (logit rms {rms(al_b):.3f}); "
              f"ids equal {same}/{8 * 9}", flush=True)
        return
    from uniaudio2_amd._lib import lib
    print(f"# ms per decode frame, graph replay, {a.frames} frames after 20 warm-up frames; order per batch: fp8, fp8 with UA2_SKINNY_W8_MAX_ROWS=0, "
          f"bf16, bf16, fp8 with UA2_SKINNY_W8_MAX_ROWS=0, fp8", flush=True)
    names = {"on": "fp8_e4m3          ", "off": "fp8_e4m3 rows=0   ", "bf16": "bf16              "}

    def limit(cfg):          # the launchers read the knob when a frame graph is captured: set it, have it re-read, drop the captured graphs
        if cfg == "off":
            os.environ["UA2_SKINNY_W8_MAX_ROWS"] = "0"
        else:
            os.environ.pop("UA2_SKINNY_W8_MAX_ROWS", None)
        lib.ua2_debug_refresh_env()

    for B in a.batches:
        res = {"on": [], "off": [], "bf16": []}
        try:
            for cfgs in (("on", "off"), ("bf16", "bf16"), ("off", "on")):
                plan(model, B, cfgs[0] != "bf16")
                for cfg in cfgs:
                    limit(cfg)
                    if cfg != "bf16":
                        model.set_w8(True)
                    res[cfg].append(time_frames(model, dev, B, a.frames))
        finally:
            limit("on")
        for cfg in ("on", "off", "bf16"):
            for i, (p50, p99, mean) in enumerate(res[cfg]):
                print(f"B={B} {names[cfg]} run {i}: p50 {p50:.3f} ms  p99 {p99:.3f} ms  mean {mean:.3f} ms", flush=True)
        best = {cfg: min(r[0] for r in res[cfg]) for cfg in res}
        spread = max(abs(res[cfg][0][0] - res[cfg][1][0]) for cfg in res)
        print(f"B={B} best p50: fp8 {best['on']:.3f} ms | fp8 rows=0 {best['off']:.3f} ms | bf16 {best['bf16']:.3f} ms | fp8 / rows=0 {best['on'] / best['off']:.3f} | "
              f"fp8 / bf16 {best['on'] / best['bf16']:.3f} | run-to-run spread (largest |run 0 - run 1| of a configuration) {spread:.3f} ms", flush=True)


if __name__ == "__main__":
    main()
