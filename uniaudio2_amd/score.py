"""Teacher-forced scoring of token sequences: python -m uniaudio2_amd.score

The measurement the reference's validation loop prints — cross-entropy and arg-max accuracy of the text stream and of every audio
codebook (llm_models/model_new.py:402-454 forward, :59-109) — on given sequences, through Model_stage3.score_sequence: deterministic,
no sampling, the same inputs for every plan (--dtype fp32 / bf16, --weight_dtype fp8_e4m3, --order_free_rows).

--sequences seqs.pt: a list of dicts {name, tokens (L, 9), mask (L, 9), loss_mask (L, 9), optional: ones}; frame t of a sequence
is scored given frames 0 .. t - 1 (frame 0 is never scored).  --results out.jsonl: one JSON line per sequence — name, frames,
its metrics (acc_text, loss_text, acc_i, loss_i) and per stream (a0 .. a7, text) sum_nll / n_tokens — and a last line "__total__"
with the same over the whole corpus.  Sequences are scored --batch_size at a time, shorter ones padded with unmasked frames behind
their end; on the default plans a sequence's figures depend neither on the batch nor on the padding.
"""
import argparse
import json

import torch

from .llm_models.model_new import metrics_from_stats, score_stats
from .multi_task_inference import _load_config_and_llm


def get_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for name in ("llm_train_config", "resume", "exp_dir", "sequences", "results"):
        p.add_argument(f"--{name}", type=str, default=None)
    p.add_argument("--dtype", type=str, default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--weight_dtype", type=str, default="none", choices=["none", "fp8_e4m3"])
    p.add_argument("--order_free_rows", type=int, default=0)
    p.add_argument("--batch_size", type=int, default=64, help="sequences scored together = rows per chunk of the device pass")
    p.add_argument("--seed", type=int, default=888)
    p.add_argument("--rank", type=int, default=0)
    return p


def _record(name, frames, stats):
    f = lambda t: [float(v) for v in t.tolist()]
    num = lambda v: None if v != v else v                    # a stream without a scored row has no figure: null, not NaN
    return {"name": name, "frames": int(frames), "metrics": {k: num(float(v)) for k, v in metrics_from_stats(stats).items()},
            "sum_nll": f(stats["sum_nll"]), "n_tokens": [int(v) for v in stats["n_tokens"].tolist()]}


def score_corpus(model, seqs, batch_size, device):
    """Yields one record per sequence, in order, then the corpus total."""
    model.setup_caches(batch_size)
    total = None
    for b0 in range(0, len(seqs), batch_size):
        group = seqs[b0:b0 + batch_size]
        L = max(int(s["tokens"].shape[0]) for s in group)
        W = int(group[0]["tokens"].shape[1])
        tokens = torch.zeros(len(group), L, W, dtype=torch.int64)
        mask = torch.zeros(len(group), L, W, dtype=torch.bool)
        loss_mask = torch.zeros(len(group), L, W, dtype=torch.bool)
        for b, s in enumerate(group):
            n = int(s["tokens"].shape[0])
            if n < 2:
                raise ValueError(f"sequence {s.get('name', b0 + b)!r} has {n} frame(s): nothing to score")
            tokens[b, :n], mask[b, :n] = s["tokens"].to(torch.int64), s["mask"].bool()
            loss_mask[b, :n] = s["loss_mask"].bool() if s.get("loss_mask") is not None else True
        tokens, mask, loss_mask = tokens.to(device), mask.to(device), loss_mask.to(device)
        out = model.score_sequence(tokens, mask, loss_mask)
        lab = tokens[:, 1:].clone()
        lab[..., -1] = torch.where(mask[:, 1:, -1], lab[..., -1], torch.full_like(lab[..., -1], -1))
        lab[..., :-1] = torch.where(mask[:, 1:, :1], lab[..., :-1], torch.full_like(lab[..., :-1], -1))
        for b, s in enumerate(group):
            stats = score_stats(out["nll"][b], out["pred"][b], lab[b], mask[b, 1:], loss_mask[b, 1:])
            stats = {k: v.cpu() for k, v in stats.items()}
            total = stats if total is None else {k: total[k] + v for k, v in stats.items()}
            yield _record(s.get("name", str(b0 + b)), s["tokens"].shape[0], stats)
    if total is not None:
        yield _record("__total__", sum(int(s["tokens"].shape[0]) for s in seqs), total)


def main(argv=None):
    args = get_parser().parse_args(argv)
    if not args.llm_train_config or not args.sequences or not args.results:
        raise ValueError("Set --llm_train_config, --sequences and --results.")
    if args.batch_size < 1:
        raise ValueError("--batch_size must be >= 1")
    seqs = torch.load(args.sequences, map_location="cpu")
    if not isinstance(seqs, (list, tuple)) or not seqs:
        raise ValueError(f"{args.sequences}: expected a non-empty list of dicts {{name, tokens, mask[, loss_mask]}}")
    _, model, device = _load_config_and_llm(args)
    with open(args.results, "w", encoding="utf-8") as f:
        for rec in score_corpus(model, list(seqs), args.batch_size, device):
            f.write(json.dumps(rec) + "\n")
    print(f"[Done] scored {len(seqs)} sequence(s) -> {args.results}")


if __name__ == "__main__":
    main()
