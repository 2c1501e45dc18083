#!/usr/bin/env python3
"""Generate golden vectors for the n-gram-constrained text loop by RUNNING THE REFERENCE.

Container-only tool, like make_golden_lm.py (whose reference import, toy model and logit tap it reuses): needs the reference
on PYTHONPATH; only its output ``tests/golden/lm_ngram.npz`` / ``.json`` travels.

The loop is evaluation/asr_task.py:359-400 (generate_asr_with_ngram_sampling) on the toy LM at fp32 with topk = 1, as the
reference CLI calls it (multi_task_inference.py:316-321): every frame's text candidate goes through the reference's own
`_should_reject_ngram` and `_update_ngrams_simple` (asr_task.py:407-432, taken out of the file with `ast` because the module
imports torchaudio and the codec tokenizer at its top), a banned candidate becomes the fallback id, and the final id is fed
back (audio zeros, text mask 1).  Two departures, both deliberate:
  * the prefill is forward_prefix (as run_loop / generate_asr do), not the training forward of asr_task.py:356;
  * the fallback id is 499 (the toy vocabulary has 500 ids) instead of 128000, and the run has a fixed length (no EOS exists
    in the toy vocabulary).
Recorded per case: the prompt, per frame the candidate id, the final id, the top-2 margin of the text logits and the tie flag;
and the ids of the plain greedy loop on the same prompt.

Usage:  PYTHONPATH=<reference checkout> python tests/golden/make_golden_ngram.py
"""
import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

from make_golden_lm import LogitTap, audio_prompt, build_model, import_reference, shrink_registry
from toy_configs import TOY_MODEL_ARGS
from weights import checksum

FALLBACK = 499
FRAMES = 48
# (case, n, prompt seed)
CASES = [("ng2", 2, 4321), ("ng3", 3, 4321), ("ng3b", 3, 987)]


def reference_rule():
    """_should_reject_ngram / _update_ngrams_simple exactly as the reference's asr_task.py defines them (methods; self unused)."""
    import llm_models
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(llm_models.__file__))), "evaluation", "asr_task.py")
    tree = ast.parse(open(path).read())
    want = {"_should_reject_ngram", "_update_ngrams_simple"}
    fns = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name in want]
    assert {f.name for f in fns} == want
    ns = {}
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, "exec"), ns)
    return ns["_should_reject_ngram"], ns["_update_ngrams_simple"]


@torch.inference_mode()
def text_loop(mn, model, tokens, mask, frames, n, fallback, rule):
    """tokens (L, 9) long, mask (L, 9) bool -> per-frame candidate / final ids, margins, ties (n = 0: the plain greedy loop)."""
    should_reject, update = rule
    tokens, mask = tokens[None], mask[None]
    L = tokens.shape[1]
    model.setup_caches(1)
    model.reset_caches()
    pos = torch.arange(0, L).unsqueeze(0).long()
    model.forward_prefix(tokens[:, :-1], labels=tokens[:, 1:, :-1], tokens_mask=mask, loss_mask=mask, input_pos=pos[:, :-1])
    curr_pos = torch.tensor([L - 1], dtype=torch.int64)
    maxp1 = L
    ct, cm = tokens[:, -1:], mask[:, -1:]
    generated, ngrams = [], {}
    cand, final = [], []
    with LogitTap(mn) as tap:
        for _ in range(frames):
            s = model.generate_frame(ct, cm, input_pos=curr_pos, input_pos_maxp1=maxp1, temperature=1.0, topk=1, forbid_prefix=0)
            c = int(s[0, 0])
            t = fallback if n > 0 and should_reject(None, c, generated, ngrams, n) else c
            cand.append(c); final.append(t)
            generated.append(t)
            if n > 0:
                update(None, generated, ngrams, n)
            ct = torch.cat([torch.zeros(1, 8, dtype=torch.long), torch.tensor([[t]])], dim=-1).unsqueeze(1)
            cm = torch.cat([torch.zeros(1, 8, dtype=torch.bool), torch.ones(1, 1, dtype=torch.bool)], dim=1).unsqueeze(1)
            curr_pos = curr_pos + 1
            maxp1 += 1
    tl = torch.stack(tap.text)[:, 0]                                   # (F, Vt)
    top2 = tl.topk(2, dim=-1).values
    return dict(cand=np.asarray(cand, np.int32), final=np.asarray(final, np.int32),
                margin=(top2[:, 0] - top2[:, 1]).numpy().astype(np.float32), ties=np.asarray(tap.ties, np.bool_))


def main():
    cfg, lm, mn = import_reference()
    shrink_registry(cfg)
    torch.set_num_threads(4)
    seed = 7                                                           # the weights of lm_toy_fp32 (make_golden_lm.py)
    model, shapes, sd = build_model(mn, seed)
    rule = reference_rule()
    vt, va = 500, TOY_MODEL_ARGS["audio_semantic_vocab_size"] + TOY_MODEL_ARGS["audio_reason_vocab_size"]
    out, cases = {}, []
    for name, n, pseed in CASES:
        g = torch.Generator().manual_seed(pseed)
        t, m = audio_prompt(g, 5, 9, vt, va)
        r = text_loop(mn, model, t, m, FRAMES, n, FALLBACK, rule)
        plain = text_loop(mn, model, t, m, FRAMES, 0, FALLBACK, rule)
        assert (plain["cand"] == plain["final"]).all()
        bans = int((r["cand"] != r["final"]).sum())
        assert bans > 0, f"{name}: no ban fired in {FRAMES} frames; lengthen the run"
        assert (r["final"] != plain["final"]).any(), f"{name}: the n-gram loop gave the plain greedy ids"
        out.update({f"{name}_tokens": t.numpy().astype(np.int32), f"{name}_mask": m.numpy(), f"{name}_cand": r["cand"],
                    f"{name}_final": r["final"], f"{name}_margin": r["margin"], f"{name}_ties": r["ties"],
                    f"{name}_plain": plain["final"]})
        cases.append(dict(name=name, n=n, prompt_seed=pseed, bans=bans, any_ties=bool(r["ties"].any())))
    meta = dict(seed=seed, checksum=checksum(sd), fallback=FALLBACK, frames=FRAMES, cases=cases, torch=torch.__version__,
                model_args=TOY_MODEL_ARGS)
    np.savez_compressed(os.path.join(HERE, "lm_ngram.npz"), **out)
    with open(os.path.join(HERE, "lm_ngram.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote lm_ngram.npz", cases)


if __name__ == "__main__":
    main()
