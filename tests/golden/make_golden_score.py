#!/usr/bin/env python3
"""Golden vectors for the teacher-forced pass by RUNNING THE REFERENCE: `Model_stage3.forward` (llm_models/model_new.py:402-454;
its `forward_prefix`, :456-507, is asserted to agree) and the two cross-entropy helpers `CrossEntropyAndAccuracy_text` (:59-73) and
`CrossEntropyAndAccuracy_residual` (:75-109), at the toy sizes (toy_configs.py), seeded weights, fp32, CPU, through the import shim of
make_golden_lm.py.

Authoring-container tool: needs the reference checkout on PYTHONPATH (see make_golden_lm.py); only its output
``tests/golden/lm_score.npz`` / ``lm_score.json`` is used by the tests.

Convention of a scored sequence (tokens (B, L, 9), mask (B, L, 9)), the one make_golden_lm.py:118 uses for the prefix:
    tokens[:, :-1] in, labels = tokens[:, 1:, :-1], tokens_mask = mask, text labels = tokens[:, 1:, -1] where mask[:, 1:, -1] else -1.

Cases
  mix1   B = 1, L = 18: 6 text, 9 audio, 3 text steps (all four text / audio transitions); loss_mask zero on the first 6 steps.
  pair2  B = 2, L = 14: aligned lengths, different contents (4 text, 7 audio, 3 text); loss_mask with seeded zeros per stream; some
         text labels -1.

Recorded per case: the inputs, forward's four outputs, the text labels / text mask handed to CrossEntropyAndAccuracy_text, both
metric dicts (residual with eight unit weights and with the default three; .json) and the top-2 margins of every logit row.

Usage:  PYTHONPATH=<reference checkout> python tests/golden/make_golden_score.py
"""
import json
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
os.environ.setdefault("NO_TORCH_COMPILE", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

from make_golden_lm import build_model, import_reference, shrink_registry
from toy_configs import TOY_MODEL_ARGS
from weights import checksum


def sequence(g, n_text0, n_audio, n_text1, vt, va):
    """(L, 9) tokens / mask: text steps carry a text id under mask [0]*8 + [1], audio steps eight ids under [1]*8 + [0]."""
    L = n_text0 + n_audio + n_text1
    t = torch.zeros(L, 9, dtype=torch.long)
    m = torch.zeros(L, 9, dtype=torch.bool)
    a0, a1 = n_text0, n_text0 + n_audio
    t[:a0, -1] = torch.randint(0, vt, (a0,), generator=g)
    t[a1:, -1] = torch.randint(0, vt, (L - a1,), generator=g)
    t[a0:a1, :-1] = torch.randint(0, va, (n_audio, 8), generator=g)
    m[:a0, -1] = True
    m[a1:, -1] = True
    m[a0:a1, :-1] = True
    return t, m


def margins(logits):
    top2 = torch.topk(logits, 2, dim=-1).values
    return (top2[..., 0] - top2[..., 1]).numpy()


@torch.inference_mode()
def run_case(mn, model_fresh, model_cached, tokens, mask, loss_mask, text_drop):
    """tokens (B, L, 9) long, mask (B, L, 9) bool, loss_mask (B, L, 9) bool, text_drop (B, L-1) bool: text labels forced to -1."""
    B, L, _ = tokens.shape
    S = L - 1
    tk, labels = tokens[:, :-1], tokens[:, 1:, :-1]
    out = model_fresh(tk, labels, mask, loss_mask)
    text_logits, ci_logits, choosed_label, choosed_mask = [o.detach() for o in out]
    pos = torch.arange(0, S).unsqueeze(0).repeat(B, 1)
    model_cached.setup_caches(B)
    model_cached.reset_caches()
    out_p = model_cached.forward_prefix(tk, labels, mask, loss_mask, input_pos=pos)
    for a, b in zip(out, out_p):
        assert a.shape == b.shape and float((a.float() - b.float()).abs().max()) <= 2e-5, "forward and forward_prefix disagree"
    text_mask = mask[:, 1:, -1] & loss_mask[:, 1:, -1]
    text_labels = torch.where(mask[:, 1:, -1] & ~text_drop, tokens[:, 1:, -1], torch.full((B, S), -1))
    _, m_text = mn.CrossEntropyAndAccuracy_text(text_logits, text_labels, text_mask)
    # ignore_id: the function's default None is refused by F.cross_entropy of current torch; -100 is F.cross_entropy's own default
    # (no label matches it), i.e. what "no ignored id" means
    _, m_res8 = mn.CrossEntropyAndAccuracy_residual(ci_logits, choosed_label, choosed_mask, loss_weights=[1] * 8, ignore_id=-100)
    _, m_res3 = mn.CrossEntropyAndAccuracy_residual(ci_logits, choosed_label, choosed_mask, ignore_id=-100)
    arrays = dict(tokens=tokens.numpy(), mask=mask.numpy(), loss_mask=loss_mask.numpy(), text_labels=text_labels.numpy(),
                  text_mask=text_mask.numpy(), text_logits=text_logits.float().numpy(), ci_logits=ci_logits.float().numpy(),
                  choosed_label=choosed_label.numpy(), choosed_mask=choosed_mask.numpy(),
                  text_margin=margins(text_logits.float()), ci_margin=margins(ci_logits.float()))
    fl = lambda d: {k: float(v) for k, v in d.items()}
    return arrays, dict(text=fl(m_text), residual8=fl(m_res8), residual3=fl(m_res3))


def main():
    cfg, lm, mn = import_reference()
    shrink_registry(cfg)
    torch.set_num_threads(4)
    seed = 7                                   # the weights of lm_toy_fp32.npz
    model_fresh, shapes, sd = build_model(mn, seed)
    model_cached, _, _ = build_model(mn, seed)
    vt, va = 500, TOY_MODEL_ARGS["audio_semantic_vocab_size"] + TOY_MODEL_ARGS["audio_reason_vocab_size"]
    g = torch.Generator().manual_seed(4321)
    out, meta = {}, dict(seed=seed, checksum=checksum(sd), torch=torch.__version__, model_args=TOY_MODEL_ARGS, metrics={})

    t, m = sequence(g, 6, 9, 3, vt, va)
    lmask = torch.ones(1, 18, 9, dtype=torch.bool)
    lmask[:, :6] = False
    arrays, metrics = run_case(mn, model_fresh, model_cached, t[None], m[None], lmask, torch.zeros(1, 17, dtype=torch.bool))
    out.update({f"mix1_{k}": v for k, v in arrays.items()}); meta["metrics"]["mix1"] = metrics

    t0, m0 = sequence(g, 4, 7, 3, vt, va)
    t1, m1 = sequence(g, 4, 7, 3, vt, va)
    lmask = torch.rand(2, 14, 9, generator=g) > 0.25
    drop = torch.rand(2, 13, generator=g) < 0.3
    arrays, metrics = run_case(mn, model_fresh, model_cached, torch.stack([t0, t1]), torch.stack([m0, m1]), lmask, drop)
    out.update({f"pair2_{k}": v for k, v in arrays.items()}); meta["metrics"]["pair2"] = metrics

    np.savez_compressed(os.path.join(HERE, "lm_score.npz"), **out)
    with open(os.path.join(HERE, "lm_score.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote lm_score.npz", {k: v.shape for k, v in out.items()})
    print(json.dumps(meta["metrics"], indent=1))


if __name__ == "__main__":
    main()
