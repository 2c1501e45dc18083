"""The no-repeat-n-gram ban of the beam search (include/ua2hip.h ua2_beam_step_groups_ngram) in float64 — test
infrastructure, not product code.  A corrected restatement of the reference's `_apply_ngram_constraint` (evaluation/asr_task.py:602-628,
applied at :504-510 before the softmax), whose own `banned_tokens` set is never filled:

for a LIVE slot with text ids h[0 .. L) and n = no_repeat_ngram_size (2 <= n <= 16; 0 = off), p = h[L - n + 1 .. L) and
ban = { h[i + n - 1] : 0 <= i <= L - n, h[i .. i + n - 1) == p }, empty when L < n; the banned columns count as -inf everywhere the
step reads the row.  `select` and `search` mask the float64 logits and then run tests/beam_ref.py's step, so everything else is that
rule; `search` restates beam_ref.search's loop, which has no hook."""
import numpy as np
import torch

import beam_ref
from beam_ref import FINISHED, INF, LIVE


def banned(ids, n):
    """The set of ids a hypothesis with text `ids` may not take next."""
    ids = [int(k) for k in ids]
    L = len(ids)
    if n < 2 or L < n:
        return set()
    p = ids[L - n + 1:]
    return {ids[i + n - 1] for i in range(L - n + 1) if ids[i:i + n - 1] == p}


def mask(logits, beam, n, cap=None):
    """A float64 copy of logits [W, V] with -inf in the banned columns of every live slot's row.  cap: a slot whose text is longer
    than the device's history capacity is not filtered (ua2hip.h)."""
    x = np.array(logits, dtype=np.float64)
    V = x.shape[1]
    for j, b in enumerate(beam):
        if b.fin != LIVE or (cap is not None and b.len > cap):
            continue
        cols = [k for k in banned(b.ids, n) if 0 <= k < V]
        x[j, cols] = -INF
    return x


def rank(logits, beam, eos, n, alpha=0.6, lp_n=None, cap=None):
    return beam_ref.rank(mask(logits, beam, n, cap), beam, eos, alpha, lp_n)


def select(logits, beam, eos, n, alpha=0.6, lp_n=None, cap=None):
    """One step under the ban: beam_ref.select on the masked logits."""
    return beam_ref.select(mask(logits, beam, n, cap), beam, eos, alpha, lp_n)


@torch.inference_mode()
def search(oracle, tokens, tmask, W, eos, n, alpha=0.6, max_length=500, early_stopping=True):
    """beam_ref.search with the ban: the same prefill, the same fork of the dense caches, `select` above in place of beam_ref.select.
    n = 0 is beam_ref.search.  Returns dict(beam, best, steps, margins=(score, logit, final), fired: steps at which a live slot had a
    non-empty ban set)."""
    L = tokens.shape[0]
    oracle.reset_caches()
    pos = torch.arange(L).unsqueeze(0)
    oracle.forward_prefix(tokens[None, :-1], tmask[None], pos[:, :-1])
    trunk = (oracle.und, oracle.backbone, oracle.gen)
    for g in trunk:
        for t in g.k + g.v:
            t[1:W] = t[0:1]
    ct = tokens[-1:].unsqueeze(0).repeat(W, 1, 1)
    cm = tmask[-1:].unsqueeze(0).repeat(W, 1, 1)
    beam = beam_ref.start(W)
    score_gap = logit_gap = INF
    steps, fired = 0, []
    for step in range(max_length):
        oracle.generate_frame(ct, cm, torch.full((W,), L - 1 + step, dtype=torch.long), L + step)
        logits = oracle.last_text_logits.double().numpy()
        if any(b.fin == LIVE and banned(b.ids, n) for b in beam):
            fired.append(step)
        beam, parents, fed, (sg, lg) = select(logits, beam, eos, n, alpha)
        score_gap, logit_gap = min(score_gap, sg), min(logit_gap, lg)
        steps = step + 1
        idx = torch.tensor(parents)
        for g in trunk:
            for t in g.k + g.v:
                t[:W] = t[idx]
        ct = torch.zeros(W, 1, tokens.shape[1], dtype=torch.long)
        ct[:, 0, -1] = torch.tensor(fed)
        cm = torch.zeros(W, 1, tokens.shape[1], dtype=torch.bool)
        cm[:, 0, -1] = True
        if early_stopping and all(b.fin == FINISHED for b in beam):
            break
    best, final_gap = beam_ref.finish(beam)
    return dict(beam=beam, best=best, steps=steps, margins=(score_gap, logit_gap, final_gap), fired=fired)
