"""The beam-search rule of DESIGN.md §2 in float64 (test infrastructure, not product code): a corrected restatement of the
reference's evaluation/asr_task.py:438-576 — candidate generation :484-557, the length-normalised score :523-524 / :553-555, the EOS
rule :518-526, the selection :560, early stopping :563, the max-length cut :567-570, the final choice :573.

`select` is one step on given logits; `search` drives it over oracle.lm_oracle.Stage3Oracle with W rows, forking the dense caches of
the three trunk GPTs with k[parent] / v[parent], and reports the margins a comparison against fp32 arithmetic has to respect;
`backtrack` recovers the hypotheses from a step log the way the host side of the product does."""
import math
from dataclasses import dataclass, field
from typing import List

import numpy as np
import torch

LIVE, FINISHED, DEAD = 0, 1, 2
INF = float("inf")


def lp(L, alpha):
    """asr_task.py:523, :554."""
    return ((5 + L) / 6) ** alpha


@dataclass
class Slot:
    score: float = -INF
    fin: int = DEAD
    ids: List[int] = field(default_factory=list)

    @property
    def len(self):
        return len(self.ids)


def start(W):
    return [Slot(0.0, LIVE, [])] + [Slot() for _ in range(W - 1)]


def log_softmax64(row):
    """float64 log-softmax of one row; a NaN is ordered as -inf; a row without a finite entry scores -inf everywhere."""
    x = np.asarray(row, dtype=np.float64).copy()
    x[np.isnan(x)] = -INF
    m = x.max()
    if m == -INF:
        return x, np.full_like(x, -INF)
    with np.errstate(divide="ignore"):
        return x, (x - m) - math.log(np.exp(x - m).sum())


def rank(logits, beam, eos, alpha=0.6):
    """All candidates of one step, best first (stable), and per live row its W + 1 largest logits.  Candidate = (score, parent,
    token or -1, fin, ids)."""
    W = len(beam)
    cands, tops = [], []
    for j, b in enumerate(beam):
        if b.fin == FINISHED:
            cands.append((b.score, j, -1, FINISHED, b.ids))
            continue
        if b.fin != LIVE:
            continue
        x, logp = log_softmax64(logits[j])
        order = np.lexsort((np.arange(x.size), -x))
        tops.append(x[order[:W + 1]])
        for k in order[:W]:
            k = int(k)
            if k == eos:                          # the EOS id is not part of the text (:518-526)
                cands.append((b.score + logp[k] / lp(b.len, alpha), j, -1, FINISHED, b.ids))
            else:
                cands.append((b.score + logp[k] / lp(b.len + 1, alpha), j, k, LIVE, b.ids + [k]))
    return sorted(cands, key=lambda c: c[0], reverse=True), tops       # stable: equal scores stay in candidate order (:560)


def select(logits, beam, eos, alpha=0.6):
    """One step.  logits [W, V] (rows of finished / dead slots are not read), beam: list of W Slots.  Returns (new beam, parents,
    fed-back ids (0 for a finished slot), margins) with margins = (gap between the W-th and the (W+1)-th candidate score, smallest gap
    between a live row's W-th and (W+1)-th logit); inf where there is no (W+1)-th."""
    W = len(beam)
    ranked, tops = rank(logits, beam, eos, alpha)
    logit_gap = min([float(t[W - 1] - t[W]) for t in tops if t.size > W and np.isfinite(t[W - 1])], default=INF)
    score_gap = float(ranked[W - 1][0] - ranked[W][0]) if len(ranked) > W and np.isfinite(ranked[W - 1][0]) else INF
    new, parents, fed = [], [], []
    for t in range(W):
        if t < len(ranked):
            s, p, k, f, ids = ranked[t]
            new.append(Slot(float(s), f, list(ids))); parents.append(p); fed.append(k if f == LIVE else 0)
        else:
            new.append(Slot()); parents.append(t); fed.append(0)
    return new, parents, fed, (score_gap, logit_gap)


def finish(beam):
    """The end of the search: live slots count as finished (:567-570), the best score wins, the first slot on ties (:573)."""
    scores = [b.score for b in beam]
    best = max(range(len(beam)), key=lambda j: (scores[j], -j))
    rest = sorted((s for j, s in enumerate(scores) if j != best), reverse=True)
    return best, (scores[best] - rest[0] if rest and np.isfinite(rest[0]) else INF)


def backtrack(log, slot):
    """log [steps, W, 4] int (parent, id or -1, score bits, fin): the text ids of the hypothesis that ends in `slot`."""
    ids, j = [], slot
    for t in range(len(log) - 1, -1, -1):
        parent, tok = int(log[t][j][0]), int(log[t][j][1])
        if tok >= 0:
            ids.append(tok)
        j = parent
    return ids[::-1]


@torch.inference_mode()
def search(oracle, tokens, mask, W, eos, alpha=0.6, max_length=500, early_stopping=True):
    """tokens (L, 9) long, mask (L, 9) bool; oracle: Stage3Oracle with caches for >= W sequences.  Prefill = forward_prefix(prompt[:-1]);
    the first step consumes the prompt's last frame.  Returns dict(beam, best, steps, margins=(score, logit, final))."""
    L = tokens.shape[0]
    oracle.reset_caches()
    pos = torch.arange(L).unsqueeze(0)
    oracle.forward_prefix(tokens[None, :-1], mask[None], pos[:, :-1])
    trunk = (oracle.und, oracle.backbone, oracle.gen)
    for g in trunk:
        for t in g.k + g.v:
            t[1:W] = t[0:1]
    ct = tokens[-1:].unsqueeze(0).repeat(W, 1, 1)
    cm = mask[-1:].unsqueeze(0).repeat(W, 1, 1)
    beam = start(W)
    score_gap = logit_gap = INF
    steps = 0
    for step in range(max_length):
        oracle.generate_frame(ct, cm, torch.full((W,), L - 1 + step, dtype=torch.long), L + step)
        logits = oracle.last_text_logits.double().numpy()
        beam, parents, fed, (sg, lg) = select(logits, beam, eos, alpha)
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
    best, final_gap = finish(beam)
    return dict(beam=beam, best=best, steps=steps, margins=(score_gap, logit_gap, final_gap))
