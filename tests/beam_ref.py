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


def rank(logits, beam, eos, alpha=0.6, lp_n=None):
    """All candidates of one step, best first (stable), and per live row its W + 1 largest logits.  Candidate = (score, parent,
    token or -1, fin, ids).  lp_n: the length of the device's table of 1 / lp — the rule with the length clamped at lp_n - 1, which is
    what ua2_beam_state states for a table shorter than the search (the product's table is longer than max_length: no clamp)."""
    W = len(beam)
    cands, tops = [], []

    def lp(L, alpha):
        return ((5 + (L if lp_n is None else min(L, lp_n - 1))) / 6) ** alpha
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


def select(logits, beam, eos, alpha=0.6, lp_n=None):
    """One step.  logits [W, V] (rows of finished / dead slots are not read), beam: list of W Slots.  Returns (new beam, parents,
    fed-back ids (0 for a finished slot), margins) with margins = (gap between the W-th and the (W+1)-th candidate score, smallest gap
    between a live row's W-th and (W+1)-th logit); inf where there is no (W+1)-th.  lp_n: as in rank."""
    W = len(beam)
    ranked, tops = rank(logits, beam, eos, alpha, lp_n)
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


# ---- plain host restatements of csrc/ua2_beam.hip's two step kernels (tests/test_beam_refs_host.py, tests/test_gpu_beam_parity.py) ----
def topw_ref(row, W):
    """What beam_topw_kernel owes for one fp32 row: (ids of the W best columns under "larger value, then lower id" — a NaN ordered as
    -inf, as rank() orders it —, float64 logp of those columns)."""
    x, logp = log_softmax64(row)
    kth = np.partition(x, x.size - W)[x.size - W]                       # the W-th largest value
    idx = np.flatnonzero(x >= kth)                                      # ascending ids, every column tied with it included
    ids = idx[np.argsort(-x[idx], kind="stable")][:W]
    return ids.astype(np.int64), logp[ids]


def logp32_replay(row, ids, width=1024, summed=None):
    """The fp32 score contract of DESIGN.md §2 in numpy fp32: m = row maximum, S = `width` partial sums of exp(x - m) (column c in
    partial c % width, ascending c, one rounded add per column) joined by the halving tree s = width / 2 .. 1, logp = f32(f32(x - m) -
    f32(log S)).  numpy's fp32 exp and log stand for expf and logf: the replay states the order, not the device's last bit.  Its
    error against log_softmax64 is E_ref.  summed: the number of leading columns that enter S (wrong models; default all)."""
    f = np.float32
    x = np.asarray(row, dtype=f).copy()
    x[np.isnan(x)] = -INF
    ids = np.asarray(ids, dtype=np.int64)
    m = x.max()
    if m == -INF:
        return np.full(ids.size, -INF, f)
    n = -(-x.size // width)
    e = np.zeros(n * width, f)                                          # the columns past V add +0: no rounding
    e[:x.size] = np.exp(x - m)
    if summed is not None:
        e[summed:] = 0
    part = np.zeros(width, f)
    for r in e.reshape(n, width):
        part = part + r
    s = width // 2
    while s >= 1:
        part[:s] = part[:s] + part[s:2 * s]
        s //= 2
    return ((x[ids] - m) - np.log(part[0])).astype(f)


def _ninf32(v):
    v = np.float32(v)
    return v if v == v else np.float32(-INF)


def select32(cand_logp, cand_id, beam_state, lp_inv, eos, W, lp_index=None, score=None, pick=None):
    """beam_select_kernel in numpy fp32, from fp32 candidates.  cand_logp / cand_id: 8 entries per slot (slot j, rank r at j * 8 + r;
    only a live slot's first W are read); beam_state: dict(score, fin, len: the W slots; step, done: ctrl[0], ctrl[1]; log_cap);
    lp_inv: the fp32 table, lp_n = its length.  Candidates in slot order, a live slot's in rank order, a finished slot's one; a NaN is
    -inf; Ln = L for the EOS id, else L + 1; score = f32(score + f32(logp * lp_inv[min(Ln, lp_n - 1)])); the W best, equal scores in
    candidate order; slots without a candidate are dead (score -inf, parent = the slot, len 0).  The ids are taken as given (the
    device's are clamped already).  Returns dict(score: fp32 bits, fin, len, parent, token: the fed-back ids, log: the W records of this
    step or None outside the log's capacity, step, done).  lp_index / score / pick replace one stated operation each (wrong models)."""
    f = np.float32
    lp_index = lp_index or (lambda L, Ln, lp_n: min(Ln, lp_n - 1))
    score = score or (lambda sc, lp, inv: f(sc) + f(f(lp) * f(inv)))    # numpy rounds each fp32 operation once
    pick = pick or (lambda cs, left: max(left, key=lambda i: (cs[i], -i)))      # the first of the best
    cand_logp, cand_id, lp_inv = np.asarray(cand_logp, dtype=f), np.asarray(cand_id), np.asarray(lp_inv, dtype=f)
    cands = []                                                          # (score, parent, token, fin, len)
    with np.errstate(all="ignore"):
        for j in range(W):
            fin, L, sc = int(beam_state["fin"][j]), max(int(beam_state["len"][j]), 0), f(beam_state["score"][j])
            if fin == FINISHED:
                cands.append((_ninf32(sc), j, -1, FINISHED, L))
            elif fin == LIVE:
                for r in range(W):
                    k = int(cand_id[j * 8 + r])
                    Ln = L if k == eos else L + 1
                    s = score(sc, _ninf32(cand_logp[j * 8 + r]), lp_inv[lp_index(L, Ln, lp_inv.size)])
                    cands.append((_ninf32(s), j, -1 if k == eos else k, FINISHED if k == eos else LIVE, Ln))
    cs = [float(c[0]) for c in cands]
    left = list(range(len(cands)))
    out = dict(score=[], fin=[], len=[], parent=[], token=[], log=[])
    for t in range(W):
        s, par, tok, fin, L = f(-INF), t, -1, DEAD, 0
        if left:
            best = pick(cs, left)
            left.remove(best)
            s, par, tok, fin, L = cands[best]
        bits = int(np.array(s, dtype=f).view(np.int32))
        out["score"].append(bits); out["fin"].append(fin); out["len"].append(L); out["parent"].append(par)
        out["token"].append(tok if fin == LIVE else 0)
        out["log"].append([par, tok if fin == LIVE else -1, bits, fin])
    step, done = int(beam_state["step"]), int(beam_state["done"])
    if not 0 <= step < int(beam_state["log_cap"]):
        out["log"] = None
    out["done"] = step if all(x == FINISHED for x in out["fin"]) and done < 0 else done
    out["step"] = step + 1
    return out
