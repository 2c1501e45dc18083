"""Plain numpy references of the nucleus (top-p) filter of include/ua2hip.h ua2_sample_topp — what the kernel must keep, not how it finds it.

Two parts:

  * float64: `kept_mask_f64` — the rule in real arithmetic.  Over the admitted columns [forbid, V), l = logits / T, K = the top-k kept set
    (l >= the k-th largest, ties kept), e = exp(l - max l), Z = sum of e over K: column c of K is kept iff S_gt(c) <= p * Z, S_gt(c) the
    mass of the columns of K whose value is strictly greater than l_c.  It also returns the MARGIN of the decision,
    min over the distinct values v of K of |S_gt(v) - p Z| / Z: how far a mass ratio has to move before the kept set changes.  The
    device forms its masses in fp32 (expf, the division by T) and truncates them to multiples of 2^-40, which moves a ratio by about
    1e-6: a test whose margin is well above that may demand the float64 set exactly.
  * exact integers: `kept_mask_int` — the header's fixed-point scheme restated with Python ints on float32 e_c:
    q_c = floor(e_c * 2^40) (0 for a NaN or non-finite e_c), Z = sum over K, P = floor(float64(float32(p)) * 2^32), kept iff
    S_gt(c) * 2^32 <= P * Z.  Z == 0: no nucleus filter.  p == 0 and p >= 1: off.

Ties: every column that ties at the threshold value is kept (the rule is on values, not on sorted positions) — the stated departure
from the reference's sample_top_p (llm_utils/sampling.py:66-82), where torch.sort splits a tie arbitrarily.  `sorted_prefix_mask` restates
that function's own mask for tie-free rows (tests/golden/topp_mask.npz pins the two against each other).
"""
import math

import numpy as np

MASS_BITS = 40          # q_c = floor(e_c * 2^MASS_BITS)
P_BITS = 32             # P = floor(top_p * 2^P_BITS)
MAX_V = 1 << 17         # Z = sum q_c <= 2^57


def _admitted(logits, temperature, forbid, dtype):
    l = np.asarray(logits, dtype=dtype) / dtype(temperature)
    adm = np.zeros(l.shape[0], dtype=bool)
    adm[max(int(forbid), 0):] = True
    return l, adm


def topk_mask(l, adm, topk):
    """K: admitted columns whose value is >= the k-th largest admitted value (ties at the threshold all kept)."""
    vals = np.sort(l[adm])[::-1]
    kth = vals[min(int(topk), vals.shape[0]) - 1]
    return adm & (l >= kth)


def kept_mask_f64(logits, temperature, forbid, topk, top_p):
    """-> (mask [V] bool, margin float).  Finite logits.  top_p == 0 or >= 1: the top-k set, margin inf."""
    l, adm = _admitted(logits, temperature, forbid, np.float64)
    K = topk_mask(l, adm, topk)
    if not 0.0 < top_p < 1.0:
        return K, math.inf
    e = np.where(K, np.exp(l - l[adm].max()), 0.0)
    Z = e.sum()
    keep = np.zeros_like(K)
    margin = math.inf
    for v in np.unique(l[K]):
        s_gt = e[K & (l > v)].sum()
        margin = min(margin, abs(s_gt - top_p * Z) / Z)
        if s_gt <= top_p * Z:
            keep |= K & (l == v)
    return keep, float(margin)


def kept_mask_int(logits, temperature, forbid, topk, top_p):
    """The header's integer rule on float32 values (numpy's float32 exp stands in for the device's expf).  -> mask [V] bool."""
    if len(logits) > MAX_V:
        raise ValueError(f"V = {len(logits)} > {MAX_V}")
    l, adm = _admitted(np.asarray(logits, dtype=np.float32), np.float32(temperature), forbid, np.float32)
    K = topk_mask(l, adm, topk)
    p32 = float(np.float32(top_p))
    if not 0.0 < p32 < 1.0:
        return K
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp((l - l[adm].max()).astype(np.float32)).astype(np.float32)
    q = [int(math.floor(float(x) * 2.0 ** MASS_BITS)) if (K[c] and np.isfinite(x)) else 0 for c, x in enumerate(e)]
    Z = sum(q)
    if Z == 0:
        return K
    P = int(math.floor(p32 * 2.0 ** P_BITS))
    keep = np.zeros_like(K)
    for v in np.unique(l[K]):
        s_gt = sum(q[c] for c in np.nonzero(K & (l > v))[0])
        if (s_gt << P_BITS) <= P * Z:
            keep |= K & (l == v)
    return keep


def kept_mask_probs(probs, top_p):
    """The float64 rule on a row of probabilities (every column admitted, no top-k): what sample_top_p's mask is restated as."""
    pr = np.asarray(probs, dtype=np.float64)
    Z = pr.sum()
    keep = np.zeros(pr.shape[0], dtype=bool)
    for v in np.unique(pr):
        if pr[pr > v].sum() <= top_p * Z:
            keep |= pr == v
    return keep


def sorted_prefix_mask(probs, top_p):
    """sample_top_p's own mask (sampling.py:75-77: sort descending, cumsum, `probs_sum - probs_sort > p` removed), scattered back to
    the columns.  A stable sort: ties are split by position, which is the arbitrariness the value rule above does not have."""
    pr = np.asarray(probs, dtype=np.float64)
    order = np.argsort(-pr, kind="stable")
    srt = pr[order]
    removed = np.cumsum(srt) - srt > top_p
    keep = np.zeros(pr.shape[0], dtype=bool)
    keep[order[~removed]] = True
    return keep
