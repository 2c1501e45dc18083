"""The repetition penalty of the samplers in numpy, written from include/ua2hip.h (ua2_sample_penalized) alone.

History ring of one (row, stream): `hist` holds cap int32 slots and `length` = n counts every id ever appended.  Entry j (0 = the
oldest) lives in hist[j % cap]; an append writes hist[n % cap] and n becomes n + 1.  With window W <= cap and penalty theta, S = the
distinct ids in [0, V) among entries [n - min(n, W), n), and every column c of S reads

    l'_c = l_c * theta  if l_c < 0  else  l_c / theta        (one fp32 operation, once per distinct id)

before the temperature division; everything after it is the existing sampler on l'.  `anchor_case` is the float64-anchored launch the
host test qualifies and the GPU test runs."""
import numpy as np

import sampler_refs as sr


def window_ids(hist, length, W):
    """The last min(length, W) entries of the ring, oldest first."""
    hist = np.asarray(hist).reshape(-1)
    n, cap = max(int(length), 0), hist.shape[0]
    assert 1 <= W <= cap
    return np.array([int(hist[j % cap]) for j in range(n - min(n, W), n)], dtype=np.int64)


def penalize(logits_f32, hist, length, W, theta):
    """fp32 logits of one row [V] -> the fp32 row l' the sampler reads.  The input is not modified."""
    l = np.array(logits_f32, dtype=np.float32, copy=True)
    assert l.ndim == 1
    ids = window_ids(hist, length, W)
    S = np.unique(ids[(ids >= 0) & (ids < l.shape[0])])
    th = np.float32(theta)
    with np.errstate(all="ignore"):
        v = l[S]
        l[S] = np.where(v < 0, v * th, v / th).astype(np.float32)
    return l


def append(hist, length, id):
    """-> (ring, length) after the sampler appended `id`; the inputs are not modified."""
    hist = np.array(hist, dtype=np.int32, copy=True).reshape(-1)
    n = max(int(length), 0)
    hist[n % hist.shape[0]] = int(id)
    return hist, n + 1


def replay_loop(rows, draw, W, theta, hist=None, length=0, cap=None):
    """One stream of one row over consecutive frames.  rows: an iterable of fp32 logit rows [V], one per frame (it may be a generator
    that produces frame f only after frame f - 1's id is known); draw(f, l') -> the id the existing sampler gives on the penalised
    row.  -> list of (id, ring after the append, length after the append), continuing from (hist, length)."""
    hist = np.zeros(W if cap is None else cap, dtype=np.int32) if hist is None else np.array(hist, dtype=np.int32, copy=True)
    out = []
    for f, row in enumerate(rows):
        tok = int(draw(f, penalize(row, hist, length, W, theta)))
        if 0 <= tok < np.asarray(row).shape[0]:
            hist, length = append(hist, length, tok)
        out.append((tok, hist.copy(), int(length)))
    return out


# ---- the float64 anchor case ---------------------------------------------------------------------------------------------------------

ANCHOR = dict(V=12296, M=64, topk=50, T=0.9, theta=1.3, W=16, seed=70)


def anchor_case(seed=None):
    """-> (raw logits [M, V] fp32, rings [M, W] int32, lengths [M] int32, sampler_refs.Launch on the PENALISED logits).  _randn rows;
    row m's history holds m % (3 W + 3) ids drawn (with repeats) from the row's own 50 largest columns, so every penalty moves a
    column the race would otherwise keep."""
    a = ANCHOR
    seed = a["seed"] if seed is None else seed
    V, M, W = a["V"], a["M"], a["W"]
    raw = sr._randn(seed, M, V)
    rng = np.random.default_rng(seed + 1)
    hist, length = np.zeros((M, W), dtype=np.int32), np.zeros(M, dtype=np.int32)
    for m in range(M):
        top = np.argsort(raw[m])[-a["topk"]:]
        for tok in rng.choice(top, m % (3 * W + 3), replace=True):
            hist[m], length[m] = append(hist[m], length[m], tok)
    pen = np.stack([penalize(raw[m], hist[m], length[m], W, a["theta"]) for m in range(M)])
    L = sr.Launch(pen, a["topk"], a["T"], None, seed=888 + seed, counter=(seed % 5, 0, 0), stream_id=2)
    return raw, hist, length, L
