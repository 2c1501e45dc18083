"""The samplers' contract in numpy (include/ua2hip.h ua2_sample_topk / _rows / ua2_sample_topp / _rows), replayed draw by draw.

A row's id is a pure function of (logits, T, forbid, topk, top_p, key, draw, row part, stream id):

  l_c   = fp32(logit_c) / fp32(T) over the admitted columns c in [forbid, V)
  kept  = l_c >= the k-th largest admitted l (ties kept; -0.0 == +0.0), and under 0 < top_p < 1 the nucleus of
          topp_ref.kept_mask_int on top of it: the race threshold is the larger of the two
  r     = Philox4x32-10(counter (c, draw, row part, stream id), key (lo, hi)),  key = (seed + device word) mod 2^64
  u_c   = uniform(r[0] >> 8) = min(RN(x + 0.5) * 2^-24, 1 - 2^-24) in fp32: strictly inside (0, 1)
  score = exp(l_c - mx) / -log(u_c),  mx = max admitted l;  the id is the arg-max, the LOWEST column among equal scores.

`race_f64` evaluates the scores in float64 on the fp32 values l, mx, u; `race_f32` is the same formula in numpy float32 and only
sizes the bar: E_ref = the largest relative score difference between the two over the kept columns of a launch,
bar = kernel_refs.bar(E_ref, 1.0) in relative score terms.  A row whose float64 gap (s1 - s2) / s1 exceeds 2 * bar (either score may
move by the bar) must give the reference id exactly; any other row must still give an id of `near`, the kept columns within
2 * bar of the best.  Inputs are finite or -inf (a row keeps at least one finite admitted column); NaN rows stay with the all-NaN
tests of test_gpu_topp.py / test_gpu_rowwise.py.

`Model` switches ONE defect into the replay (tests/test_sampler_refs_host.py shows that each moves the ids the GPU tests assert).
`CASES` are the launches of tests/test_gpu_sampler_replay.py: the host test holds every one of them to 0 rows outside the exact
assertion and E_ref <= 1e-4, so the inputs — not the kernel's output — decide what is asserted."""
import math
from dataclasses import dataclass, replace
from typing import Optional

import numpy as np

import kernel_refs as kr
import topp_ref

U32 = 0xFFFFFFFF
MUL0, MUL1 = 0xD2511F53, 0xCD9E8D57
WEYL0, WEYL1 = 0x9E3779B9, 0xBB67AE85
U_MAX = np.float32(1.0 - 2.0 ** -24)          # the largest fp32 below 1
MARGIN = 1e-4                                 # nucleus decisions nearer than this to top_p are not asserted exactly
CAP = 0.01                                    # at most this share of a launch's rows may fall outside the exact assertion


def philox4x32_10(c0, c1, c2, c3, k0, k1, rounds=10, mul=(MUL0, MUL1)):
    """Philox4x32 (Salmon et al., SC'11) as csrc/ua2_sample.hip writes its rounds; words as uint64 arrays (or ints) holding 32-bit
    values, broadcast against each other.  -> (r0, r1, r2, r3) uint64 arrays."""
    c0, c1, c2, c3 = (np.asarray(x, dtype=np.uint64) & np.uint64(U32) for x in (c0, c1, c2, c3))
    k0, k1 = int(k0) & U32, int(k1) & U32
    for _ in range(rounds):
        p0, p1 = np.uint64(mul[0]) * c0, np.uint64(mul[1]) * c2                 # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & np.uint64(U32),
                          (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & np.uint64(U32))
        k0, k1 = (k0 + WEYL0) & U32, (k1 + WEYL1) & U32
    return c0, c1, c2, c3


def uniform(x):
    """x = r[0] >> 8 in [0, 2^24) -> u in (0, 1): min(RN(x + 0.5) * 2^-24, 1 - 2^-24), every operation in fp32.  x + 0.5 needs 25
    significant bits from x = 2^23 on and rounds to even; at x = 2^24 - 1 it rounds to 2^24, which the min brings back below 1."""
    x = np.asarray(x).astype(np.float32)
    return np.minimum((x + np.float32(0.5)) * np.float32(2.0 ** -24), U_MAX)


def key_words(seed, dev_lo=0, dev_hi=0, carry=True):
    """(lo, hi) of (seed + the device word) mod 2^64; dev_lo / dev_hi are the int32 words of `counter` read as unsigned."""
    seed = int(seed) & (2 ** 64 - 1)
    if carry:
        k = (seed + ((int(dev_lo) & U32) | ((int(dev_hi) & U32) << 32))) & (2 ** 64 - 1)
        return k & U32, k >> 32
    return ((seed & U32) + (int(dev_lo) & U32)) & U32, ((seed >> 32) + (int(dev_hi) & U32)) & U32


@dataclass(frozen=True)
class Model:
    """The contract (defaults) or the contract with one defect."""
    rounds: int = 10
    swap_mul: bool = False
    u_word: int = 0               # which Philox output word feeds u
    drop_stream: bool = False
    drop_draw: bool = False
    flip_shift: bool = False      # row part m under row_key_shift = 1, m >> 1 under 0
    carry: bool = True            # the carry from the low to the high half of seed + device word
    draw_sign_extends: bool = False   # the draw index widened as a signed 64-bit value: its sign fills the next counter word
    tie_high: bool = False        # equal scores go to the higher column
    times_t: bool = False         # logit * T
    rank_off: int = 0             # the top-k threshold taken at rank topk + rank_off
    ignore_forbid: bool = False


CONTRACT = Model()


def _scaled(logits, T, model=CONTRACT):
    x, t = np.asarray(logits, dtype=np.float32), np.float32(T)
    return x * t if model.times_t else x / t


_mask_cache = {}


def kept_mask(logits, T, forbid, topk, top_p):
    """Kept columns of one row under the contract: topp_ref's fp32 top-k set, with its integer nucleus under 0 < top_p < 1."""
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    p32 = float(np.float32(top_p))
    if not 0.0 < p32 < 1.0:
        l = _scaled(logits, T)
        adm = np.arange(l.shape[0]) >= max(int(forbid), 0)
        return topp_ref.topk_mask(l, adm, topk)
    k = (logits.tobytes(), float(T), int(forbid), int(topk), p32)
    if k not in _mask_cache:
        _mask_cache[k] = topp_ref.kept_mask_int(logits, T, forbid, topk, top_p)
    return _mask_cache[k]


def nucleus_margin(logits, T, forbid, topk, top_p):
    """Margin of the float64 nucleus decision on the fp32-scaled logits (inf with the filter off)."""
    if not 0.0 < float(np.float32(top_p)) < 1.0:
        return math.inf
    k = ("margin", np.ascontiguousarray(logits, dtype=np.float32).tobytes(), float(T), int(forbid), int(topk), float(top_p))
    if k not in _mask_cache:
        _mask_cache[k] = topp_ref.kept_mask_f64(np.asarray(logits, dtype=np.float64), T, forbid, topk, top_p)[1]
    return _mask_cache[k]


def _race(dt, logits, T, forbid, topk, top_p, key, draw, row_part, stream_id, model=CONTRACT, mask=None):
    """Scores of the kept columns of one row in `dt`.  key = (lo, hi).  -> (columns [n] ascending, scores [n], ident [n]): ident holds
    the bits of (l_c, u_c) — columns of equal ident score bit-equal in ANY arithmetic, so the tie rule decides between them."""
    l = _scaled(logits, T, model)
    V = l.shape[0]
    fb = 0 if model.ignore_forbid else max(int(forbid), 0)
    if mask is None:
        if model is CONTRACT:
            mask = kept_mask(logits, T, fb, topk, top_p)
        else:                                                                   # the wrong models are top-k only
            assert not 0.0 < top_p < 1.0
            adm = np.arange(V) >= fb
            mask = topp_ref.topk_mask(l, adm, min(max(topk + model.rank_off, 1), V))
    cols = np.nonzero(mask)[0]
    mx = l[fb:].max()
    assert np.isfinite(mx) and not np.isnan(l[fb:]).any(), "rows are finite or -inf with one finite admitted column"
    d = int(draw) & U32
    part = int(row_part) & U32
    if model.draw_sign_extends and d >= 1 << 31:
        part |= U32
    r = philox4x32_10(cols, 0 if model.drop_draw else d, part, 0 if model.drop_stream else int(stream_id) & U32, key[0], key[1],
                      rounds=model.rounds, mul=(MUL1, MUL0) if model.swap_mul else (MUL0, MUL1))
    u = uniform(r[model.u_word] >> np.uint64(8))
    with np.errstate(divide="ignore", over="ignore"):
        if dt is np.float64:
            s = np.exp(l[cols].astype(np.float64) - np.float64(mx)) / -np.log(u.astype(np.float64))
        else:
            s = (np.exp((l[cols] - mx).astype(np.float32)) / -np.log(u)).astype(np.float32)
    ident = (np.ascontiguousarray(l[cols]).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.ascontiguousarray(u).view(np.uint32).astype(np.uint64)
    return cols, s, ident


def _winner(cols, s, ident, bar, tie_high=False):
    """-> (id, s1, s2, near): best column (lowest among equal scores), best score, the best score of the columns that are not the
    winner's twins (equal ident: rounding cannot part them from it, the tie rule alone decides), columns within 2 * bar of the best
    with the winner standing for its twins."""
    s1 = s.max()
    top = cols[s == s1]
    wid = int(top[-1] if tie_high else top[0])
    twin = (ident == ident[cols == wid][0]) & (cols != wid)
    rest = s[(cols != wid) & ~twin]
    s2 = float(rest.max()) if rest.size else 0.0
    near = cols[((s1 - s) <= 2.0 * bar * s1) & ~twin]
    return wid, float(s1), s2, near


def race_f64(logits, T, forbid, topk, top_p, key, draw, row_part, stream_id, bar=0.0, model=CONTRACT):
    """The float64 replay of one row.  -> (id, kept columns, s1, s2, near)."""
    cols, s, ident = _race(np.float64, logits, T, forbid, topk, top_p, key, draw, row_part, stream_id, model)
    wid, s1, s2, near = _winner(cols, s, ident, bar, model.tie_high)
    return wid, cols, s1, s2, near


def race_f32(logits, T, forbid, topk, top_p, key, draw, row_part, stream_id):
    """The same formula in numpy float32: sizes the bar, decides nothing.  -> (kept columns, scores fp32)."""
    return _race(np.float32, logits, T, forbid, topk, top_p, key, draw, row_part, stream_id)[:2]


# ---- a launch and its replay ---------------------------------------------------------------------------------------------------

@dataclass
class Launch:
    """One sampler launch: the arguments of include/ua2hip.h.  form 'shared' = ua2_sample_topk / ua2_sample_topp (seed, counter,
    key_shift), 'rows' = the _rows entry points (keys, draws); top_p 0 = the top-k entry point."""
    logits: np.ndarray                       # [M, V] fp32
    topk: int
    T: float
    forbid: Optional[np.ndarray] = None      # [M] int32 or None
    top_p: float = 0.0
    form: str = "shared"
    seed: int = 888
    counter: tuple = (0, 0, 0)               # int32 words: draw index, device seed word lo, hi
    key_shift: int = 0
    keys: Optional[list] = None              # rows form: 64-bit key per row
    draws: Optional[list] = None             # rows form: int32 draw index per row
    stream_id: int = 2
    note: object = None                      # rows-tie: the (draw, column a, column b) of every row

    @property
    def M(self):
        return self.logits.shape[0]

    @property
    def V(self):
        return self.logits.shape[1]


def row_stream(L, m, model=CONTRACT):
    """(key (lo, hi), draw, row part) of row m of launch L."""
    if L.form == "rows":
        k = int(L.keys[m]) & (2 ** 64 - 1)
        return (k & U32, k >> 32), L.draws[m], 0
    shift = L.key_shift ^ 1 if model.flip_shift else L.key_shift
    return key_words(L.seed, L.counter[1], L.counter[2], model.carry), L.counter[0], m >> shift


def ids_of(L, model=CONTRACT):
    """Ids of every row of L under `model`, float64 scores."""
    out = np.zeros(L.M, dtype=np.int64)
    for m in range(L.M):
        key, draw, part = row_stream(L, m, model)
        fb = 0 if L.forbid is None else int(L.forbid[m])
        out[m] = race_f64(L.logits[m], L.T, fb, L.topk, L.top_p, key, draw, part, L.stream_id, model=model)[0]
    return out


@dataclass
class Replay:
    ids: np.ndarray            # [M] reference ids
    near: list                 # per row: columns the device id may take
    exact: np.ndarray          # [M] bool: asserted exactly
    e_ref: float
    bar: float
    min_gap: float
    min_margin: float = math.inf

    def mismatches(self, got):
        """Rows whose device id breaks the contract: not the reference id on an exact row, outside `near` on another."""
        got = np.asarray(got).reshape(-1)
        return [m for m in range(len(self.ids)) if (int(got[m]) != int(self.ids[m]) if self.exact[m] else int(got[m]) not in set(self.near[m].tolist()))]

    def line(self, case):
        n = len(self.ids)
        return (f"PARITY sampler {case}: rows {n} exact {int(self.exact.sum())} near {n - int(self.exact.sum())} E_ref {self.e_ref:.3e} "
                f"bar {self.bar:.3e} min_gap {self.min_gap:.3e}")


def replay_rows(rows):
    """rows: list of dicts(logits, T, forbid, topk, top_p, key, draw, row_part, stream_id) -> Replay.  E_ref and the bar are taken over
    all of them (one launch, or the launches of one frame)."""
    f64, e_ref = [], 0.0
    for r in rows:
        a = (r["logits"], r["T"], r["forbid"], r["topk"], r["top_p"], r["key"], r["draw"], r["row_part"], r["stream_id"])
        cols, s, ident = _race(np.float64, *a)
        s32 = _race(np.float32, *a)[1]
        pos = s > 0
        assert pos.any() and np.array_equal(s32[~pos], s[~pos]), "a kept column of zero mass scores zero in both"
        e_ref = max(e_ref, float((np.abs(s32[pos].astype(np.float64) - s[pos]) / s[pos]).max()))
        f64.append((cols, s, ident))
    bar = kr.bar(e_ref, 1.0)
    ids, near, exact, min_gap, min_margin = [], [], [], math.inf, math.inf
    for r, (cols, s, ident) in zip(rows, f64):
        wid, s1, s2, nr = _winner(cols, s, ident, bar)
        gap = (s1 - s2) / s1
        ok = gap > 2.0 * bar
        margin = nucleus_margin(r["logits"], r["T"], r["forbid"], r["topk"], r["top_p"])
        if margin <= MARGIN:
            # the nucleus decision is within fp32's reach: the id may be that of either neighbouring set, and no more than that
            ok = False
            sets = [set(nr.tolist())]
            for p in (r["top_p"] - MARGIN, r["top_p"] + MARGIN):
                mask = topp_ref.kept_mask_f64(np.asarray(r["logits"], dtype=np.float32).astype(np.float64), r["T"], r["forbid"], r["topk"], min(max(p, 1e-9), 1 - 1e-9))[0]
                c2, sc2, id2 = _race(np.float64, r["logits"], r["T"], r["forbid"], r["topk"], r["top_p"], r["key"], r["draw"], r["row_part"], r["stream_id"], mask=mask)
                sets.append(set(_winner(c2, sc2, id2, bar)[3].tolist()))
            nr = np.array(sorted(set().union(*sets)))
        ids.append(wid); near.append(nr); exact.append(ok)
        min_gap, min_margin = min(min_gap, gap), min(min_margin, margin)
    return Replay(np.array(ids), near, np.array(exact), e_ref, bar, min_gap, min_margin)


def replay(L):
    rows = []
    for m in range(L.M):
        key, draw, part = row_stream(L, m)
        rows.append(dict(logits=L.logits[m], T=L.T, forbid=0 if L.forbid is None else int(L.forbid[m]), topk=L.topk, top_p=L.top_p, key=key,
                         draw=draw, row_part=part, stream_id=L.stream_id))
    return replay_rows(rows)


# ---- searches with the reference Philox -----------------------------------------------------------------------------------------

# Counters whose r[0] >> 8 is 0xFFFFFF, where RN(x + 0.5) * 2^-24 == 1.0f before the min: key (888, 0), row part 0, stream 1.
# U_EDGE = find_u_edge(888, 0, 1, 1000) is the launch of the GPU test; U_EDGE_WIDE = (draw 310, column 54294) is the first one found,
# over a text-head-sized row.  tests/test_sampler_refs_host.py checks both constants (not the search, which takes a second).
U_EDGE = dict(seed=888, row_part=0, stream_id=1, draw=3443, column=431)
U_EDGE_WIDE = dict(seed=888, row_part=0, stream_id=1, draw=310, column=54294)


def find_u_edge(seed, row_part, stream_id, V, draws=range(0, 1 << 20), x=0xFFFFFF):
    """The first (draw, column < V) whose r[0] >> 8 == x under key (seed, 0): about 2^24 / V draws."""
    lo, hi = key_words(seed)
    return next(((d, int(c[0])) for d in draws for c in [np.nonzero(philox4x32_10(np.arange(V), d, row_part, stream_id, lo, hi)[0] >> np.uint64(8) == np.uint64(x))[0]] if c.size), None)


def find_ties(key, V, n, stream_id=2):
    """n (draw, column a < column b < V) with equal r[0] >> 8 under `key`, row part 0: two columns that draw the same u, so equal
    logits give them bit-equal scores in any arithmetic.  About one draw in 2^25 / V^2 holds such a pair."""
    lo, hi = key & U32, key >> 32
    out, d = [], 0
    while len(out) < n:
        x = philox4x32_10(np.arange(V), d, 0, stream_id, lo, hi)[0] >> np.uint64(8)
        vals, first, cnt = np.unique(x, return_index=True, return_counts=True)
        if (cnt == 2).any() and not (cnt > 2).any():
            v = vals[cnt == 2][0]
            a, b = np.nonzero(x == v)[0]
            out.append((d, int(a), int(b)))
        d += 1
    return out


# ---- the launches of tests/test_gpu_sampler_replay.py --------------------------------------------------------------------------

BASE_V, BASE_M, BASE_TOPK, BASE_T, BASE_FB = 1000, 300, 50, 0.7, 3
NINF = np.float32("-inf")


def _randn(seed, M, V):
    return (np.random.default_rng(seed).standard_normal((M, V)) * 2.0).astype(np.float32)


def _twin_logits(lg, rows):
    """Rows whose two largest logits are exactly equal (different u: no score tie, but a threshold tie at topk 2)."""
    for m in rows:
        a, b = np.argsort(lg[m])[-2:]
        lg[m, a] = lg[m, b]
    return lg


def _row_forbid(seed, M, hi):
    """forbid by row in [0, hi], with 0 and hi themselves among them."""
    fb = np.random.default_rng(seed).integers(0, hi + 1, M).astype(np.int32)
    fb[0], fb[1], fb[M - 1] = 0, hi, hi
    return fb


def _shape_case(V, M, topk, T, forbid, seed, ninf=0, stream_id=2):
    """Shared stream, top-k only.  forbid: None, an int (constant) or 'row' (by row up to V - topk: forbid + topk == V occurs).
    ninf > 0: that many columns of every row hold -inf, placed so that rows with few admitted columns keep some inside the kept set."""
    lg = _twin_logits(_randn(seed, M, V), range(1, M, 7))
    hi = V - topk if topk < V else V - 1                                  # (topk = V: any prefix leaves fewer than topk columns)
    fb = None if forbid is None else (_row_forbid(seed + 1, M, hi) if forbid == "row" else np.full(M, forbid, dtype=np.int32))
    if ninf:
        rng = np.random.default_rng(seed + 2)
        for m in range(M):
            lo = 0 if fb is None else int(fb[m])
            adm = np.arange(lo, V)
            n = min(ninf, adm.shape[0] - 1)                               # one finite admitted column at least
            lg[m, rng.choice(adm, n, replace=False)] = NINF
    return Launch(lg, topk, T, fb, seed=888 + seed, counter=(seed % 5, 0, 0), stream_id=stream_id)


def _base(**kw):
    """The base launch of the counter-word cases: each of them differs from it in the words `kw` names."""
    L = Launch(_randn(20, BASE_M, BASE_V), BASE_TOPK, BASE_T, np.full(BASE_M, BASE_FB, dtype=np.int32), seed=888, counter=(5, 0, 0), stream_id=2)
    return replace(L, **kw)


def _pairs():
    """row_key_shift = 1: rows 2p and 2p + 1 share a draw; every other pair also holds equal logits (a guidance pair) and must hold one id."""
    L = _base(key_shift=1)
    L.logits[1::4] = L.logits[0::4]
    return L


ROW_KEYS = [0x0123456789ABCDEF, 7, 0xFFFFFFFFFFFFFFFF, 0x80000000, 0xDEADBEEF00000001, 0xFFFFFFFF, 0x100000000, 0x8000000000000000]
ROW_DRAWS = [0, 1, 0x7FFFFFFF, -1, -(1 << 31), 6, -2, 12345]


def _rows_case(top_p, M=64, seed=30):
    """Per-row streams: distinct keys and draws per row, the edge values of both among them.  Under top_p the rows are the first M
    candidates whose float64 nucleus margin is above MARGIN."""
    cand = _randn(seed, 2 * M, BASE_V)
    fb = (np.arange(2 * M) % 5).astype(np.int32)
    if top_p:
        ok = [m for m in range(2 * M) if nucleus_margin(cand[m], BASE_T, int(fb[m]), BASE_TOPK, top_p) > 2 * MARGIN][:M]
        cand, fb = cand[ok], fb[ok]
    keys = [ROW_KEYS[m % 8] + 977 * (m // 8) & (2 ** 64 - 1) for m in range(M)]
    draws = [ROW_DRAWS[(m + m // 8) % 8] for m in range(M)]
    return Launch(np.ascontiguousarray(cand[:M]), BASE_TOPK, BASE_T, np.ascontiguousarray(fb[:M]), top_p=top_p, form="rows", keys=keys, draws=draws, stream_id=4)


TIE_KEY = 0x5EED0000FFFFFFF0


def _tie_case(M=16):
    """Two columns that tie BY CONSTRUCTION: find_ties gives, per row, a draw at which columns a < b receive the same 24 random bits,
    hence the same u; both hold the same logit, 8 above the row's other columns, so their scores are bit-equal in any arithmetic and
    far above the rest.  The contract gives the id a; a sampler that breaks ties upwards gives b."""
    ties = find_ties(TIE_KEY, BASE_V, M, stream_id=3)
    lg = _randn(40, M, BASE_V)
    for m, (_, a, b) in enumerate(ties):
        lg[m, a] = lg[m, b] = lg[m].max() + np.float32(8.0)
    L = Launch(lg, 8, 1.0, None, form="rows", keys=[TIE_KEY] * M, draws=[d for d, _, _ in ties], stream_id=3)
    L.note = ties
    return L


def topp_base_row():
    """The base row of tests/test_gpu_topp.py (1000 logits with one exact tie), whose nucleus margins that module asserts."""
    import torch
    base = torch.randn(BASE_V, generator=torch.Generator().manual_seed(0)) * 2
    base[10] = base[11]
    return base.numpy().astype(np.float32)


def _topp_base(topk, p, M=128):
    return Launch(np.ascontiguousarray(np.tile(topp_base_row(), (M, 1))), topk, BASE_T, np.full(M, BASE_FB, dtype=np.int32), top_p=p, seed=888,
                  counter=(2, 0, 0), stream_id=2)


def _topp_randn(M=64, top_p=0.8, seed=50):
    cand = _randn(seed, 2 * M, BASE_V)
    ok = [m for m in range(2 * M) if nucleus_margin(cand[m], BASE_T, BASE_FB, BASE_TOPK, top_p) > 2 * MARGIN][:M]
    return Launch(np.ascontiguousarray(cand[ok]), BASE_TOPK, BASE_T, np.full(M, BASE_FB, dtype=np.int32), top_p=top_p, seed=889, counter=(1, 0, 0), stream_id=6)


def _u_edge(M=4):
    """Row 0 meets the counter U_EDGE at the column that holds its largest logit; topk 8 keeps it with seven others.  u = 1 - 2^-24
    makes q = 6e-8, the smallest a column can draw: the contract says it wins."""
    lg = _randn(60, M, BASE_V)
    lg[0, U_EDGE["column"]] = lg[0].max() + np.float32(0.5)
    return Launch(lg, 8, 1.0, None, seed=U_EDGE["seed"], counter=(U_EDGE["draw"], 0, 0), stream_id=U_EDGE["stream_id"])


CASES = {
    # shapes (shared stream): V, topk, T and the forbid forms
    "v37-k2-T1.0-fbrow": lambda: _shape_case(37, 40, 2, 1.0, "row", 1),
    "v37-k8-T0.7-fb3-ninf": lambda: _shape_case(37, 40, 8, 0.7, 3, 2, ninf=30, stream_id=0),
    "v37-kV-T1.3-ninf": lambda: _shape_case(37, 40, 37, 1.3, None, 3, ninf=5, stream_id=8),
    "v1000-k2-T0.7": lambda: _shape_case(1000, 300, 2, 0.7, None, 4),
    "v1000-k2-T1.3": lambda: _shape_case(1000, 300, 2, 1.3, None, 11),    "v1000-k8-T1.3-fbrow": lambda: _shape_case(1000, 300, 8, 1.3, "row", 5, stream_id=1),
    "v1000-k50-T0.7-fb3": lambda: _shape_case(1000, 300, 50, 0.7, 3, 6),
    "v1000-kV-T1.0-fbrow-ninf": lambda: _shape_case(1000, 100, 1000, 1.0, "row", 7, ninf=40),
    "v1030-k50-T1.0-fbrow": lambda: _shape_case(1030, 64, 50, 1.0, "row", 8),
    "v1030-kV-T0.7": lambda: _shape_case(1030, 64, 1030, 0.7, None, 9),
    "v128256-k50-T0.7-fb3": lambda: _shape_case(128256, 8, 50, 0.7, 3, 10),
    # counter words: one word of the base launch (stream 2) changed
    **{f"ctr-stream{i}": (lambda i=i: _base(stream_id=i)) for i in range(9)},
    "ctr-seed-high": lambda: _base(seed=888 + (0x9E3779B9 << 32)),
    "ctr-carry": lambda: _base(seed=0xFFFFFFFF, counter=(5, 1, 0)),
    "ctr-dev-negative": lambda: _base(counter=(5, -5, -(1 << 31) + 7)),
    "ctr-draw-max": lambda: _base(counter=(0x7FFFFFFF, 0, 0)),
    "ctr-draw-m1": lambda: _base(counter=(-1, 0, 0)),
    "ctr-draw-min": lambda: _base(counter=(-(1 << 31), 0, 0)),
    "ctr-shift1": _pairs,
    # per-row streams
    "rows-topk": lambda: _rows_case(0.0),
    "rows-topp0.8": lambda: _rows_case(0.8),
    "rows-tie": _tie_case,
    # nucleus, shared stream
    **{f"topp-base-k{k}-p{p}": (lambda k=k, p=p: _topp_base(k, p)) for k in (8, 50, 1000) for p in (0.1, 0.5, 0.8, 0.95)},
    "topp-randn-k50-p0.8": _topp_randn,
    # the u edge: fails before the fix of the uniform mapping
    "u-edge": _u_edge,
}
_case_cache = {}


def case(name):
    """(Launch, Replay) of a case, built once per process and not to be written to."""
    if name not in _case_cache:
        L = CASES[name]()
        _case_cache[name] = (L, replay(L))
    return _case_cache[name]
