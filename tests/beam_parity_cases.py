"""The launches of tests/test_gpu_beam_parity.py, built on the host alone (numpy; tests/test_beam_refs_host.py walks the same list
without a GPU): shapes, row kinds, beam states, what every launch owes (tests/beam_ref.py: topw_ref, logp32_replay, select32, select),
and host models of beam_topw_kernel's per-thread lists with one defect each.

Shapes: the smallest at which each path of beam_topw_kernel exists (an outer iteration is 16 x 1024 columns, a thread keeps 8
entries) and the released vocabulary.  V = 9217: thread 0 meets 10 columns, so its list overflows; 16384: one full outer iteration;
16385: a second one of a single column; 33000: three, the last ragged; 128256: eight, the last of 256 columns, 125 - 126 per thread.
Columns [V, ld) hold 777: read, they would win every comparison.

Every launch is decided by construction: the W + 1 largest logits of a row are exact ties or >= 1e-3 apart (spread_top), and the
slot scores are drawn until the float64 rule's W + 1 best candidate scores are, too (at most TRIES draws, from the reference alone)."""
import functools
import zlib
from dataclasses import dataclass
from typing import List

import numpy as np

import beam_ref
import kernel_refs as kr
from beam_ref import DEAD, FINISHED, INF, LIVE, Slot

PAD = 777.0
SMALL = [9217, 16384, 16385, 33000]
RELEASED = 128256
WIDTHS = [1, 5, 8]
THREADS, BATCH, ENTRIES = 1024, 16, 8                 # beam_topw_kernel's geometry
OUTER = THREADS * BATCH
NONE = 0x7fffffff
CAP = 4                                               # steps of the log; a launch at step CAP writes no record
TRIES = 20
KINDS = ["randn4", "flat", "res0_asc", "res0_desc", "res0_straddle", "resL_asc", "resL_desc", "resL_straddle", "last_w", "ties",
         "ninf3", "nans", "few_finite", "none"]
STATE_KINDS = [KINDS[(5 + 3 * j) % len(KINDS)] for j in range(8)]     # the rows of the state launches: eight different kinds again


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def spread_top(x, W, step):
    """The W + 1 largest entries of x, where they stand, respaced `step` apart above the (W + 2)-th."""
    ids, _ = beam_ref.topw_ref(x, W + 2)
    for k in range(W + 1):
        x[ids[k]] = np.float32(x[ids[W + 1]] + step * (W + 1 - k))
    return x


def make_row(kind, V, W, rng):
    f = np.float32
    x = (rng.standard_normal(V) * (0.01 if kind == "flat" else 4.0)).astype(f)
    top = f(np.ceil(x.max()) + 2)
    if kind == "randn4":
        return spread_top(x, W, 0.125)
    if kind == "flat":                                  # every column matters to S
        return spread_top(x, W, 4e-3)
    if kind.startswith("res"):                          # the W + 1 largest values in one thread's columns
        res = 0 if kind.startswith("res0") else (V - 1) % THREADS
        cols = np.arange(res, V, THREADS)
        order = kind.split("_")[1]
        if order == "asc":                              # the last W + 1 of them, each better than all before it: the list is full by then
            pick, ranks = cols[-(W + 1):], np.arange(W, -1, -1)
        elif order == "desc":                           # the first W + 1, best first: nothing later may displace them
            pick, ranks = cols[:W + 1], np.arange(W + 1)
        else:                                           # on both sides of the first outer iteration's end (the middle where V <= 16384)
            at = int(np.searchsorted(cols, OUTER)) if V > OUTER else cols.size // 2
            lo = min(max(at - (W + 1) // 2, 0), cols.size - (W + 1))
            pick, ranks = cols[lo:lo + W + 1], rng.permutation(W + 1)
        x[pick] = (top + 0.125 * (W - ranks)).astype(f)
        return x
    if kind == "last_w":
        x[V - W:] = (top + 0.125 * rng.permutation(W)).astype(f)
        return x
    if kind == "ties":                                  # one value in more than W columns: different threads, one thread in one
        want = [0, THREADS, OUTER if V > OUTER else 2 * THREADS, V - 1, 700, 1023, 1101, V - 300, 3000, 4242, 8000, 9000, 6001, 7007]
        cols = list(dict.fromkeys(want))[:W + 3]        # outer iteration (0, 1024) and in two (0, 16384); the lowest ids must win
        x[cols] = top
        return x
    if kind == "ninf3":
        x[::3] = -INF
        return spread_top(x, W, 0.125)
    if kind == "nans":
        x[1::7] = np.nan
        x[int(np.nanargmax(x))] = np.nan                # the would-be maximum
        return spread_top(x, W, 0.125)
    x[:] = -INF
    x[5] = np.nan
    if kind == "few_finite":                            # W - 1 finite entries: the last candidate is a -inf column, the lowest such id
        cols = rng.choice(V, size=W - 1, replace=False)
        x[cols] = (0.125 * rng.permutation(W - 1)).astype(f)
    return x


@dataclass
class Case:
    name: str
    V: int
    ld: int
    W: int
    kinds: List[str]
    x: np.ndarray                                       # [W, ld] fp32
    beam: List[Slot]
    eos: int
    lp_n: int
    step: int


def decided(ranked, tops, W, gap=1e-3):
    """tests/test_gpu_beam.py's _decided: every deciding comparison is an exact tie or at least `gap` wide."""
    s = [c[0] for c in ranked[:W + 1] if np.isfinite(c[0])]
    d = [a - b for a, b in zip(s, s[1:])] + [float(a - b) for t in tops for a, b in zip(t, t[1:]) if np.isfinite(a) and np.isfinite(b)]
    return all(v == 0.0 or v >= gap for v in d)


def build_case(name, V, ld, W, kinds, state, i, eos=None):
    """state: "live" (all slots live, lens 5 .. 9 turning with i), "start", "mixed" (a finished and, W >= 4, a dead slot), "equal"
    (slots 0 and 1: the same row, score and len).  lp_n = 8 on odd i and on mixed / equal: with lens 5 .. 9, Ln runs over
    lp_n - 3 .. lp_n + 2, so the Ln index and its clamp both decide scores.  eos: an id, "in" (slot r's rank r, r = i % W: inside the
    top W) or None ("in" on every third launch and on mixed, else an id >= V)."""
    rng = _rng(name)
    x = np.full((W, ld), PAD, np.float32)
    kinds = list(kinds[:W])
    for j, kind in enumerate(kinds):
        x[j, :V] = make_row(kind, V, W, rng)
    lens = [5 + (j + i) % 5 for j in range(W)]
    lp_n = 8 if i % 2 or state in ("mixed", "equal") else 64
    if state == "equal" and W >= 2:
        x[1], lens[1], kinds[1] = x[0], lens[0], kinds[0]
    if eos is None:
        eos = "in" if i % 3 == 0 or state == "mixed" else V + 3
    if eos == "in":
        r = i % W
        eos = int(beam_ref.topw_ref(x[r, :V], W)[0][r])
    for t in range(TRIES):
        jit = 0.01 * rng.integers(0, 50, size=W)
        if state == "start":
            beam = beam_ref.start(W)
        else:
            beam = [Slot(float(-1.5 - 0.8 * j + jit[j]), LIVE, [1 + (j + n) % 7 for n in range(lens[j])]) for j in range(W)]
            if state == "mixed" and W >= 2:
                beam[1] = Slot(-0.9, FINISHED, [5, 6])
            if state == "mixed" and W >= 4:
                beam[W - 1] = Slot(-INF, DEAD, [])
            if state == "equal" and W >= 2:
                beam[1] = Slot(beam[0].score, LIVE, beam[0].ids[::-1])
        if decided(*beam_ref.rank(x[:, :V], beam, eos, lp_n=lp_n), W):
            return Case(name, V, ld, W, kinds, x, beam, eos, lp_n, i % (CAP + 1))
    raise AssertionError(f"{name}: no decided draw of the slot scores in {TRIES}")


def _chunks(W):
    """The kinds W at a time, the last launch filled up from the start: every row of a launch is a different kind."""
    n = -(-len(KINDS) // W)
    return [[KINDS[(i * W + j) % len(KINDS)] for j in range(W)] for i in range(n)]


@functools.lru_cache(maxsize=None)
def single_cases(V, W):
    """The single-step launches of one (V, W).  Below the released vocabulary every kind at ld = V and at ld = V + 8, then the states;
    at the released one the kinds once, the launches alternating between the two."""
    out = []
    for pad in ((0, 8) if V != RELEASED else (None,)):
        for i, kinds in enumerate(_chunks(W)):
            ld = V + (8 * (i % 2) if pad is None else pad)
            out.append(build_case(f"V{V}-ld{ld}-W{W}-kinds{i}", V, ld, W, kinds, "live", i + (pad or 0)))
    for i, state in enumerate(["start", "mixed", "equal"][:3 if W >= 2 else 1]):
        out.append(build_case(f"V{V}-ld{V + 8}-W{W}-{state}", V, V + 8, W, STATE_KINDS, state, i + 1))
    return out


GROUPED = [(8, 8), (5, 3)]                               # 64 rows, the maximum; state stride 8 next to row stride 3


@functools.lru_cache(maxsize=None)
def group_cases(G, W):
    """One grouped launch at the released vocabulary: G cases under one EOS id (inside the top W of group 0's row 0), one lp_n, one
    ld; the kinds run on through the groups, the states change with the group."""
    V, ld = RELEASED, RELEASED + 8
    states = ["live", "mixed", "live", "equal", "start"]
    out, eos = [], "in"
    for g in range(G):
        kinds = [KINDS[(g * W + j) % len(KINDS)] for j in range(W)]
        out.append(build_case(f"V{V}-G{G}-W{W}-group{g}", V, ld, W, kinds, states[g % len(states)], 2 * g + 1, eos))
        eos = out[0].eos
    assert len({c.lp_n for c in out}) == 1
    return out


def all_cases():
    for V in SMALL:
        for W in WIDTHS:
            yield from single_cases(V, W)
    yield from single_cases(RELEASED, 8)
    for G, W in GROUPED:
        yield from group_cases(G, W)


def lp_table(lp_n, alpha=0.6):
    """The host's float64 1 / lp as fp32, as DeviceBeam builds it."""
    return np.array([1.0 / beam_ref.lp(n, alpha) for n in range(lp_n)], dtype=np.float64).astype(np.float32)


def state_of(case, log_cap=CAP):
    f = np.float32
    return dict(score=[f(b.score) for b in case.beam], fin=[b.fin for b in case.beam], len=[b.len for b in case.beam], step=case.step,
                done=-1, log_cap=log_cap)


_expect = {}


def expect(case):
    """What the launch owes, computed once: per live slot the ids, float64 logp and fp32 replay of its W candidates; E_ref and the bar
    of cand_logp (absolute, scale = max(1, max |logp|) over the finite candidates); the float64 rule's step; the fp32 replay of the
    whole step (select32 on the replayed candidates) and with it E_ref and the bar of the scores."""
    if case.name in _expect:
        return _expect[case.name]
    W, V = case.W, case.V
    ids = np.zeros((W, W), np.int64)
    logp = np.full((W, W), -INF)
    rep = np.full((W, W), -INF, np.float32)
    live = [j for j, b in enumerate(case.beam) if b.fin == LIVE]
    for j in live:
        ids[j], logp[j] = beam_ref.topw_ref(case.x[j, :V], W)
        rep[j] = beam_ref.logp32_replay(case.x[j, :V], ids[j])
    fin = np.isfinite(logp[live])
    assert (np.isfinite(rep[live]) == fin).all(), case.name
    scale = max(1.0, float(np.abs(logp[live][fin]).max())) if fin.any() else 1.0
    e_ref = float(np.abs(rep[live][fin] - logp[live][fin]).max()) if fin.any() else 0.0
    ranked, tops = beam_ref.rank(case.x[:, :V], case.beam, case.eos, lp_n=case.lp_n)
    want, parents, fed, _ = beam_ref.select(case.x[:, :V], case.beam, case.eos, lp_n=case.lp_n)
    cl, ci = np.zeros(64, np.float32), np.zeros(64, np.int64)
    for j in live:
        cl[j * 8:j * 8 + W], ci[j * 8:j * 8 + W] = rep[j], ids[j]
    host = beam_ref.select32(cl, ci, state_of(case), lp_table(case.lp_n), case.eos, W)
    s64 = np.array([b.score for b in want])
    s32 = np.array(host["score"], dtype=np.int32).view(np.float32).astype(np.float64)
    sf = np.isfinite(s64)
    s_scale = max(1.0, float(np.abs(s64[sf]).max())) if sf.any() else 1.0
    s_e_ref = float(np.abs(s32[sf] - s64[sf]).max()) if sf.any() else 0.0
    out = dict(live=live, ids=ids, logp=logp, replay=rep, scale=scale, e_ref=e_ref, bar=kr.bar(e_ref, scale), decided=decided(ranked, tops, W),
               ranked=ranked, tops=tops, want=want, parents=parents, fed=fed, host=host, cand=(cl, ci), s64=s64, s_scale=s_scale,
               s_e_ref=s_e_ref, s_bar=kr.bar(s_e_ref, s_scale))
    _expect[case.name] = out
    return out


# ---- host models of beam_topw_kernel's selection: the per-thread lists, then the best W of their union ---------------------------
def topw_model(row, W, entries=ENTRIES, displace_last=True, low_id_wins=True):
    """Thread t meets columns t, t + 1024, .. in ascending order and keeps the `entries` best it has met, sorted; the guard compares
    with the list's last entry, the insertion carries the displaced entry down and drops what falls off the end; the W best of all
    lists win.  With the defaults this is the kernel's algorithm and must equal topw_ref.  entries = 7: a shorter list;
    displace_last = False: the last entry, once filled, is never replaced (what is pushed out of the entry before it is lost);
    low_id_wins = False: equal values go to the higher id."""
    x = np.asarray(row, dtype=np.float32).copy()
    x[np.isnan(x)] = -INF
    V = x.size
    n = -(-V // THREADS)
    xp = np.full(n * THREADS, -INF, np.float32)
    xp[:V] = x

    def better(av, ai, bv, bi):
        if low_id_wins:
            return (av > bv) | ((av == bv) & (ai < bi))
        return (av > bv) | ((av == bv) & (ai != NONE) & ((ai > bi) | (bi == NONE)))       # an empty entry still loses to a column

    lv = np.full((THREADS, entries), -INF, np.float32)
    li = np.full((THREADS, entries), NONE, np.int64)
    for it in range(n):
        ci = it * THREADS + np.arange(THREADS, dtype=np.int64)
        cv = xp[it * THREADS:(it + 1) * THREADS].copy()
        go = (ci < V) & better(cv, ci, lv[:, -1], li[:, -1])
        full = li[:, -1] != NONE
        for k in range(entries):
            sw = go & better(cv, ci, lv[:, k], li[:, k])
            if k == entries - 1 and not displace_last:
                sw &= ~full
            tv, ti = lv[sw, k].copy(), li[sw, k].copy()
            lv[sw, k], li[sw, k] = cv[sw], ci[sw]
            cv[sw], ci[sw] = tv, ti
    keep = li.ravel() != NONE
    v, c = lv.ravel()[keep], li.ravel()[keep]
    order = np.lexsort((c if low_id_wins else -c, -v))[:W]
    return c[order]


WRONG_LISTS = {"c: a list of 7 entries": dict(entries=ENTRIES - 1),
               "d: the last entry is not displaced once the list is full": dict(displace_last=False),
               "e: ties broken to the higher id": dict(low_id_wins=False)}
WRONG_SUMS = {"a: a sum over the first outer iteration only": lambda V: OUTER,
              "b: a sum that drops the ragged last batch": lambda V: V - V % THREADS}


def _fma(sc, lp, inv):
    with np.errstate(all="ignore"):
        return np.float32(np.float64(sc) + np.float64(lp) * np.float64(inv))          # the product is exact in float64: one rounding


WRONG_SELECTS = {"f: lp_inv[L] instead of lp_inv[Ln]": dict(lp_index=lambda L, Ln, lp_n: min(L, lp_n - 1)),
                 "g: the score as one fused multiply-add": dict(score=_fma),
                 "h: lp_inv index clamped one early": dict(lp_index=lambda L, Ln, lp_n: min(Ln, lp_n - 2)),
                 "i: an unstable selection among equal scores": dict(pick=lambda cs, left: max(left, key=lambda i: (cs[i], i)))}
