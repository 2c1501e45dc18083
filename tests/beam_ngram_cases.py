"""The launches of tests/test_gpu_beam_ngram.py, built on the host alone (numpy; tests/test_beam_ngram_host.py walks the same list
without a GPU), in the style of tests/beam_parity_cases.py: every launch is decided by construction, from the reference alone.

A live slot's history is built for the ban it shall carry: the prefix p (n - 1 ids from 9000 on), B occurrences of (p, banned id)
spread over the text — the last one directly in front of the closing p, so a history of more than 1024 + n ids has a window in the
second trip of a 1024-thread strided scan —, position-numbered filler ids (2000 + position) in between, which never equal an id of
p.  L = n: the one window overlaps the prefix, so the text is one id n times and that id is banned; L < n: nothing is.

A row with B banned columns among its largest entries is respaced with beam_parity_cases.spread_top(x, W + B, step), the banned
columns then swapped into ranks 0, 2, 4 of those W + B + 1 entries: after masking, W + 1 spaced entries remain.  The slot scores are
drawn, at most TRIES times, until beam_parity_cases.decided holds for beam_ref.rank on the MASKED rows.

Banned columns (BANS): column 0 and column V - 1; two and three in one thread's residue (c % 1024 equal); one id banned twice; one
outside the top W + 1 (it only leaves S); the first banned id of every kind is the row maximum."""
import functools
from dataclasses import dataclass
from typing import List

import numpy as np

import beam_ngram_ref
import beam_parity_cases as bc
import beam_ref
from beam_ref import DEAD, FINISHED, INF, LIVE, Slot

PAD = bc.PAD
TRIES = bc.TRIES
SMALL = [9217, 16385]
RELEASED = bc.RELEASED
WIDTHS = [1, 5, 8]
SIZES = [2, 3, 4]
CAP = 48                                             # ids one history holds, where a case does not say otherwise
LOG_CAP = bc.CAP
P0, FILL0 = 9000, 2000                               # prefix ids 9000 .. 9014, filler ids 2000 + position: all below the smallest V
# kind: (banned ids in the order of their occurrences, V - 1 written as -1; how many of the distinct ones sit among the row's largest)
BANS = {"edges": ([0, -1, 1029], 3), "residue": ([5, 5 + 1024, 5 + 2048], 3), "twice": ([77, 77, 300], 2), "outside": ([400, 500, 600], 2)}
ROTATIONS = [0, 1, 2, 4]                             # of the length pattern below: slot 0 gets 40, n, n - 1, n - 2


def lengths(n, W, r):
    pattern = [40, n, n - 1, 40, n - 2, 40, n, 40]
    return [pattern[(j + r) % 8] for j in range(W)]


def history(L, n, ids):
    """A text of L ids whose ban set under n is as much of `ids` as fits (see the module docstring).  Returns (text, banned set)."""
    if L < n:
        return [FILL0 + i for i in range(L)], set()
    if L == n:
        return [ids[0]] * n, {ids[0]}
    p = [P0 + k for k in range(n - 1)]
    last = L - (n - 1) - n                            # where the last (p, id) starts
    B = max(1, min(len(ids), 1 + last // n if last >= 0 else 0))
    assert last >= 0, (L, n)
    h = [FILL0 + i for i in range(L)]
    for k in range(B):
        at = last if B == 1 or k == B - 1 else (k * last) // (B - 1)
        h[at:at + n] = p + [ids[k]]
    h[L - (n - 1):] = p
    want = set(ids[:B])
    assert beam_ngram_ref.banned(h, n) == want, (L, n, ids)
    return h, want


@dataclass
class Case:
    name: str
    V: int
    ld: int
    W: int
    n: int
    cap: int
    kind: str
    x: np.ndarray                                     # [W, ld] fp32
    beam: List[Slot]
    eos: int
    lp_n: int
    step: int
    matters: bool                                     # the step without the ban takes a banned column


def masked(case):
    """The rows the existing step has to be given to owe what the banned step owes: fp32, -inf in the banned columns."""
    x = case.x.copy()
    live = beam_ngram_ref.mask(case.x[:, :case.V], case.beam, case.n, case.cap)
    x[:, :case.V][np.isneginf(live) & ~np.isneginf(case.x[:, :case.V].astype(np.float64))] = -INF
    return x


def make_row(V, W, ban, top_count, rng):
    """ban: the slot's banned ids in kind order; the first top_count distinct ones go to ranks 0, 2, 4 of the W + B + 1 largest."""
    f = np.float32
    x = (rng.standard_normal(V) * 4.0).astype(f)
    distinct = list(dict.fromkeys(ban))
    x[distinct] = f(-9.0)                             # not among the largest by accident
    tops = distinct[:top_count]
    bc.spread_top(x, W + len(tops), 0.125)
    order = beam_ref.topw_ref(x, W + len(tops) + 1)[0]
    for k, b in enumerate(tops):
        r = int(order[min(2 * k, W + len(tops))])
        x[b], x[r] = x[r], x[b]
    return x


def build_case(name, V, ld, W, n, kind, state, i, L=None, cap=CAP, eos=None):
    """state: "live" (every slot live, lengths(n, W, ROTATIONS[i % 4]) or L for all), "start", "mixed" (slot 1 finished with a text
    that would ban, slot W - 1 dead where W >= 4).  eos: an id, or None: on even i the second (on odd draws the third) best column of the
    first live row after masking — an EOS candidate is scored under another length than its neighbours, which no draw of the slot
    scores moves —, else an id >= V."""
    rng = bc._rng("ngram", name)
    ids, top_count = BANS[kind]
    ids = [V - 1 if k < 0 else k for k in ids]
    Ls = [L] * W if L is not None else lengths(n, W, ROTATIONS[i % 4])
    texts, bans = zip(*[history(Ls[j], n, ids[j % len(ids):] + ids[:j % len(ids)] if Ls[j] == n else ids) for j in range(W)])
    x = np.full((W, ld), PAD, np.float32)
    fin = [LIVE] * W
    if state == "start":
        fin, texts, bans = [LIVE] + [DEAD] * (W - 1), [[]] * W, [set()] * W
    if state == "mixed" and W >= 2:
        fin[1] = FINISHED
    if state == "mixed" and W >= 4:
        fin[W - 1], texts, bans = DEAD, list(texts[:-1]) + [[]], list(bans[:-1]) + [set()]
    for j in range(W):
        # (a text longer than cap is not filtered: its row is built as if it were, so a kernel that filters it shows)
        b = [k for k in ids if k in bans[j]] if fin[j] == LIVE else []
        x[j, :V] = make_row(V, W, b, min(top_count, len(set(b))), rng)
    lp_n = 8 if i % 2 else 64
    for t in range(TRIES):
        jit = 0.01 * rng.integers(0, 50, size=W)
        beam = [Slot(float(-1.5 - 0.8 * j + jit[j]) if fin[j] != DEAD else -INF, fin[j], list(texts[j])) for j in range(W)]
        if state == "start":
            beam = beam_ref.start(W)
        if state == "mixed" and W >= 2:
            beam[1].score = -0.9
        e = eos
        if e is None:
            first = next(j for j in range(W) if beam[j].fin == LIVE)
            e = int(beam_ref.topw_ref(beam_ngram_ref.mask(x[:, :V], beam, n, cap)[first], 3)[0][1 + t % 2]) if i % 2 == 0 else V + 3
        if bc.decided(*beam_ngram_ref.rank(x[:, :V], beam, e, n, lp_n=lp_n, cap=cap), W):
            # from the rule WITHOUT the ban: its new beam takes a column the ban forbids its parent, so the banned step cannot
            plain, parents, _, _ = beam_ref.select(x[:, :V], beam, e, lp_n=lp_n)
            matters = any(s.fin == LIVE and beam[p].len <= cap and s.ids[-1] in bans[p] for s, p in zip(plain, parents))
            return Case(name, V, ld, W, n, cap, kind, x, beam, e, lp_n, i % (LOG_CAP + 1), matters)
    raise AssertionError(f"{name}: no decided draw of the slot scores in {TRIES}")


@functools.lru_cache(maxsize=None)
def single_cases(V, W):
    """The single-group launches of one (V, W): n = 2, 3, 4 under every kind of banned column and every rotation of the lengths, then
    the slot states."""
    out = []
    for n in SIZES:
        for i, kind in enumerate(BANS):
            out.append(build_case(f"V{V}-W{W}-n{n}-{kind}", V, V + 8 * (i % 2), W, n, kind, "live", i))
    for i, state in enumerate(["start", "mixed"][:2 if W >= 2 else 1]):
        out.append(build_case(f"V{V}-W{W}-n3-{state}", V, V + 8, W, 3, "edges", state, 2 * i))
    return out


@functools.lru_cache(maxsize=None)
def special_cases():
    """n = 16 (a prefix of 15 ids) under every rotation; the released vocabulary once; a history of 1030 ids under cap = 1100: windows
    in the second trip of the strided scan; L = cap + 1: not filtered."""
    out = [build_case(f"V9217-W5-n16-{kind}", 9217, 9217 + 8, 5, 16, kind, "live", i) for i, kind in enumerate(BANS)]
    out.append(build_case(f"V{RELEASED}-W8-n3-edges", RELEASED, RELEASED + 8, 8, 3, "edges", "live", 0))
    out.append(build_case("V9217-W5-n3-L1030", 9217, 9217, 5, 3, "residue", "live", 2, L=1030, cap=1100))
    out.append(build_case("V9217-W1-n2-over-cap", 9217, 9217, 1, 2, "edges", "live", 0, L=40, cap=39))
    return out


@functools.lru_cache(maxsize=None)
def group_cases(V, W):
    """One launch of G = 3 groups: n = 3, one EOS id (outside the vocabulary), one lp_n; a kind, a rotation and a state per group."""
    plan = [("edges", "live", 1), ("twice", "mixed" if W >= 2 else "live", 3), ("residue", "live", 5)]
    out = [build_case(f"V{V}-G3-W{W}-group{g}", V, V + 8, W, 3, kind, state, i, eos=V + 3) for g, (kind, state, i) in enumerate(plan)]
    assert len({c.lp_n for c in out}) == 1
    return out


def all_cases():
    for V in SMALL:
        for W in WIDTHS:
            yield from single_cases(V, W)
            yield from group_cases(V, W)
    yield from special_cases()


def after(case):
    """What the float64 rule leaves: (new beam, parents, fed-back ids) of the step under the ban."""
    new, parents, fed, _ = beam_ngram_ref.select(case.x[:, :case.V], case.beam, case.eos, case.n, lp_n=case.lp_n, cap=case.cap)
    return new, parents, fed


# ---- a sequence of steps whose parents include a swap and a fan-out -------------------------------------------------------------
SEQ_V, SEQ_W, SEQ_N, SEQ_STEPS, SEQ_CAP = 9217, 5, 2, 6, 8
SEQ_ALPHABET = [0, SEQ_V - 1, 5, 1029, 77, 300]       # the texts run over six ids, so bigrams repeat within six steps
SEQ_SEED = 3                                         # the first seed under which the reference run has the properties tests/test_beam_ngram_host.py asserts


def sequence_rows(seed=SEQ_SEED):
    """Six launches' rows [6][W, V]: the alphabet's columns are the six largest of every row, W + 7 entries respaced."""
    rng = bc._rng("ngram-sequence", seed)
    rows = np.zeros((SEQ_STEPS, SEQ_W, SEQ_V), np.float32)
    for t in range(SEQ_STEPS):
        for j in range(SEQ_W):
            x = (rng.standard_normal(SEQ_V) * 4.0).astype(np.float32)
            x[SEQ_ALPHABET] = np.float32(-9.0)
            bc.spread_top(x, SEQ_W + len(SEQ_ALPHABET), 0.125)
            order = beam_ref.topw_ref(x, len(SEQ_ALPHABET))[0]
            for r, a in zip(order, rng.permutation(SEQ_ALPHABET)):
                x[a], x[r] = x[r], x[a]
            rows[t, j] = x
    return rows


@functools.lru_cache(maxsize=None)
def sequence(seed=SEQ_SEED):
    """The reference's run over sequence_rows: per step dict(beam before, new beam, parents, fed, decided, bans: the live slots' ban
    sets), and the unbanned run's final texts.  EOS is outside the vocabulary."""
    rows = sequence_rows(seed)
    eos = SEQ_V + 3
    beam, plain, out = beam_ref.start(SEQ_W), beam_ref.start(SEQ_W), []
    for t in range(SEQ_STEPS):
        ok = bc.decided(*beam_ngram_ref.rank(rows[t], beam, eos, SEQ_N), SEQ_W)
        bans = [beam_ngram_ref.banned(b.ids, SEQ_N) if b.fin == LIVE else set() for b in beam]
        new, parents, fed, _ = beam_ngram_ref.select(rows[t], beam, eos, SEQ_N)
        out.append(dict(before=beam, beam=new, parents=parents, fed=fed, decided=ok, bans=bans))
        beam = new
        plain = beam_ref.select(rows[t], plain, eos)[0]
    return out, [b.ids for b in plain]


def has_swap(parents):
    return any(parents[a] == b and parents[b] == a for a in range(len(parents)) for b in range(a + 1, len(parents)))


def has_fan_out(parents):
    return any(parents.count(p) >= 3 for p in set(parents))
