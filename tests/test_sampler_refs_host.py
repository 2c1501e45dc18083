"""tests/sampler_refs.py on the host: the Philox transcription against the Random123 known answers, the uniform mapping at its
rounding edges, the committed u-edge counters, the input conditions of every launch of tests/test_gpu_sampler_replay.py (no row
outside the exact assertion, E_ref <= 1e-4, nucleus margins), and a set of wrong models — the contract with one defect each —
that must move the ids those launches assert.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import sampler_refs as sr
from sampler_refs import Model

KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("ctr,key,want", KAT, ids=["zeros", "ones", "pi"])
def test_philox_known_answers(ctr, key, want):
    assert " ".join(f"{int(x):08x}" for x in sr.philox4x32_10(*ctr, *key)) == want
    many = sr.philox4x32_10(*(np.full(5, c, dtype=np.uint64) for c in ctr), *key)        # the vectorised form is the scalar one
    assert all(" ".join(f"{int(w[i]):08x}" for w in many) == want for i in range(5))
    assert " ".join(f"{int(x):08x}" for x in sr.philox4x32_10(*ctr, *key, rounds=9)) != want


def test_uniform_mapping_at_its_rounding_edges():
    """u = min(RN(x + 0.5) * 2^-24, 1 - 2^-24): exact below 2^23, round-to-even of the 25-bit sum from there on, and the one value
    that would be 1.0 brought back to the largest fp32 below it.  Every value is strictly inside (0, 1)."""
    want = {0: Fraction(1, 2 ** 25),                        # 0.5 * 2^-24
            1: Fraction(3, 2 ** 25),
            2 ** 23 - 1: Fraction(2 ** 24 - 1, 2 ** 25),      # 24 significant bits: still exact
            2 ** 23: Fraction(2 ** 23, 2 ** 24),              # 2^23 + 0.5 is a tie: to even, 2^23
            2 ** 23 + 1: Fraction(2 ** 23 + 2, 2 ** 24),      # 2^23 + 1.5 -> 2^23 + 2
            2 ** 24 - 2: Fraction(2 ** 24 - 2, 2 ** 24),      # 2^24 - 1.5 -> 2^24 - 2
            2 ** 24 - 1: Fraction(2 ** 24 - 1, 2 ** 24)}      # 2^24 - 0.5 -> 2^24, i.e. 1.0: the min gives 1 - 2^-24
    got = sr.uniform(np.array(list(want), dtype=np.uint64))
    assert got.dtype == np.float32
    for x, u in zip(want, got):
        assert Fraction(float(u)) == want[x], (x, float(u))
    every = sr.uniform(np.arange(1 << 24, dtype=np.uint64))
    assert float(every.min()) == 2.0 ** -25 and float(every.max()) == 1.0 - 2.0 ** -24 and bool((np.diff(every) >= 0).all())
    q = -np.log(every.astype(np.float64))
    assert bool((q > 0).all()) and bool(np.isfinite(q).all())                          # Exp(1) draws: positive and finite
    # without the min the last value is exactly 1.0, -log is -0.0 and the column's score -inf: the defect this contract closes
    assert float((np.float32(2 ** 24 - 1) + np.float32(0.5)) * np.float32(2.0 ** -24)) == 1.0


@pytest.mark.parametrize("edge", [sr.U_EDGE, sr.U_EDGE_WIDE], ids=["v1000", "wide"])
def test_committed_u_edge_counters_hit_the_last_value(edge):
    lo, hi = sr.key_words(edge["seed"])
    r0 = sr.philox4x32_10(edge["column"], edge["draw"], edge["row_part"], edge["stream_id"], lo, hi)[0]
    assert int(r0) >> 8 == 0xFFFFFF
    # the search that found it, one draw wide
    assert sr.find_u_edge(edge["seed"], edge["row_part"], edge["stream_id"], edge["column"] + 1, draws=[edge["draw"]]) == (edge["draw"], edge["column"])


def test_u_edge_launch_puts_the_hit_column_on_top_of_a_kept_set_of_eight():
    L, R = sr.case("u-edge")
    c = sr.U_EDGE["column"]
    key, draw, part = sr.row_stream(L, 0)
    wid, kept, s1, s2, near = sr.race_f64(L.logits[0], L.T, 0, L.topk, 0.0, key, draw, part, L.stream_id, bar=R.bar)
    assert (key, draw, part, L.stream_id) == ((888, 0), sr.U_EDGE["draw"], 0, 1)
    assert int(L.logits[0].argmax()) == c and c in kept and len(kept) == 8
    assert wid == c and near.tolist() == [c] and s2 / s1 < 1e-3


@pytest.mark.parametrize("name", list(sr.CASES))
def test_every_gpu_launch_is_asserted_exactly(name):
    """The input condition of the GPU module: the reference alone leaves no row out of the exact assertion (cap 1 %), the fp32
    evaluation of the formula is within 1e-4 of the float64 one, and nucleus decisions sit above the margin."""
    L, R = sr.case(name)
    print(R.line(name), f"nucleus margin {R.min_margin:.3e}")
    left_out = int((~R.exact).sum())
    assert left_out <= sr.CAP * L.M and left_out == 0, (name, left_out)
    assert R.e_ref <= 1e-4 and R.min_gap > 2 * R.bar
    assert R.min_margin > sr.MARGIN
    assert all(n.tolist() == [i] for n, i in zip(R.near, R.ids))
    lo = np.zeros(L.M, dtype=np.int64) if L.forbid is None else L.forbid
    assert bool((R.ids >= lo).all()) and bool((R.ids < L.V).all())
    assert L.logits.dtype == np.float32 and not np.isnan(L.logits).any()


def test_cases_cover_what_they_are_named_for():
    L = sr.case("v37-k2-T1.0-fbrow")[0]
    assert (L.forbid + L.topk == L.V).any() and (L.forbid == 0).any() and len(set(L.forbid.tolist())) > 10
    L = sr.case("v37-k8-T0.7-fb3-ninf")[0]
    kept_inf = [np.isinf(L.logits[m][sr.kept_mask(L.logits[m], L.T, 3, L.topk, 0.0)]).sum() for m in range(L.M)]
    assert min(kept_inf) >= 1                                                          # -inf columns inside the kept set
    L = sr.case("v1000-k2-T0.7")[0]
    top2 = np.sort(L.logits[1])[-2:]
    assert top2[0] == top2[1]                                                          # a row of two exactly equal (top) logits
    L = sr.case("ctr-shift1")[0]
    ids = sr.case("ctr-shift1")[1].ids
    assert np.array_equal(L.logits[0], L.logits[1]) and bool((ids[0::4] == ids[1::4]).all()) and bool((ids[2::4] != ids[3::4]).any())
    L = sr.case("rows-topk")[0]
    assert len(set(zip(L.keys, L.draws))) == L.M and {0x7FFFFFFF, -1, -(1 << 31)} <= set(L.draws) and max(L.keys) == 2 ** 64 - 1
    # every counter-word case draws other ids than the base launch it differs from in one word
    base = sr.case("ctr-stream2")[1].ids
    for name in sr.CASES:
        if name.startswith("ctr-") and name not in ("ctr-stream2", "ctr-shift1"):
            assert (sr.case(name)[1].ids != base).mean() > 0.2, name
    # the carry case: the low halves of seed and device word overflow
    L = sr.case("ctr-carry")[0]
    assert (L.seed & sr.U32) + (L.counter[1] & sr.U32) > sr.U32 and sr.key_words(L.seed, L.counter[1], L.counter[2]) == (0, 1)


def test_tie_rows_tie_by_construction():
    """rows-tie: per row two columns with the same 24 random bits and the same logit — equal (l, u), so equal scores in any arithmetic —
    that beat every other column; the lowest wins."""
    L, R = sr.case("rows-tie")
    for m, (d, a, b) in enumerate(L.note):
        key, draw, part = sr.row_stream(L, m)
        r0 = sr.philox4x32_10(np.array([a, b]), draw, part, L.stream_id, *key)[0] >> np.uint64(8)
        assert a < b and draw == d and int(r0[0]) == int(r0[1]) and L.logits[m, a] == L.logits[m, b] == L.logits[m].max()
        cols, s = sr.race_f32(L.logits[m], L.T, 0, L.topk, 0.0, key, draw, part, L.stream_id)
        assert s[cols == a][0] == s[cols == b][0] == s.max()
        assert R.ids[m] == a and R.exact[m] and R.near[m].tolist() == [a]


# (model, the cases it is run on, the rows it concerns or None = all)
WRONG = {
    "nine rounds": (Model(rounds=9), ["ctr-stream2"], None),
    "multipliers swapped": (Model(swap_mul=True), ["ctr-stream2"], None),
    "u from r[1]": (Model(u_word=1), ["ctr-stream2"], None),
    "stream id dropped": (Model(drop_stream=True), ["ctr-stream1", "ctr-stream5", "ctr-stream8", "rows-topk"], None),
    "draw index dropped": (Model(drop_draw=True), ["ctr-stream2", "ctr-draw-m1"], None),
    "row part shifted the wrong way": (Model(flip_shift=True), ["ctr-shift1", "ctr-stream2"], lambda L: np.arange(L.M) >= 2),
    "seed carry dropped": (Model(carry=False), ["ctr-carry"], None),
    "draw index sign-extended": (Model(draw_sign_extends=True), ["ctr-draw-m1", "ctr-draw-min"], None),
    "equal scores to the higher column": (Model(tie_high=True), ["rows-tie"], None),
    "logit * T": (Model(times_t=True), ["ctr-stream2", "v1000-k50-T0.7-fb3"], None),
    # (rank topk - 1: at topk 2 the second column never wins.  The other direction, rank topk + 1, lets one column in, which wins in
    # proportion to its mass: 17 % / 19 % of these rows — under the 20 % asked here, though one moved row fails the GPU module.)
    "threshold one rank off": (Model(rank_off=-1), ["v1000-k2-T1.3", "v1000-k2-T0.7"], None),
    "forbid prefix ignored": (Model(ignore_forbid=True), ["v1000-k8-T1.3-fbrow"], lambda L: L.forbid > 0),
}


@pytest.mark.parametrize("name", list(WRONG))
def test_wrong_models_move_the_asserted_ids(name):
    """Each defect changes at least 20 % of the ids (of the rows it concerns) of a launch at V = 1000 whose every row the GPU module
    asserts exactly: the module would reject a kernel that had it."""
    model, cases, concerns = WRONG[name]
    for c in cases:
        L, R = sr.case(c)
        assert L.V == 1000 and bool(R.exact.all())
        rows = np.ones(L.M, dtype=bool) if concerns is None else concerns(L)
        moved = (sr.ids_of(L, model) != R.ids)[rows].mean()
        print(f"{name} on {c}: {moved:.3f} of {int(rows.sum())} rows change id")
        assert rows.sum() >= 14 and moved >= 0.2, (name, c, moved)
    assert np.array_equal(sr.ids_of(sr.case(cases[0])[0]), sr.case(cases[0])[1].ids)  # the same loop with no defect reproduces them
