"""tests/beam_ref.py's host restatements of the beam step (topw_ref, logp32_replay, select32) on the host: pinned to the float64 rule
they stand beside, the bars of tests/test_gpu_beam_parity.py measured on that module's own launches (tests/beam_parity_cases.py), and
nine wrong models — the kernels' contract with one defect each — that those launches must reject.  No GPU."""
import numpy as np
import pytest

import beam_parity_cases as bc
import beam_ref
from beam_ref import LIVE
from test_gpu_beam import _decided, _scenarios

EXISTING = [(V, ld, W) for V, ld in [(512, 512), (1000, 1008), (4100, 4100)] for W in [1, 3, 5, 8]]


@pytest.mark.parametrize("V,ld,W", EXISTING)
def test_topw_ref_is_the_order_of_rank_on_the_existing_scenarios(V, ld, W):
    for name, x, beam, eos in _scenarios(V, ld, W, 1000 + V + W):
        ranked, _ = beam_ref.rank(x[:, :V], beam, eos)
        for j, b in enumerate(beam):
            if b.fin != LIVE:
                continue
            ids, logp = beam_ref.topw_ref(x[j, :V], W)
            x64, logp64 = beam_ref.log_softmax64(x[j, :V])
            assert ids.tolist() == np.lexsort((np.arange(V), -x64))[:W].tolist(), (name, j)      # rank()'s own statement
            assert (logp == logp64[ids]).all(), (name, j)
            # ... and what rank() made of it: slot j's candidates (the EOS one is scored at another length, so not in rank order)
            assert sorted(eos if c[2] < 0 else c[2] for c in ranked if c[1] == j) == sorted(ids.tolist()), (name, j)


@pytest.mark.parametrize("V,ld,W", EXISTING)
def test_select32_decides_as_select_on_exact_inputs(V, ld, W):
    """The existing scenarios' logits are multiples of 1/8 (exact in fp32 and float64) and decided: from float64 logp rounded once to
    fp32, select32 must take the float64 rule's decisions, and its scores lie within fp32 rounding of the rule's."""
    for name, x, beam, eos in _scenarios(V, ld, W, 1000 + V + W):
        assert _decided(*beam_ref.rank(x[:, :V], beam, eos), W), name
        want, parents, fed, _ = beam_ref.select(x[:, :V], beam, eos)
        cl, ci = np.zeros(64, np.float32), np.zeros(64, np.int64)
        for j, b in enumerate(beam):
            if b.fin == LIVE:
                ci[j * 8:j * 8 + W], logp = beam_ref.topw_ref(x[j, :V], W)
                cl[j * 8:j * 8 + W] = logp.astype(np.float32)
        state = dict(score=[b.score for b in beam], fin=[b.fin for b in beam], len=[b.len for b in beam], step=3, done=-1, log_cap=4)
        got = beam_ref.select32(cl, ci, state, bc.lp_table(64), eos, W)
        assert got["fin"] == [b.fin for b in want] and got["len"] == [b.len for b in want], name
        assert got["parent"] == parents and got["token"] == fed, name
        assert [r[1] for r in got["log"]] == [b.ids[-1] if b.fin == LIVE else -1 for b in want], name
        assert [r[2] for r in got["log"]] == got["score"] and [r[0] for r in got["log"]] == parents and [r[3] for r in got["log"]] == got["fin"]
        assert got["step"] == 4 and got["done"] == (3 if all(b.fin == beam_ref.FINISHED for b in want) else -1)
        s32 = np.array(got["score"], dtype=np.int32).view(np.float32).astype(np.float64)
        for a, b in zip(s32, want):
            # four fp32 roundings: logp, the table entry, the product, the sum — each relative to the larger of |logp| and |score|
            big = max(1.0, abs(b.score), float(np.abs(cl[np.isfinite(cl)]).max()))
            assert a == b.score if not np.isfinite(b.score) else abs(a - b.score) <= 4 * 2.0 ** -24 * big, name
    state["step"] = 4                                                     # past the log's capacity: no record
    assert beam_ref.select32(cl, ci, state, bc.lp_table(64), eos, W)["log"] is None


def _list_cases():
    """The launches the list models are run on: every kind of every shape once (the second ld repeats the kinds)."""
    return [c for c in bc.all_cases() if (c.ld == c.V or c.V == bc.RELEASED) and "-G" not in c.name and c.W > 1]


def test_topw_model_with_no_defect_is_topw_ref():
    n = 0
    for c in _list_cases():
        e = bc.expect(c)
        for j in e["live"]:
            assert bc.topw_model(c.x[j, :c.V], c.W).tolist() == e["ids"][j].tolist(), (c.name, j, c.kinds[j])
            n += 1
    assert n >= 4 * 2 * len(bc.KINDS)


def test_every_launch_is_decided_and_its_bars_are_measured():
    """No launch of the GPU module is excused from the exact assertions, and the fp32 replay of the stated order stays where fp32
    rounding puts it: 136 rounded adds at most (126 columns per partial, a tree of 10) bound E_ref by 136 * 2^-24 ~ 8e-6 relative at
    the worst and ~sqrt(136) * 2^-24 ~ 7e-7 typically; the figures are printed."""
    groups = {}
    for c in bc.all_cases():
        e = bc.expect(c)
        assert e["decided"] and _decided(e["ranked"], e["tops"], c.W), c.name
        assert e["e_ref"] <= 1e-6 * e["scale"] and e["s_e_ref"] <= 1e-6 * e["s_scale"], (c.name, e["e_ref"], e["s_e_ref"])
        assert e["bar"] <= 4e-6 * e["scale"] and e["s_bar"] <= 4e-6 * e["s_scale"]
        g = groups.setdefault(c.V, [0, 0.0, 0.0, 0.0, 0.0])
        g[0] += 1
        g[1], g[2] = max(g[1], e["e_ref"] / e["scale"]), max(g[2], e["bar"] / e["scale"])
        g[3], g[4] = max(g[3], e["s_e_ref"] / e["s_scale"]), max(g[4], e["s_bar"] / e["s_scale"])
    for V, (n, er, br, es, bs) in groups.items():
        print(f"  BARS beam V={V}: {n} launches, logp E_ref <= {er:.3e} bar <= {br:.3e}, score E_ref <= {es:.3e} bar <= {bs:.3e} "
              f"(relative to the launch's scale)")
    assert set(groups) == set(bc.SMALL) | {bc.RELEASED}


@pytest.mark.parametrize("name", sorted(bc.WRONG_SUMS))
def test_wrong_sums_leave_the_bar(name):
    hit, worst, n = 0, (0.0, None), 0
    for c in bc.all_cases():
        e = bc.expect(c)
        bad = False
        for j in e["live"]:
            fin = np.isfinite(e["logp"][j])
            if not fin.any():
                continue
            with np.errstate(all="ignore"):                              # a sum of no column at all: log 0
                got = beam_ref.logp32_replay(c.x[j, :c.V], e["ids"][j], summed=bc.WRONG_SUMS[name](c.V)).astype(np.float64)
                r = float(np.abs(got[fin] - e["logp"][j][fin]).max()) / e["bar"]
            worst = max(worst, (r, c.name))
            bad = bad or not r <= 1.0
        hit, n = hit + bad, n + 1
    print(f"  WRONG {name}: outside the bar on {hit} of {n} launches, worst err/bar {worst[0]:.3g} ({worst[1]})")
    assert hit >= 1 and worst[0] > 100.0                                  # not by a rounding: the sum is missing columns


@pytest.mark.parametrize("name", sorted(bc.WRONG_LISTS))
def test_wrong_lists_move_an_asserted_id(name):
    hit, rows, where = 0, 0, None
    for c in _list_cases():
        e = bc.expect(c)
        for j in e["live"]:
            rows += 1
            if bc.topw_model(c.x[j, :c.V], c.W, **bc.WRONG_LISTS[name]).tolist() != e["ids"][j].tolist():
                hit, where = hit + 1, where or f"{c.name} row {j} {c.kinds[j]}"
    print(f"  WRONG {name}: moves cand_id on {hit} of {rows} rows, first {where}")
    assert hit >= 1


@pytest.mark.parametrize("name", sorted(bc.WRONG_SELECTS))
def test_wrong_selects_change_the_bits_of_the_state(name):
    hit, n, where = 0, 0, None
    for c in bc.all_cases():
        e = bc.expect(c)
        got = beam_ref.select32(*e["cand"], bc.state_of(c), bc.lp_table(c.lp_n), c.eos, c.W, **bc.WRONG_SELECTS[name])
        n += 1
        if got != e["host"]:
            hit, where = hit + 1, where or c.name
    print(f"  WRONG {name}: another state than select32 on {hit} of {n} launches, first {where}")
    assert hit >= 1
