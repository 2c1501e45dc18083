"""ua2_beam_step / ua2_beam_step_groups (csrc/ua2_beam.hip: beam_topw_kernel, beam_select_kernel) against float64 at the shapes the
released text head takes them to.  The launches are tests/beam_parity_cases.py's (V = 9217, 16384, 16385, 33000: the smallest at
which a thread's 8-entry list overflows, an outer iteration of 16 384 columns is full, a second and a third one exist; V = 128 256:
the released vocabulary), what each owes is tests/beam_ref.py's: after every launch

* cand_id equals topw_ref exactly (a total order: no tolerance);
* cand_logp lies within kernel_refs.bar(E_ref, scale) of float64, E_ref = logp32_replay (the stated order in numpy fp32) against
  float64 on the launch's own rows, scale = max(1, max |logp|); -inf where float64 is -inf;
* the state after beam_select_kernel equals select32 on the DEVICE's candidates bit for bit: scores, fin, len, parent, the token
  column, the log record, ctrl;
* ids, parents, fin and len equal the float64 rule (every launch is decided, asserted first), scores within the bar of the replayed step;
* everything the step does not own keeps its bits: the candidates of finished and dead slots and beyond rank W, the state beyond
  slot W, the other token columns and log steps, the logits.

tests/test_beam_refs_host.py shows on the same launches that these assertions reject nine wrong models of the two kernels.  On the
kernels as they were before this module, 15 of its 16 tests failed: a row with fewer than W finite entries named -inf columns 1024 too
high (cand_id [1024] for [0]), and every score was a fused multiply-add, one ulp off select32 on most launches; both are fixed in
csrc/ua2_beam.hip, the figures before and after are in profiles/kernel_parity_errors.txt."""
import ctypes as C

import numpy as np
import pytest
import torch

import beam_parity_cases as bc
import beam_ref
from beam_ref import FINISHED, LIVE
from test_gpu_beam import DeviceBeam, _decided
from test_gpu_beam_groups import DeviceBeams

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT_LOGP, SENT_ID = 12345.0, -77                                         # what no launch writes


def _bits(t):
    return t.view(torch.int32).cpu().numpy().copy()


def _check(case, cand_logp, cand_id, f, tag=""):
    """cand_logp [64] fp32, cand_id [64] int32: the slot-major candidates of the case's group after the launch; f: the group's state as
    integers — score (fp32 bits), fin, len, parent: 8 each; ctrl: 4; log: [steps][W][4]; token: [W][9].  Prints the PARITY line."""
    e = bc.expect(case)
    W, name = case.W, case.name + tag
    assert e["decided"] and _decided(e["ranked"], e["tops"], W), name      # on the host, from the reference alone
    # 1. the candidates
    err = 0.0
    for j in range(W):
        got_l, got_i = cand_logp[j * 8:j * 8 + 8], cand_id[j * 8:j * 8 + 8]
        n = W if j in e["live"] else 0
        assert (got_l[n:].view(np.int32) == np.float32(SENT_LOGP).view(np.int32)).all() and (got_i[n:] == SENT_ID).all(), (name, j)
        if n:
            assert got_i[:W].tolist() == e["ids"][j].tolist(), (name, j, case.kinds[j])
            fin = np.isfinite(e["logp"][j])
            assert (got_l[:W][~fin] == -np.inf).all() and np.isfinite(got_l[:W][fin]).all(), (name, j, case.kinds[j])
            if fin.any():
                err = max(err, float(np.abs(got_l[:W][fin].astype(np.float64) - e["logp"][j][fin]).max()))
    # 2. beam_select_kernel, bit for bit, from the device's own candidates
    want = beam_ref.select32(cand_logp, cand_id, bc.state_of(case), bc.lp_table(case.lp_n), case.eos, W)
    assert f["score"][:W] == want["score"] and f["fin"][:W] == want["fin"] and f["len"][:W] == want["len"], name
    assert f["parent"][:W] == want["parent"] and [r[0] for r in f["token"]] == want["token"], name
    assert f["ctrl"] == [want["step"], want["done"], 0, 0], name
    assert len(f["log"]) == bc.CAP
    for t, rec in enumerate(f["log"]):
        assert rec == (want["log"] if t == case.step else [[-7] * 4] * W), (name, t)
    # 3. what the step does not own
    assert f["score"][W:] == [int(np.float32(-np.inf).view(np.int32))] * (8 - W) and f["fin"][W:] == [2] * (8 - W), name
    assert f["len"][W:] == [0] * (8 - W) and f["parent"][W:] == [-9] * (8 - W), name
    assert all(r[1:] == [-5] * 8 for r in f["token"]), name
    # 4. the float64 rule
    ref = e["want"]
    assert f["fin"][:W] == [b.fin for b in ref] and f["len"][:W] == [b.len for b in ref], name
    assert f["parent"][:W] == e["parents"] and [r[0] for r in f["token"]] == e["fed"], name
    if want["log"] is not None:
        assert [r[1] for r in want["log"]] == [b.ids[-1] if b.fin == LIVE else -1 for b in ref], name
    assert want["done"] == (case.step if all(b.fin == FINISHED for b in ref) else -1), name
    got_s = np.array(f["score"][:W], dtype=np.int32).view(np.float32).astype(np.float64)
    sfin = np.isfinite(e["s64"])
    assert (got_s[~sfin] == e["s64"][~sfin]).all(), name
    s_err = float(np.abs(got_s[sfin] - e["s64"][sfin]).max()) if sfin.any() else 0.0
    print(f"  PARITY beam {name}: err {err:.3e} E_ref {e['e_ref']:.3e} bar {e['bar']:.3e} err/bar {err / e['bar']:.3f} "
          f"score err {s_err:.3e} E_ref {e['s_e_ref']:.3e} bar {e['s_bar']:.3e} err/bar {s_err / e['s_bar']:.3f} [{' '.join(case.kinds)}]")
    assert err <= e["bar"], (name, err, e["bar"])
    assert s_err <= e["s_bar"], (name, s_err, e["s_bar"])


def _single(case):
    """One ua2_beam_step on caller-owned state.  Returns (cand_logp, cand_id, fields)."""
    W = case.W
    st = DeviceBeam(W, cap=bc.CAP, lp_n=case.lp_n)
    st.load(case.beam)
    st.ctrl[0] = case.step
    st.cand_logp.fill_(SENT_LOGP)
    st.cand_id.fill_(SENT_ID)
    logits = torch.from_numpy(case.x).to(DEV)
    st.step(logits, case.V, case.eos)
    assert np.array_equal(_bits(logits), case.x.view(np.int32)), case.name             # the logits: bit-unchanged
    f = dict(score=_bits(st.score).tolist(), fin=st.fin.cpu().tolist(), len=st.len.cpu().tolist(), parent=st.parent.cpu().tolist(),
             ctrl=st.ctrl.cpu().tolist(), log=st.log[:bc.CAP].cpu().tolist(), token=st.token.cpu().tolist())
    assert (st.log[bc.CAP] == -7).all(), case.name                                     # the guard step behind the log's capacity
    return st.cand_logp.cpu().numpy(), st.cand_id.cpu().numpy(), f


@pytest.mark.parametrize("W", bc.WIDTHS)
@pytest.mark.parametrize("V", bc.SMALL)
def test_single_step_at_the_smallest_shapes_of_each_path(V, W):
    for case in bc.single_cases(V, W):
        _check(case, *_single(case))


def test_single_step_at_the_released_vocabulary():
    for case in bc.single_cases(bc.RELEASED, 8):
        _check(case, *_single(case))


_grouped = {}


def _group_launch(G, W):
    """The grouped launch of bc.group_cases(G, W), once: (cases, cand_logp [G, 64], cand_id [G, 64], [fields per group])."""
    if (G, W) not in _grouped:
        from uniaudio2_amd import ops
        from uniaudio2_amd._lib import check, lib
        cases = bc.group_cases(G, W)
        V, ld = cases[0].V, cases[0].ld
        st = DeviceBeams(W, G, cap=bc.CAP, lp_n=cases[0].lp_n)
        for g, c in enumerate(cases):
            st.load(g, c.beam, c.step)
        st.cand_logp.fill_(SENT_LOGP)
        st.cand_id.fill_(SENT_ID)
        x = np.concatenate([c.x for c in cases] + [np.full((W, ld), 555.0, np.float32)])          # + the guard group's rows
        logits = torch.from_numpy(x).to(DEV)
        guard = st.fields(G)
        check(lib.ua2_beam_step_groups(logits.data_ptr(), ld, V, W, G, cases[0].eos, C.byref(st.c), st.token.data_ptr(), 9, ops.stream()), "groups")
        torch.cuda.synchronize()
        assert np.array_equal(_bits(logits), x.view(np.int32))
        assert st.fields(G) == guard and (st.cand_logp[G] == SENT_LOGP).all() and (st.cand_id[G] == SENT_ID).all()
        _grouped[(G, W)] = (cases, st.cand_logp.cpu().numpy(), st.cand_id.cpu().numpy(), [st.fields(g) for g in range(G)])
    return _grouped[(G, W)]


@pytest.mark.parametrize("G,W", bc.GROUPED)
def test_grouped_step_at_the_released_vocabulary(G, W):
    cases, cl, ci, fields = _group_launch(G, W)
    assert cases[0].V == bc.RELEASED and len(cases) == G
    for g, case in enumerate(cases):
        _check(case, cl[g], ci[g], fields[g], tag=f" (of {G})")
        one_l, one_i, one = _single(case)                                  # the group's rows in a single-step launch: the same bits
        assert np.array_equal(one_l.view(np.int32), cl[g].view(np.int32)) and np.array_equal(one_i, ci[g]), case.name
        assert one == fields[g], case.name


def test_a_row_alone_has_the_bits_it_has_among_64():
    """a row's log-sum-exp has the same bits whatever else runs.  Every live row of the 64-row launch, launched alone
    (W = 1, slot 0 live): the logp of its best column."""
    cases, cl, ci, _ = _group_launch(8, 8)
    n = 0
    for g, case in enumerate(cases):
        for j in bc.expect(case)["live"]:
            st = DeviceBeam(1, cap=bc.CAP, lp_n=case.lp_n)
            st.load(beam_ref.start(1))
            st.cand_logp.fill_(SENT_LOGP)
            st.cand_id.fill_(SENT_ID)
            st.step(torch.from_numpy(case.x[j:j + 1]).to(DEV), case.V, case.eos)
            got_l, got_i = st.cand_logp.cpu().numpy(), st.cand_id.cpu().numpy()
            assert got_i[0] == ci[g][j * 8] and got_l[:1].view(np.int32)[0] == cl[g][j * 8:j * 8 + 1].view(np.int32)[0], (case.name, j, case.kinds[j])
            assert (got_i[1:] == SENT_ID).all() and (got_l[1:] == SENT_LOGP).all()
            n += 1
    assert n >= 48
