"""On-device beam search of the text loop (include/ua2hip.h ua2_beam_step, ua2_beam_reorder, ua2_stage3_set_beam, frame mode 3;
Model_stage3.beam_search): the two entry points alone against tests/beam_ref.py and a torch gather, the search end to end against
the float64 rule over the CPU oracle, and identities that do not depend on any margin (W = 1 == greedy, replay of every hypothesis,
chunking, graph, expert skipping, restored page tables)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import beam_ref
from beam_ref import DEAD, FINISHED, LIVE, Slot
from helpers import build_oracle, build_product_model, load_golden_lm, toy_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEG = float("-inf")


@pytest.fixture(scope="module")
def golden():
    return load_golden_lm()


@pytest.fixture(scope="module")
def sd(golden):
    return toy_state_dict(golden[1])


def scaled_sd(sd, s):
    out = dict(sd)
    out["backbone.lm_head.weight"] = sd["backbone.lm_head.weight"] * s
    return out


def asr1(golden):
    d = golden[0]
    return torch.from_numpy(d["asr1_tokens"]).long(), torch.from_numpy(d["asr1_mask"]).bool()


def tiled_prompt(golden, L=62):
    """asr1 with its audio frames tiled up to L rows: prefill of 61 positions, so the search's step 3 writes position 64 — a new page."""
    t, m = asr1(golden)
    audio = torch.nonzero(m[:, 0]).flatten()
    a0, a1 = int(audio[0]), int(audio[-1]) + 1
    n = L - (t.shape[0] - (a1 - a0))
    idx = torch.arange(n) % (a1 - a0) + a0
    return torch.cat([t[:a0], t[idx], t[a1:]]), torch.cat([m[:a0], m[idx], m[a1:]])


# ---- 1. ua2_beam_step alone ------------------------------------------------------------------------------------------------------
class DeviceBeam:
    """Caller-owned state of ua2_beam_state for the direct calls."""

    def __init__(self, W, alpha=0.6, cap=4, lp_n=64):
        from uniaudio2_amd._lib import BeamState
        i32 = dict(dtype=torch.int32, device=DEV)
        self.W = W
        self.score = torch.full((8,), NEG, dtype=torch.float32, device=DEV)
        self.fin = torch.full((8,), 2, **i32)
        self.len = torch.zeros(8, **i32)
        self.parent = torch.full((8,), -9, **i32)
        self.ctrl = torch.tensor([0, -1, 0, 0], **i32)
        self.cand_logp = torch.zeros(64, dtype=torch.float32, device=DEV)
        self.cand_id = torch.zeros(64, **i32)
        self.log = torch.full((cap + 1, W, 4), -7, **i32)                    # one guard step behind the capacity
        self.lp_inv = torch.tensor([1.0 / beam_ref.lp(n, alpha) for n in range(lp_n)], dtype=torch.float64).float().to(DEV)
        self.token = torch.full((W, 9), -5, **i32)
        self.cap = cap
        self.c = BeamState(self.score.data_ptr(), self.fin.data_ptr(), self.len.data_ptr(), self.parent.data_ptr(), self.ctrl.data_ptr(),
                           self.cand_logp.data_ptr(), self.cand_id.data_ptr(), self.log.data_ptr(), cap, self.lp_inv.data_ptr(), lp_n)

    def load(self, beam):
        self.score[:self.W] = torch.tensor([b.score for b in beam], dtype=torch.float32)
        self.fin[:self.W] = torch.tensor([b.fin for b in beam], dtype=torch.int32)
        self.len[:self.W] = torch.tensor([b.len for b in beam], dtype=torch.int32)

    def step(self, logits, V, eos):
        from uniaudio2_amd import ops
        from uniaudio2_amd._lib import check, lib
        check(lib.ua2_beam_step(logits.data_ptr(), logits.shape[1], V, self.W, eos, C.byref(self.c), self.token.data_ptr(), 9,
                                ops.stream()), "ua2_beam_step")
        torch.cuda.synchronize()


def _decided(ranked, tops, W, gap=1e-3):
    """Every comparison that decides the step is either an exact tie (identical inputs) or at least `gap` wide."""
    s = [c[0] for c in ranked[:W + 1] if np.isfinite(c[0])]
    d = [a - b for a, b in zip(s, s[1:])] + [float(a - b) for t in tops for a, b in zip(t, t[1:]) if np.isfinite(a) and np.isfinite(b)]
    return all(x == 0.0 or x >= gap for x in d)


def _scenarios(V, ld, W, seed):
    """(name, logits [W, ld] fp32, beam, eos).  Rows are multiples of 1/8 plus per-row distinct offsets where ties are not wanted: the
    gaps between different values are then >= 1/8 in the logits, and the candidate scores are checked by _decided."""
    g = np.random.default_rng(seed)
    pad = 777.0                                                           # columns [V, ld) must never be read: they would win everything

    def rows(quant, distinct=True):
        x = np.full((W, ld), pad, np.float32)
        for j in range(W):
            if distinct:
                x[j, :V] = (g.permutation(V) * quant - 0.37 * j).astype(np.float32)      # all different within a row
            else:
                x[j, :V] = (g.integers(0, 12, size=V) * quant).astype(np.float32)        # many exactly equal logits
        return x

    out = []
    out.append(("start", rows(0.125), beam_ref.start(W), 128001))         # slot 0 live, the others dead; an EOS id >= V
    beam = [Slot(-1.5 - 0.8 * j, LIVE, list(range(3 + j))) for j in range(W)]
    if W >= 2:
        beam[1] = Slot(-0.9, FINISHED, [5, 6])
    if W >= 4:
        beam[W - 1] = Slot(NEG, DEAD, [])
    x = rows(0.125)
    out.append(("mixed_eos_in", x, beam, int(np.argmax(x[0, :V]))))       # EOS inside the top W of slot 0
    out.append(("mixed_eos_out", x, beam, int(np.argmin(x[0, :V]))))      # ... and far outside it
    xt = rows(1.0, distinct=False)
    bt = [Slot(-2.0 - 0.45 * j, LIVE, list(range(2))) for j in range(W)]
    if W >= 2:                                                            # two slots with identical rows and equal scores
        xt[1] = xt[0]
        bt[1] = Slot(bt[0].score, LIVE, [7, 8])
    out.append(("ties", xt, bt, int(np.argmax(xt[W - 1, :V]))))
    xs = rows(0.125)
    xs[0, :V:3] = NEG
    xs[0, 1:V:7] = np.nan
    xs[0, int(np.argmax(np.nan_to_num(xs[0, :V], nan=-1e30, neginf=-1e30)))] = np.nan     # the would-be maximum is a NaN
    if W >= 3:
        xs[2, :V] = NEG                                                   # a row without a finite entry: every candidate scores -inf
        xs[2, 5] = np.nan
    # a flat row: every column contributes to the sum of exponentials (values 2e-3 apart: the smallest gap the bound allows for)
    out.append(("flat", rows(0.002), [Slot(-1.5 - 0.8 * j, LIVE, [2] * j) for j in range(W)], 128001))
    out.append(("specials", xs, [Slot(-1.0 - 0.3 * j, LIVE, [1] * j) for j in range(W)], 4))
    return out


@pytest.mark.parametrize("W", [1, 3, 5, 8])
@pytest.mark.parametrize("V,ld", [(512, 512), (1000, 1008), (4100, 4100)])
def test_beam_step_against_the_rule(V, ld, W):
    worst = 0.0
    for name, x, beam, eos in _scenarios(V, ld, W, 1000 + V + W):
        ranked, tops = beam_ref.rank(x[:, :V], beam, eos)
        assert _decided(ranked, tops, W), name
        want, parents, fed, _ = beam_ref.select(x[:, :V], beam, eos)
        st = DeviceBeam(W)
        st.load(beam)
        st.step(torch.from_numpy(x).to(DEV), V, eos)
        got_s = st.score[:W].cpu().double().numpy()
        assert st.fin[:W].cpu().tolist() == [b.fin for b in want], name
        assert st.len[:W].cpu().tolist() == [b.len for b in want], name
        assert st.parent[:W].cpu().tolist() == parents, name
        assert st.token[:, 0].cpu().tolist() == fed, name
        assert (st.token[:, 1:] == -5).all()
        rec = st.log.cpu().numpy()
        assert rec[0, :, 0].tolist() == parents and rec[0, :, 3].tolist() == [b.fin for b in want], name
        assert rec[0, :, 1].tolist() == [b.ids[-1] if b.fin == LIVE else -1 for b in want], name
        assert (rec[0, :, 2].view(np.float32).astype(np.float64) == got_s).all() and (rec[1:] == -7).all(), name
        assert st.ctrl.cpu().tolist() == [1, 0 if all(b.fin == FINISHED for b in want) else -1, 0, 0], name
        for a, b in zip(got_s, want):
            if np.isfinite(b.score):
                err = abs(a - b.score) / max(1.0, abs(b.score))
                worst = max(worst, err)
                assert err <= 1e-5, (name, a, b.score)
            else:
                assert a == b.score, name
    print(f"  beam step V={V} W={W}: worst score error {worst:.2e} (bound 1e-5 relative to max(1, |score|))")


def test_beam_step_all_finished_is_a_fixed_point_and_bad_arguments():
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import check, lib
    W, V = 3, 512
    beam = [Slot(-1.0, FINISHED, [3]), Slot(-1.0, FINISHED, [4, 5]), Slot(-2.5, FINISHED, [])]
    st = DeviceBeam(W, cap=2)
    st.load(beam)
    x = torch.randn(W, V, device=DEV)
    for step in range(3):                                                  # the third step is past the log's capacity: not logged
        st.step(x, V, 7)
        assert st.score[:W].cpu().tolist() == [-1.0, -1.0, -2.5] and st.fin[:W].cpu().tolist() == [1, 1, 1]
        assert st.parent[:W].cpu().tolist() == [0, 1, 2] and st.token[:, 0].cpu().tolist() == [0, 0, 0]
    assert st.ctrl.cpu().tolist() == [3, 0, 0, 0] and (st.log[2] == -7).all()
    for bad_w in (0, 9):
        with pytest.raises(RuntimeError, match="beam width"):
            check(lib.ua2_beam_step(x.data_ptr(), V, V, bad_w, 7, C.byref(st.c), st.token.data_ptr(), 9, ops.stream()), "W")
    with pytest.raises(RuntimeError):
        check(lib.ua2_beam_step(x.data_ptr(), V - 1, V, W, 7, C.byref(st.c), st.token.data_ptr(), 9, ops.stream()), "ld < V")


# ---- 2. ua2_beam_reorder alone ---------------------------------------------------------------------------------------------------
PATTERNS = {"identity": lambda W: list(range(W)), "all_equal": lambda W: [W - 1] * W,
            "permutation": lambda W: list(range(W))[::-1], "duplicates": lambda W: [j - j % 2 for j in range(W)]}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("n0", [63, 64, 126])        # next-position offsets in the page: (63, 0, 1), (0, 1, 2), (62, 63, 0)
def test_beam_reorder_against_a_torch_gather(dtype, pattern, n0):
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import BeamPool, check, lib, vp
    W, rows, max_pages = 4, 9, 4                                           # tables of 2 W + 1 rows: the last one must never change
    geoms = [(2, 16), (1, 8 if dtype == torch.float32 else 16)]            # (n_kv, head_size) of two GPTs, two layers each
    esz = torch.empty(0, dtype=dtype).element_size()
    pools, descs = [], []
    for ti, (n_kv, hs) in enumerate(geoms):
        for layer in range(4):                                             # K and V of two layers
            pg, hd, ps, el = torch.meshgrid(torch.arange(rows * max_pages), torch.arange(n_kv), torch.arange(64), torch.arange(hs), indexing="ij")
            v = ((ti * 4 + layer) * 7 + pg * 3 + hd * 5 + ps * 11 + el) % 251 - 125       # (layer, page, head, position)-coded, exact in bf16
            pools.append(v.to(dtype).to(DEV))
            descs.append(BeamPool(pools[-1].data_ptr(), ti, n_kv, hs * esz, 0))
    pools_dev = torch.frombuffer(bytearray(bytes((BeamPool * len(descs))(*descs))), dtype=torch.uint8).to(DEV)
    tables = [torch.arange(rows * max_pages, dtype=torch.int32, device=DEV).view(rows, max_pages).clone() for _ in geoms]
    tabs = (vp * 2)(*[t.data_ptr() for t in tables])
    ref_pools, ref_tables = [p.clone() for p in pools], [t.clone() for t in tables]
    row_pos = torch.full((W,), n0, dtype=torch.int32, device=DEV)
    parents = PATTERNS[pattern](W)
    par_dev = torch.tensor(parents, dtype=torch.int32, device=DEV)

    def reference(par, n):
        c, fill = n // 64, n % 64
        for ti in range(len(geoms)):
            old = ref_tables[ti].clone()
            olds = [p.clone() for p in ref_pools]
            for j in range(W):
                p = par[j]
                dst = ((n & 1) * W + j) * max_pages + c
                src = int(old[p, c])
                ref_tables[ti][j, :c] = old[p, :c]
                ref_tables[ti][j, c] = dst
                if fill and src != dst:
                    for k in range(ti * 4, ti * 4 + 4):
                        ref_pools[k][dst, :, :fill] = olds[k][src, :, :fill]

    def write_position(n, stamp):
        """What a frame's trunk does between two forks: slot j writes position n into its current page."""
        for ti in range(len(geoms)):
            for k in range(ti * 4, ti * 4 + 4):
                for j in range(W):
                    val = (stamp * 13 + k * 5 + j * 3) % 97 - 48
                    for pool, tab in ((pools[k], tables[ti]), (ref_pools[k], ref_tables[ti])):
                        pool[int(tab[j, n // 64]), :, n % 64] = val

    def call(par, pos_add):
        check(lib.ua2_beam_reorder(W, par, row_pos.data_ptr(), pos_add, pools_dev.data_ptr(), len(descs), tabs, 2, rows, max_pages,
                                   ops.stream()), "ua2_beam_reorder")
        torch.cuda.synchronize()

    def same():
        return all(torch.equal(a, b) for a, b in zip(tables, ref_tables)) and all(torch.equal(a, b) for a, b in zip(pools, ref_pools))

    call(None, 0)                                                          # the start: every parent is slot 0
    reference([0] * W, n0)
    assert same()
    for step in range(2):                                                  # two consecutive steps: both page sets
        n = n0 + step
        write_position(n, step)
        call(par_dev.data_ptr(), 1)
        reference(parents, n + 1)
        assert same(), step
        row_pos += 1
    assert torch.equal(tables[0][2 * W:], torch.arange(2 * W * max_pages, rows * max_pages, dtype=torch.int32, device=DEV).view(-1, max_pages))
    for p in tables:                                                       # slots only ever point into the two page sets
        assert int(p[:W].min()) >= 0 and int(p[:W].max()) < 2 * W * max_pages
    with pytest.raises(RuntimeError, match="page tables"):
        check(lib.ua2_beam_reorder(W, None, row_pos.data_ptr(), 0, pools_dev.data_ptr(), len(descs), tabs, 2, 2 * W - 1, max_pages, ops.stream()), "rows")
    with pytest.raises(RuntimeError, match="beam width"):
        check(lib.ua2_beam_reorder(9, None, row_pos.data_ptr(), 0, pools_dev.data_ptr(), len(descs), tabs, 2, rows, max_pages, ops.stream()), "W")


# ---- 3. end to end against the float64 rule over the CPU oracle -----------------------------------------------------------------
CASES = {   # name: (lm_head factor, W, max_length, EOS)
    "A": (1, 3, 12, 128001), "B": (8, 4, 500, 125), "C": (8, 3, 12, 13), "D": (8, 3, 16, 16)}
_oracle_runs = {}


def oracle_run(sd, golden, name):
    if name not in _oracle_runs:
        s, W, ml, eos = CASES[name]
        tok, msk = asr1(golden)
        _oracle_runs[name] = beam_ref.search(build_oracle(scaled_sd(sd, s), "fp32", batch=W), tok, msk, W, eos, max_length=ml)
    return _oracle_runs[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_search_fp32_equals_the_rule_over_the_oracle(sd, golden, name):
    s, W, ml, eos = CASES[name]
    ref = oracle_run(sd, golden, name)
    steps = ref["steps"]
    tol = 2 * (5e-5 * s) * steps                  # the project's fp32 logit bar (5e-5, x the lm_head factor), twice per step (logit and log-sum-exp)
    print(f"  case {name}: steps {steps}, oracle margins score / logit / final = " + " / ".join(f"{m:.3g}" for m in ref["margins"]) + f", tol {tol:.3g}")
    assert ref["margins"][0] >= tol and ref["margins"][2] >= tol and ref["margins"][1] >= 2 * 5e-5 * s and ref["margins"][1] >= tol
    tok, msk = asr1(golden)
    m = build_product_model(scaled_sd(sd, s), torch.float32, batch=2 * W)
    ids, score, hyps = m.beam_search(tok, msk, beam_width=W, max_length=ml, eos_id=eos)
    worst = max(abs(h["score"] - b.score) for h, b in zip(hyps, ref["beam"]))
    print(f"  case {name}: worst score difference {worst:.3g}")
    assert [h["ids"] for h in hyps] == [b.ids for b in ref["beam"]]
    assert [h["finished"] for h in hyps] == [b.fin == FINISHED for b in ref["beam"]]
    assert worst <= tol
    assert ids == ref["beam"][ref["best"]].ids and score == hyps[ref["best"]]["score"]
    assert m.beam_info["steps"] >= steps
    if name == "B":
        assert steps == 14 and all(h["finished"] for h in hyps) and m.beam_info["all_finished"] == 13
    if name == "C":
        assert all(h["finished"] for h in hyps) and ids == [9]
    if name == "D":
        assert steps == 16 and m.beam_info["all_finished"] == -1 and hyps[0]["finished"] and not hyps[1]["finished"] and ids == hyps[0]["ids"]


# ---- 4. W = 1 is the greedy text loop ------------------------------------------------------------------------------------------
def greedy_ids(m, tok, msk, frames):
    m.begin_ragged([(tok.to(DEV), msk.to(DEV))])
    return m.generate_frames(frames, 1, 1, skip_audio_experts=True)[:, 0, 0].cpu().tolist()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_beam_of_one_is_the_greedy_loop(sd, golden, dtype):
    tok, msk = asr1(golden)
    m = build_product_model(sd, dtype, batch=2)
    want = greedy_ids(m, tok, msk, 24)
    ids, _, hyps = m.beam_search(tok, msk, beam_width=1, max_length=24, eos_id=128001)
    assert torch.equal(torch.tensor(ids), torch.tensor(want)) and not hyps[0]["finished"]
    eos = want[7]
    k = want.index(eos)                                                    # up to the first EOS
    ids, _, hyps = m.beam_search(tok, msk, beam_width=1, max_length=24, eos_id=eos)
    assert torch.equal(torch.tensor(ids, dtype=torch.long), torch.tensor(want[:k], dtype=torch.long)) and hyps[0]["finished"]
    assert m.beam_info["all_finished"] == k


# ---- 5. K/V integrity: every hypothesis replayed alone ------------------------------------------------------------------------------
def replay_score(m, tok, msk, ids, finished, eos, alpha=0.6):
    """forward_prefix + generate_frame along the hypothesis; the score re-accumulated in float64 from the device's own text logits."""
    tok, msk = tok.to(DEV), msk.to(DEV)
    L = tok.shape[0]
    m.reset_caches()
    pos = torch.arange(0, L, device=DEV).unsqueeze(0)
    m.forward_prefix(tok[None, :-1], tokens_mask=msk[None], input_pos=pos[:, :-1])
    ct, cm = tok[None, -1:], msk[None, -1:]
    score = 0.0
    for n, k in enumerate(list(ids) + ([eos] if finished else [])):
        m.generate_frame(ct, cm, input_pos=torch.tensor([L - 1 + n], device=DEV), temperature=1.0, topk=1)
        logp = torch.log_softmax(m.buffer("text_logits", 1)[0].double(), dim=-1)
        score += float(logp[k]) / beam_ref.lp(n if k == eos and n == len(ids) else n + 1, alpha)
        ct = torch.zeros(1, 1, 9, dtype=torch.long, device=DEV); ct[0, 0, -1] = k
        cm = torch.zeros(1, 1, 9, dtype=torch.bool, device=DEV); cm[0, 0, -1] = True
    return score


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("prompt", ["asr1", "tiled62"])
@pytest.mark.parametrize("s,eos", [(1, 128001), (8, 13)])
def test_every_hypothesis_replays_to_its_score(sd, golden, dtype, prompt, s, eos):
    W = 3
    tok, msk = asr1(golden) if prompt == "asr1" else tiled_prompt(golden)
    assert prompt == "asr1" or tok.shape[0] == 62
    m = build_product_model(scaled_sd(sd, s), dtype, batch=2 * W)
    _, _, hyps = m.beam_search(tok, msk, beam_width=W, max_length=12, eos_id=eos)
    assert len({tuple(h["ids"]) for h in hyps}) == W
    for h in hyps:
        got = replay_score(m, tok, msk, h["ids"], h["finished"], eos)
        assert abs(got - h["score"]) <= 1e-4, (h, got)


# ---- 6. identities -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_search_does_not_depend_on_chunking_graph_or_expert_skipping(sd, golden, dtype):
    tok, msk = tiled_prompt(golden)
    W = 4
    m = build_product_model(scaled_sd(sd, 8), dtype, batch=2 * W)
    before = greedy_ids(m, tok, msk, 20)
    kw = dict(beam_width=W, max_length=40, eos_id=125)
    base = m.beam_search(tok, msk, chunk_frames=16, **kw)
    assert m.beam_info["all_finished"] >= 0 or m.beam_info["steps"] == 40
    assert m.beam_search(tok, msk, chunk_frames=1, **kw) == base
    assert m.beam_search(tok, msk, use_graph=False, **kw) == base
    assert m.beam_search(tok, msk, skip_audio_experts=False, **kw) == base
    assert greedy_ids(m, tok, msk, 20) == before                           # the page tables are restored, the beam state detached
    for g in (m.audio_understanding_expert, m.backbone, m.audio_generation_expert):
        pt = g.kv_cache.page_table
        assert torch.equal(pt.flatten(), torch.arange(pt.numel(), dtype=torch.int32, device=DEV))


def test_plan_and_frame_checks(sd, golden):
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import Ua2Error, check, lib
    tok, msk = asr1(golden)
    m = build_product_model(sd, torch.float32, batch=5)
    with pytest.raises(ValueError, match="max_batch_size=6"):
        m.beam_search(tok, msk, beam_width=3)
    with pytest.raises(ValueError, match="beam_width"):
        m.beam_search(tok, msk, beam_width=9)
    with pytest.raises(ValueError, match="begin_beams"):
        m.generate_frames(1, 2, 3)
    with pytest.raises(Ua2Error, match="needs a beam"):                    # the C side refuses before any launch
        check(lib.ua2_stage3_frame(m._h, 2, 3, -1, 0, 0, ops.stream()), "ua2_stage3_frame")
    m.begin_beams(tok, msk, beam_width=2, max_length=4)
    try:
        with pytest.raises(Ua2Error, match="one row per slot"):
            check(lib.ua2_stage3_frame(m._h, 1, 3, -1, 0, 0, ops.stream()), "ua2_stage3_frame")
        with pytest.raises(ValueError, match="step log full"):
            m.generate_frames(5, 2, 3)
        m.generate_frames(4, 2, 3)
    finally:
        ids, score, hyps = m.end_beams()
    assert len(ids) == 4 and math.isfinite(score) and m._beam is None
    m.set_ngram(3, 499, capacity=8)
    with pytest.raises(ValueError, match="n-gram"):
        m.beam_search(tok, msk, beam_width=2, max_length=4)
    m.set_ngram(0)
    assert m.beam_search(tok, msk, beam_width=2, max_length=4)[0] == ids
