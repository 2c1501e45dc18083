"""Several beams in one decode frame (include/ua2hip.h ua2_beam_step_groups, ua2_beam_reorder_groups, ua2_stage3_set_beam_groups;
Model_stage3.beam_search_batch): the grouped step against the single step bit for bit and against tests/beam_ref.py, the grouped fork
against a torch gather, and the batched search against one beam_search per prompt (==), against the float64 rule over the CPU oracle,
and in reversed order."""
import ctypes as C

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
    """asr1 with its audio frames tiled up to L rows (L = 62: prefill of 61 positions, so the search's step 3 opens a new page)."""
    t, m = asr1(golden)
    audio = torch.nonzero(m[:, 0]).flatten()
    a0, a1 = int(audio[0]), int(audio[-1]) + 1
    n = L - (t.shape[0] - (a1 - a0))
    idx = torch.arange(n) % (a1 - a0) + a0
    return torch.cat([t[:a0], t[idx], t[a1:]]), torch.cat([m[:a0], m[idx], m[a1:]])


def four_prompts(golden):
    """Four prompts that behave differently under the search of the tests below (lm_head x 8, EOS 13): lengths 62, 40 and 30 besides asr1."""
    out = [asr1(golden), tiled_prompt(golden, 62), tiled_prompt(golden, 40), tiled_prompt(golden, 30)]
    assert [p[0].shape[0] for p in out[1:]] == [62, 40, 30]
    return out


# ---- 1. ua2_beam_step_groups against ua2_beam_step -------------------------------------------------------------------------------
class DeviceBeams:
    """Caller-owned state of ua2_beam_state for `groups` groups at the strides of the header, every buffer one group longer: the
    guard group behind the last one must stay as it was."""

    def __init__(self, W, groups, alpha=0.6, cap=4, lp_n=64):
        from uniaudio2_amd._lib import BeamState
        i32 = dict(dtype=torch.int32, device=DEV)
        n = groups + 1
        self.W, self.G, self.cap = W, groups, cap
        self.score = torch.full((n, 8), NEG, dtype=torch.float32, device=DEV)
        self.fin = torch.full((n, 8), 2, **i32)
        self.len = torch.zeros(n, 8, **i32)
        self.parent = torch.full((n, 8), -9, **i32)
        self.ctrl = torch.tensor([[0, -1, 0, 0]] * n, **i32)
        self.cand_logp = torch.zeros(n, 64, dtype=torch.float32, device=DEV)
        self.cand_id = torch.zeros(n, 64, **i32)
        self.log = torch.full((n, cap, W, 4), -7, **i32)
        self.lp_inv = torch.tensor([1.0 / beam_ref.lp(k, alpha) for k in range(lp_n)], dtype=torch.float64).float().to(DEV)
        self.token = torch.full((n * W, 9), -5, **i32)
        self.c = BeamState(self.score.data_ptr(), self.fin.data_ptr(), self.len.data_ptr(), self.parent.data_ptr(), self.ctrl.data_ptr(),
                           self.cand_logp.data_ptr(), self.cand_id.data_ptr(), self.log.data_ptr(), cap, self.lp_inv.data_ptr(), lp_n)

    def load(self, g, beam, step):
        W = self.W
        self.score[g, :W] = torch.tensor([b.score for b in beam], dtype=torch.float32)
        self.fin[g, :W] = torch.tensor([b.fin for b in beam], dtype=torch.int32)
        self.len[g, :W] = torch.tensor([b.len for b in beam], dtype=torch.int32)
        self.ctrl[g, 0] = step

    def fields(self, g):
        """Everything a step may write for group g, as integers (scores by their bits)."""
        W = self.W
        return dict(score=self.score[g].view(torch.int32).cpu().tolist(), fin=self.fin[g].cpu().tolist(), len=self.len[g].cpu().tolist(),
                    parent=self.parent[g].cpu().tolist(), ctrl=self.ctrl[g].cpu().tolist(), log=self.log[g].cpu().tolist(),
                    token=self.token[g * W:(g + 1) * W].cpu().tolist())


def _decided(ranked, tops, W, gap=1e-3):
    """Every comparison that decides the step is either an exact tie (identical inputs) or at least `gap` wide."""
    s = [c[0] for c in ranked[:W + 1] if np.isfinite(c[0])]
    d = [a - b for a, b in zip(s, s[1:])] + [float(a - b) for t in tops for a, b in zip(t, t[1:]) if np.isfinite(a) and np.isfinite(b)]
    return all(x == 0.0 or x >= gap for x in d)


KINDS = ["mixed", "start", "ties", "all_finished", "specials"]


def _group_scenarios(V, ld, W, G, seed):
    """One scenario per group, built as tests/test_gpu_beam.py builds its own (rows are multiples of 1/8 plus per-row offsets where
    ties are not wanted), under the one EOS id a call has: the best column of group 0's first row.  Returns ([(kind, logits [W, ld],
    beam)], eos)."""
    rng = np.random.default_rng(seed)
    pad = 777.0                                                           # columns [V, ld) must never be read: they would win everything

    def rows(quant, distinct=True):
        x = np.full((W, ld), pad, np.float32)
        for j in range(W):
            if distinct:
                x[j, :V] = (rng.permutation(V) * quant - 0.37 * j).astype(np.float32)
            else:
                x[j, :V] = (rng.integers(0, 12, size=V) * quant).astype(np.float32)
        return x

    out = []
    for g in range(G):
        kind = KINDS[g % len(KINDS)]
        if kind == "mixed":                                               # live, finished and (W >= 4) dead slots
            beam = [Slot(-1.5 - 0.8 * j, LIVE, list(range(3 + j))) for j in range(W)]
            if W >= 2:
                beam[1] = Slot(-0.9, FINISHED, [5, 6])
            if W >= 4:
                beam[W - 1] = Slot(NEG, DEAD, [])
            x = rows(0.125)
        elif kind == "start":                                             # slot 0 live, the others dead
            beam, x = beam_ref.start(W), rows(0.125)
        elif kind == "ties":                                              # many equal logits; two slots with identical rows and scores
            x = rows(1.0, distinct=False)
            beam = [Slot(-2.0 - 0.45 * j, LIVE, list(range(2))) for j in range(W)]
            if W >= 2:
                x[1] = x[0]
                beam[1] = Slot(beam[0].score, LIVE, [7, 8])
        elif kind == "all_finished":                                      # a fixed point, whatever its rows hold
            beam, x = [Slot(-1.0 - 0.25 * (j // 2), FINISHED, [3] * j) for j in range(W)], rows(0.125)
        else:                                                             # -inf, NaN, a row without a finite entry
            x = rows(0.125)
            x[0, :V:3] = NEG
            x[0, 1:V:7] = np.nan
            x[0, int(np.argmax(np.nan_to_num(x[0, :V], nan=-1e30, neginf=-1e30)))] = np.nan
            if W >= 3:
                x[2, :V] = NEG
                x[2, 5] = np.nan
            beam = [Slot(-1.0 - 0.3 * j, LIVE, [1] * j) for j in range(W)]
        out.append((kind, x, beam))
    return out, int(np.argmax(out[0][1][0, :V]))                          # EOS inside the top W of group 0's slot 0


@pytest.mark.parametrize("G", [1, 2, 5])
@pytest.mark.parametrize("W", [1, 3, 8])
@pytest.mark.parametrize("V,ld", [(512, 512), (4100, 4100)])
def test_grouped_step_equals_the_single_step_and_the_rule(V, ld, W, G):
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import check, lib
    scen, eos = _group_scenarios(V, ld, W, G, 3000 + V + 10 * W + G)
    logits = torch.from_numpy(np.concatenate([x for _, x, _ in scen] + [np.full((W, ld), 555.0, np.float32)])).to(DEV)   # + the guard rows
    st = DeviceBeams(W, G)
    for g, (_, _, beam) in enumerate(scen):
        st.load(g, beam, g % 2)                                           # groups at different steps: their log records differ in place
    guard = st.fields(G)
    check(lib.ua2_beam_step_groups(logits.data_ptr(), ld, V, W, G, eos, C.byref(st.c), st.token.data_ptr(), 9, ops.stream()), "groups")
    torch.cuda.synchronize()
    assert st.fields(G) == guard and (st.cand_logp[G] == 0).all() and (st.cand_id[G] == 0).all()
    worst = 0.0
    for g, (kind, x, beam) in enumerate(scen):
        one = DeviceBeams(W, 1)
        one.load(0, beam, g % 2)
        check(lib.ua2_beam_step(logits[g * W:].data_ptr(), ld, V, W, eos, C.byref(one.c), one.token.data_ptr(), 9, ops.stream()), "single")
        torch.cuda.synchronize()
        got = st.fields(g)
        assert got == one.fields(0), (kind, g)                            # every field, the token column, the log, ctrl: the same bits
        assert torch.equal(st.cand_logp[g].view(torch.int32), one.cand_logp[0].view(torch.int32)) and torch.equal(st.cand_id[g], one.cand_id[0])
        # ... and the rule itself, as tests/test_gpu_beam.py checks the single step
        ranked, tops = beam_ref.rank(x[:, :V], beam, eos)
        assert _decided(ranked, tops, W), kind
        want, parents, fed, _ = beam_ref.select(x[:, :V], beam, eos)
        assert got["fin"][:W] == [b.fin for b in want] and got["len"][:W] == [b.len for b in want], kind
        assert got["parent"][:W] == parents and [r[0] for r in got["token"]] == fed, kind
        assert all(r[1:] == [-5] * 8 for r in got["token"])
        assert got["ctrl"] == [g % 2 + 1, g % 2 if all(b.fin == FINISHED for b in want) else -1, 0, 0], kind
        rec = got["log"][g % 2]
        assert [r[0] for r in rec] == parents and [r[3] for r in rec] == [b.fin for b in want], kind
        assert [r[1] for r in rec] == [b.ids[-1] if b.fin == LIVE else -1 for b in want], kind
        assert [r[2] for r in rec] == got["score"][:W] and all(r == [-7] * 4 for t in range(st.cap) if t != g % 2 for r in got["log"][t])
        for a, b in zip(st.score[g, :W].cpu().double().tolist(), want):
            if np.isfinite(b.score):
                err = abs(a - b.score) / max(1.0, abs(b.score))
                worst = max(worst, err)
                assert err <= 1e-5, (kind, a, b.score)
            else:
                assert a == b.score, kind
    print(f"  grouped step V={V} W={W} G={G}: worst score error {worst:.2e} (bound 1e-5 relative to max(1, |score|))")


# ---- 2. ua2_beam_reorder_groups against a torch gather ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_grouped_reorder_against_a_torch_gather(dtype):
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import BeamPool, check, lib, vp
    G, W, max_pages = 3, 4, 4
    R = G * W
    rows = 2 * R + 1                                                       # one table row more than the fork may touch
    n0 = (63, 64, 126)                                                     # the groups stand at different positions
    parents = [[3, 2, 1, 0], [3, 3, 3, 3], [0, 0, 2, 2]]                   # permutation, all equal, duplicates
    geoms = [(2, 16), (1, 8 if dtype == torch.float32 else 16)]            # (n_kv, head_size) of two GPTs, K and V of two layers each
    esz = torch.empty(0, dtype=dtype).element_size()
    pools, descs = [], []
    for ti, (n_kv, hs) in enumerate(geoms):
        for layer in range(4):
            pg, hd, ps, el = torch.meshgrid(torch.arange(rows * max_pages), torch.arange(n_kv), torch.arange(64), torch.arange(hs), indexing="ij")
            v = ((ti * 4 + layer) * 7 + pg * 3 + hd * 5 + ps * 11 + el) % 251 - 125       # (layer, page, head, position)-coded, exact in bf16
            pools.append(v.to(dtype).to(DEV))
            descs.append(BeamPool(pools[-1].data_ptr(), ti, n_kv, hs * esz, 0))
    pools_dev = torch.frombuffer(bytearray(bytes((BeamPool * len(descs))(*descs))), dtype=torch.uint8).to(DEV)
    tables = [torch.arange(rows * max_pages, dtype=torch.int32, device=DEV).view(rows, max_pages).clone() for _ in geoms]
    tabs = (vp * 2)(*[t.data_ptr() for t in tables])
    ref_pools, ref_tables = [p.clone() for p in pools], [t.clone() for t in tables]
    row_pos = torch.tensor([n0[g] for g in range(G) for _ in range(W)], dtype=torch.int32, device=DEV)
    par = torch.full((G, 8), 99, dtype=torch.int32)                        # strided 8 per group; the entries past W are never read
    for g in range(G):
        par[g, :W] = torch.tensor(parents[g], dtype=torch.int32)
    par_dev = par.to(DEV)

    def reference(par_of, add):
        """Today's single-beam rule per group, with the page sets of R rows."""
        for ti in range(len(geoms)):
            old = ref_tables[ti].clone()
            olds = [p.clone() for p in ref_pools]
            for g in range(G):
                n = int(row_pos[g * W]) + add
                c, fill = n // 64, n % 64
                for j in range(W):
                    r, p = g * W + j, g * W + par_of[g][j]
                    dst = ((n & 1) * R + r) * max_pages + c
                    src = int(old[p, c])
                    ref_tables[ti][r, :c] = old[p, :c]
                    ref_tables[ti][r, c] = dst
                    if fill and src != dst:
                        for k in range(ti * 4, ti * 4 + 4):
                            ref_pools[k][dst, :, :fill] = olds[k][src, :, :fill]

    def write_positions(stamp):
        """What a frame's trunk does between two forks: every row writes its position into its current page."""
        for ti in range(len(geoms)):
            for k in range(ti * 4, ti * 4 + 4):
                for r in range(R):
                    n = int(row_pos[r])
                    val = (stamp * 13 + k * 5 + r * 3) % 97 - 48
                    for pool, tab in ((pools[k], tables[ti]), (ref_pools[k], ref_tables[ti])):
                        pool[int(tab[r, n // 64]), :, n % 64] = val

    def call(p, pos_add, table_rows=rows, w=W, g=G):
        check(lib.ua2_beam_reorder_groups(w, g, p, row_pos.data_ptr(), pos_add, pools_dev.data_ptr(), len(descs), tabs, 2, table_rows, max_pages,
                                          ops.stream()), "ua2_beam_reorder_groups")
        torch.cuda.synchronize()

    def same():
        return all(torch.equal(a, b) for a, b in zip(tables, ref_tables)) and all(torch.equal(a, b) for a, b in zip(pools, ref_pools))

    call(None, 0)                                                          # the start: every parent is slot 0 of its group
    reference([[0] * W] * G, 0)
    assert same()
    for step in range(2):                                                  # two consecutive steps: both page sets of every group
        write_positions(step)
        call(par_dev.data_ptr(), 1)
        reference(parents, 1)
        assert same(), step
        row_pos += 1
    for t in tables:
        assert torch.equal(t[2 * R:], torch.arange(2 * R * max_pages, rows * max_pages, dtype=torch.int32, device=DEV).view(-1, max_pages))
        assert int(t[:R].min()) >= 0 and int(t[:R].max()) < 2 * R * max_pages                # slots only ever point into the two page sets
        assert torch.equal(t[R:2 * R], torch.arange(R * max_pages, 2 * R * max_pages, dtype=torch.int32, device=DEV).view(-1, max_pages))
    before = [t.clone() for t in tables]
    with pytest.raises(RuntimeError, match="page tables"):
        call(None, 0, table_rows=2 * R - 1)
    with pytest.raises(RuntimeError, match="64"):
        call(None, 0, w=5, g=13)                                           # 65 rows
    with pytest.raises(RuntimeError, match="beam width"):
        call(None, 0, w=9, g=1)
    with pytest.raises(RuntimeError):
        call(None, 0, g=0)
    assert all(torch.equal(a, b) for a, b in zip(tables, before))          # refused before any launch


# ---- 3. the batched search is one search per prompt ------------------------------------------------------------------------------
KW = dict(beam_width=3, eos_id=13, max_length=24)
_runs = {}


def greedy_ids(m, tok, msk, frames):
    m.begin_ragged([(tok.to(DEV), msk.to(DEV))])
    return m.generate_frames(frames, 1, 1, skip_audio_experts=True)[:, 0, 0].cpu().tolist()


def search_runs(sd, golden, dtype):
    """(model, prompts, greedy ids before any search, one beam_search per prompt) — computed once per dtype and left unchanged."""
    if dtype not in _runs:
        prompts = four_prompts(golden)
        m = build_product_model(scaled_sd(sd, 8), dtype, batch=2 * len(prompts) * KW["beam_width"])
        before = greedy_ids(m, *prompts[1], 20)
        singles = [m.beam_search(t, k, **KW) for t, k in prompts]
        _runs[dtype] = (m, prompts, before, singles)
    return _runs[dtype]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_batched_search_equals_one_search_per_prompt(sd, golden, dtype):
    m, prompts, before, singles = search_runs(sd, golden, dtype)
    done = [all(h["finished"] for h in hyps) for _, _, hyps in singles]
    print(f"  {dtype}: finished slots per prompt {[sum(h['finished'] for h in hyps) for _, _, hyps in singles]}")
    assert any(done) and not all(done)          # a finished group runs on as a fixed point beside live ones
    base = m.beam_search_batch(prompts, **KW)
    info = list(m.beam_info_groups)
    assert base == singles                      # ids, fp32 scores, finished flags, every hypothesis
    assert len(info) == len(prompts) and all((i["all_finished"] >= 0) == d for i, d in zip(info, done))
    assert m.beam_search_batch(prompts, chunk_frames=1, **KW) == singles
    assert m.beam_search_batch(prompts, use_graph=False, **KW) == singles
    assert m.beam_search_batch(prompts, skip_audio_experts=False, **KW) == singles
    assert greedy_ids(m, *prompts[1], 20) == before                        # the page tables are restored, the beam state detached
    assert m._beam is None
    for g in (m.audio_understanding_expert, m.backbone, m.audio_generation_expert):
        pt = g.kv_cache.page_table
        assert torch.equal(pt.flatten(), torch.arange(pt.numel(), dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_order_of_the_prompts_does_not_matter(sd, golden, dtype):
    m, prompts, _, singles = search_runs(sd, golden, dtype)
    assert m.beam_search_batch(prompts[::-1], **KW) == singles[::-1]


# ---- 5. against the float64 rule over the CPU oracle -------------------------------------------------------------------------------
def test_batched_search_fp32_equals_the_rule_over_the_oracle(sd, golden):
    s, W, ml, eos = 8, 2, 12, 13
    prompts = four_prompts(golden)
    oracle = build_oracle(scaled_sd(sd, s), "fp32", batch=W)
    refs = [beam_ref.search(oracle, tok, msk, W, eos, max_length=ml) for tok, msk in prompts]
    m = build_product_model(scaled_sd(sd, s), torch.float32, batch=2 * len(prompts) * W)
    got = m.beam_search_batch(prompts, beam_width=W, max_length=ml, eos_id=eos)
    for g, (ref, (ids, score, hyps)) in enumerate(zip(refs, got)):
        steps = ref["steps"]
        tol = 2 * (5e-5 * s) * steps            # the project's fp32 logit bar (5e-5, x the lm_head factor), twice per step (logit and log-sum-exp)
        print(f"  prompt {g}: steps {steps}, oracle margins score / logit / final = " + " / ".join(f"{x:.3g}" for x in ref["margins"]) + f", tol {tol:.3g}")
        assert ref["margins"][0] >= tol and ref["margins"][2] >= tol and ref["margins"][1] >= 2 * 5e-5 * s and ref["margins"][1] >= tol
        worst = max(abs(h["score"] - b.score) for h, b in zip(hyps, ref["beam"]))
        print(f"  prompt {g}: worst score difference {worst:.3g}")
        assert [h["ids"] for h in hyps] == [b.ids for b in ref["beam"]]
        assert [h["finished"] for h in hyps] == [b.fin == FINISHED for b in ref["beam"]]
        assert worst <= tol
        assert ids == ref["beam"][ref["best"]].ids and score == hyps[ref["best"]]["score"]
        assert m.beam_info_groups[g]["steps"] >= steps


# ---- 6. checks -------------------------------------------------------------------------------------------------------------------
def test_plan_and_frame_checks_of_the_groups(sd, golden):
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import Ua2Error, check, lib
    tok, msk = asr1(golden)
    other = tiled_prompt(golden, 30)
    m = build_product_model(sd, torch.float32, batch=11)
    with pytest.raises(ValueError, match="max_batch_size=12"):            # 2 * G * W
        m.beam_search_batch([(tok, msk), other], beam_width=3)
    with pytest.raises(ValueError, match="beam_width"):
        m.beam_search_batch([(tok, msk)], beam_width=9)
    with pytest.raises(ValueError, match="64"):
        m.beam_search_batch([(tok, msk)] * 9, beam_width=8)
    with pytest.raises(ValueError):
        m.beam_search_batch([])
    assert m._beam is None
    m.begin_beams_groups([(tok, msk), other], beam_width=2, max_length=4)
    try:
        for bad_rows in (2, 3, 5):                                         # the C side refuses before any launch
            with pytest.raises(Ua2Error, match="one row per slot"):
                check(lib.ua2_stage3_frame(m._h, bad_rows, 3, -1, 0, 0, ops.stream()), "ua2_stage3_frame")
        with pytest.raises(ValueError, match="batch must be 4"):
            m.generate_frames(1, 2, 3)
        with pytest.raises(ValueError, match="step log full"):
            m.generate_frames(5, 4, 3)
        m.generate_frames(4, 4, 3)
    finally:
        out = m.end_beams_groups()
    assert len(out) == 2 and m._beam is None
    kw = dict(beam_width=2, max_length=4)
    assert out == [m.beam_search(tok, msk, **kw), m.beam_search(*other, **kw)]
    assert m.beam_search_batch([(tok, msk)], **kw) == [m.beam_search(tok, msk, **kw)]      # a single-element list is the single search
    with pytest.raises(Ua2Error, match="12 sequences"):                    # 2 G W beyond the plan: the executor refuses as well
        check(lib.ua2_stage3_set_beam_groups(m._h, 2, 3, 13, None, None, 0), "ua2_stage3_set_beam_groups")
