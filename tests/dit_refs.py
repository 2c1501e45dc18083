"""Float64 anchor of the flow-matching DiT step (Transformer1DModel + BasicTransformerBlock + ProjectLayer, composed of ua2_linear,
ua2_attn, ua2_ew_fma and ua2_layernorm_rows launches), used by tests/test_dit_refs_host.py and tests/test_gpu_dit_parity.py.

Same convention as tests/kernel_refs.py and tests/linear_refs.py: everything takes `dt`.  torch.float64 is the reference; torch.float32
evaluates the SAME contract in plain fp32 on the host, and its distance from the float64 result is the E_ref that sizes a stage's
bar, kr.bar(E_ref).  Errors are per element, divided by scale = max(1, max |ref64|) of the stage: one wrong row among hundreds
shows in full, where a relative RMS over the whole output divides it by the square root of the row count.

Stages (the `taps` of oracle/codec_model_oracle.py dit_forward and of Transformer1DModel.forward): 0 = the residual stream after
proj_in + positions, l + 1 = after block l, layers + 1 = the output.

Plans.  "fp32" is the oracle's formula (dit_contract hands it to the oracle's own functions: bit for bit dit_forward).  The bf16
plans round where include/ua2hip.h says the launches round: weights once to bf16 (ProjectLayer's k^-0.5 folded into the conv taps
and their bias in fp32 BEFORE that rounding, as ProjectLayer.prepare does); every GEMM operand once to bf16 (UA2_PRO_CAST rows, the
LayerNorm-modulated rows of UA2_PRO_NORM / the y_ln hand-over, the attention output, the GELU output); K and V stored in bf16; q and
the softmax weights by kr.ROUNDERS["split"] ("bf16_invariant", sum_order = 0) or ["bf16"] ("bf16_free", UA2_ATTN_BF16_QP); sums,
epilogues, the residual stream and the element-wise glue in `dt`.  The float32 evaluation of a bf16 plan differs from its float64
one mostly by operand elements that land on the other side of a bf16 rounding midpoint (2^-9 of one product each): E_ref of a bf16
plan measures exactly that entitlement, which is why it is ~1e-3 of scale where the fp32 plan's is ~3e-7.

One timestep for the whole batch, as solve_euler passes it and as the product's launches assume (one modulation vector per launch).
Nothing here is copied from a kernel; nothing here touches a device."""
import numpy as np
import torch
import torch.nn.functional as F

import dit_toy
import kernel_refs as kr
import linear_refs as lr
from oracle import codec_model_oracle as oc
from weights import seeded_tensor

F64, F32 = torch.float64, torch.float32
PLANS = ("fp32", "bf16_invariant", "bf16_free")
SUM_ORDER = {"bf16_invariant": 0, "bf16_free": 1}
ATTN_MODE = {"bf16_invariant": "split", "bf16_free": "bf16"}
MAX_POS = 3000                       # Transformer1DModel's num_positional_embeddings
EPS = 1e-6

# ---- cases --------------------------------------------------------------------------------------------------------------------

RELEASED = dict(heads=24, head_dim=64, layers=2, in_channels=1040, out_channels=136)     # models/model_config.json's widths, 2 of its 32 layers
CASES = {
    # M = 9 <= 16: the few-row route (no workspace, no packed hand-off)
    "few": dict(cfg=dit_toy.CFG, B=1, T=9, seed=5, x_seed=31, t=0.35),
    # 63 rows, three sequences: two inner boundaries + the buffer's end in ProjectLayer's flat [B (T + 2), C] GEMMs
    "odd": dict(cfg=dit_toy.CFG, B=3, T=21, seed=5, x_seed=32, t=0.6),
    # the shape and input of test_dit_forward_vs_oracle: one part-filled page, the last 16-row tile holds 10 of 74 rows
    "one-page": dict(cfg=dit_toy.CFG, B=2, T=37, seed=5, x_seed=9, t=0.35),
    # pages 64 + 64 + 20, two query groups per sequence (128 + 20 rows, the second padded with -1), 296 rows >= the order-free kernel's 256
    "three-page": dict(cfg=dit_toy.CFG, B=2, T=148, seed=5, x_seed=33, t=0.8),
    # the released instantiation of every launch (D = 1536 = 24 x 64, K = 6144 in FF2, in 1040: not a multiple of 32, out 136)
    "released": dict(cfg=RELEASED, B=2, T=148, seed=7, x_seed=34, t=0.45),
}
BF16_CASES = {"bf16_invariant": ("one-page", "three-page", "released"), "bf16_free": ("three-page", "released")}
_inputs = {}


def n_stages(cfg):
    return cfg["layers"] + 2


def stage_name(cfg, s):
    return "proj_in" if s == 0 else "out" if s == cfg["layers"] + 1 else f"block{s - 1}"


def case_inputs(name):
    """dict(cfg, B, T, sd, x (B, T, in) fp32, t): seeded weights (dit_toy.state_dict: fan-in scaled) and unit-variance input rows;
    everything that indexes is asserted in range here, on the host, before any launch sees it."""
    if name not in _inputs:
        c = CASES[name]
        cfg, B, T = c["cfg"], c["B"], c["T"]
        assert 1 <= T <= MAX_POS, "positions beyond the table"
        assert cfg["head_dim"] == 64 and cfg["heads"] * cfg["head_dim"] % 32 == 0
        assert 0.0 <= c["t"] <= 1.0
        sd = dit_toy.state_dict(c["seed"], cfg)
        x = seeded_tensor((B, T, cfg["in_channels"]), c["x_seed"], std=1.0)
        assert bool(torch.isfinite(x).all()) and all(bool(torch.isfinite(v).all()) for v in sd.values())
        _inputs[name] = dict(cfg=cfg, B=B, T=T, sd=sd, x=x, t=c["t"], name=name)
    return _inputs[name]


def check_plan(kv, B, T, heads):
    """The index-carrying tensors of a DenseKV plan, copied to the host and asserted in range: row tables, page table, query groups."""
    pages = (T + kr.PAGE - 1) // kr.PAGE
    assert kv.k.shape[0] == kv.v.shape[0] == B * pages and kv.k.shape[1:] == (heads, kr.PAGE, 64)
    table = kv.table.cpu().numpy()
    assert table.shape == (B, pages) and table.min() >= 0 and table.max() < kv.k.shape[0] and len(np.unique(table)) == table.size
    pos, seq, allp = kv.row_pos.cpu().numpy(), kv.row_seq.cpu().numpy(), kv.all_pos.cpu().numpy()
    assert np.array_equal(pos, np.tile(np.arange(T), B)) and np.array_equal(seq, np.repeat(np.arange(B), T))
    assert np.array_equal(allp, np.full(B * T, T - 1)) and (T - 1) // kr.PAGE < pages
    if kv.groups is not None:
        rows, gseq, nkeys, qt = kv.groups
        rows, gseq, nkeys = rows.cpu().numpy(), gseq.cpu().numpy(), nkeys.cpu().numpy()
        assert rows.shape[1] == 16 * qt and rows.min() >= -1 and rows.max() < B * T
        live = rows[rows >= 0]
        assert np.array_equal(np.sort(live), np.arange(B * T)), "every row in exactly one group"
        assert gseq.min() >= 0 and gseq.max() < B and bool((nkeys == T).all())
        for g in range(rows.shape[0]):
            r = rows[g][rows[g] >= 0]
            assert len(r) > 0 and bool((seq[r] == gseq[g]).all()), "a group mixes sequences"


# ---- K sums -------------------------------------------------------------------------------------------------------------------

def ksum_slabs4(a, w, dtype, dt=F64):
    """Another legal order of the K sum: the MFMA chunks dealt round-robin to four slabs, one left-to-right chain per slab, the slabs
    added last to first.  (float64: a matmul, as lr.ksum_ref.)"""
    if dt == F64:
        return lr.ksum_ref(a, w, dtype, dt)
    a, w = a.float(), w.float()
    c, K = lr.kc(dtype), a.shape[1]
    starts = list(range(0, K, c))
    slabs = []
    for s in range(4):
        acc = torch.zeros(a.shape[0], w.shape[0], dtype=F32)
        for k0 in starts[s::4]:
            acc = acc + a[:, k0:k0 + c] @ w[:, k0:k0 + c].t()
        slabs.append(acc)
    return ((slabs[3] + slabs[2]) + slabs[1]) + slabs[0]


# ---- the contract, stage by stage -----------------------------------------------------------------------------------------------

WRONG_KINDS = ("window", "positions", "zero_key", "gate", "final_ts")
WRONG_STAGE = {"window": 0, "positions": 0, "zero_key": 1, "gate": 1, "final_ts": -1}      # where the defect enters (-1: the output)
NEEDS_TWO_SEQUENCES = ("window", "positions")


class _Eval:
    """One evaluation of the contract: plan, dt, K-sum order and (for the wrong models) one planted defect."""

    def __init__(self, sd, heads, head_dim, plan, dt, ksum=None, defect=None):
        assert plan in PLANS and defect in (None,) + WRONG_KINDS
        self.sd, self.heads, self.hd, self.D = sd, heads, head_dim, heads * head_dim
        self.plan, self.dt, self.defect = plan, dt, defect
        self.ksum = ksum or lr.ksum_ref
        self.dtype = torch.float32 if plan == "fp32" else torch.bfloat16
        self.layers = oc.dit_layers(sd)

    def rnd(self, v):
        """A GEMM operand / a stored K or V element: once to bf16 under the bf16 plans."""
        if self.plan == "fp32":
            return v
        return lr.bf16_round64(v) if self.dt == F64 else kr.bf16_once(v)

    def gemm(self, a, W):
        """a [M, K] (already the operand) times W [N, K]^T, the weight as the plan holds it."""
        W = W.to(self.dt) if self.plan == "fp32" else lr.weights_ref(W, self.dtype, self.dt)
        return self.ksum(a, W, self.dtype, self.dt)

    def cast_linear(self, x, prefix):
        """A UA2_PRO_CAST / UA2_EPI_STORE launch over nn.Linear `prefix`."""
        return lr.store_ref(self.gemm(self.rnd(x.to(self.dt)), self.sd[prefix + "weight"]), self.sd[prefix + "bias"], self.dt)

    def project(self, prefix, x, k=3, next_first=None):
        """ProjectLayer (transformer_1d_flow.py:19-33): tap j of the k-tap conv reads frame t + j - k // 2 (zero outside the
        sequence), the taps accumulate, k^-0.5, Linear.  next_first (wrong model "window"): what the trailing pad frame holds."""
        dt = self.dt
        B, T, Cin = x.shape
        W, b = self.sd[prefix + "ffn_1.weight"], self.sd[prefix + "ffn_1.bias"]
        s = k ** -0.5
        xp = F.pad(x.to(dt), (0, 0, k // 2, k // 2))
        if next_first is not None:
            xp[:, T + k // 2:] = next_first.to(dt)
        y = None
        for j in range(k):
            if self.plan == "fp32":
                Wj, bj = W[:, :, j].to(dt) * s, b.to(dt) * s
            else:
                Wj, bj = W[:, :, j].float() * s, b.float() * s             # folded in fp32, then packed (rounded) as a weight
            sj = self.gemm(self.rnd(xp[:, j:j + T].reshape(B * T, Cin)), Wj)
            y = lr.store_ref(sj, bj, dt) if j == 0 else lr.residual_ref(sj, y, dt=dt)
        return self.cast_linear(y, prefix + "ffn_2.").view(B, T, -1)

    def timestep(self, t):
        """adaln_single.run: (ts [6 D], embedded timestep [D]) of the one timestep."""
        v = oc.timestep_embedding(torch.tensor([float(t)], dtype=F32)).to(self.dt)          # fp32 data of the formula, widened
        e = self.cast_linear(lr.silu_ref(self.cast_linear(v, "adaln_single.emb.timestep_embedder.linear_1.")), "adaln_single.emb.timestep_embedder.linear_2.")
        return self.cast_linear(lr.silu_ref(e), "adaln_single.linear.").view(-1), e.view(-1)

    def stage0(self, x):
        B, T, _ = x.shape
        nf = None
        if self.defect == "window":                       # the last frame's window runs on into the next sequence's first frame
            nf = torch.cat([x[1:, :1], torch.zeros_like(x[:1, :1])], 0)
        pe = oc.sinusoidal_pos_embed(B * T if self.defect == "positions" else T, self.D).to(self.dt)
        pe = pe.view(B, T, self.D) if self.defect == "positions" else pe[None]
        return self.project("proj_in.", x, next_first=nf) + pe

    def attention(self, q, k, v, B, T):
        """q [B T, D]; k, v [B T, D] as stored -> softmax(q k^T / 8) v, every row over the T frames of its sequence."""
        H, hd, dt = self.heads, self.hd, self.dt
        K = [k[b * T:(b + 1) * T].view(T, H, hd) for b in range(B)]
        V = [v[b * T:(b + 1) * T].view(T, H, hd) for b in range(B)]
        n = T
        if self.defect == "zero_key":                     # one all-zero slot after T - 1 is admitted too
            K = [torch.cat([t, torch.zeros(1, H, hd, dtype=dt)]) for t in K]
            V = [torch.cat([t, torch.zeros(1, H, hd, dtype=dt)]) for t in V]
            n = T + 1
        pos, seq = np.full(B * T, n - 1), np.repeat(np.arange(B), T)
        if self.plan == "fp32":
            return kr.attn_ref(q, K, V, pos, seq, H, H, dt=dt)
        return kr.attn_flash_model(q, K, V, pos, seq, H, H, ATTN_MODE[self.plan], 64, score_dt=dt, dt=dt)

    def block(self, i, h, ts):
        sd, dt, D = self.sd, self.dt, self.D
        B, T, _ = h.shape
        p = f"transformer_blocks.{i}."
        mod = sd[p + "scale_shift_table"].to(dt) + ts.view(6, D)                                # attention.py:308-310
        sh_a, sc_a, g_a, sh_m, sc_m, g_m = (mod[j] for j in range(6))
        if self.defect == "gate":
            g_m = g_a
        ln = lambda y, w, b: lr.operand_ref(y, lr.PRO_NORM, lr.NORM_LAYERNORM, w, b, EPS, self.dtype, dt)   # (y - mean) rstd w + b, rounded as an operand
        h = h.reshape(B * T, D).to(dt)
        Wqkv = torch.cat([sd[p + f"attn1.to_{c}.weight"] for c in "qkv"], 0)
        bqkv = torch.cat([sd[p + f"attn1.to_{c}.bias"] for c in "qkv"], 0)
        q, k, v = lr.store_ref(self.gemm(ln(h, 1 + sc_a, sh_a), Wqkv), bqkv, dt).split(D, dim=-1)   # :311-319
        o = self.attention(q, self.rnd(k), self.rnd(v), B, T)
        h = lr.residual_ref(self.gemm(self.rnd(o), sd[p + "attn1.to_out.0.weight"]), h, sd[p + "attn1.to_out.0.bias"], g_a, dt)      # :345-349
        f = lr.gelu_epi_ref(self.gemm(ln(h, 1 + sc_m, sh_m), sd[p + "ff.net.0.proj.weight"]), sd[p + "ff.net.0.proj.bias"], lr.GELU_TANH, dt)
        h = lr.residual_ref(self.gemm(self.rnd(f), sd[p + "ff.net.2.weight"]), h, sd[p + "ff.net.2.bias"], g_m, dt)                 # :401-405
        return h.view(B, T, D)

    def final(self, h, ts, e):
        dt, D = self.dt, self.D
        src = ts.view(6, D)[:2] if self.defect == "final_ts" else e[None]
        shift, scale = (self.sd["scale_shift_table"].to(dt) + src).unbind(0)                   # transformer_1d_flow.py:378
        hm = kr.layernorm_ref(h, None, None, 1e-6, dt) * (1 + scale) + shift                    # :379-381
        return self.project("proj_out.", hm)


@torch.no_grad()
def dit_contract(sd, x, t, heads, head_dim, plan, dt, start=None, stop=None, ksum=None, defect=None):
    """The DiT step under `plan` in `dt` -> the list of its stages (entries before `start` and after `stop` are None).
    start = (stage, h): evaluate from that tap onward — teacher forcing on a residual stream the caller supplies (the device's own).
    stop: the last stage wanted.  ksum: another K-sum order (ksum_slabs4).  defect: one of WRONG_KINDS (the wrong models).
    plan "fp32" without ksum / defect runs the oracle's own functions: the bits of oc.dit_forward for dt = float32."""
    layers = oc.dit_layers(sd)
    last = layers + 1
    stop = last if stop is None else stop
    taps = [None] * (last + 1)
    if plan == "fp32" and ksum is None and defect is None:
        sdt = {k: v.to(dt) for k, v in sd.items()}
        ts, emb = oc.dit_timestep(sdt, torch.full((x.shape[0],), float(t), dtype=F32), dt)
        stage0 = lambda: oc.project_layer(sdt, "proj_in.", x.to(dt)) + oc.sinusoidal_pos_embed(x.shape[1], heads * head_dim).to(dt)[None]
        block = lambda i, h: oc.dit_block(sdt, i, h, ts, heads, head_dim, dt, EPS)
        final = lambda h: oc.dit_final(sdt, h, emb)
    else:
        ev = _Eval(sd, heads, head_dim, plan, dt, ksum, defect)
        ts, emb = ev.timestep(t)
        stage0, block, final = (lambda: ev.stage0(x)), (lambda i, h: ev.block(i, h, ts)), (lambda h: ev.final(h, ts, emb))
    if start is None:
        s, h = 0, stage0()
    else:
        s, h = start[0], start[1].detach().cpu().to(dt)
        assert 0 <= s <= layers and h.shape == (x.shape[0], x.shape[1], heads * head_dim)
    taps[s] = h
    while s < stop:
        h = block(s, h) if s < layers else final(h)
        s += 1
        taps[s] = h
    return taps


def wrong_model(kind, case):
    """The float64 formula with one planted defect, up to the stage where it enters -> (stage, tensor)."""
    c = case
    s = WRONG_STAGE[kind] if WRONG_STAGE[kind] >= 0 else c["cfg"]["layers"] + 1
    taps = dit_contract(c["sd"], c["x"], c["t"], c["cfg"]["heads"], c["cfg"]["head_dim"], "fp32", F64, stop=s, defect=kind)
    return s, taps[s]


# ---- cached references ----------------------------------------------------------------------------------------------------------

_refs = {}


def reference(name, plan, dt, ksum=None, x=None, t=None, key=None):
    """All stages of case `name` under `plan` in `dt`, from the input; computed once per process and never modified (x, t, key:
    another input of the same shape, cached under `key`)."""
    k = (name, plan, dt, getattr(ksum, "__name__", None), key)
    if k not in _refs:
        c = case_inputs(name)
        _refs[k] = dit_contract(c["sd"], c["x"] if x is None else x, c["t"] if t is None else t, c["cfg"]["heads"], c["cfg"]["head_dim"],
                                plan, dt, ksum=ksum)
    return _refs[k]


# ---- judgement ------------------------------------------------------------------------------------------------------------------

def stage_err(got, ref64):
    """(err, (sequence, frame, column) of the worst element): per-element max |got - ref64| / max(1, max |ref64|); an element that is
    not finite is an error of inf."""
    got, ref64 = got.detach().cpu().to(F64), ref64.to(F64)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    scale = max(1.0, float(ref64.abs().max()))
    d = (got - ref64).abs()
    d = torch.where(torch.isfinite(got), d, torch.full_like(d, float("inf")))
    i = int(d.argmax())
    where = tuple(int(v) for v in np.unravel_index(i, tuple(d.shape)))
    return float(d.reshape(-1)[i]) / scale, where


def judge(case, stage, got, ref64, ref32):
    """(err, E_ref, bar) of one stage, printed as a PARITY line with the (sequence, frame) of the worst element.  The caller asserts
    err <= bar after it has judged every stage, so that a failing run still shows them all."""
    err, where = stage_err(got, ref64)
    e_ref, _ = stage_err(ref32, ref64)
    b = kr.bar(e_ref)
    print(f"PARITY dit {case} {stage}: err {err:.3e} E_ref {e_ref:.3e} bar {b:.3e} err/bar {err / b:.3f} worst at sequence {where[0]} frame {where[1]}")
    return err, e_ref, b
