"""Plain restatements of the row-wise kernels, used by tests/test_gpu_attn_decode.py (whose inputs and wrong models are in
tests/attn_decode_cases.py), tests/test_gpu_attn_flash_parity.py and tests/test_gpu_rowwise.py (and, through tests/encoder_refs.py, by
tests/test_gpu_encoder_parity.py).

Every helper takes `dt`: torch.float64 is the reference a kernel is compared with; torch.float32 evaluates the SAME formula in
plain fp32 on the host, whose error against the float64 result (`E_ref`) sizes the bar of a tolerance test:
bar = max(4 * E_ref, 8 * 2^-24 * scale) (two legal fp32 summation orders differ by about twice the single-order error, and the
kernels' exp / tanh / rsqrt are good to 1-2 ulp; the floor because E_ref can be exactly 0 on short rows).
tests/test_kernel_refs.py pins each helper to the torch library function it restates (CPU, float64, rtol 1e-12).
attn_flash_model is no reference but a host model of the MFMA flash form's arithmetic contract (16-bit or bf16 q and weights,
blocked online softmax): its error against attn_ref sizes the flash bars, which a plain fp32 evaluation would set ~10x too tight.
All helpers are vectorised over rows and heads."""
import math

import numpy as np
import torch

PAGE = 64
F64 = torch.float64


def bar(e_ref, scale=1.0):
    return max(4.0 * float(e_ref), 8.0 * 2.0 ** -24 * float(scale))


# ---- paged caches -----------------------------------------------------------------------------------------------------------

def page_slot(p, ring_pages):
    lp = p // PAGE
    return lp % ring_pages if ring_pages > 0 else lp


class PagedCache:
    """Paged K / V cache on the host: pools [pages, n_kv, 64, hs] of `dtype`, a scattered page table [B, max_pages].
    ring_pages > 0 (a power of two): position p lives in table column (p // 64) % ring_pages, and only the positions a sequence
    of length L still holds (those whose page was not overwritten by a later one) are materialised.  K[b], V[b]: the values of
    every position as drawn (fp32); stored(b, p) returns what the pool holds at the slot of position p, widened to float64."""

    def __init__(self, lens, n_kv, hs, dtype, seed=0, ring_pages=0, K=None, V=None, fill=0.0, extra_pages=0):
        g = torch.Generator().manual_seed(seed)
        self.lens, self.n_kv, self.hs, self.dtype, self.ring_pages = list(lens), n_kv, hs, dtype, ring_pages
        B = len(lens)
        self.max_pages = ring_pages if ring_pages > 0 else (max(lens) + PAGE - 1) // PAGE
        n_pages = B * self.max_pages + extra_pages
        self.table = torch.randperm(n_pages, generator=g)[:B * self.max_pages].to(torch.int32).view(B, self.max_pages)
        self.k = torch.full((n_pages, n_kv, PAGE, hs), fill, dtype=dtype)
        self.v = torch.full((n_pages, n_kv, PAGE, hs), fill, dtype=dtype)
        self.K = K if K is not None else [torch.randn(L, n_kv, hs, generator=g) for L in lens]
        self.V = V if V is not None else [torch.randn(L, n_kv, hs, generator=g) for L in lens]
        for b, L in enumerate(lens):
            ps = self.held(b)
            pg = self.table[b, page_slot(ps, ring_pages)].long()
            self.k[pg, :, ps % PAGE] = self.K[b][ps].to(dtype)
            self.v[pg, :, ps % PAGE] = self.V[b][ps].to(dtype)
        assert int(self.table.min()) >= 0 and int(self.table.max()) < n_pages

    def held(self, b):
        """Positions of sequence b the pool holds."""
        L = self.lens[b]
        first = 0 if self.ring_pages == 0 else max(0, ((L - 1) // PAGE - self.ring_pages + 1) * PAGE)
        return torch.arange(first, L)

    def stored(self, b, ps):
        ps = torch.as_tensor(ps)
        pg = self.table[b, page_slot(ps, self.ring_pages)].long()
        return self.k[pg, :, ps % PAGE].to(F64), self.v[pg, :, ps % PAGE].to(F64)

    def stored_seq(self, b):
        """(K, V) [L, n_kv, hs] float64 as stored; positions the ring no longer holds are NaN (a reference must not touch them)."""
        L = self.lens[b]
        K = torch.full((L, self.n_kv, self.hs), float("nan"), dtype=F64)
        V = K.clone()
        ps = self.held(b)
        K[ps], V[ps] = self.stored(b, ps)
        return K, V


def attn_ref(q, K, V, pos, seq, n_head, n_kv, window=0, dt=F64, score_bias=None, q_prescaled=False):
    """softmax(q k^T / sqrt(hs)) v over keys max(0, pos + 1 - window) .. pos of the row's sequence.  q [R, n_head * hs];
    K, V: per sequence [L, n_kv, hs], the values actually stored (already rounded to the cache dtype); pos, seq [R] ints.
    score_bias(rows, keys) -> [r, n_kv, G, l] in `dt` (rows: indices into the launch's rows, keys: positions) is added to the
    scores before the mask; q_prescaled: q already carries 1 / sqrt(hs) (tests/encoder_refs.py: ua2_attn_relbias)."""
    q = torch.as_tensor(q).to(dt)
    pos, seq = np.asarray(pos, dtype=np.int64), np.asarray(seq, dtype=np.int64)
    R, G = q.shape[0], n_head // n_kv
    hs = q.shape[1] // n_head
    out = torch.zeros(R, n_head * hs, dtype=dt)
    for b in np.unique(seq):
        rows = np.nonzero(seq == b)[0]
        p = torch.from_numpy(pos[rows])
        n = int(p.max()) + 1
        lo = torch.clamp(p + 1 - window, min=0) if window > 0 else torch.zeros_like(p)
        first = int(lo.min())
        Kb, Vb = K[b][first:n].to(dt), V[b][first:n].to(dt)                        # [n', n_kv, hs]
        qb = q[rows].view(len(rows), n_kv, G, hs)
        s = torch.einsum("rkgd,lkd->rkgl", qb, Kb)
        if not q_prescaled:
            s = s / math.sqrt(hs)
        key = torch.arange(first, n)
        if score_bias is not None:
            s = s + score_bias(rows, key).to(dt)
        vis = (key[None, :] <= p[:, None]) & (key[None, :] >= lo[:, None])         # [r, n']
        s = s.masked_fill(~vis[:, None, None, :], float("-inf"))
        w = torch.softmax(s, dim=-1)
        Vz = torch.where(torch.isnan(Vb), torch.zeros_like(Vb), Vb)                # slots no row may see carry weight 0
        assert not bool(torch.isnan(torch.where(vis[:, None, None, :], s, torch.zeros_like(s))).any()), "a visible key is not stored"
        out[rows] = torch.einsum("rkgl,lkd->rkgd", w, Vz).reshape(len(rows), n_head * hs)
    return out


# ---- glue kernels -----------------------------------------------------------------------------------------------------------

def rmsnorm_blend_ref(x, w, eps, other=None, mask=None, col_a=-1, col_b=-1, dt=F64):
    """n = x * rsqrt(mean(x^2) + eps) * w; out1 = n * fa + other * fb (fa = mask[:, col_a] or 1; fb = mask[:, col_b] with `other`)."""
    x, w = x.to(dt), w.to(dt)
    n = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps) * w
    out1 = n * mask[:, col_a:col_a + 1].to(dt) if col_a >= 0 else n.clone()
    if other is not None:
        out1 = out1 + other.to(dt) * mask[:, col_b:col_b + 1].to(dt)
    return out1, n


def layernorm_ref(x, w=None, b=None, eps=1e-5, dt=F64):
    x = x.to(dt)
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    y = d * torch.rsqrt((d * d).mean(-1, keepdim=True) + eps)
    if w is not None:
        y = y * w.to(dt)
    if b is not None:
        y = y + b.to(dt)
    return y


def embed_frame_ref(tokens, mask, audio_emb, wte, va, dt=F64):
    """audio_sum = sum_i mask[:, i] * audio_emb[tok[:, i] + i * va] added in the order i = 0 .. n_cb - 1; text = wte[tok[:, n_cb]]."""
    tokens = tokens.long()
    ncb = tokens.shape[1] - 1
    s = torch.zeros(tokens.shape[0], audio_emb.shape[1], dtype=dt)
    for i in range(ncb):
        e = audio_emb[tokens[:, i] + i * va].to(dt)
        s = s + torch.where(mask[:, i:i + 1] != 0, e, torch.zeros_like(e))
    return s, wte[tokens[:, ncb]].to(dt)


def cfg_mix_ref(l0, l1, scale, dt=F64):
    """guided = l1 + (l0 - l1) * scale, every operation rounded once in `dt`."""
    l0, l1 = l0.to(dt), l1.to(dt)
    return l1 + (l0 - l1) * torch.tensor(scale, dtype=torch.float32).to(dt)


def argmax_partials(row, forbid=0):
    """Per-16-column (max, arg-max) of a 1-D fp32 row: lowest index on ties, columns < forbid excluded, a group without an
    admitted column = (-inf, its first column)."""
    row = np.asarray(row, dtype=np.float32)
    V = row.shape[0]
    nb = (V + 15) // 16
    pad = np.full(nb * 16, -np.inf, dtype=np.float32)
    pad[:V] = row
    pad[:min(forbid, V)] = -np.inf
    g = pad.reshape(nb, 16)
    idx = g.argmax(1)                                   # numpy: first occurrence
    return g.max(1), (idx + 16 * np.arange(nb)).astype(np.int32)


def time_film_ref(params, x, batch_mask, rows_per_batch, gamma_scale, dt=F64):
    C = x.shape[1]
    p, x = params.to(dt), x.to(dt)
    gamma = 1.0 + gamma_scale * torch.tanh(p[:, :C])
    beta = p[:, C:]
    out = gamma * x + beta
    if batch_mask is not None:
        masked = batch_mask.bool()[torch.arange(x.shape[0]) // rows_per_batch]
        out = torch.where(masked[:, None], x, out)
    return out


def ew_act_ref(x, act, dt=F64):
    x = x.to(dt)
    return {1: lambda v: v / (1.0 + torch.exp(-v)), 2: lambda v: 1.0 / (1.0 + torch.exp(-v)), 3: torch.tanh}[act](x)


def rotate_half(x):
    x1, x2 = x[..., :x.shape[-1] // 2], x[..., x.shape[-1] // 2:]
    return torch.cat((-x2, x1), dim=-1)


def qknorm_rope_ref(qkv, pos, n_head, hs, qw=None, qb=None, kw=None, kb=None, eps=1e-5, cos=None, sin=None, rot_dim=0, dt=F64):
    """qkv [R, 3 * n_head * hs] = (q | k | v): LayerNorm over the head dim with affine on q and k (when weights are given), then
    rotate-half rotary on the first rot_dim dims with freqs = cat(f, f) (cos / sin [max_pos, rot_dim / 2]) -> q, k, v [R, n_head, hs]."""
    R = qkv.shape[0]
    q, k, v = (t.reshape(R, n_head, hs) for t in qkv.to(dt).chunk(3, dim=-1))
    if qw is not None:
        q = layernorm_ref(q, qw, qb, eps, dt)
        k = layernorm_ref(k, kw, kb, eps, dt)
    if rot_dim > 0:
        p = torch.as_tensor(pos).long()
        c = torch.cat((cos[p], cos[p]), -1).to(dt)[:, None, :]
        s = torch.cat((sin[p], sin[p]), -1).to(dt)[:, None, :]

        def rot(t):
            a, rest = t[..., :rot_dim], t[..., rot_dim:]
            return torch.cat((a * c + rotate_half(a) * s, rest), -1)
        q, k = rot(q), rot(k)
    return q, k, v


def dwconv_ref(x, w, bias=None, *, stride=1, dilation=1, pad_left=0, Tout=None, transposed=False, dt=F64):
    """Depthwise conv: y[b,c,t] = bias[c] + sum_j w[c,j] x[b,c, t*stride + j*dilation - pad_left] (zero outside);
    transposed: y[b,c,t] = bias[c] + sum_{ti*stride + j == t + pad_left} w[c,j] x[b,c,ti].  Written index by index over the taps
    (not through F.conv1d, which tests/test_kernel_refs.py compares it with)."""
    x, w = x.to(dt), w.to(dt)
    B, C, Tin = x.shape
    K = w.shape[1]
    y = torch.zeros(B, C, Tout, dtype=dt)
    t = torch.arange(Tout)
    for j in range(K):
        if not transposed:
            ti = t * stride + j * dilation - pad_left
            ok = (ti >= 0) & (ti < Tin)
        else:
            r = t + pad_left - j
            ok = (r >= 0) & (r % stride == 0) & (r // stride < Tin)
            ti = r // stride
        y[:, :, t[ok]] += w[None, :, j:j + 1] * x[:, :, ti[ok]]
    if bias is not None:
        y = y + bias.to(dt)[None, :, None]
    return y


# ---- the flash (prefill / dense) form: a host model of its arithmetic contract, hostile inputs, the packed layout ---------------

def bf16_round(x):
    """RNE to bf16 of an fp32 tensor, as fp32."""
    return x.float().to(torch.bfloat16).float()


def bf16_once(x):
    """RNE to bf16, returned in the dtype it came in."""
    return x.to(torch.bfloat16).to(x.dtype)


def split16_round(x):
    """hi = bf16(x), lo = bf16(x - hi); the value used is hi + lo (16 significant bits)."""
    hi = bf16_once(x)
    return hi + bf16_once(x - hi)


ROUNDERS = {"split": split16_round, "bf16": bf16_once, "fp32": lambda x: x}


def causal_visible(key, pos):
    return key <= pos


def attn_flash_model(q, K, V, pos, seq, n_head, n_kv, mode, keys_per_step=64, score_dt=torch.float32, dt=torch.float32,
                     visible=causal_visible, score_bias=None, q_prescaled=False):
    """The arithmetic contract of attn_flash_kernel (header comment in csrc/ua2_attn.hip), nothing of its lane layout:
    q * log2(e) / sqrt(hs) in fp32, rounded by `mode` ("split": 16 significant bits as bf16 hi + lo; "bf16": one bf16; "fp32":
    left alone); scores accumulated in `score_dt` and handed on in `dt`; keys visited in steps of `keys_per_step` with the running
    max / alpha / l recurrence on exp2; masked keys contribute exact zeros; l sums the unrounded weights; the weights entering
    P V are rounded by `mode`; O accumulates in `dt`.  dt = score_dt = float64 with mode "fp32" is attn_ref in another order.
    mode may be a pair (q rounder, p rounder) of names or callables, and `visible(key, pos)` another mask: the hooks with which
    tests/test_kernel_refs.py builds deliberately wrong models.  score_bias(rows, keys) -> [r, n_kv, G, l] in `dt`, already in
    the log2 domain, is added to the handed-on scores with one rounding before the mask; q_prescaled: q carries 1 / sqrt(hs)
    already and is scaled by log2(e) alone (both: the contract of attn_relbias_flash_kernel, tests/encoder_refs.py)."""
    rq, rp = (mode, mode) if isinstance(mode, str) else mode
    rq, rp = ROUNDERS.get(rq, rq) if isinstance(rq, str) else rq, ROUNDERS.get(rp, rp) if isinstance(rp, str) else rp
    q = torch.as_tensor(q).to(dt)
    pos, seq = np.asarray(pos, dtype=np.int64), np.asarray(seq, dtype=np.int64)
    R, G = q.shape[0], n_head // n_kv
    hs = q.shape[1] // n_head
    sc = torch.tensor(1.44269504088896340736, dtype=dt)
    if not q_prescaled:
        sc = sc / torch.sqrt(torch.tensor(float(hs), dtype=dt))
    qs = rq(q * sc)
    ninf = float("-inf")
    out = torch.zeros(R, n_head * hs, dtype=dt)
    for b in np.unique(seq):
        rows = np.nonzero(seq == b)[0]
        p = torch.from_numpy(pos[rows])
        n = int(p.max()) + 1
        Kb, Vb = K[b][:n], V[b][:n]
        Vb = torch.where(torch.isnan(Vb), torch.zeros_like(Vb), Vb).to(dt)
        qb = qs[rows].view(len(rows), n_kv, G, hs)
        s_all = torch.einsum("rkgd,lkd->rkgl", qb.to(score_dt), Kb.to(score_dt)).to(dt)
        if score_bias is not None:
            s_all = s_all + score_bias(rows, torch.arange(n)).to(dt)
        vis = visible(torch.arange(n)[None, :], p[:, None])                               # [r, n]
        assert not bool(torch.isnan(torch.where(vis[:, None, None, :], s_all, torch.zeros_like(s_all))).any()), "a visible key is not stored"
        s_all = s_all.masked_fill(~vis[:, None, None, :], ninf)
        m = torch.full(s_all.shape[:3], ninf, dtype=dt)
        l = torch.zeros_like(m)
        o = torch.zeros(*m.shape, hs, dtype=dt)
        for k0 in range(0, n, keys_per_step):
            s = s_all[..., k0:k0 + keys_per_step]
            m_new = torch.maximum(m, s.amax(-1))
            dead = m_new == ninf
            alpha = torch.where(dead, torch.ones_like(m), torch.exp2(m - torch.where(dead, torch.zeros_like(m), m_new)))
            pv = torch.where(s == ninf, torch.zeros_like(s), torch.exp2(s - torch.where(dead, torch.zeros_like(m), m_new)[..., None]))
            l = l * alpha + pv.sum(-1)
            o = o * alpha[..., None] + torch.einsum("rkgl,lkd->rkgd", rp(pv), Vb[k0:k0 + keys_per_step])
            m = m_new
        out[rows] = (o * (1.0 / l)[..., None]).reshape(len(rows), n_head * hs)
    return out


def rel_row_err(y, ref):
    """max |y - ref| relative to each row's max magnitude; an unwritten (NaN) or non-finite element is an error of inf."""
    y = y.detach().cpu().to(F64)
    if not bool(torch.isfinite(y).all()):
        return float("inf")
    scale = ref.abs().amax(dim=1, keepdim=True).clamp_min(1e-30)
    return float(((y - ref).abs() / scale).max())


def abs_err(y, ref):
    y = y.detach().cpu().to(F64)
    return float((y - ref).abs().max()) if bool(torch.isfinite(y).all()) else float("inf")


HOSTILE_LENS = [3, 40, 130, 300]
HOSTILE_KINDS = ["peaked_q", "dominant_key-k128", "dominant_key-k63", "dominant_key-k64", "dominant_key-last", "wide_v", "equal_keys",
                 "rising_max", "falling_max"]
RAMP = 140.0          # span of the rising / falling score ramp in natural units (202 in log2 units: past the underflow of exp2)


def all_rows(lens, seed=None, dense=False):
    """(pos, seq) int32: one query row per position of every sequence (dense: every row at the last position), shuffled by `seed`."""
    pos = np.concatenate([np.full(L, L - 1) if dense else np.arange(L) for L in lens]).astype(np.int32)
    seq = np.concatenate([np.full(L, b) for b, L in enumerate(lens)]).astype(np.int32)
    if seed is not None:
        perm = np.random.default_rng(seed).permutation(len(pos))
        pos, seq = pos[perm], seq[perm]
    return pos, seq


def hostile_inputs(kind, n_head, n_kv, hs, lens=HOSTILE_LENS, seed=13):
    """Hostile but finite inputs (K, V per sequence as drawn, q, pos, seq), every position a query row.  peaked_q: q x 8 (scores of
    +-100); dominant_key-<where>: one key x 10 at position 128 (slot 0 of a block and of a pair of blocks), 63, 64 (each clamped
    to the sequence) or the last position; wide_v: V entries of +-1e4 next to 1e-4; equal_keys: runs of four identical keys (ties
    in the running max); rising_max / falling_max: a common direction d added to q and d * linspace(0, c, L) (reversed: c .. 0) to
    the keys, c = RAMP / sqrt(hs): the block maximum rises at every step and rescales everything accumulated so far towards
    zero / the maximum sits in block 0 and the later weights run down past the underflow of exp2."""
    g = torch.Generator().manual_seed(seed)
    K = [torch.randn(L, n_kv, hs, generator=g) for L in lens]
    V = [torch.randn(L, n_kv, hs, generator=g) for L in lens]
    pos, seq = all_rows(lens, seed=4)
    q = torch.randn(len(pos), n_head * hs, generator=g)
    if kind == "peaked_q":
        q = q * 8.0
    elif kind.startswith("dominant_key"):
        where = kind.split("-")[1]
        for k in K:
            k[len(k) - 1 if where == "last" else min(int(where[1:]), len(k) - 1)] *= 10.0
    elif kind == "wide_v":
        for v in V:
            mag = torch.where(torch.rand(v.shape, generator=g) < 0.5, torch.tensor(1e4), torch.tensor(1e-4))
            v.copy_(torch.sign(v) * mag)
    elif kind == "equal_keys":
        for k in K:
            k[1:] = k[1:][(torch.arange(len(k) - 1) // 4) * 4 % max(len(k) - 1, 1)]
    elif kind in ("rising_max", "falling_max"):
        d = torch.where(torch.rand(hs, generator=g) < 0.5, -1.0, 1.0)
        q = (q.view(-1, n_head, hs) + d).reshape(-1, n_head * hs)
        for k in K:
            t = torch.linspace(0.0, RAMP / math.sqrt(hs), len(k))
            k += (t.flip(0) if kind == "falling_max" else t)[:, None, None] * d
    else:
        raise ValueError(kind)
    return K, V, q, pos, seq


def packed_index(m, k, K, dtype):
    """Element (row m, column k) of an [M, K] operand in ua2_linear's operand order [ceil(M/16)][K / KC][64 lanes][EPL]
    (csrc/ua2_common.h store_packed_operand): k = c * KC + g * EPL + e lies at (((m >> 4) * (K / KC) + c) * 64 + g * 16 + (m & 15)) * EPL + e."""
    KC, EPL = (32, 8) if dtype == torch.bfloat16 else (16, 4)
    c, r = k // KC, k % KC
    g, e = r // EPL, r % EPL
    return (((m >> 4) * (K // KC) + c) * 64 + g * 16 + (m & 15)) * EPL + e


def decode_packed(pk, R, K, dtype):
    """The first R rows [R, K] of a packed operand (the same layout as packed_index, written as a view)."""
    KC, EPL = (32, 8) if dtype == torch.bfloat16 else (16, 4)
    t = pk.view(-1, K // KC, KC // EPL, 16, EPL)                      # [tile, c, g, m & 15, e]
    return t.permute(0, 3, 1, 2, 4).reshape(-1, K)[:R]


def encode_packed(y, dtype, fill, index=packed_index):
    """Host image of a packed operand: the rows of y [R, K] rounded to `dtype` at index(m, k, K, dtype), `fill` elsewhere."""
    R, K = y.shape
    pk = torch.full(((R + 15) // 16 * 16 * K,), fill, dtype=dtype)
    m, k = torch.meshgrid(torch.arange(R), torch.arange(K), indexing="ij")
    pk[index(m, k, K, dtype).reshape(-1)] = y.to(dtype).reshape(-1)
    return pk


def packed_mismatch(pk, y, R, K, dtype, fill):
    """Why a packed buffer is not (the R rows of y rounded RNE to `dtype`, bit for bit, then rows of `fill`); None if it is."""
    bits = lambda t: t.contiguous().view(torch.int16 if dtype == torch.bfloat16 else torch.int32)
    pk, y = pk.detach().cpu(), y.detach().cpu()
    full = decode_packed(pk, (R + 15) // 16 * 16, K, dtype)
    if not torch.equal(bits(full[:R]), bits(y.to(dtype))):
        return "a live element differs from the row-major output"
    if not torch.equal(bits(full[R:]), bits(torch.full_like(full[R:], fill))):
        return "a row beyond R was written"
    return None
