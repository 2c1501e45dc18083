"""Inputs of tests/test_gpu_attn_decode.py (the row-by-row form of ua2_attn), built on the host so that tests/test_kernel_refs.py
judges the very tensors the device sees: the ragged parity batch, the position lists, the hostile generators, and
decode_wrong_model — the float64 reference with ONE deliberate defect, which the host test shows the decode bar rejects.
Everything here is finite; nothing here touches a device."""
import math

import numpy as np
import torch

import kernel_refs as kr

F64 = torch.float64
LOUD = 3.0e4                # what every slot no row may read holds (finite: nothing non-finite goes to a kernel)
EXTRA_PAGES = 4             # pool pages no table names, of the same loud value
LENS = [1, 2, 7, 8, 9, 31, 63, 64, 65, 127, 128, 129, 200, 535, 2047]
LONG_LENS = [4097, 8191]
HOSTILE_LENS = kr.HOSTILE_LENS          # [3, 40, 130, 300]
HOSTILE_KINDS = ["peaked_q", "dominant_key", "wide_v", "equal_keys", "rising", "falling", "zero_q", "common_offset"]
RAMP = 140.0                # span of the rising / falling score ramp in natural units (past the underflow of exp2: 87)
OFFSET = 90.0               # common score term of common_offset in natural units (exp(90) overflows fp32)


def positions(L):
    """Every position of a short sequence; first, last and the page-edge positions 64k - 1, 64k, 64k + 1 of a long one."""
    if L <= 129:
        return np.arange(L)
    edge = [p for k in range(1, (L + 63) // 64 + 1) for p in (64 * k - 1, 64 * k, 64 * k + 1)]
    return np.unique([p for p in [0, L - 1] + edge if 0 <= p < L])


def long_positions(L):
    """First, last, and 64k - 1, 64k, 64k + 1 for k in {1, 2, 63, 64, 65, 127} where the sequence holds them."""
    edge = [p for k in (1, 2, 63, 64, 65, 127) for p in (64 * k - 1, 64 * k, 64 * k + 1)]
    return np.unique([p for p in [0, L - 1] + edge if 0 <= p < L])


def rows(lens, positions, seed, shuffle=True):
    pos = np.concatenate([positions(L) for L in lens]).astype(np.int32)
    seq = np.concatenate([np.full(len(positions(L)), b) for b, L in enumerate(lens)]).astype(np.int32)
    if shuffle:
        perm = np.random.default_rng(seed).permutation(len(pos))
        pos, seq = pos[perm], seq[perm]
    return pos, seq


def check_indices(cache, pos, seq):
    """Index-carrying inputs are asserted in range on the host before any launch."""
    assert len(pos) == len(seq) and seq.min() >= 0 and seq.max() < len(cache.lens)
    assert pos.min() >= 0 and bool((pos < np.asarray(cache.lens)[seq]).all())
    n_pages = cache.k.shape[0]
    assert int(cache.table.min()) >= 0 and int(cache.table.max()) < n_pages
    if cache.ring_pages == 0:
        assert int(pos.max()) // 64 < cache.max_pages


def linear_cache(lens, n_kv, hs, dtype, seed, K=None, V=None):
    """A linear cache as every decode test builds it: unused slots and EXTRA_PAGES unnamed pages hold LOUD."""
    return kr.PagedCache(lens, n_kv, hs, dtype, seed=seed, K=K, V=V, fill=LOUD, extra_pages=EXTRA_PAGES)


def stored(cache):
    KV = [cache.stored_seq(b) for b in range(len(cache.lens))]
    return [k for k, _ in KV], [v for _, v in KV]


def parity_inputs(dtype, nh, nkv, hs):
    """test_decode_attention_parity: 15 ragged sequences of 1 .. 2047 keys, 766 rows, shuffled -> (cache, q, pos, seq)."""
    cache = linear_cache(LENS, nkv, hs, dtype, seed=nh * 1000 + hs)
    pos, seq = rows(LENS, positions, seed=1)
    q = torch.randn(len(pos), nh * hs, generator=torch.Generator().manual_seed(hs + nh))
    return cache, q, pos, seq


def unit_err(y, ref, ref32=None):
    """(err, E_ref, bar) of a unit-scale launch: absolute errors divided by scale = max(1, max |ref|)."""
    scale = max(1.0, float(ref.abs().max()))
    err = kr.abs_err(y, ref) / scale
    e_ref = kr.abs_err(ref32, ref) / scale if ref32 is not None else 0.0
    return err, e_ref, kr.bar(e_ref)


def hostile_inputs(kind, nh, nkv, hs, lens=HOSTILE_LENS, seed=13):
    """Hostile but finite (K, V per sequence as drawn, q, pos, seq), every position a query row.
    peaked_q: q x 8 (a peaked soft-max); dominant_key: the middle key x 10; wide_v: V entries of +-1e4 next to 1e-4; equal_keys:
    runs of four identical keys (ties in the running max);
    rising / falling: K = t * d + 0.01 randn for one sign vector d, t = linspace(0, RAMP / sqrt(hs), L) (falling: reversed), and d
    added to q: a row's scores rise (fall) with position by RAMP / L per key, so every step of every row group moves the running
    maximum (the maximum is set at the first key and the last weights underflow);
    zero_q: q = 0, every weight equal: the result is the plain mean of the visible V rows;
    common_offset: K = 20 u + 0.1 randn for one unit vector u per kv head, and q = randn + OFFSET / 20 * sqrt(hs) * u: every score
    of a row carries the common term OFFSET (exp(OFFSET) overflows fp32) and only the soft-max of the remainder, of spread about
    0.5, is the answer: the maximum must be subtracted before the exponentials."""
    g = torch.Generator().manual_seed(seed)
    K = [torch.randn(L, nkv, hs, generator=g) for L in lens]
    V = [torch.randn(L, nkv, hs, generator=g) for L in lens]
    pos, seq = rows(lens, np.arange, seed=4)
    q = torch.randn(len(pos), nh * hs, generator=g)
    if kind == "peaked_q":
        q = q * 8.0
    elif kind == "dominant_key":
        for k in K:
            k[len(k) // 2] *= 10.0
    elif kind == "wide_v":
        for v in V:
            mag = torch.where(torch.rand(v.shape, generator=g) < 0.5, torch.tensor(1e4), torch.tensor(1e-4))
            v.copy_(torch.sign(v) * mag)
    elif kind == "equal_keys":
        for k in K:
            k[1:] = k[1:][(torch.arange(len(k) - 1) // 4) * 4 % max(len(k) - 1, 1)]      # runs of four identical keys
    elif kind in ("rising", "falling"):
        d = torch.where(torch.rand(hs, generator=g) < 0.5, -1.0, 1.0)
        q = (q.view(-1, nh, hs) + d).reshape(-1, nh * hs)
        for k in K:
            t = torch.linspace(0.0, RAMP / math.sqrt(hs), len(k))
            k.copy_(0.01 * k + (t.flip(0) if kind == "falling" else t)[:, None, None] * d)
    elif kind == "zero_q":
        q = torch.zeros_like(q)
    elif kind == "common_offset":
        u = torch.randn(nkv, hs, generator=g)
        u = u / u.norm(dim=1, keepdim=True)
        for k in K:
            k.copy_(20.0 * u + 0.1 * k)
        G = nh // nkv
        q = (q.view(-1, nkv, G, hs) + (OFFSET / 20.0 * math.sqrt(hs)) * u[None, :, None, :]).reshape(-1, nh * hs)
    else:
        raise ValueError(kind)
    return K, V, q, pos, seq


def mean_of_v(V, pos, seq, nh, nkv):
    """zero_q's answer written without a soft-max: the mean of V[0 .. pos] of the row's kv head, float64."""
    G = nh // nkv
    out = []
    for p, b in zip(pos, seq):
        m = V[b][:int(p) + 1].to(F64).mean(0)                       # [n_kv, hs]
        out.append(m[:, None, :].expand(nkv, G, m.shape[-1]).reshape(-1))
    return torch.stack(out)


WRONG_KINDS = ["q16", "p16", "scale17", "stale_key"]


def decode_wrong_model(kind, q, K, V, pos, seq, nh, nkv, window=0, fill=LOUD):
    """kr.attn_ref in float64 with one defect (kind "none": no defect, equal to attn_ref).
    q16: q / sqrt(hs) kept to 16 significant bits (bf16 hi + lo), the flash form's q; p16: the normalised weights kept to 16 bits
    the same way; scale17: the scores times 1 + 2^-17; stale_key: a row of at least 1000 keys also admits the slot after
    row_pos, holding `fill` in every element of K and V."""
    q = torch.as_tensor(q).to(F64)
    pos, seq = np.asarray(pos, dtype=np.int64), np.asarray(seq, dtype=np.int64)
    R, G = q.shape[0], nh // nkv
    hs = q.shape[1] // nh
    qs = q / math.sqrt(hs)
    if kind == "q16":
        qs = kr.split16_round(qs)
    out = torch.zeros(R, nh * hs, dtype=F64)
    for b in np.unique(seq):
        sel = np.nonzero(seq == b)[0]
        p = torch.from_numpy(pos[sel])
        n = int(p.max()) + 1
        lo = torch.clamp(p + 1 - window, min=0) if window > 0 else torch.zeros_like(p)
        Kb, Vb = K[b][:n].to(F64), V[b][:n].to(F64)
        key = torch.arange(n)
        vis = (key[None, :] <= p[:, None]) & (key[None, :] >= lo[:, None])
        assert not bool(torch.isnan(Kb[vis.any(0)]).any()), "a visible key is not stored"
        Kb, Vb = torch.nan_to_num(Kb, nan=0.0), torch.nan_to_num(Vb, nan=0.0)
        qb = qs[sel].view(len(sel), nkv, G, hs)
        s = torch.einsum("rkgd,lkd->rkgl", qb, Kb)
        if kind == "scale17":
            s = s * (1.0 + 2.0 ** -17)
        s = s.masked_fill(~vis[:, None, None, :], float("-inf"))
        if kind == "stale_key":
            stale = torch.einsum("rkgd,kd->rkg", qb, torch.full((nkv, hs), fill, dtype=F64))
            stale = stale.masked_fill((p + 1 < 1000)[:, None, None], float("-inf"))
            s = torch.cat((s, stale[..., None]), -1)
            Vb = torch.cat((Vb, torch.full((1, nkv, hs), fill, dtype=F64)), 0)
        w = torch.softmax(s, dim=-1)
        if kind == "p16":
            w = kr.split16_round(w)
        out[sel] = torch.einsum("rkgl,lkd->rkgd", w, Vb).reshape(len(sel), nh * hs)
    return out
