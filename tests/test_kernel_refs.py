"""The float64 references of tests/kernel_refs.py against the torch library functions they restate (CPU, float64, rtol 1e-12)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kernel_refs as kr

RTOL = 1e-12
F64 = torch.float64


def _close(a, b):
    np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=RTOL, atol=1e-13)


@pytest.mark.parametrize("nh,nkv,hs,window", [(6, 2, 32, 0), (4, 4, 64, 0), (8, 2, 16, 5), (3, 1, 32, 64), (4, 2, 32, 1)])
def test_attn_ref_vs_sdpa(nh, nkv, hs, window):
    g = torch.Generator().manual_seed(1)
    lens = [1, 7, 70, 130]
    c = kr.PagedCache(lens, nkv, hs, torch.bfloat16, seed=2)
    pos = np.concatenate([np.arange(L) for L in lens])
    seq = np.concatenate([np.full(L, b) for b, L in enumerate(lens)])
    perm = torch.randperm(len(pos), generator=g).numpy()
    pos, seq = pos[perm], seq[perm]
    q = torch.randn(len(pos), nh * hs, generator=g)
    KV = [c.stored_seq(b) for b in range(len(lens))]
    got = kr.attn_ref(q, [k for k, _ in KV], [v for _, v in KV], pos, seq, nh, nkv, window)
    G = nh // nkv
    for b, L in enumerate(lens):
        rows = np.nonzero(seq == b)[0]
        K, V = KV[b]
        assert torch.equal(K, c.K[b].to(torch.bfloat16).to(F64))                       # the builder stores the rounded values
        kk = K.permute(1, 0, 2).repeat_interleave(G, dim=0)                             # [nh, L, hs]
        vv = V.permute(1, 0, 2).repeat_interleave(G, dim=0)
        qq = q[rows].to(F64).view(len(rows), nh, hs).permute(1, 0, 2)                   # [nh, r, hs]
        p = torch.from_numpy(pos[rows])[:, None]
        key = torch.arange(L)[None, :]
        mask = (key <= p) & ((key > p - window) if window > 0 else torch.ones_like(key, dtype=torch.bool))
        ref = F.scaled_dot_product_attention(qq[None], kk[None], vv[None], attn_mask=mask[None, None])[0]
        _close(got[rows], ref.permute(1, 0, 2).reshape(len(rows), nh * hs))


@pytest.mark.parametrize("ring_pages,L", [(2, 50), (2, 128), (2, 129), (4, 700), (8, 64 * 8 * 5 + 17)])
def test_ring_builder_vs_linear_builder(ring_pages, L):
    """A ring cache holds what a linear one holds on the positions it keeps (at least the last (ring_pages - 1) * 64 + 1), each
    at table column (p // 64) % ring_pages; the reference on either gives the same row."""
    nkv, hs = 2, 32
    lin = kr.PagedCache([L], nkv, hs, torch.float32, seed=7)
    ring = kr.PagedCache([L], nkv, hs, torch.float32, seed=8, ring_pages=ring_pages, K=lin.K, V=lin.V)
    held = ring.held(0)
    w = (ring_pages - 1) * 64 + 1
    assert int(held[-1]) == L - 1 and len(held) >= min(L, w) and len(held) <= ring_pages * 64
    for a, b in zip(ring.stored(0, held), lin.stored(0, held)):
        assert torch.equal(a, b)
    assert ring.table.shape == (1, ring_pages)
    q = torch.randn(1, 4 * hs, generator=torch.Generator().manual_seed(3))
    Kl, Vl = lin.stored_seq(0)
    Kr, Vr = ring.stored_seq(0)
    a = kr.attn_ref(q, [Kl], [Vl], [L - 1], [0], 4, nkv, window=w)
    b = kr.attn_ref(q, [Kr], [Vr], [L - 1], [0], 4, nkv, window=w)
    assert torch.equal(a, b)


@pytest.mark.parametrize("C", [1, 63, 257])
@pytest.mark.parametrize("affine", [False, True])
def test_layernorm_ref_vs_torch(C, affine):
    g = torch.Generator().manual_seed(C)
    x = torch.randn(5, C, generator=g, dtype=F64) + 3.0
    w = torch.randn(C, generator=g, dtype=F64) if affine else None
    b = torch.randn(C, generator=g, dtype=F64) if affine else None
    _close(kr.layernorm_ref(x, w, b, 1e-5), F.layer_norm(x, (C,), w, b, 1e-5))


def test_rmsnorm_blend_ref_vs_formula():
    g = torch.Generator().manual_seed(0)
    x, other = torch.randn(6, 128, generator=g, dtype=F64), torch.randn(6, 128, generator=g, dtype=F64)
    w = torch.randn(128, generator=g, dtype=F64)
    mask = torch.tensor([[0, 1, 1], [1, 0, 0], [1, 1, 0], [0, 0, 1], [1, 1, 1], [0, 0, 0]], dtype=torch.uint8)
    n = x * torch.rsqrt(torch.mean(x * x, dim=-1, keepdim=True) + 1e-5) * w
    o1, nn = kr.rmsnorm_blend_ref(x, w, 1e-5)
    _close(nn, n), _close(o1, n)
    o1, _ = kr.rmsnorm_blend_ref(x, w, 1e-5, mask=mask, col_a=1)
    _close(o1, n * mask[:, 1:2])
    o1, _ = kr.rmsnorm_blend_ref(x, w, 1e-5, other=other, mask=mask, col_a=0, col_b=2)
    _close(o1, n * mask[:, 0:1] + other * mask[:, 2:3])
    o1, _ = kr.rmsnorm_blend_ref(x, w, 1e-5, other=other, mask=mask, col_a=-1, col_b=2)
    _close(o1, n + other * mask[:, 2:3])


@pytest.mark.parametrize("K,stride,dilation,pad_left", [(3, 1, 1, 0), (4, 2, 1, 3), (5, 4, 3, 4), (7, 1, 3, 6)])
def test_dwconv_ref_forward_vs_conv1d(K, stride, dilation, pad_left):
    g = torch.Generator().manual_seed(K)
    x, w, b = torch.randn(2, 5, 37, generator=g, dtype=F64), torch.randn(5, K, generator=g, dtype=F64), torch.randn(5, generator=g, dtype=F64)
    for extra in (0, 6):                                  # natural length, and a zero-padded tail
        pad_r = (K - 1) * dilation + extra * stride
        ref = F.conv1d(F.pad(x, (pad_left, pad_r)), w[:, None, :], b, stride=stride, dilation=dilation, groups=5)
        _close(kr.dwconv_ref(x, w, b, stride=stride, dilation=dilation, pad_left=pad_left, Tout=ref.shape[-1]), ref)


@pytest.mark.parametrize("K,stride,pad_left", [(4, 2, 0), (4, 2, 2), (8, 4, 4), (5, 2, 3), (12, 6, 6), (7, 6, 1)])
def test_dwconv_ref_transposed_vs_conv_transpose1d(K, stride, pad_left):
    g = torch.Generator().manual_seed(K)
    x, w = torch.randn(2, 3, 11, generator=g, dtype=F64), torch.randn(3, K, generator=g, dtype=F64)
    full = F.conv_transpose1d(x, w[:, None, :], None, stride=stride, groups=3)
    for Tout in (full.shape[-1] - pad_left - 3, full.shape[-1] - pad_left + 5):
        ref = F.pad(full, (0, 8))[..., pad_left:pad_left + Tout]
        _close(kr.dwconv_ref(x, w, None, stride=stride, pad_left=pad_left, Tout=Tout, transposed=True), ref)


def test_qknorm_rope_ref_vs_layer_norm_and_rotary():
    g = torch.Generator().manual_seed(4)
    R, nh, hs, rd = 5, 3, 48, 24
    qkv = torch.randn(R, 3 * nh * hs, generator=g, dtype=F64)
    qw, qb, kw, kb = (torch.randn(hs, generator=g, dtype=F64) for _ in range(4))
    pos = torch.tensor([0, 3, 63, 64, 9])
    ang = torch.arange(80, dtype=F64)[:, None] * (10000.0 ** (-torch.arange(rd // 2, dtype=F64) / (rd // 2)))[None, :]
    q, k, v = kr.qknorm_rope_ref(qkv, pos, nh, hs, qw, qb, kw, kb, 1e-5, ang.cos(), ang.sin(), rd)
    q0, k0, v0 = (t.view(R, nh, hs) for t in qkv.chunk(3, -1))
    assert torch.equal(v, v0)
    freqs = torch.cat((ang[pos], ang[pos]), -1)[:, None, :]
    for got, x, w, b in ((q, q0, qw, qb), (k, k0, kw, kb)):
        n = F.layer_norm(x, (hs,), w, b, 1e-5)
        t, rest = n[..., :rd], n[..., rd:]
        t1, t2 = t[..., :rd // 2], t[..., rd // 2:]
        ref = torch.cat((t * freqs.cos() + torch.cat((-t2, t1), -1) * freqs.sin(), rest), -1)
        _close(got, ref)


def test_argmax_partials_and_fp32_replays():
    row = np.array([1, 5, 5, 2] + [0] * 12 + [7] * 16 + [3, 9], dtype=np.float32)
    pm, pi = kr.argmax_partials(row, forbid=2)
    assert pm.tolist() == [5, 7, 9] and pi.tolist() == [2, 16, 33]
    pm, pi = kr.argmax_partials(row, forbid=32)
    assert pm.tolist() == [-np.inf, -np.inf, 9] and pi.tolist() == [0, 16, 33]
    l0, l1 = torch.tensor([1.1, -2.3]), torch.tensor([0.7, 4.0])
    got = kr.cfg_mix_ref(l0, l1, 3.0, torch.float32).numpy()
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, np.float32(l1.numpy()) + (np.float32(l0.numpy()) - np.float32(l1.numpy())) * np.float32(3.0))
    assert kr.bar(0.0) == 8 * 2.0 ** -24 and kr.bar(1e-3) == 4e-3
