"""The float64 references of tests/kernel_refs.py against the torch library functions they restate (CPU, float64, rtol 1e-12); the
host model of the flash attention contract against attn_ref; the conditions every hostile input generator must meet; and a dry
run in which deliberately wrong host models stand in for the device result of tests/test_gpu_attn_flash_parity.py and must
fail its assertions; the same for the decode form: the inputs of tests/test_gpu_attn_decode.py (tests/attn_decode_cases.py), the
conditions on its hostile generators, and the wrong models its bar must reject and the old 2e-4 did not."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attn_decode_cases as dc
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


# ---- the host model of the flash contract (kernel_refs.attn_flash_model) ----------------------------------------------------------

FLASH_BAR, FLASH_BAR_QP, FLOOR = 2e-4, 1e-2, 8.0 * 2.0 ** -24          # the bars of tests/test_gpu_attn_flash_parity.py


def _stored(lens, nkv, hs, K=None, V=None, seed=2):
    c = kr.PagedCache(lens, nkv, hs, torch.bfloat16, seed=seed, K=K, V=V, fill=3.0e4, extra_pages=2)
    KV = [c.stored_seq(b) for b in range(len(lens))]
    return [k for k, _ in KV], [v for _, v in KV]


_RANDN = {}


def _randn_case(nh, nkv, hs):
    """300 causal rows over 300 keys (+ a short sequence): inputs, float64 reference, and the model error per (mode, keys per step)."""
    if (nh, nkv, hs) not in _RANDN:
        lens = [300, 70]
        K, V = _stored(lens, nkv, hs)
        pos, seq = kr.all_rows(lens, seed=1)
        q = torch.randn(len(pos), nh * hs, generator=torch.Generator().manual_seed(hs))
        ref = kr.attn_ref(q, K, V, pos, seq, nh, nkv)
        out = {(m, kps): kr.attn_flash_model(q, K, V, pos, seq, nh, nkv, m, kps) for m in ("fp32", "split", "bf16") for kps in (64, 128)}
        _RANDN[(nh, nkv, hs)] = (q, K, V, pos, seq, ref, out)
    return _RANDN[(nh, nkv, hs)]


@pytest.mark.parametrize("nh,nkv,hs", [(4, 4, 32), (8, 2, 64), (6, 2, 128)])
def test_flash_model_vs_attn_ref(nh, nkv, hs):
    q, K, V, pos, seq, ref, out = _randn_case(nh, nkv, hs)
    # fp32 end to end: fp32 noise, sized by the plain fp32 evaluation of the reference formula
    e_ref = kr.rel_row_err(kr.attn_ref(q, K, V, pos, seq, nh, nkv, dt=torch.float32), ref)
    E = {key: kr.rel_row_err(y, ref) for key, y in out.items()}
    assert E[("fp32", 64)] <= kr.bar(e_ref) and E[("fp32", 128)] <= kr.bar(e_ref)
    # float64 end to end: the reference itself in another order, whatever the step
    for kps in (7, 64, 128):
        _close(kr.attn_flash_model(q, K, V, pos, seq, nh, nkv, "fp32", kps, F64, dt=F64), ref)
    # the three grades are ordered, and both step sizes stay inside the bar the device test applies to that grade
    for kps in (64, 128):
        assert E[("fp32", kps)] < E[("split", kps)] < E[("bf16", kps)]
        assert kr.abs_err(out[("split", kps)], ref) < FLASH_BAR and kr.abs_err(out[("bf16", kps)], ref) < FLASH_BAR_QP
        assert kr.abs_err(out[("fp32", kps)], ref) < FLASH_BAR


@pytest.mark.parametrize("kind", kr.HOSTILE_KINDS)
@pytest.mark.parametrize("nh,nkv,hs", [(24, 8, 128), (8, 2, 64), (4, 4, 32), (24, 24, 64)])
def test_hostile_inputs_are_finite_and_keep_the_bar_narrow(nh, nkv, hs, kind):
    """A condition on the inputs: the float64 reference is finite, and the bar 4 * E_model(split) never grows past 1e-3."""
    K, V, q, pos, seq = kr.hostile_inputs(kind, nh, nkv, hs)
    assert len(pos) == sum(kr.HOSTILE_LENS) and all(bool(torch.isfinite(t).all()) for t in K + V + [q])
    K, V = _stored(kr.HOSTILE_LENS, nkv, hs, K, V)
    ref = kr.attn_ref(q, K, V, pos, seq, nh, nkv)
    assert bool(torch.isfinite(ref).all())
    for kps in (64, 128):
        e = kr.rel_row_err(kr.attn_flash_model(q, K, V, pos, seq, nh, nkv, "split", kps), ref)
        assert 4.0 * e <= 1e-3, (kps, e)


def test_ramp_kinds_drive_the_online_softmax_hard():
    """rising_max: the running max of the last row rises at every 64-key step, by more than 16 bits at a full step (alpha < 2^-16:
    what was accumulated so far drops below the 16 significant bits of the weights);
    falling_max: it is set in step 0 and the weights of the last step are below the underflow of exp2."""
    nh, nkv, hs = 4, 4, 32
    for kind in ("rising_max", "falling_max"):
        K, V, q, pos, seq = kr.hostile_inputs(kind, nh, nkv, hs)
        K, V = _stored(kr.HOSTILE_LENS, nkv, hs, K, V)
        r = int(np.nonzero((seq == 3) & (pos == 299))[0][0])
        s = torch.einsum("hd,lhd->hl", q[r].view(nh, hs).to(F64), K[3]) * (1.4426950408889634 / hs ** 0.5)          # log2 units
        step_max = torch.stack([s[:, k0:k0 + 64].max(1).values for k0 in range(0, 300, 64)], 1)                      # [head, step]
        if kind == "rising_max":
            rise = step_max[:, 1:] - step_max[:, :-1]
            assert bool((rise[:, :3] > 16).all()) and bool((rise[:, 3] > 8).all())          # the last step holds 44 keys
        else:
            assert bool((step_max.argmax(1) == 0).all()) and bool((s[:, 256:].min(1).values - step_max[:, 0] < -126).all())


def test_wrong_models_fail_the_flash_assertions():
    """Dry run of tests/test_gpu_attn_flash_parity.py on the host: the model stands in for the device and passes; a mask off by one
    key at a block edge and a q whose lo half is dropped in one 32-dim chunk fail the unit-scale bar and the hostile bar; against
    the bf16 forms the wrong mask fails assertion (a) and the several times narrower (b)."""
    nh, nkv, hs = 8, 2, 64
    q, K, V, pos, seq, ref, out = _randn_case(nh, nkv, hs)

    def edge_mask(key, p):                               # the row at the first slot of a key block does not see that slot
        return (key <= p) & ~((key == p) & (p % 64 == 0) & (p > 0))

    def drop_lo_chunk(x):                                # dims 32 .. 63 of every head: hi only
        x = kr.split16_round(x).view(-1, nh, hs).clone()
        x[..., 32:64] = kr.bf16_once(x[..., 32:64])
        return x.view(-1, nh * hs)

    wrong = {"mask": dict(mode="split", visible=edge_mask), "lo": dict(mode=(drop_lo_chunk, "split"))}
    assert kr.abs_err(out[("split", 64)], ref) < FLASH_BAR
    for name, kw in wrong.items():
        y = kr.attn_flash_model(q, K, V, pos, seq, nh, nkv, kw["mode"], visible=kw.get("visible", kr.causal_visible))
        assert not kr.abs_err(y, ref) < FLASH_BAR, name
    # NaN left in an unwritten element fails too
    y = out[("split", 64)].clone()
    y[5, 3] = float("nan")
    assert not kr.abs_err(y, ref) < FLASH_BAR and not kr.rel_row_err(y, ref) <= 1.0
    # the hostile bar
    Kh, Vh, qh, ph, sh = kr.hostile_inputs("rising_max", nh, nkv, hs)
    Kh, Vh = _stored(kr.HOSTILE_LENS, nkv, hs, Kh, Vh)
    refh = kr.attn_ref(qh, Kh, Vh, ph, sh, nh, nkv)
    bar = max(4.0 * kr.rel_row_err(kr.attn_flash_model(qh, Kh, Vh, ph, sh, nh, nkv, "split"), refh), FLOOR)
    assert kr.rel_row_err(kr.attn_flash_model(qh, Kh, Vh, ph, sh, nh, nkv, "split", 128), refh) <= bar
    for name, kw in wrong.items():
        y = kr.attn_flash_model(qh, Kh, Vh, ph, sh, nh, nkv, kw["mode"], visible=kw.get("visible", kr.causal_visible))
        assert not kr.rel_row_err(y, refh) <= bar, name
    # the bf16 forms: (a) against float64, (b) against the model
    m32, m64 = out[("bf16", 64)].to(F64), kr.attn_flash_model(q, K, V, pos, seq, nh, nkv, "bf16", 64, F64).to(F64)
    bar_a, bar_b = 4.0 * kr.rel_row_err(m32, ref), max(4.0 * kr.rel_row_err(m32, m64), FLOOR)
    assert bar_b < bar_a / 4
    y = kr.attn_flash_model(q, K, V, pos, seq, nh, nkv, "bf16", visible=edge_mask)
    assert not kr.rel_row_err(y, ref) <= bar_a and not kr.rel_row_err(y, m32) <= bar_b
    assert kr.rel_row_err(m64, ref) <= bar_a and kr.rel_row_err(m64, m32) <= bar_b
    assert not kr.rel_row_err(out[("bf16", 128)], m32) <= FLOOR            # the two step sizes give different bits


def test_wrong_packed_index_fails_the_packed_assertion():
    """packed_index (index arithmetic) and decode_packed (a view) state one layout; an image written with two index factors swapped,
    or one that writes a row beyond R, is refused."""
    fill = 12352.0
    for dtype, K in ((torch.bfloat16, 256), (torch.float32, 48)):
        R = 37
        y = torch.randn(R, K, generator=torch.Generator().manual_seed(K))
        good = kr.encode_packed(y, dtype, fill)
        assert kr.packed_mismatch(good, y, R, K, dtype, fill) is None
        assert torch.equal(kr.decode_packed(good, R, K, dtype), y.to(dtype))

        def swapped(m, k, K, dtype):
            KC, EPL = (32, 8) if dtype == torch.bfloat16 else (16, 4)
            c, r = k // KC, k % KC
            return (((m >> 4) * (K // KC) + c) * 64 + (m & 15) * (KC // EPL) + r // EPL) * EPL + r % EPL

        assert kr.packed_mismatch(kr.encode_packed(y, dtype, fill, index=swapped), y, R, K, dtype, fill) is not None
        beyond = good.clone()
        beyond[kr.packed_index(torch.tensor(R), torch.tensor(3), K, dtype)] = 1.0
        assert kr.packed_mismatch(beyond, y, R, K, dtype, fill) == "a row beyond R was written"
        if dtype == torch.bfloat16:                      # not rounded to nearest: truncated
            trunc = kr.encode_packed((y.view(torch.int32) & -65536).view(torch.float32), dtype, fill)
            assert kr.packed_mismatch(trunc, y, R, K, dtype, fill) is not None


# ---- the decode form: inputs, hostile generators and wrong models (tests/attn_decode_cases.py) -----------------------------------

OLD_DECODE_BAR = 2e-4          # what tests/test_gpu_attn_decode.py asserted before it took kr.bar


@functools.lru_cache(maxsize=None)
def _decode_parity(nh, nkv, hs):
    """The bf16 parity batch of the GPU module with its float64 reference, fp32 evaluation and bar, as that module computes them."""
    cache, q, pos, seq = dc.parity_inputs(torch.bfloat16, nh, nkv, hs)
    dc.check_indices(cache, pos, seq)
    K, V = dc.stored(cache)
    ref = kr.attn_ref(q, K, V, pos, seq, nh, nkv)
    ref32 = kr.attn_ref(q, K, V, pos, seq, nh, nkv, dt=torch.float32)
    return cache, q, pos, seq, K, V, ref, ref32


@pytest.mark.parametrize("nh,nkv,hs", [(24, 8, 128), (4, 2, 32)])
def test_decode_bar_rejects_wrong_models(nh, nkv, hs):
    """Dry run of test_decode_attention_parity on the host, a wrong model standing in for the device.  The fp32 evaluation passes
    its own bar by construction; q or the weights kept to 16 bits (the flash form's contract) and a score scale off by 2^-17 exceed
    it, and all three lay below the 2e-4 the module used to assert; a read of the slot after row_pos exceeds it by more than 100x
    because that slot holds LOUD (with a fill of 0.0 it is 20 .. 27x: the old caches would have shown it 100x fainter).
    Measured x bar at 24/8/128 and 4/2/32: q16 1.8, 1.8; p16 2.0, 3.6; scale17 3.8, 5.8; stale_key 4.9e9, 8.6e9."""
    cache, q, pos, seq, K, V, ref, ref32 = _decode_parity(nh, nkv, hs)
    assert len(pos) == 766 and max(cache.lens) == 2047
    scale = max(1.0, float(ref.abs().max()))
    err, e_ref, bar = dc.unit_err(ref32, ref, ref32)
    assert err == e_ref <= bar and bar < OLD_DECODE_BAR / 20
    _close(dc.decode_wrong_model("none", q, K, V, pos, seq, nh, nkv), ref)
    fill = float(cache.k[cache.table[0, 0], 0, cache.lens[0], 0])                 # the slot after the one-key sequence: as stored
    assert fill == float(torch.tensor(dc.LOUD).to(cache.dtype)) and bool((cache.k[-1] == fill).all())
    for kind in ("q16", "p16", "scale17"):
        e = dc.unit_err(dc.decode_wrong_model(kind, q, K, V, pos, seq, nh, nkv), ref)[0]
        assert e > bar, (kind, e / bar)
        assert e * scale < OLD_DECODE_BAR, kind                                 # the old bar hid it
    e = dc.unit_err(dc.decode_wrong_model("stale_key", q, K, V, pos, seq, nh, nkv, fill=fill), ref)[0]
    assert e > 100.0 * bar, e / bar
    y = ref32.clone()
    y[5, 3] = float("nan")                                                      # an unwritten element
    assert not dc.unit_err(y, ref)[0] <= bar


def test_decode_case_generators_are_finite_and_in_range():
    for lens, positions in ((dc.LENS, dc.positions), (dc.LONG_LENS, dc.long_positions)):
        pos, seq = dc.rows(lens, positions, seed=1)
        assert pos.dtype == np.int32 and seq.dtype == np.int32 and len(pos) == len(seq)
        assert seq.min() >= 0 and seq.max() < len(lens) and pos.min() >= 0 and bool((pos < np.asarray(lens)[seq]).all())
        for b, L in enumerate(lens):                                            # first and last position of every sequence
            assert {0, L - 1} <= set(pos[seq == b].tolist())
    p = dc.long_positions(8191)
    assert {63, 64, 65, 4031, 4032, 4033, 4095, 4096, 4097, 8127, 8128, 8129, 8190} <= set(p.tolist()) and len(p) == 20
    assert set(dc.long_positions(4097).tolist()) == {0, 63, 64, 65, 127, 128, 129, 4031, 4032, 4033, 4095, 4096}
    cache, q, pos, seq = dc.parity_inputs(torch.float32, 4, 2, 32)
    dc.check_indices(cache, pos, seq)
    assert bool(torch.isfinite(q).all()) and bool(torch.isfinite(cache.k).all()) and bool(torch.isfinite(cache.v).all())
    named = torch.zeros(cache.k.shape[0], dtype=torch.bool)
    named[cache.table.long().reshape(-1)] = True
    assert int((~named).sum()) == dc.EXTRA_PAGES and bool((cache.k[~named] == dc.LOUD).all()) and bool((cache.v[~named] == dc.LOUD).all())


@pytest.mark.parametrize("kind", dc.HOSTILE_KINDS)
@pytest.mark.parametrize("nh,nkv,hs", [(24, 8, 128), (8, 2, 32), (4, 4, 64)])
def test_decode_hostile_inputs_keep_fp32_useful(nh, nkv, hs, kind):
    """Every hostile kind is finite, its float64 reference and its plain-fp32 evaluation are finite, and E_ref (fp32 against float64,
    relative to the row's max magnitude) is at most 1e-3: the bar 4 E_ref of the device test stays a statement about the kernel.
    Measured E_ref over the three geometries and both cache dtypes: peaked_q 3.0e-6 .. 7.3e-6, dominant_key 1.1e-6 .. 1.6e-6,
    wide_v 7.4e-7 .. 1.1e-6, equal_keys 9.2e-7 .. 1.5e-6, rising 2.5e-5 .. 4.5e-5, falling 3.0e-5 .. 5.6e-5, zero_q 6.2e-7 .. 8.0e-7,
    common_offset 1.7e-5 .. 2.9e-5 (RAMP = 140, OFFSET = 90 needed no adjustment)."""
    K, V, q, pos, seq = dc.hostile_inputs(kind, nh, nkv, hs)
    assert len(pos) == sum(dc.HOSTILE_LENS) and all(bool(torch.isfinite(t).all()) for t in K + V + [q])
    for dtype in (torch.bfloat16, torch.float32):
        cache = dc.linear_cache(dc.HOSTILE_LENS, nkv, hs, dtype, 1, K, V)
        dc.check_indices(cache, pos, seq)
        Ks, Vs = dc.stored(cache)
        ref = kr.attn_ref(q, Ks, Vs, pos, seq, nh, nkv)
        ref32 = kr.attn_ref(q, Ks, Vs, pos, seq, nh, nkv, dt=torch.float32)
        assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(ref32).all())
        assert kr.rel_row_err(ref32, ref) <= 1e-3
        if kind == "zero_q":
            np.testing.assert_allclose(ref.numpy(), dc.mean_of_v(Vs, pos, seq, nh, nkv).numpy(), rtol=0, atol=1e-12)
        r = int(np.nonzero((seq == 3) & (pos == 299))[0][0])
        s = torch.einsum("kgd,lkd->kgl", q[r].view(nkv, nh // nkv, hs).to(F64), Ks[3]) / hs ** 0.5                 # natural units
        if kind in ("rising", "falling"):
            step = s[..., 16:] - s[..., :-16] if dtype == torch.bfloat16 else s[..., 1:] - s[..., :-1]            # bf16 keys plateau
            assert bool((step > 0).all() if kind == "rising" else (step < 0).all())
            assert float((s.amax(-1) - s.amin(-1)).min()) > 87.0                                                    # past exp2's underflow
        if kind == "common_offset":
            assert float(s.min()) > 70.0 and float(s.amax(-1).max()) > 89.0                                         # exp overflows fp32
            assert 0.5 < float((s.amax(-1) - s.amin(-1)).max()) < 10.0                                              # a real soft-max remains
