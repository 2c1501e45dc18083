"""GPU parity of the row-by-row (decode) form of ua2_attn — attn_fused_kernel, called directly (ops.attn without `groups`) —
against the float64 reference of tests/kernel_refs.py on the values the cache actually stores: both cache dtypes, every group
size at every head size, contexts from one key to 2047, sliding windows, ring caches, launch-form invariance (bit for bit),
the packed output, and hostile but finite values.  Only finite inputs: no NaN / Inf is fed to an attention kernel.

Bars: unit-scale randn inputs use the project's bar of 2e-4 absolute (tests/test_gpu_attn.py).  The hostile-value cases have no
measured bar: each computes E_ref = error of the same formula in plain fp32 on the host against float64, on its own inputs,
relative to the row's max magnitude, and asserts err <= max(4 * E_ref, 8 * 2^-24) (kernel_refs.bar)."""
import numpy as np
import pytest
import torch

import kernel_refs as kr

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float32]
# every G in {1, 2, 3, 4} at every head size; 24/8/128 is the Llama trunk, 32/8/64 the depth decoder
GEOMS = [(4, 4, 32), (4, 2, 32), (6, 2, 32), (8, 2, 32),
         (4, 4, 64), (4, 2, 64), (6, 2, 64), (32, 8, 64),
         (4, 4, 128), (4, 2, 128), (24, 8, 128), (8, 2, 128)]
LENS = [1, 2, 7, 8, 9, 31, 63, 64, 65, 127, 128, 129, 200, 535, 2047]
BAR = 2e-4


def _positions(L):
    """Every position of a short sequence; first, last and the page-edge positions 64k - 1, 64k, 64k + 1 of a long one."""
    if L <= 129:
        return np.arange(L)
    edge = [p for k in range(1, (L + 63) // 64 + 1) for p in (64 * k - 1, 64 * k, 64 * k + 1)]
    return np.unique([p for p in [0, L - 1] + edge if 0 <= p < L])


def _rows(lens, positions, seed, shuffle=True):
    pos = np.concatenate([positions(L) for L in lens]).astype(np.int32)
    seq = np.concatenate([np.full(len(positions(L)), b) for b, L in enumerate(lens)]).astype(np.int32)
    if shuffle:
        perm = np.random.default_rng(seed).permutation(len(pos))
        pos, seq = pos[perm], seq[perm]
    return pos, seq


def _check_indices(cache, pos, seq):
    """Index-carrying inputs are asserted in range on the host before any launch."""
    assert len(pos) == len(seq) and seq.min() >= 0 and seq.max() < len(cache.lens)
    assert pos.min() >= 0 and all(pos[r] < cache.lens[seq[r]] for r in range(len(pos)))
    n_pages = cache.k.shape[0]
    assert int(cache.table.min()) >= 0 and int(cache.table.max()) < n_pages
    if cache.ring_pages == 0:
        assert int(pos.max()) // 64 < cache.max_pages


class _Dev:
    """The cache on the device + launches of the decode form."""

    def __init__(self, cache, nh):
        from uniaudio2_amd import ops
        self.ops, self.cache, self.nh = ops, cache, nh
        self.k, self.v, self.t = cache.k.cuda(), cache.v.cuda(), cache.table.cuda()
        self.geom = ops.kv_geom(self.k, self.v, self.t, nh, cache.n_kv, cache.hs, ring_pages=cache.ring_pages)
        self.KV = [cache.stored_seq(b) for b in range(len(cache.lens))]

    def run(self, q, pos, seq, window=0, row_seq=True, y_packed=None):
        _check_indices(self.cache, pos, seq)
        qd, pd, sd = q.cuda(), torch.from_numpy(pos).cuda(), torch.from_numpy(seq).cuda()
        y = torch.full((len(pos), q.shape[1]), float("nan"), device="cuda")          # an unwritten element stays NaN
        self.ops.attn(dtype=self.cache.dtype, R=len(pos), q=qd, row_pos=pd, row_seq=sd if row_seq else None, kv=self.geom, y=y,
                      window=window, y_packed=y_packed)
        torch.cuda.synchronize()
        return y

    def ref(self, q, pos, seq, window=0, dt=torch.float64):
        return kr.attn_ref(q, [k for k, _ in self.KV], [v for _, v in self.KV], pos, seq, self.nh, self.cache.n_kv, window, dt)


def _abs_err(y, ref):
    y = y.cpu().to(torch.float64)
    assert bool(torch.isfinite(y).all()), "non-finite / unwritten output element"
    return float((y - ref).abs().max())


@pytest.mark.parametrize("nh,nkv,hs", GEOMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_decode_attention_parity(dtype, nh, nkv, hs):
    """One ragged batch of 15 sequences (1 .. 2047 keys: fewer keys than soft-max states, page edges, long contexts), rows shuffled."""
    cache = kr.PagedCache(LENS, nkv, hs, dtype, seed=nh * 1000 + hs)
    dev = _Dev(cache, nh)
    pos, seq = _rows(LENS, _positions, seed=1)
    q = torch.randn(len(pos), nh * hs, generator=torch.Generator().manual_seed(hs + nh))
    err = _abs_err(dev.run(q, pos, seq), dev.ref(q, pos, seq))
    print(f"PARITY decode parity {dtype} {nh}/{nkv}/{hs} rows={len(pos)}: err {err:.3e} bar {BAR:.1e}")
    assert err < BAR


@pytest.mark.parametrize("nh,nkv,hs", [(24, 8, 128), (32, 8, 64), (4, 2, 32)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_decode_attention_row_seq_none(dtype, nh, nkv, hs):
    """row_seq = NULL: row r is sequence r (decode batches), each at its last position."""
    cache = kr.PagedCache(LENS, nkv, hs, dtype, seed=5)
    dev = _Dev(cache, nh)
    pos = np.array([L - 1 for L in LENS], dtype=np.int32)
    seq = np.arange(len(LENS), dtype=np.int32)
    q = torch.randn(len(pos), nh * hs, generator=torch.Generator().manual_seed(2))
    err = _abs_err(dev.run(q, pos, seq, row_seq=False), dev.ref(q, pos, seq))
    print(f"PARITY decode row_seq=None {dtype} {nh}/{nkv}/{hs}: err {err:.3e} bar {BAR:.1e}")
    assert err < BAR


@pytest.mark.parametrize("window", [1, 2, 63, 64, 65, 250])
@pytest.mark.parametrize("nh,nkv,hs", [(24, 8, 128), (4, 2, 64), (8, 2, 32), (4, 4, 32)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_decode_attention_window(dtype, nh, nkv, hs, window):
    """Sliding window on a linear cache, every position a query row: pos + 1 <, ==, > window, and windows whose first key is the
    last / first slot of a page."""
    lens = [1, 64, 65, 300, 700]
    cache = kr.PagedCache(lens, nkv, hs, dtype, seed=window)
    dev = _Dev(cache, nh)
    pos, seq = _rows(lens, np.arange, seed=window)
    q = torch.randn(len(pos), nh * hs, generator=torch.Generator().manual_seed(3))
    err = _abs_err(dev.run(q, pos, seq, window=window), dev.ref(q, pos, seq, window=window))
    print(f"PARITY decode window={window} {dtype} {nh}/{nkv}/{hs} rows={len(pos)}: err {err:.3e} bar {BAR:.1e}")
    assert err < BAR


@pytest.mark.parametrize("ring_pages", [2, 4, 8])
@pytest.mark.parametrize("nh,nkv,hs", [(4, 4, 64), (6, 2, 128), (8, 2, 32)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_decode_attention_ring_cache(dtype, nh, nkv, hs, ring_pages):
    """Ring caches with the largest legal window and a small one; the query is the last position of its sequence, placed before
    the first wrap, exactly at a wrap (pos % (64 * ring_pages) in {0, 63, 64}) and several wraps in."""
    span = 64 * ring_pages
    poss = [0, 10, span - 1, span, span + 63, span + 64, 2 * span, 5 * span + 17]
    lens = [p + 1 for p in poss]
    cache = kr.PagedCache(lens, nkv, hs, dtype, seed=ring_pages, ring_pages=ring_pages, fill=3.0e4)   # stale slots hold a loud value
    dev = _Dev(cache, nh)
    pos, seq = np.array(poss, dtype=np.int32), np.arange(len(poss), dtype=np.int32)
    perm = np.random.default_rng(0).permutation(len(pos))
    pos, seq = pos[perm], seq[perm]
    q = torch.randn(len(pos), nh * hs, generator=torch.Generator().manual_seed(4))
    for window in ((ring_pages - 1) * 64 + 1, 5):
        err = _abs_err(dev.run(q, pos, seq, window=window), dev.ref(q, pos, seq, window=window))
        print(f"PARITY decode ring_pages={ring_pages} window={window} {dtype} {nh}/{nkv}/{hs}: err {err:.3e} bar {BAR:.1e}")
        assert err < BAR


@pytest.mark.parametrize("ring_pages,window", [(3, 5), (6, 5), (4, 0), (4, 3 * 64 + 2), (2, 66)])
def test_ring_cache_refusals(ring_pages, window):
    """The launcher refuses a ring that is not a power of two, a ring without a window, and a window the ring cannot hold — on the
    host, before any launch."""
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import Ua2Error
    k = torch.zeros(8, 2, 64, 32, dtype=torch.bfloat16, device="cuda")
    table = torch.arange(8, dtype=torch.int32, device="cuda").view(1, 8)
    geom = ops.kv_geom(k, k.clone(), table, 4, 2, 32, ring_pages=ring_pages)
    q, y = torch.zeros(1, 128, device="cuda"), torch.zeros(1, 128, device="cuda")
    pos = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(Ua2Error, match="ring cache .* needs a power-of-two page count and 0 < window"):
        ops.attn(dtype=torch.bfloat16, R=1, q=q, row_pos=pos, row_seq=None, kv=geom, y=y, window=window)


def test_unsupported_geometries_are_refused():
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import Ua2Error
    pos = torch.zeros(1, dtype=torch.int32, device="cuda")
    table = torch.zeros(1, 1, dtype=torch.int32, device="cuda")
    for nh, nkv, hs, msg in ((2, 2, 48, "head_size 48 not supported"), (10, 2, 32, "group size <= 4")):
        k = torch.zeros(1, nkv, 64, hs, device="cuda")
        q, y = torch.zeros(1, nh * hs, device="cuda"), torch.zeros(1, nh * hs, device="cuda")
        with pytest.raises(Ua2Error, match=msg):
            ops.attn(dtype=torch.float32, R=1, q=q, row_pos=pos, row_seq=None, kv=ops.kv_geom(k, k.clone(), table, nh, nkv, hs), y=y)


INV_LENS = [196, 33, 70, 5, 64, 65]


@pytest.mark.parametrize("nh,nkv,hs", GEOMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_row_bits_do_not_depend_on_the_launch(dtype, nh, nkv, hs):
    """A row's output in a launch of R rows equals, bit for bit, its output when launched alone (R = 1).  R * n_kv > 256: the bf16
    batch takes the two-per-CU form with G <= 3 and must stay on the prefetch form with G = 4 (the single-row launches always take
    the prefetch form); fp32 has one form."""
    cache = kr.PagedCache(INV_LENS, nkv, hs, dtype, seed=9)
    dev = _Dev(cache, nh)
    pos, seq = _rows(INV_LENS, np.arange, seed=2)
    R = len(pos)
    assert R * nkv > 256
    q = torch.randn(R, nh * hs, generator=torch.Generator().manual_seed(6))
    y_all = dev.run(q, pos, seq)
    qd, pd, sd = q.cuda(), torch.from_numpy(pos).cuda(), torch.from_numpy(seq).cuda()
    y_one = torch.full_like(y_all, float("nan"))
    for r in range(R):
        dev.ops.attn(dtype=dtype, R=1, q=qd[r:r + 1], row_pos=pd[r:r + 1], row_seq=sd[r:r + 1], kv=dev.geom, y=y_one[r:r + 1])
    torch.cuda.synchronize()
    assert torch.equal(y_all, y_one)
    assert _abs_err(y_all, dev.ref(q, pos, seq)) < BAR


_decode_packed = kr.decode_packed          # one layout formula for this file and tests/test_gpu_attn_flash_parity.py


@pytest.mark.parametrize("nh,nkv,hs", [(24, 8, 128), (4, 2, 32), (32, 8, 64)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_packed_output_equals_row_major_output(dtype, nh, nkv, hs):
    """y_packed holds the rows of y rounded to the cache dtype, in the consumer's operand order; R is not a multiple of 16.
    Checked two ways: decoded on the host with the layout formula (every element, exact bits: RNE-bf16 of y, or y itself), and
    through a consumer — ua2_linear reading y as x= and y_packed as x_packed= must produce the same bits."""
    from uniaudio2_amd import ops
    lens = [37, 70, 64]
    cache = kr.PagedCache(lens, nkv, hs, dtype, seed=11)
    dev = _Dev(cache, nh)
    pos, seq = _rows(lens, np.arange, seed=3)
    R, K = len(pos), nh * hs
    assert R % 16 != 0
    q = torch.randn(R, K, generator=torch.Generator().manual_seed(7))
    pk = torch.zeros((R + 15) // 16 * 16 * K, dtype=dtype, device="cuda")
    y = dev.run(q, pos, seq, y_packed=pk)
    assert torch.equal(_decode_packed(pk, R, K, dtype), y.to(dtype))
    N = 96
    w = ops.pack_linear(torch.randn(N, K, generator=torch.Generator().manual_seed(8)).cuda(), dtype)
    z_x, z_pk = torch.zeros(R, N, device="cuda"), torch.zeros(R, N, device="cuda")
    ops.linear(dtype=dtype, M=R, N=N, K=K, w0=w, x=y, y=z_x)
    ops.linear(dtype=dtype, M=R, N=N, K=K, w0=w, x_packed=pk, y=z_pk)
    torch.cuda.synchronize()
    assert torch.equal(z_x, z_pk)


def _rel_row_err(y, ref):
    scale = ref.abs().amax(dim=1, keepdim=True).clamp_min(1e-30)
    return float(((y.to(torch.float64) - ref).abs() / scale).max())


@pytest.mark.parametrize("kind", ["peaked_q", "dominant_key", "wide_v", "equal_keys"])
@pytest.mark.parametrize("nh,nkv,hs", [(24, 8, 128), (8, 2, 32), (4, 4, 64)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_decode_attention_hostile_finite_values(dtype, nh, nkv, hs, kind):
    """q scaled x 8 (scores of +-100, a peaked soft-max); one key dominating; V entries of +-1e4 next to 1e-4; exactly equal keys
    (ties in the running max).  Error relative to the row's max magnitude against float64; bar from the fp32 host evaluation."""
    lens = [3, 40, 130, 300]
    g = torch.Generator().manual_seed(13)
    K = [torch.randn(L, nkv, hs, generator=g) for L in lens]
    V = [torch.randn(L, nkv, hs, generator=g) for L in lens]
    pos, seq = _rows(lens, np.arange, seed=4)
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
    else:
        for k in K:
            k[1:] = k[1:][(torch.arange(len(k) - 1) // 4) * 4 % max(len(k) - 1, 1)]      # runs of four identical keys
    cache = kr.PagedCache(lens, nkv, hs, dtype, seed=1, K=K, V=V)
    dev = _Dev(cache, nh)
    y = dev.run(q, pos, seq).cpu()
    assert bool(torch.isfinite(y).all())
    ref = dev.ref(q, pos, seq)
    err = _rel_row_err(y, ref)
    e_ref = _rel_row_err(dev.ref(q, pos, seq, dt=torch.float32), ref)
    b = kr.bar(e_ref)
    print(f"PARITY decode hostile {kind} {dtype} {nh}/{nkv}/{hs}: err {err:.3e} E_ref {e_ref:.3e} bar {b:.3e}")
    assert err <= b
