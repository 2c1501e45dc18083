"""GPU parity of the row-by-row (decode) form of ua2_attn — attn_fused_kernel, called directly (ops.attn without `groups`) —
against the float64 reference of tests/kernel_refs.py on the values the cache actually stores: both cache dtypes, every group
size at every head size, contexts from one key to 8191, sliding windows, ring caches, the prefetch and the two-per-CU form on
each of them, launch-form invariance (bit for bit), the packed output with and without y, and eight hostile but finite value
classes.  The inputs come from tests/attn_decode_cases.py, where tests/test_kernel_refs.py holds them to their conditions on the
host.  Only finite inputs: no NaN / Inf is fed to an attention kernel, and no case is built to make a launch fault.

Bar.  Every value comparison is err <= kernel_refs.bar(E_ref) = max(4 E_ref, 8 * 2^-24): E_ref is the same formula evaluated in
plain fp32 on the host (attn_ref(dt=float32)) on the launch's own inputs, against float64.  err and E_ref are divided by
scale = max(1, max |ref|) of the launch on the randn families and by each row's max magnitude on the hostile kinds.  The R = 1
launches that repeat rows of a batch are held to the bar of that batch (the bar belongs to the inputs) and to the batch's bits.
No input class needed a host model of the kernel's roundings (q pre-scaled by 1 / sqrt(hs), exp2 of a pre-scaled argument, one
online soft-max per row group): the kernel sits under the plain-fp32 bar everywhere; the figures are in
profiles/kernel_parity_errors.txt.  tests/test_kernel_refs.py shows on the parity inputs that this bar rejects q or weights kept
to 16 bits (the flash form's contract), a score scale off by 2^-17 and a read of the slot after row_pos, of which the first three
passed the 2e-4 absolute this module asserted before.

Cache state.  Every slot no row may read — the tail of a sequence's last page, four pool pages no table names, the stale slots of
a ring — holds 3e4.  Guards on every launch: y lives inside a larger device buffer with 4096 elements of a finite bit pattern on
each side and under it, and afterwards the margins must be bit-unchanged and every element of y written; y_packed is allocated
with a fill value and must hold the rows of y rounded to the cache dtype bit for bit and the fill in its pad rows; q, row_pos,
row_seq, both pools and the page table must be bit-unchanged.  Index-carrying inputs are asserted in range on the host before
every launch.  Every batch launch prints a `PARITY decode` line, every set of R = 1 launches that is judged one line for the set."""
import numpy as np
import pytest
import torch

import attn_decode_cases as dc
import kernel_refs as kr

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float32]
# every G in {1, 2, 3, 4} at every head size; 24/8/128 is the Llama trunk, 32/8/64 the depth decoder
GEOMS = [(4, 4, 32), (4, 2, 32), (6, 2, 32), (8, 2, 32),
         (4, 4, 64), (4, 2, 64), (6, 2, 64), (32, 8, 64),
         (4, 4, 128), (4, 2, 128), (24, 8, 128), (8, 2, 128)]
LENS = dc.LENS
MARGIN = 4096                          # elements of sentinel on each side of y
SENT = 0x7E7E7E7E                      # a finite bit pattern (8.5e37) around and under y
PK_FILL = 12352.0                      # what y_packed holds before the launch (exact in bf16)
INT_OF = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.int32: torch.int32}

_rows, _check_indices = dc.rows, dc.check_indices


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(INT_OF[a.dtype]), b.contiguous().view(INT_OF[b.dtype]))


class _Dev:
    """The cache on the device + guarded launches of the decode form."""

    def __init__(self, cache, nh):
        from uniaudio2_amd import ops
        self.ops, self.cache, self.nh = ops, cache, nh
        self.k, self.v, self.t = cache.k.cuda(), cache.v.cuda(), cache.table.cuda()
        self.pristine = (self.k.clone(), self.v.clone(), self.t.clone())
        self.geom = ops.kv_geom(self.k, self.v, self.t, nh, cache.n_kv, cache.hs, ring_pages=cache.ring_pages)
        self.K, self.V = dc.stored(cache)

    def _inputs(self, q, pos, seq):
        _check_indices(self.cache, pos, seq)
        assert bool(torch.isfinite(q).all())
        return q.cuda(), torch.from_numpy(pos).cuda(), torch.from_numpy(seq).cuda()

    def _guarded_y(self, R, C):
        buf = torch.empty(2 * MARGIN + R * C, dtype=torch.float32, device="cuda")
        buf.view(torch.int32).fill_(SENT)
        return buf, buf[MARGIN:MARGIN + R * C].view(R, C)

    def _assert_guards(self, buf, y, written, dev_in, host_in):
        bits = buf.view(torch.int32)
        n = y.numel()
        assert bool((bits[:MARGIN] == SENT).all()) and bool((bits[MARGIN + n:] == SENT).all()), "store outside y"
        if written:
            assert bool((bits[MARGIN:MARGIN + n] != SENT).all()), "an element of y was never written"
        else:
            assert bool((bits[MARGIN:MARGIN + n] == SENT).all()), "y was written though it was not passed"
        for d, h, what in zip(dev_in, host_in, ("q", "row_pos", "row_seq")):
            assert _bits_equal(d.cpu(), torch.as_tensor(h)), f"{what} was written to"
        for d, p, what in zip((self.k, self.v, self.t), self.pristine, ("the K pool", "the V pool", "the page table")):
            assert _bits_equal(d, p), f"{what} was written to"

    def run(self, q, pos, seq, window=0, row_seq=True, packed=False, want_y=True):
        """One guarded launch -> y [R, n_head * hs] on the device (packed: (y, y_packed))."""
        qd, pd, sd = self._inputs(q, pos, seq)
        R, C = q.shape
        buf, y = self._guarded_y(R, C)
        pk = torch.full(((R + 15) // 16 * 16 * C,), PK_FILL, dtype=self.cache.dtype, device="cuda") if packed else None
        self.ops.attn(dtype=self.cache.dtype, R=R, q=qd, row_pos=pd, row_seq=sd if row_seq else None, kv=self.geom,
                      y=y if want_y else None, window=window, y_packed=pk)
        torch.cuda.synchronize()
        self._assert_guards(buf, y, want_y, (qd, pd, sd), (q, pos, seq))
        if packed and want_y:
            assert kr.packed_mismatch(pk, y, R, C, self.cache.dtype, PK_FILL) is None
        return (y, pk) if packed else y

    def run_single(self, q, pos, seq, rows, window=0):
        """The rows `rows` of a batch, each as a launch of its own (R = 1, the prefetch form) -> [len(rows), n_head * hs]."""
        qd, pd, sd = self._inputs(q, pos, seq)
        buf, y = self._guarded_y(len(rows), q.shape[1])
        for i, r in enumerate(rows):
            self.ops.attn(dtype=self.cache.dtype, R=1, q=qd[r:r + 1], row_pos=pd[r:r + 1], row_seq=sd[r:r + 1], kv=self.geom,
                          y=y[i:i + 1], window=window)
        torch.cuda.synchronize()
        self._assert_guards(buf, y, True, (qd, pd, sd), (q, pos, seq))
        return y

    def ref(self, q, pos, seq, window=0, dt=torch.float64):
        return kr.attn_ref(q, self.K, self.V, pos, seq, self.nh, self.cache.n_kv, window, dt)

    def refs(self, q, pos, seq, window=0):
        ref = self.ref(q, pos, seq, window)
        assert bool(torch.isfinite(ref).all())
        return ref, self.ref(q, pos, seq, window, dt=torch.float32)


def _report(case, err, e_ref, bar, extra=""):
    print(f"PARITY decode {case}: err {err:.3e} E_ref {e_ref:.3e} bar {bar:.3e} err/bar {err / bar:.3f}{extra}")


def _judge(case, y, ref, ref32, extra=""):
    """Unit-scale inputs: errors divided by scale = max(1, max |ref|) of the launch."""
    err, e_ref, bar = dc.unit_err(y, ref, ref32)
    _report(case, err, e_ref, bar, extra)
    assert err <= bar
    return bar


def _judge_rows(case, y, ref, ref32):
    """Hostile values: errors relative to each row's max magnitude."""
    err, e_ref = kr.rel_row_err(y, ref), kr.rel_row_err(ref32, ref)
    bar = kr.bar(e_ref)
    _report(case, err, e_ref, bar)
    assert err <= bar
    return bar


def _name(dtype, nh, nkv, hs):
    return f"{'bf16' if dtype == torch.bfloat16 else 'fp32'} {nh}/{nkv}/{hs}"


@pytest.mark.parametrize("nh,nkv,hs", GEOMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_decode_attention_parity(dtype, nh, nkv, hs):
    """One ragged batch of 15 sequences (1 .. 2047 keys: fewer keys than soft-max states, page edges, long contexts), rows shuffled."""
    cache, q, pos, seq = dc.parity_inputs(dtype, nh, nkv, hs)
    dev = _Dev(cache, nh)
    y = dev.run(q, pos, seq)
    ref, ref32 = dev.refs(q, pos, seq)
    longest = np.nonzero(pos == 2046)[0].tolist()
    _judge(f"parity {_name(dtype, nh, nkv, hs)} rows={len(pos)}", y, ref, ref32,
           f" abs@2047keys {kr.abs_err(y[longest], ref[longest]):.3e}")


@pytest.mark.parametrize("nh,nkv,hs", [(24, 8, 128), (32, 8, 64), (4, 2, 32)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_decode_attention_row_seq_none(dtype, nh, nkv, hs):
    """row_seq = NULL: row r is sequence r (decode batches), each at its last position."""
    cache = dc.linear_cache(LENS, nkv, hs, dtype, seed=5)
    dev = _Dev(cache, nh)
    pos = np.array([L - 1 for L in LENS], dtype=np.int32)
    seq = np.arange(len(LENS), dtype=np.int32)
    q = torch.randn(len(pos), nh * hs, generator=torch.Generator().manual_seed(2))
    _judge(f"row_seq=None {_name(dtype, nh, nkv, hs)}", dev.run(q, pos, seq, row_seq=False), *dev.refs(q, pos, seq))


@pytest.mark.parametrize("window", [1, 2, 63, 64, 65, 250])
@pytest.mark.parametrize("nh,nkv,hs", [(24, 8, 128), (4, 2, 64), (8, 2, 32), (4, 4, 32)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_decode_attention_window(dtype, nh, nkv, hs, window):
    """Sliding window on a linear cache, every position a query row: pos + 1 <, ==, > window, and windows whose first key is the
    last / first slot of a page."""
    lens = [1, 64, 65, 300, 700]
    cache = dc.linear_cache(lens, nkv, hs, dtype, seed=window)
    dev = _Dev(cache, nh)
    pos, seq = _rows(lens, np.arange, seed=window)
    q = torch.randn(len(pos), nh * hs, generator=torch.Generator().manual_seed(3))
    _judge(f"window={window} {_name(dtype, nh, nkv, hs)} rows={len(pos)}", dev.run(q, pos, seq, window=window),
           *dev.refs(q, pos, seq, window=window))


def _ring_positions(ring_pages):
    """Before the first wrap, exactly at a wrap (pos % (64 * ring_pages) in {0, 63, 64}) and several wraps in."""
    span = 64 * ring_pages
    return [0, 10, span - 1, span, span + 63, span + 64, 2 * span, 5 * span + 17]


def _ring_windows(ring_pages):
    return ((ring_pages - 1) * 64 + 1, 5)                # the largest legal window and a small one


@pytest.mark.parametrize("ring_pages", [2, 4, 8])
@pytest.mark.parametrize("nh,nkv,hs", [(4, 4, 64), (6, 2, 128), (8, 2, 32)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_decode_attention_ring_cache(dtype, nh, nkv, hs, ring_pages):
    """Ring caches with the largest legal window and a small one; the query is the last position of its sequence, placed before
    the first wrap, exactly at a wrap (pos % (64 * ring_pages) in {0, 63, 64}) and several wraps in."""
    poss = _ring_positions(ring_pages)
    lens = [p + 1 for p in poss]
    cache = kr.PagedCache(lens, nkv, hs, dtype, seed=ring_pages, ring_pages=ring_pages, fill=dc.LOUD, extra_pages=dc.EXTRA_PAGES)
    dev = _Dev(cache, nh)
    pos, seq = np.array(poss, dtype=np.int32), np.arange(len(poss), dtype=np.int32)
    perm = np.random.default_rng(0).permutation(len(pos))
    pos, seq = pos[perm], seq[perm]
    q = torch.randn(len(pos), nh * hs, generator=torch.Generator().manual_seed(4))
    for window in _ring_windows(ring_pages):
        _judge(f"ring_pages={ring_pages} window={window} {_name(dtype, nh, nkv, hs)}", dev.run(q, pos, seq, window=window),
               *dev.refs(q, pos, seq, window=window))


DENSE_ROWS_PER_SEQ = 40


@pytest.mark.parametrize("ring_pages", [2, 4, 8])
@pytest.mark.parametrize("nh,nkv,hs", [(4, 4, 64), (6, 2, 128), (8, 2, 32)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_two_per_cu_form_on_ring_and_window(dtype, nh, nkv, hs, ring_pages):
    """The ring test's eight sequences with 40 query rows each at the last position, independent q: R * n_kv > 256, so the bf16
    launch takes the two-per-CU form at G <= 3 (8/2/32, G = 4, must stay on the prefetch form; fp32 has one form).  The first row
    of each sequence equals its R = 1 launch (the prefetch form) bit for bit.  Then the same rows with row_seq = NULL on a cache
    of R sequences, sequence r a copy of the sequence row r read before, on pages of its own: the same bits again."""
    poss = _ring_positions(ring_pages)
    lens = [p + 1 for p in poss]
    cache = kr.PagedCache(lens, nkv, hs, dtype, seed=ring_pages, ring_pages=ring_pages, fill=dc.LOUD, extra_pages=dc.EXTRA_PAGES)
    dev = _Dev(cache, nh)
    seq = np.repeat(np.arange(len(poss)), DENSE_ROWS_PER_SEQ).astype(np.int32)
    seq = seq[np.random.default_rng(1).permutation(len(seq))]
    pos = np.asarray(poss, dtype=np.int32)[seq]
    R = len(pos)
    assert R == 320 and R * nkv > 256
    q = torch.randn(R, nh * hs, generator=torch.Generator().manual_seed(14))
    first = [int(np.nonzero(seq == b)[0][0]) for b in range(len(poss))]
    wide = kr.PagedCache([int(lens[b]) for b in seq], nkv, hs, dtype, seed=ring_pages + 100, ring_pages=ring_pages, fill=dc.LOUD,
                         extra_pages=dc.EXTRA_PAGES, K=[cache.K[b] for b in seq], V=[cache.V[b] for b in seq])
    dev_wide = _Dev(wide, nh)
    own = np.arange(R, dtype=np.int32)
    for window in _ring_windows(ring_pages):
        ref, ref32 = dev.refs(q, pos, seq, window=window)
        case = f"ring_pages={ring_pages} window={window} {_name(dtype, nh, nkv, hs)}"
        y = dev.run(q, pos, seq, window=window)
        _judge(f"two-per-CU {case} rows={R}", y, ref, ref32)
        assert torch.equal(y[first], dev.run_single(q, pos, seq, first, window=window))
        y_own = dev_wide.run(q, pos, own, window=window, row_seq=False)
        _judge(f"two-per-CU row_seq=None {case} rows={R}", y_own, ref, ref32)
        assert torch.equal(y_own, y)


@pytest.mark.parametrize("nh,nkv,hs", [(24, 8, 128), (32, 8, 64), (4, 4, 32)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_decode_attention_long_contexts(dtype, nh, nkv, hs):
    """4097 and 8191 keys in one cache (65 and 128 pages): the first and last position and the page edges 64k - 1, 64k, 64k + 1 for
    k in {1, 2, 63, 64, 65, 127}, as one batch and, for the last position of each sequence, as an R = 1 launch."""
    cache = dc.linear_cache(dc.LONG_LENS, nkv, hs, dtype, seed=hs + 7)
    dev = _Dev(cache, nh)
    pos, seq = _rows(dc.LONG_LENS, dc.long_positions, seed=5)
    q = torch.randn(len(pos), nh * hs, generator=torch.Generator().manual_seed(15))
    y = dev.run(q, pos, seq)
    ref, ref32 = dev.refs(q, pos, seq)
    last = [int(np.nonzero((seq == b) & (pos == L - 1))[0][0]) for b, L in enumerate(dc.LONG_LENS)]
    case = f"long {_name(dtype, nh, nkv, hs)}"
    bar = _judge(f"{case} rows={len(pos)}", y, ref, ref32, f" abs@8191keys {kr.abs_err(y[last[1:]], ref[last[1:]]):.3e}")
    y1 = dev.run_single(q, pos, seq, last)
    scale = max(1.0, float(ref.abs().max()))
    err = kr.abs_err(y1, ref[last]) / scale
    _report(f"{case} R=1 x{len(last)} (last positions)", err, kr.abs_err(ref32[last], ref[last]) / scale, bar)
    assert err <= bar
    assert torch.equal(y1, y[last])


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
INV_HOSTILE_ROWS = 64


@pytest.mark.parametrize("nh,nkv,hs", GEOMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_row_bits_do_not_depend_on_the_launch(dtype, nh, nkv, hs):
    """A row's output in a launch of R rows equals, bit for bit, its output when launched alone (R = 1).  R * n_kv > 256: the bf16
    batch takes the two-per-CU form with G <= 3 and must stay on the prefetch form with G = 4 (the single-row launches always take
    the prefetch form); fp32 has one form.  On randn every row is launched alone; on the peaked_q and common_offset inputs (scores
    whose exponentials span the fp32 range, where a form that rounded or ordered differently would show first) 64 rows drawn
    from the batch are."""
    pos, seq = _rows(INV_LENS, np.arange, seed=2)
    R = len(pos)
    assert R * nkv > 256
    cache = dc.linear_cache(INV_LENS, nkv, hs, dtype, seed=9)
    dev = _Dev(cache, nh)
    q = torch.randn(R, nh * hs, generator=torch.Generator().manual_seed(6))
    y_all = dev.run(q, pos, seq)
    assert torch.equal(y_all, dev.run_single(q, pos, seq, list(range(R))))
    _judge(f"launch-invariance randn {_name(dtype, nh, nkv, hs)} rows={R}", y_all, *dev.refs(q, pos, seq))
    some = sorted(np.random.default_rng(3).choice(R, INV_HOSTILE_ROWS, replace=False).tolist())
    for kind in ("peaked_q", "common_offset"):
        K, V, q, hpos, hseq = dc.hostile_inputs(kind, nh, nkv, hs, lens=INV_LENS)
        assert len(hpos) == R
        dev = _Dev(dc.linear_cache(INV_LENS, nkv, hs, dtype, 9, K, V), nh)
        y_all = dev.run(q, hpos, hseq)
        assert torch.equal(y_all[some], dev.run_single(q, hpos, hseq, some))
        _judge_rows(f"launch-invariance {kind} {_name(dtype, nh, nkv, hs)} rows={R}", y_all, *dev.refs(q, hpos, hseq))


_decode_packed = kr.decode_packed          # one layout formula for this file and tests/test_gpu_attn_flash_parity.py
PACKED_LENS = [37, 70, 64]


@pytest.mark.parametrize("nh,nkv,hs", [(24, 8, 128), (4, 2, 32), (32, 8, 64)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_packed_output_equals_row_major_output(dtype, nh, nkv, hs):
    """y_packed holds the rows of y rounded to the cache dtype, in the consumer's operand order; R is not a multiple of 16.
    Checked three ways: against the host image of the layout (every element of the buffer, exact bits: RNE-bf16 of y, or y itself,
    and the fill in the pad rows), decoded with the layout's view, and through a consumer — ua2_linear reading y as x= and
    y_packed as x_packed= must produce the same bits."""
    from uniaudio2_amd import ops
    cache = dc.linear_cache(PACKED_LENS, nkv, hs, dtype, seed=11)
    dev = _Dev(cache, nh)
    pos, seq = _rows(PACKED_LENS, np.arange, seed=3)
    R, K = len(pos), nh * hs
    assert R % 16 != 0
    q = torch.randn(R, K, generator=torch.Generator().manual_seed(7))
    y, pk = dev.run(q, pos, seq, packed=True)
    assert pk.numel() == (R + 15) // 16 * 16 * K
    assert _bits_equal(pk.cpu(), kr.encode_packed(y.cpu(), dtype, PK_FILL))
    assert torch.equal(_decode_packed(pk, R, K, dtype), y.to(dtype))
    _judge(f"packed {_name(dtype, nh, nkv, hs)} rows={R}", y, *dev.refs(q, pos, seq))
    N = 96
    w = ops.pack_linear(torch.randn(N, K, generator=torch.Generator().manual_seed(8)).cuda(), dtype)
    z_x, z_pk = torch.zeros(R, N, device="cuda"), torch.zeros(R, N, device="cuda")
    ops.linear(dtype=dtype, M=R, N=N, K=K, w0=w, x=y.contiguous(), y=z_x)
    ops.linear(dtype=dtype, M=R, N=N, K=K, w0=w, x_packed=pk, y=z_pk)
    torch.cuda.synchronize()
    assert torch.equal(z_x, z_pk)


@pytest.mark.parametrize("nh,nkv,hs", [(24, 8, 128), (4, 2, 32)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_packed_output_alone(dtype, nh, nkv, hs):
    """y = NULL with y_packed given (include/ua2hip.h allows it): the packed buffer equals, bit for bit and pad rows included, the
    one of a launch that wrote both, and the y that was not passed stays untouched."""
    cache = dc.linear_cache(PACKED_LENS, nkv, hs, dtype, seed=12)
    dev = _Dev(cache, nh)
    pos, seq = _rows(PACKED_LENS, np.arange, seed=6)
    R, K = len(pos), nh * hs
    assert R % 16 != 0
    q = torch.randn(R, K, generator=torch.Generator().manual_seed(16))
    y, pk_both = dev.run(q, pos, seq, packed=True)
    _judge(f"y=NULL {_name(dtype, nh, nkv, hs)} rows={R} (the launch with both)", y, *dev.refs(q, pos, seq))
    _, pk_alone = dev.run(q, pos, seq, packed=True, want_y=False)
    assert _bits_equal(pk_alone, pk_both)
    assert kr.packed_mismatch(pk_alone, y, R, K, dtype, PK_FILL) is None


def _hostile_single_rows(lens, pos, seq):
    """Per sequence: the first position, a page-edge position (the last multiple of 64 it holds; the middle of a sequence shorter
    than a page) and the last position."""
    want = [(b, p) for b, L in enumerate(lens) for p in sorted({0, 64 * ((L - 1) // 64) if L > 64 else L // 2, L - 1})]
    return [int(np.nonzero((seq == b) & (pos == p))[0][0]) for b, p in want]


@pytest.mark.parametrize("kind", dc.HOSTILE_KINDS)
@pytest.mark.parametrize("nh,nkv,hs", [(24, 8, 128), (8, 2, 32), (4, 4, 64)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_decode_attention_hostile_finite_values(dtype, nh, nkv, hs, kind):
    """q scaled x 8 (a peaked soft-max); one key dominating; V entries of +-1e4 next to 1e-4; exactly equal keys (ties in the
    running max); scores rising / falling with position across 140 natural units; q = 0 (the mean of V); scores with a common
    term of 90.  Error relative to the row's max magnitude against float64; bar from the fp32 host evaluation.  Once as a batch
    (G <= 3 and bf16: the two-per-CU form), then the first, a page-edge and the last row of each sequence as R = 1 launches (the
    prefetch form): under the same bar, and the batch's bits."""
    lens = dc.HOSTILE_LENS
    K, V, q, pos, seq = dc.hostile_inputs(kind, nh, nkv, hs)
    dev = _Dev(dc.linear_cache(lens, nkv, hs, dtype, 1, K, V), nh)
    y = dev.run(q, pos, seq)
    ref, ref32 = dev.refs(q, pos, seq)
    if kind == "zero_q":
        np.testing.assert_allclose(ref.numpy(), dc.mean_of_v(dev.V, pos, seq, nh, nkv).numpy(), rtol=0, atol=1e-12)
    case = f"hostile {kind} {_name(dtype, nh, nkv, hs)}"
    bar = _judge_rows(f"{case} rows={len(pos)}", y, ref, ref32)
    rows = _hostile_single_rows(lens, pos, seq)
    assert len(rows) == 12
    y1 = dev.run_single(q, pos, seq, rows)
    err = kr.rel_row_err(y1, ref[rows])
    _report(f"{case} R=1 x{len(rows)}", err, kr.rel_row_err(ref32[rows], ref[rows]), bar)
    assert err <= bar
    assert torch.equal(y1, y[rows])
