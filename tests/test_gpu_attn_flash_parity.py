"""GPU parity of the MFMA flash form of ua2_attn (attn_flash_kernel: prefill, dense encoders, DiT) and of the depth decoder's local
attention (attn_local_kernel / LocalAttn) against the float64 reference of tests/kernel_refs.py on the values the cache stores.
Every instantiation launch_flash dispatches is launched (its name is in the case id), on ragged batches that walk the 16-row tile
edges, the 64-key page edges and the 128-key pair edges, with scattered pages, loud stale slots (3e4, never NaN / Inf), shuffled
rows and outputs prefilled with NaN.  Only finite inputs are fed to an attention kernel; index-carrying inputs are asserted in
range on the host before any launch.

Bars.  Unit-scale randn inputs: the project's 2e-4 absolute against float64 (1e-2 for the bf16 q / weights form).  Hostile values:
relative to each row's max magnitude, err <= max(4 * E_model, 8 * 2^-24), E_model = error of kernel_refs.attn_flash_model (the
kernel's arithmetic contract evaluated on the host: 16-bit or bf16 q and weights, blocked online softmax) against float64 on the
same inputs; tests/test_kernel_refs.py holds every hostile generator to 4 * E_model(split) <= 1e-3.  The bf16 q / weights forms
are also compared with the model itself: err <= max(4 * E_flip, 8 * 2^-24), E_flip = the distance between two host evaluations
of the model with fp32 and with float64 scores (how far legal fp32 noise in the scores moves the bf16 roundings).  The local
kernel is plain single-rounding fp32: kernel_refs.bar(E_ref) from the fp32 host evaluation of the reference formula."""
import functools

import numpy as np
import pytest
import torch

import kernel_refs as kr

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
BAR = 2e-4
BAR_QP = 1e-2
FLOOR = 8.0 * 2.0 ** -24
LOUD = 3.0e4
LENS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 300]
# (n_head, n_kv, hs, q_tiles): the fewest heads that reach each fp32-grade instantiation (hs, G, QT) of launch_flash
FLASH_GEOMS = [(24, 8, 128, 2), (4, 4, 128, 4), (4, 4, 64, 4), (4, 4, 64, 8), (4, 2, 64, 2), (8, 2, 64, 2), (4, 2, 128, 2), (4, 2, 32, 2),
               (4, 4, 32, 4)]
QP_LENS = [1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257, 500]
QP_GEOM = (24, 24, 64, 8)


def _inst(nh, nkv, hs, qt, qp=""):
    return f"hs{hs}-G{nh // nkv}-QT{qt}{qp}"


def _geom_params(geoms):
    return [pytest.param(*g, id=_inst(*g)) for g in geoms]


class _Host:
    """One batch on the host: the paged bf16 cache (scattered pages, loud stale slots), the values it stores, q, and the float64
    reference / model evaluations, each computed once and shared by the tests of the batch."""

    def __init__(self, lens, nh, nkv, hs, pos, seq, q, K=None, V=None, seed=0):
        self.lens, self.nh, self.nkv, self.hs, self.pos, self.seq, self.q = list(lens), nh, nkv, hs, pos, seq, q
        self.cache = kr.PagedCache(lens, nkv, hs, BF16, seed=seed, K=K, V=V, fill=LOUD, extra_pages=3)
        KV = [self.cache.stored_seq(b) for b in range(len(lens))]
        self.K, self.V = [k for k, _ in KV], [v for _, v in KV]

    @functools.lru_cache(maxsize=None)
    def ref(self, window=0):
        r = kr.attn_ref(self.q, self.K, self.V, self.pos, self.seq, self.nh, self.nkv, window)
        assert bool(torch.isfinite(r).all())
        return r

    @functools.lru_cache(maxsize=None)
    def model(self, mode, keys_per_step=64, score_dt=torch.float32):
        return kr.attn_flash_model(self.q, self.K, self.V, self.pos, self.seq, self.nh, self.nkv, mode, keys_per_step, score_dt).to(torch.float64)

    def e_model(self, mode, keys_per_step=64):
        return kr.rel_row_err(self.model(mode, keys_per_step), self.ref())


@functools.lru_cache(maxsize=None)
def _randn_batch(nh, nkv, hs, dense=False, lens=tuple(LENS)):
    pos, seq = kr.all_rows(lens, seed=nh + hs, dense=dense)
    q = torch.randn(len(pos), nh * hs, generator=torch.Generator().manual_seed(hs * 100 + nh))
    return _Host(lens, nh, nkv, hs, pos, seq, q, seed=nh * 1000 + hs + dense)


@functools.lru_cache(maxsize=None)
def _hostile_batch(kind, nh, nkv, hs):
    K, V, q, pos, seq = kr.hostile_inputs(kind, nh, nkv, hs)
    return _Host(kr.HOSTILE_LENS, nh, nkv, hs, pos, seq, q, K=K, V=V, seed=1)


def _cut_groups(pos, seq, per, live=None):
    """Rows of one sequence in position order, `live` (<= per) of them at the head of each group of `per` slots."""
    live = live or per
    rows, gseq, nkeys = [], [], []
    for b in np.unique(seq):
        idx = np.nonzero(seq == b)[0]
        idx = idx[np.argsort(pos[idx], kind="stable")]
        for c in range(0, len(idx), live):
            sel = idx[c:c + live]
            rows.append(np.concatenate([sel, np.full(per - len(sel), -1)]))
            gseq.append(b)
            nkeys.append(int(pos[sel].max()) + 1)
    return np.stack(rows).astype(np.int32), np.asarray(gseq, dtype=np.int32), np.asarray(nkeys, dtype=np.int32)


def _hostile_groups(pos, seq, per, seed=0):
    """Groups built by hand: per sequence, first a group holding ONE live row, then groups whose live rows alternate between the
    two ends of the sequence (position 0 next to position L - 1, 1 next to L - 2, ...: whole key blocks fully masked for some lanes
    and fully visible for others), per // 3 of them scattered over the `per` slots among padding."""
    rng = np.random.default_rng(seed)
    rows, gseq, nkeys = [], [], []

    def put(sel, b):
        slot = np.full(per, -1)
        slot[rng.choice(per, len(sel), replace=False)] = sel
        rows.append(slot); gseq.append(b); nkeys.append(int(pos[sel].max()) + 1)

    for b in np.unique(seq):
        idx = np.nonzero(seq == b)[0]
        idx = idx[np.argsort(pos[idx], kind="stable")]
        far = np.empty_like(idx)
        far[0::2], far[1::2] = idx[:(len(idx) + 1) // 2], idx[::-1][:len(idx) // 2]
        put(far[:1], b)
        for c in range(1, len(far), per // 3):
            put(far[c:c + per // 3], b)
    return np.stack(rows).astype(np.int32), np.asarray(gseq, dtype=np.int32), np.asarray(nkeys, dtype=np.int32)


def _check_groups(host, groups, qt):
    """Every index a launch carries is asserted in range on the host: rows, positions, sequences, page ids, the group lists."""
    rows, gseq, nkeys = groups
    pos, seq, cache = host.pos, host.seq, host.cache
    R = len(pos)
    assert len(seq) == R and seq.min() >= 0 and seq.max() < len(cache.lens)
    assert pos.min() >= 0 and bool((pos < np.asarray(cache.lens)[seq]).all())
    assert int(cache.table.min()) >= 0 and int(cache.table.max()) < cache.k.shape[0] and int(pos.max()) // 64 < cache.max_pages
    assert rows.ndim == 2 and rows.shape[1] == qt * 16 and len(gseq) == len(nkeys) == rows.shape[0]
    assert rows.min() >= -1 and rows.max() < R
    live = rows[rows >= 0]
    assert len(live) == R and len(np.unique(live)) == R                         # every row in exactly one slot
    for g in range(rows.shape[0]):
        sel = rows[g][rows[g] >= 0]
        assert len(sel) > 0 and 0 <= gseq[g] < len(cache.lens) and bool((seq[sel] == gseq[g]).all())
        assert pos[sel].max() + 1 <= nkeys[g] <= cache.lens[gseq[g]]


class _Dev:
    """The batch on the device + launches of the grouped form."""

    def __init__(self, host):
        from uniaudio2_amd import ops
        self.ops, self.h = ops, host
        c = host.cache
        self.k, self.v, self.t = c.k.cuda(), c.v.cuda(), c.table.cuda()
        self.geom = ops.kv_geom(self.k, self.v, self.t, host.nh, c.n_kv, c.hs)
        self.q, self.pos, self.seq = host.q.cuda(), torch.from_numpy(host.pos).cuda(), torch.from_numpy(host.seq).cuda()

    def groups(self, qt):
        rows, gseq, nkeys, got = self.ops.attn_groups(self.h.pos, self.h.seq, self.h.nh, self.h.nkv, "cpu", q_tiles=qt)
        assert got == qt
        return rows.numpy(), gseq.numpy(), nkeys.numpy()

    def run(self, groups, qt, flags=0, window=0, want_y=True, y_packed=None, chunk=None, expect_one_page=None):
        """One launch, or launches of at most `chunk` groups.  expect_one_page: the side of the bf16-QP dispatch rule
        (n_groups * n_kv > 256) every launch must fall on, asserted on the host."""
        _check_groups(self.h, groups, qt)
        R = len(self.h.pos)
        y = torch.full((R, self.h.nh * self.h.hs), float("nan"), device="cuda") if want_y else None     # an unwritten element stays NaN
        n = groups[0].shape[0]
        for c in range(0, n, chunk or n):
            part = tuple(torch.from_numpy(np.ascontiguousarray(a[c:c + (chunk or n)])).cuda() for a in groups)
            if expect_one_page is not None:
                assert (part[0].shape[0] * self.h.nkv > 256) == expect_one_page
            self.ops.attn(dtype=BF16, R=R, q=self.q, row_pos=self.pos, row_seq=self.seq, kv=self.geom, y=y, window=window,
                          groups=part + (qt,), y_packed=y_packed, flags=flags)
        torch.cuda.synchronize()
        return y


def _report(tag, err, e_model, bar):
    print(f"PARITY {tag}: err {err:.3e} E_model {e_model:.3e} bar {bar:.3e}")


# ---- every fp32-grade instantiation, at the edges -----------------------------------------------------------------------------------

@pytest.mark.parametrize("nh,nkv,hs,qt", _geom_params(FLASH_GEOMS))
def test_flash_causal_parity(nh, nkv, hs, qt):
    """Every position of 18 sequences (1 .. 300 keys: below, at and past every 16-row tile, 64-key page and 128-key pair edge) is a
    query row, grouped by ops.attn_groups."""
    host = _randn_batch(nh, nkv, hs)
    dev = _Dev(host)
    y = dev.run(dev.groups(qt), qt)
    err, e_model = kr.abs_err(y, host.ref()), host.e_model("split")
    _report(f"flash causal {_inst(nh, nkv, hs, qt)} {nh}/{nkv}/{hs} rows={len(host.pos)}", err, e_model, BAR)
    assert err < BAR


@pytest.mark.parametrize("nh,nkv,hs,qt", _geom_params([g for g in FLASH_GEOMS if g[0] == g[1]]))
def test_flash_dense_parity(nh, nkv, hs, qt):
    """Every row at pos = L - 1 (how the encoders and the DiT call it): the G = 1 geometries."""
    host = _randn_batch(nh, nkv, hs, dense=True)
    dev = _Dev(host)
    y = dev.run(dev.groups(qt), qt)
    err, e_model = kr.abs_err(y, host.ref()), host.e_model("split")
    _report(f"flash dense {_inst(nh, nkv, hs, qt)} {nh}/{nkv}/{hs} rows={len(host.pos)}", err, e_model, BAR)
    assert err < BAR


@pytest.mark.parametrize("nh,nkv,hs,qt", _geom_params([(4, 4, 64, 4), (8, 2, 64, 2)]))
def test_flash_hostile_grouping(nh, nkv, hs, qt):
    """Hand-built groups (far-apart positions in one tile, live rows scattered among padding, a group of one live row): the bits of
    the ops.attn_groups launch, and the same float64 bar."""
    host = _randn_batch(nh, nkv, hs)
    dev = _Dev(host)
    base = dev.run(dev.groups(qt), qt)
    groups = _hostile_groups(host.pos, host.seq, qt * 16)
    live = (groups[0] >= 0).sum(1)
    assert live.min() == 1 and live.max() < qt * 16
    spread = max(int(np.ptp(host.pos[r[r >= 0]])) for r in groups[0])
    assert spread >= 256                                                            # some tile holds rows more than four key blocks apart
    y = dev.run(groups, qt)
    assert torch.equal(y, base)
    err, e_model = kr.abs_err(y, host.ref()), host.e_model("split")
    _report(f"flash hostile-grouping {_inst(nh, nkv, hs, qt)} {nh}/{nkv}/{hs} groups={len(live)}", err, e_model, BAR)
    assert err < BAR


@pytest.mark.parametrize("window", [1, 64, 65])
@pytest.mark.parametrize("nh,nkv,hs,qt", [pytest.param(4, 2, 64, 2, id="row-kernel-4/2/64"), pytest.param(24, 8, 128, 2, id="row-kernel-24/8/128")])
def test_groups_with_a_window_give_the_windowed_result(nh, nkv, hs, qt, window):
    """A launch with `groups` and window > 0 has no flash kernel: the dispatcher drops to the row kernel, and the result is the
    windowed one (not the full-context result a flash launch that ignored the window would give)."""
    host = _randn_batch(nh, nkv, hs, lens=(1, 64, 65, 130, 300))
    dev = _Dev(host)
    y = dev.run(dev.groups(qt), qt, window=window)
    err = kr.abs_err(y, host.ref(window))
    print(f"PARITY flash groups+window={window} {nh}/{nkv}/{hs} rows={len(host.pos)}: err {err:.3e} bar {BAR:.1e}")
    assert err < BAR
    assert kr.abs_err(y, host.ref()) > 100 * BAR                                    # the two results are far apart: the check can tell


# ---- hostile but finite values ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", kr.HOSTILE_KINDS)
@pytest.mark.parametrize("nh,nkv,hs,qt", _geom_params([(24, 8, 128, 2), (8, 2, 64, 2), (4, 4, 32, 4)]))
def test_flash_hostile_finite_values(nh, nkv, hs, qt, kind):
    """kernel_refs.hostile_inputs: the four kinds of the decode test, plus a block maximum that rises at every step and one that
    sits in block 0 while the later weights underflow.  Relative to the row's max magnitude; bar from the host model."""
    host = _hostile_batch(kind, nh, nkv, hs)
    dev = _Dev(host)
    y = dev.run(dev.groups(qt), qt)
    err, e_model = kr.rel_row_err(y, host.ref()), host.e_model("split")
    b = max(4.0 * e_model, FLOOR)
    _report(f"flash hostile {kind} {_inst(nh, nkv, hs, qt)} {nh}/{nkv}/{hs}", err, e_model, b)
    assert 4.0 * e_model <= 1e-3                                                    # the inputs' own condition (tests/test_kernel_refs.py)
    assert err <= b


# ---- the bf16 q / weights forms -----------------------------------------------------------------------------------------------------

def _qp_check(tag, host, y, kps, unit_scale):
    """(a) against float64 at the model's own error; (b) against the model, at the distance legal score noise moves it."""
    ref = host.ref()
    err, e_model = kr.rel_row_err(y, ref), host.e_model("bf16", kps)
    m32, m64 = host.model("bf16", kps), host.model("bf16", kps, torch.float64)
    err_m, e_flip = kr.rel_row_err(y, m32), kr.rel_row_err(m32, m64)
    bar_a, bar_b = 4.0 * e_model, max(4.0 * e_flip, FLOOR)
    print(f"PARITY flash-qp {tag} keys/step={kps} (a): err {err:.3e} E_model {e_model:.3e} bar {bar_a:.3e}")
    print(f"PARITY flash-qp {tag} keys/step={kps} (b): err {err_m:.3e} E_flip {e_flip:.3e} bar {bar_b:.3e}")
    if unit_scale:
        abs_e = kr.abs_err(y, ref)
        print(f"PARITY flash-qp {tag} keys/step={kps} abs: err {abs_e:.3e} bar {BAR_QP:.1e}")
        assert abs_e < BAR_QP
    assert err <= bar_a
    assert err_m <= bar_b


QP_FORMS = {"hs64-G1-QT8-QP-1page": 64, "hs64-G1-QT8-QP-2pages": 128}           # instantiation -> keys per softmax step


def _qp_run(host, form, small=False):
    """The dispatch goes by n_groups * n_kv > 256, asserted per launch on the host.  One page per step: every group in one launch.
    Two pages per step: launches of at most ten groups.
    small: a batch of fewer than eleven full groups reaches the one-page form cut into groups of 32 live rows."""
    from uniaudio2_amd._lib import ATTN_BF16_QP
    nh, nkv, hs, qt = QP_GEOM
    dev = _Dev(host)
    if QP_FORMS[form] == 64:
        return dev.run(_cut_groups(host.pos, host.seq, qt * 16, live=32) if small else dev.groups(qt), qt, flags=ATTN_BF16_QP,
                       expect_one_page=True)
    return dev.run(dev.groups(qt), qt, flags=ATTN_BF16_QP, chunk=10, expect_one_page=False)


@pytest.mark.parametrize("dense", [True, False], ids=["dense", "causal"])
@pytest.mark.parametrize("form", QP_FORMS)
def test_flash_bf16_qp_parity(form, dense):
    """UA2_ATTN_BF16_QP, hs 64, G 1, 8 query tiles, twelve sequences of 1 .. 500 keys: in one launch (more than 256 workgroups: one
    page per step), and in launches of ten groups (two pages per step)."""
    host = _randn_batch(*QP_GEOM[:3], dense=dense, lens=tuple(QP_LENS))
    _qp_check(f"{'dense' if dense else 'causal'} {form}", host, _qp_run(host, form), QP_FORMS[form], unit_scale=True)


@pytest.mark.parametrize("dense", [True, False], ids=["dense", "causal"])
def test_flash_bf16_qp_forms_differ_past_128_keys(dense):
    """The kernel comment documents that the two forms' bits differ (other block boundaries of the online softmax): both really ran."""
    host = _randn_batch(*QP_GEOM[:3], dense=dense, lens=tuple(QP_LENS))
    y1, y2 = (_qp_run(host, form) for form in QP_FORMS)
    far = torch.from_numpy(host.pos >= 128).cuda()                                  # rows with more than 128 keys
    assert int(far.sum()) > 0 and not torch.equal(y1[far], y2[far])


@pytest.mark.parametrize("kind", kr.HOSTILE_KINDS)
@pytest.mark.parametrize("form", QP_FORMS)
def test_flash_bf16_qp_hostile_finite_values(form, kind):
    """The hostile kinds through both bf16 q / weights forms.  A row's bits do not depend on the grouping, so the one-page form is
    reached with 32 live rows per group (18 groups x 24 heads), the two-page form with full groups (7 x 24)."""
    host = _hostile_batch(kind, *QP_GEOM[:3])
    _qp_check(f"hostile {kind} {form}", host, _qp_run(host, form, small=True), QP_FORMS[form], unit_scale=False)


# ---- packed output of the flash form ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nh,nkv,hs,qt,qp", [pytest.param(24, 8, 128, 2, False, id=_inst(24, 8, 128, 2)), pytest.param(4, 4, 64, 8, False, id=_inst(4, 4, 64, 8)),
                                              pytest.param(4, 4, 64, 8, True, id=_inst(4, 4, 64, 8, "-QP-2pages"))])
def test_flash_packed_output(nh, nkv, hs, qt, qp):
    """y_packed of the flash form (what the DiT and the Whisper encoder consume) = RNE-bf16 of y in ua2_linear's operand order, bit
    for bit, with y and without it (y = None, as the product launches it); rows beyond R untouched; and ua2_linear reads the same
    bits from x = y and from x_packed = y_packed."""
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import ATTN_BF16_QP
    host = _randn_batch(nh, nkv, hs, lens=(37, 70, 64))
    dev = _Dev(host)
    R, K = len(host.pos), nh * hs
    assert R % 16 != 0
    sentinel = 12352.0                                                              # a bf16 number no attention output of randn values reaches
    groups, flags = dev.groups(qt), ATTN_BF16_QP if qp else 0
    pk = torch.full(((R + 15) // 16 * 16 * K,), sentinel, dtype=BF16, device="cuda")
    pk_alone = pk.clone()
    y = dev.run(groups, qt, flags=flags, y_packed=pk)
    assert dev.run(groups, qt, flags=flags, y_packed=pk_alone, want_y=False) is None
    assert bool(torch.isfinite(y).all())
    assert kr.packed_mismatch(pk, y, R, K, BF16, sentinel) is None
    assert torch.equal(pk.view(torch.int16), pk_alone.view(torch.int16))
    N = 96
    w = ops.pack_linear(torch.randn(N, K, generator=torch.Generator().manual_seed(8)).cuda(), BF16)
    z_x, z_pk = torch.zeros(R, N, device="cuda"), torch.zeros(R, N, device="cuda")
    ops.linear(dtype=BF16, M=R, N=N, K=K, w0=w, x=y, y=z_x)
    ops.linear(dtype=BF16, M=R, N=N, K=K, w0=w, x_packed=pk_alone, y=z_pk)
    torch.cuda.synchronize()
    assert torch.equal(z_x, z_pk)


# ---- local (depth decoder) attention ------------------------------------------------------------------------------------------------

LOCAL_POS = [0, 1, 2, 3, 4, 5, 6, 7, 3, 7, 0]          # one row for every position, 11 rows


@pytest.mark.parametrize("kind", ["randn", "peaked_q"])
@pytest.mark.parametrize("permuted", [False, True], ids=["row_seq=None", "row_seq=perm"])
@pytest.mark.parametrize("nh,nkv,hs", [(32, 8, 64), (4, 2, 32), (8, 4, 128), (24, 8, 128), (40, 8, 64)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_local_attention_parity(dtype, nh, nkv, hs, permuted, kind):
    """ua2_attn_local against float64 on an 8-key cache whose slots above pos, and the rest of the page, are loud.  24/8/128 and
    40/8/64 need a second, partial pass of the head loop (n_head / (128 / hs) = 24, 20 > 16 waves)."""
    from uniaudio2_amd import ops
    B = len(LOCAL_POS)
    lens = [p + 1 for p in LOCAL_POS]
    cache = kr.PagedCache(lens, nkv, hs, dtype, seed=nh + hs, fill=LOUD, extra_pages=2)
    assert cache.table.shape == (B, 1) and max(lens) <= 8
    seq = np.random.default_rng(3).permutation(B).astype(np.int32) if permuted else np.arange(B, dtype=np.int32)
    pos = np.asarray(LOCAL_POS, dtype=np.int32)[seq]
    assert int(cache.table.min()) >= 0 and int(cache.table.max()) < cache.k.shape[0] and seq.min() >= 0 and seq.max() < B
    assert bool((pos < np.asarray(lens)[seq]).all()) and pos.min() >= 0 and pos.max() < 8
    q = torch.randn(B, nh * hs, generator=torch.Generator().manual_seed(hs + nh)) * (8.0 if kind == "peaked_q" else 1.0)
    k, v, t = cache.k.cuda(), cache.v.cuda(), cache.table.cuda()
    y = torch.full((B, nh * hs), float("nan"), device="cuda")
    ops.attn_local(dtype=dtype, R=B, q=q.cuda(), row_pos=torch.from_numpy(pos).cuda(), row_seq=torch.from_numpy(seq).cuda() if permuted else None,
                   kv=ops.kv_geom(k, v, t, nh, nkv, hs), y=y)
    torch.cuda.synchronize()
    KV = [cache.stored_seq(b) for b in range(B)]
    Ks, Vs = [a for a, _ in KV], [b for _, b in KV]
    ref = kr.attn_ref(q, Ks, Vs, pos, seq, nh, nkv)
    err = kr.rel_row_err(y, ref)
    e_ref = kr.rel_row_err(kr.attn_ref(q, Ks, Vs, pos, seq, nh, nkv, dt=torch.float32), ref)
    b = kr.bar(e_ref)
    print(f"PARITY local {kind} {dtype} {nh}/{nkv}/{hs} {'row_seq=perm' if permuted else 'row_seq=None'}: err {err:.3e} E_ref {e_ref:.3e} bar {b:.3e}")
    assert err <= b
