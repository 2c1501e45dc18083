"""GPU parity of the kernels that turn raw audio into tokens — csrc/ua2_wavlm.hip (ua2_wavlm_conv0, ua2_conv1d_grouped,
ua2_relpos_gate, ua2_attn_relbias in both forms), csrc/ua2_conv2d.hip and csrc/ua2_bestrq.hip (ua2_layernorm_rope_rows,
ua2_melspec_db) — against the float64 restatements of tests/encoder_refs.py, under the project's bar kr.bar(E, scale) =
max(4 E, 8 * 2^-24 * scale).  E is the error of the same formula replayed in fp32 on the host (the convolutions: in the kernel's
reduction order; conv0: the contract of include/ua2hip.h); for the bf16 flash form of ua2_attn_relbias it is the error of
encoder_refs.relbias_flash_model (16-bit q and weights, one page per step, the bias in the log2 domain), and the device is held to
the model under kr.bar(E_model, scale) and to float64 of the stored K / V under that bar + E_model.

Every launch prints `PARITY encoder <kernel> <case>: err .. E .. bar ..`.  Outputs are prefilled with a finite sentinel (NaN for
the attention outputs, as tests/test_gpu_wavlm.py does); the kernels that store 16 bytes at a time write into the middle of a
larger buffer whose guard bands must keep their bits; every index a launch carries is asserted in range on the host; only finite
values are sent to a kernel, stale cache slots hold 3e4.  tests/test_encoder_refs_host.py holds the generators below to narrow
bars on the CPU and shows that wrong models fail the assertions used here."""
import functools

import numpy as np
import pytest
import torch

import bestrq_ref as br
import encoder_refs as er
import kernel_refs as kr
import wavlm_ref as wr

pytestmark = pytest.mark.gpu

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
SENT = 12352.0                                  # a bf16 number none of these outputs reaches
GUARD = 64                                      # floats on either side of a guarded output (16-byte aligned)
MEL_MEAN, MEL_STD = br.MEL_MEAN, br.MEL_STD


def _line(kernel, case, err, e, bar, what="E_ref"):
    print(f"PARITY encoder {kernel} {case}: err {err:.3e} {what} {e:.3e} bar {bar:.3e}")


def _guarded(n):
    """(whole buffer, the n floats in its middle) on the device, all sentinel."""
    buf = torch.full((n + 2 * GUARD,), SENT, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all())


def _dev(t):
    return None if t is None else t.contiguous().cuda()


# ---- ua2_attn_relbias -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def batch(hs, dtype, dense):
    if dense:
        H, T = er.DENSE[hs]
        return er.RelbiasBatch([T], H, hs, dtype, dense=True)
    H, lens = er.RAGGED[hs]
    return er.RelbiasBatch(lens, H, hs, dtype)


@functools.lru_cache(maxsize=None)
def hostile(kind, hs, dtype):
    return er.RelbiasBatch(er.HOSTILE_LENS, 2, hs, dtype, kind=kind, seed=1)


def _check_batch(b):
    """Every index the launch carries, on the host."""
    c = b.cache
    R = len(b.pos)
    assert len(b.seq) == len(b.q_pos) == R and b.seq.min() >= 0 and b.seq.max() < len(c.lens)
    assert b.pos.min() >= 0 and bool((b.pos < np.asarray(c.lens)[b.seq]).all())
    assert int(c.table.min()) >= 0 and int(c.table.max()) < c.k.shape[0] and int(b.pos.max()) // 64 < c.max_pages
    assert b.tab.shape == (b.H, 2 * b.tab_half + 1) and b.gate.shape == (R, b.H) and b.q.shape == (R, b.H * b.hs)
    assert all(bool(torch.isfinite(t).all()) for t in (b.q, b.gate, b.tab, c.k.float(), c.v.float()))


def _check_groups(b, groups, qt):
    rows, gseq, nkeys = groups
    R = len(b.pos)
    assert rows.ndim == 2 and rows.shape[1] == qt * 16 and len(gseq) == len(nkeys) == rows.shape[0]
    assert rows.min() >= -1 and rows.max() < R
    live = rows[rows >= 0]
    assert len(live) == R and len(np.unique(live)) == R                               # every row in exactly one slot
    for g in range(rows.shape[0]):
        sel = rows[g][rows[g] >= 0]
        assert len(sel) > 0 and 0 <= gseq[g] < len(b.lens) and bool((b.seq[sel] == gseq[g]).all())
        assert b.pos[sel].max() + 1 <= nkeys[g] <= b.lens[gseq[g]]


def _far_groups(b, per, seed=0):
    """Groups built by hand: per sequence the rows alternate between the two ends (position 0 next to L - 1, 1 next to L - 2, ...),
    per // 3 of them scattered over the `per` slots of a group among -1 padding."""
    rng = np.random.default_rng(seed)
    rows, gseq, nkeys = [], [], []
    for s in np.unique(b.seq):
        idx = np.nonzero(b.seq == s)[0]
        idx = idx[np.argsort(b.q_pos[idx], kind="stable")]
        far = np.empty_like(idx)
        far[0::2], far[1::2] = idx[:(len(idx) + 1) // 2], idx[::-1][:len(idx) // 2]
        for c in range(0, len(far), per // 3):
            sel = far[c:c + per // 3]
            slot = np.full(per, -1)
            slot[rng.choice(per, len(sel), replace=False)] = sel
            rows.append(slot); gseq.append(s); nkeys.append(int(b.pos[sel].max()) + 1)
    return np.stack(rows).astype(np.int32), np.asarray(gseq, dtype=np.int32), np.asarray(nkeys, dtype=np.int32)


class _Attn:
    """The batch on the device + launches of either form."""

    def __init__(self, b):
        from uniaudio2_amd import ops
        _check_batch(b)
        self.ops, self.b = ops, b
        c = b.cache
        self.k, self.v, self.t = c.k.cuda(), c.v.cuda(), c.table.cuda()
        self.geom = ops.kv_geom(self.k, self.v, self.t, b.H, b.H, b.hs)
        self.q, self.gate, self.tab = _dev(b.q), _dev(b.gate), _dev(b.tab)
        self.pos, self.seq, self.q_pos = (torch.from_numpy(a).cuda() for a in (b.pos, b.seq, b.q_pos))

    def groups(self, qt):
        rows, gseq, nkeys, got = self.ops.attn_groups(self.b.pos, self.b.seq, self.b.H, self.b.H, "cpu", q_tiles=qt)
        assert got == qt
        return rows.numpy(), gseq.numpy(), nkeys.numpy()

    def run(self, groups=None, qt=None, want_y=True, y_packed=None):
        b = self.b
        R = len(b.pos)
        assert (groups is not None) == (b.dtype == BF16)
        g = None
        if groups is not None:
            _check_groups(b, groups, qt)
            self.keep = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in groups)
            g = self.keep + (qt,)
        y = torch.full((R, b.H * b.hs), float("nan"), device="cuda") if want_y else None   # an unwritten element stays NaN
        self.ops.attn_relbias(dtype=b.dtype, R=R, q=self.q, row_pos=self.pos, row_seq=self.seq, kv=self.geom, q_pos=self.q_pos, gate=self.gate,
                              rel_tab=self.tab, y=y, groups=g, y_packed=y_packed)
        torch.cuda.synchronize()
        return None if y is None else y.cpu()


def _rows_case(tag, b):
    ok, err, e, bar = er.check_rows_fp32(_Attn(b).run(), b)
    _line(f"attn_relbias rows<{b.hs}>", f"{tag} lens={b.lens if len(b.lens) > 1 else b.lens[0]} H={b.H} max|ref|={float(b.ref().abs().max()):.2f}", err, e, bar)
    assert ok


def _flash_case(tag, b, y, qt):
    ok, err_m, err_r, e, bar = er.check_flash_bf16(y, b)
    _line(f"attn_relbias flash<{b.hs},{qt}>", f"{tag} lens={b.lens if len(b.lens) > 1 else b.lens[0]} H={b.H} vs float64 {err_r:.3e}", err_m, e, bar, "E_model")
    assert ok


@pytest.mark.parametrize("hs", [64, 128], ids=["rows64", "rows128"])
def test_relbias_rows_ragged(hs):
    """Every position of every sequence a query row with its own row_pos (rows of 1 and 7 keys: waves without a key)."""
    _rows_case("ragged", batch(hs, F32, False))


@pytest.mark.parametrize("hs", [64, 128], ids=["rows64-T1500", "rows128-T300"])
def test_relbias_rows_dense(hs):
    """row_pos = T - 1 for all rows, q_pos = arange: T = 1500 with tab_half 1499 is the released call of one head pair."""
    _rows_case("dense", batch(hs, F32, True))


@pytest.mark.parametrize("kind", er.HOSTILE_KINDS)
@pytest.mark.parametrize("hs", [64, 128], ids=["rows64", "rows128"])
def test_relbias_rows_hostile(hs, kind):
    _rows_case(kind, hostile(kind, hs, F32))


FLASH = [pytest.param(64, 4, id="flash64x4"), pytest.param(64, 8, id="flash64x8"), pytest.param(128, 4, id="flash128x4")]


@pytest.mark.parametrize("hs,qt", FLASH)
def test_relbias_flash_ragged_and_grouping(hs, qt):
    """The ragged batch through ops.attn_groups, then through hand-built groups (positions 0 and L - 1 = 129 of one sequence in one tile,
    live rows among -1 padding): the same bits, and the two bars."""
    b = batch(hs, BF16, False)
    dev = _Attn(b)
    y = dev.run(dev.groups(qt), qt)
    _flash_case("ragged", b, y, qt)
    far = _far_groups(b, qt * 16)
    live = (far[0] >= 0).sum(1)
    assert live.max() < qt * 16 and any({0, max(b.lens) - 1} <= set(b.q_pos[r[r >= 0]].tolist()) for r in far[0])
    assert torch.equal(dev.run(far, qt), y), "a row's result depends on how the rows are grouped"


def test_relbias_flash_instantiations_agree():
    """<64,4> and <64,8> on the ragged batch: torch.equal (head size 128 has one instantiation)."""
    dev = _Attn(batch(64, BF16, False))
    assert torch.equal(dev.run(dev.groups(4), 4), dev.run(dev.groups(8), 8))


@pytest.mark.parametrize("hs,qt", [pytest.param(64, 8, id="flash64x8-T1500"), pytest.param(128, 4, id="flash128x4-T300")])
def test_relbias_flash_dense(hs, qt):
    """T = 1500: 24 pages and a table row of 2 999 floats in LDS; head size 128: the big-LDS path."""
    b = batch(hs, BF16, True)
    dev = _Attn(b)
    _flash_case("dense", b, dev.run(dev.groups(qt), qt), qt)


@pytest.mark.parametrize("kind", er.HOSTILE_KINDS)
@pytest.mark.parametrize("hs,qt", [pytest.param(64, 4, id="flash64x4"), pytest.param(128, 4, id="flash128x4")])
def test_relbias_flash_hostile(hs, qt, kind):
    b = hostile(kind, hs, BF16)
    dev = _Attn(b)
    _flash_case(kind, b, dev.run(dev.groups(qt), qt), qt)


@pytest.mark.parametrize("dtype,qt", [pytest.param(F32, None, id="rows64-packed"), pytest.param(BF16, 8, id="flash64x8-packed")])
def test_relbias_packed_output(dtype, qt):
    """y_packed of both forms = the row-major output rounded to the operand dtype in ua2_linear's operand order, bit for bit, with y
    and alone; rows beyond R (R no multiple of 16) keep the sentinel."""
    b = batch(64, dtype, False)
    dev = _Attn(b)
    R, K = len(b.pos), b.H * b.hs
    assert R % 16 != 0
    groups = dev.groups(qt) if qt else None
    pk = torch.full(((R + 15) // 16 * 16 * K,), SENT, dtype=dtype, device="cuda")
    pk_alone = pk.clone()
    y = dev.run(groups, qt, y_packed=pk)
    assert dev.run(groups, qt, want_y=False, y_packed=pk_alone) is None
    assert bool(torch.isfinite(y).all())
    assert kr.packed_mismatch(pk, y, R, K, dtype, SENT) is None
    bits = torch.int16 if dtype == BF16 else torch.int32
    assert torch.equal(pk.view(bits), pk_alone.view(bits))


# ---- ua2_conv1d_grouped ---------------------------------------------------------------------------------------------------------
# (B, T, C, groups, K, act, resid, bias).  C / groups = 16, 32, 48, 64: 1, 2 (one dead slot of the three), 3 and 4 (a second row block
# with one live slot) row tiles per group; T below, at and past the 128-step workgroup edge; K = 1, 2, odd, and the released 128;
# the epilogue arms apart from one another
GCONV_CASES = [(1, 37, 64, 4, 16, True, True, True), (2, 37, 64, 2, 16, True, True, True), (1, 37, 96, 2, 16, True, True, True),
               (1, 37, 128, 2, 16, True, True, True),
               (1, 1, 32, 2, 16, True, True, True), (1, 127, 32, 2, 16, True, True, True), (1, 128, 32, 2, 16, True, True, True),
               (1, 129, 32, 2, 16, True, True, True), (1, 200, 64, 2, 16, True, True, True),
               (1, 19, 32, 2, 1, True, True, True), (1, 19, 32, 2, 2, True, True, True), (2, 19, 32, 2, 5, True, True, True),
               (1, 50, 768, 16, 128, True, True, True), (1, 200, 768, 16, 128, False, False, True),
               (1, 37, 64, 4, 16, True, True, False), (1, 37, 64, 4, 16, True, False, True), (1, 37, 64, 4, 16, False, True, True),
               (1, 37, 64, 4, 16, False, False, False)]


def _gconv_id(c):
    B, T, C, g, K, act, resid, bias = c
    return f"B{B}-T{T}-C{C}-g{g}-K{K}-tiles{C // g // 16}" + ("-gelu" if act else "") + ("-resid" if resid else "") + ("" if bias else "-nobias")


@functools.lru_cache(maxsize=None)
def gconv_host(case):
    B, T, C, groups, K, act, resid, bias = case
    x, w, b, r = er.gconv_case(B, T, C, groups, K, resid, bias, 6800 + GCONV_CASES.index(case))
    return x, w, b, r, er.grouped_conv_ref(x, w, b, groups, act, r), er.grouped_conv_replay(x, w, b, groups, act, r)


def _gconv_run(x, w, b, r, groups, act):
    """(output [B, T, C] on the host, guards intact)."""
    from uniaudio2_amd import ops
    B, T, C = x.shape
    buf, out = _guarded(B * T * C)
    ops.conv1d_grouped(_dev(x).view(B * T, C), ops.pack_conv1d_grouped_weight(_dev(w), groups), B, T, groups, w.shape[-1], bias=_dev(b),
                       resid=None if r is None else _dev(r).view(B * T, C), gelu=act, out=out.view(B * T, C))
    torch.cuda.synchronize()
    return out.cpu().view(B, T, C), _guards_intact(buf)


@pytest.mark.parametrize("case", GCONV_CASES, ids=_gconv_id)
def test_conv1d_grouped_parity(case):
    x, w, b, r, ref, replay = gconv_host(case)
    got, intact = _gconv_run(x, w, b, r, case[3], case[5])
    ok, err, e, bar = er.conv_check(got, ref, replay)
    _line("conv1d_grouped", _gconv_id(case), err, e, bar, "E_replay")
    assert intact, "a store landed outside the output"
    assert ok
    if case[0] == 2 and case[2] // case[3] == 32:
        alone, _ = _gconv_run(x[:1], w, b, None if r is None else r[:1], case[3], case[5])
        assert torch.equal(alone[0], got[0]), "row 0 of B = 2 differs from the row run alone"


def test_conv1d_grouped_refuses_the_wavlm_large_geometry():
    """1024 channels in 16 groups with K = 128: a window of 64 channels x 260 floats = 66 560 B does not fit 64 KiB of LDS; the
    launch is refused and nothing is written."""
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import Ua2Error
    T, C, groups, K = 8, 1024, 16, 128
    buf, out = _guarded(T * C)
    wpk = torch.zeros(C * (C // groups) * K, device="cuda")
    with pytest.raises(Ua2Error, match="does not fit LDS"):
        ops.conv1d_grouped(torch.zeros(T, C, device="cuda"), wpk, 1, T, groups, K, out=out.view(T, C))
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())


# ---- ua2_wavlm_conv0 ------------------------------------------------------------------------------------------------------------
# (B, T0, extra, C, K, stride, dc): N = (T0 - 1) stride + K + extra.  T0 on the 64-frame apply / run edges and the 256-frame chunk
# edges, half of them with (N - K) % stride != 0; K = 1; a second, partial channel block of the statistics kernel (C = 68) with
# K = 16 and stride 32; the released C = 512; B = 2; a clip with a DC offset (mean / std ~ 140)
CONV0_CASES = [(1, 1, 0, 32, 10, 5, 0.0), (1, 63, 3, 32, 10, 5, 0.0), (1, 64, 0, 32, 10, 5, 0.0), (1, 65, 2, 32, 10, 5, 0.0),
               (1, 255, 0, 32, 10, 5, 0.0), (1, 256, 4, 32, 10, 5, 0.0), (1, 257, 0, 32, 10, 5, 0.0), (1, 1025, 1, 32, 10, 5, 0.0),
               (1, 70, 0, 4, 1, 1, 0.0), (1, 300, 5, 68, 16, 32, 0.0), (1, 300, 2, 512, 10, 5, 0.0), (2, 300, 0, 32, 10, 5, 0.0),
               (1, 799, 0, 32, 10, 5, 30.0)]


def _conv0_id(c):
    B, T0, extra, C, K, stride, dc = c
    return f"B{B}-T0_{T0}+{extra}-C{C}-K{K}-s{stride}" + (f"-dc{dc:g}" if dc else "")


def _conv0_run(x, w, gw, gb, stride, eps=1e-5):
    """(output [B, T0, C] on the host, guards intact); the output lies in the middle of a larger buffer."""
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import lib
    B, N = x.shape
    C, K = w.shape
    assert N >= K and C % 4 == 0 and 1 <= K <= 16 and 1 <= stride <= 32
    T0 = (N - K) // stride + 1
    n = lib.ua2_wavlm_conv0_workspace_bytes(B, N, C, K, stride)
    ws = torch.empty(max(n // 8, 1), dtype=F64, device="cuda")
    buf, out = _guarded(B * T0 * C)
    xd, wd, gwd, gbd = _dev(x), _dev(w), _dev(gw), _dev(gb)
    ops.check(lib.ua2_wavlm_conv0(ops.ptr(out), ops.ptr(xd), ops.ptr(wd), ops.ptr(gwd), ops.ptr(gbd), B, N, C, K, stride, eps, ops.ptr(ws),
                                  ws.numel() * 8, ops.stream()), "ua2_wavlm_conv0")
    torch.cuda.synchronize()
    return out.cpu().view(B, T0, C), _guards_intact(buf)


@pytest.mark.parametrize("case", CONV0_CASES, ids=_conv0_id)
def test_wavlm_conv0_parity(case):
    B, T0, extra, C, K, stride, dc = case
    N = (T0 - 1) * stride + K + extra
    assert (N - K) // stride + 1 == T0
    x = er.conv0_clip(B, N, 6600 + CONV0_CASES.index(case), dc)
    w, gw, gb = er.conv0_weights(C, K, 6700 + CONV0_CASES.index(case))
    got, intact = _conv0_run(x, w, gw, gb, stride)
    ref = er.conv0_ref(x, w, gw, gb, stride)
    replay = er.conv0_replay(x, w, gw, gb, stride)
    ok, err, e, bar = er.conv_check(got, ref, replay)
    e_plain = kr.abs_err(er.conv0_ref(x, w, gw, gb, stride, dt=F32), ref)
    _line("wavlm_conv0", f"{_conv0_id(case)} plain-fp32 {e_plain:.3e} max|ref|={float(ref.abs().max()):.2f}", err, e, bar, "E_replay")
    assert intact, "a store landed outside the output"
    assert ok
    if B == 2:
        alone, _ = _conv0_run(x[:1], w, gw, gb, stride)
        assert torch.equal(alone[0], got[0]), "row 0 of B = 2 differs from the row run alone"


def test_wavlm_conv0_constant_clip_is_the_one_frame_launch():
    """A constant non-zero clip: every conv value of a channel is the same fp32 number and the mean (sums in double) is that number,
    so v - mean is exactly 0 and every frame is GELU(gn_b) whatever rstd: the bits of the one-frame launch of the same weights."""
    C, K, stride, T0 = 32, 10, 5, 300
    w, gw, gb = er.conv0_weights(C, K, 6790)
    many, intact = _conv0_run(torch.full((1, (T0 - 1) * stride + K), 0.7), w, gw, gb, stride)
    one, _ = _conv0_run(torch.full((1, K), 0.7), w, gw, gb, stride)
    assert intact and torch.equal(many[0], one[0].expand(T0, C))
    assert kr.abs_err(one[0, 0], wr.gelu(gb.double())) <= 2.0 ** -22 * float(wr.gelu(gb.double()).abs().max())


# ---- ua2_relpos_gate ------------------------------------------------------------------------------------------------------------
# (R, H, hs, scale of w): 255 and 256 threads' worth of (row, head) pairs, a second workgroup with one live thread, the smallest head
# size, the two cases of tests/test_gpu_wavlm.py; w x 40 saturates both sigmoids
GATE_CASES = [(51, 5, 64, 1.0), (64, 4, 64, 1.0), (257, 1, 128, 1.0), (3, 2, 4, 1.0), (37, 2, 64, 1.0), (5, 12, 64, 1.0), (51, 5, 64, 40.0)]


@pytest.mark.parametrize("case", GATE_CASES, ids=lambda c: f"R{c[0]}-H{c[1]}-hs{c[2]}" + (f"-wx{c[3]:g}" if c[3] != 1 else ""))
def test_relpos_gate_parity(case):
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import lib
    R, H, hs, ws = case
    h, w, b, c = wr.gate_case(R, H, hs)
    w = (w * ws).contiguous()
    ref = er.gate_ref(h, w, b, c, H)
    if ws != 1:                                          # both sigmoids saturate: g -> 2 - a (b = 0) or a (c - 1) + 2 (b = 1), a in {0, 1}
        corners = torch.stack([torch.full_like(ref, 2.0), torch.full_like(ref, 1.0), (c.double() + 1.0).expand_as(ref)])
        assert float((corners - ref).abs().amin(0).median()) < 1e-6
    hd, wd, bd, cd = _dev(h), _dev(w), _dev(b), _dev(c)
    g = torch.full((R, H), SENT, device="cuda")
    ops.check(lib.ua2_relpos_gate(ops.ptr(g), ops.ptr(hd), ops.ptr(wd), ops.ptr(bd), ops.ptr(cd), R, H, hs, ops.stream()), "ua2_relpos_gate")
    torch.cuda.synchronize()
    err, e = kr.abs_err(g, ref), kr.abs_err(er.gate_ref(h, w, b, c, H, dt=F32), ref)
    bar = kr.bar(e)
    _line("relpos_gate", f"R={R} H={H} hs={hs} w x{ws:g}", err, e, bar)
    assert bool(torch.isfinite(g).all()) and err <= bar


# ---- ua2_layernorm_rope_rows ------------------------------------------------------------------------------------------------------
# (C, hs): one lane group, one wave, all four waves loaded once, a second partial pass of the c += 256 loops, the released width, the
# widest the entry point takes
LNROPE_CASES = [(32, 32), (64, 32), (256, 64), (320, 64), (1024, 64), (8192, 128)]
N_POS = 11


@functools.lru_cache(maxsize=None)
def lnrope_host(case):
    """Rows as in test_layernorm_rows: unit scale; mean 1e3; constant 2.5; x 1e-3; unit scale."""
    C, hs = case
    g = torch.Generator().manual_seed(9200 + C)
    x = torch.randn(5, C, generator=g)
    x[1] += 1e3
    x[2] = 2.5
    x[3] *= 1e-3
    w, b = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    cos, sin = br.rotary_tables(N_POS, hs, 10000)
    return x, w, b, cos.contiguous().float(), sin.contiguous().float(), torch.tensor([3, 0, 7, 10, 5], dtype=torch.int32), C, hs


def _lnrope_run(x, w, b, cos, sin, pos, hs):
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import lib
    R, C = x.shape
    assert cos.shape == sin.shape == (N_POS, hs) and C % hs == 0 and hs % 2 == 0 and C <= 8192 and pos.dtype == torch.int32
    out = torch.full((R, 2 * C), SENT, device="cuda")
    t = [_dev(a) for a in (x, w, b, cos, sin, pos)]
    ops.check(lib.ua2_layernorm_rope_rows(ops.ptr(out), *(ops.ptr(a) for a in t), N_POS, R, C, hs, 1e-5, ops.stream()), "ua2_layernorm_rope_rows")
    torch.cuda.synchronize()
    return out.cpu()


def _lnrope_check(case, use_w, use_b):
    from uniaudio2_amd import ops
    x, w, b, cos, sin, pos, C, hs = lnrope_host(case)
    w, b = (w if use_w else None), (b if use_b else None)
    got = _lnrope_run(x, w, b, cos, sin, pos, hs)
    ref = er.layernorm_rope_ref(x, w, b, 1e-5, cos, sin, pos, hs)
    ok, err, e, bar = er.rows_check(got, ref, er.layernorm_rope_ref(x, w, b, 1e-5, cos, sin, pos, hs, dt=F32))
    _line("layernorm_rope_rows", f"C={C} hs={hs} w={use_w} b={use_b}", err, e, bar)
    assert ok
    # the same rule row by row: the mean-1e3 row sets the launch's E_ref and must not hide the unit-scale rows behind its bar
    ref32 = er.layernorm_rope_ref(x, w, b, 1e-5, cos, sin, pos, hs, dt=F32)
    for r in range(x.shape[0]):
        ok_r, err_r, e_r, bar_r = er.rows_check(got[r], ref[r], ref32[r])
        assert ok_r, (r, err_r, e_r, bar_r)
    assert torch.equal(got[:, C:], ops.layernorm_rows(_dev(x), _dev(w), _dev(b), 1e-5).cpu())        # the plain half is ua2_layernorm_rows
    # the constant row: LayerNorm gives b (or 0) exactly, the rotation RN(RN(b cos) + RN(partner sin))
    bb = b if use_b else torch.zeros(C)
    assert torch.equal(got[2, C:], bb)
    bh = bb.view(C // hs, hs)
    assert torch.equal(got[2, :C], (bh * cos[int(pos[2])] + kr.rotate_half(bh) * sin[int(pos[2])]).reshape(C))
    return got


@pytest.mark.parametrize("case", LNROPE_CASES, ids=lambda c: f"C{c[0]}-hs{c[1]}")
def test_layernorm_rope_rows_parity(case):
    got = _lnrope_check(case, True, True)
    x, w, b, cos, sin, pos, C, hs = lnrope_host(case)
    wild = pos.clone()
    wild[1], wild[3] = -3, N_POS + 5                       # clamped to 0 and N_POS - 1: what rows 1 and 3 hold
    assert torch.equal(_lnrope_run(x, w, b, cos, sin, wild, hs), got)


@pytest.mark.parametrize("use_w,use_b", [(False, False), (True, False), (False, True)], ids=["plain", "w-only", "b-only"])
def test_layernorm_rope_rows_null_arms(use_w, use_b):
    _lnrope_check((1024, 64), use_w, use_b)


# ---- ua2_melspec_db ---------------------------------------------------------------------------------------------------------------
# (n_bins, n_mels, ld): the smallest; the released geometry; a second pass of the m0 += 128 loop with one live mel; an even bin
# count and a wider ld; three passes of the mel loop over a spectrum shorter than a workgroup
MEL_CASES = [(5, 1, 10), (1025, 128, 2064), (1025, 129, 2064), (1024, 200, 2080), (33, 300, 66)]


@functools.lru_cache(maxsize=None)
def mel_host(case):
    """spec [B T, ld]: randn x a per-frame scale of 1e-6, 1 or 1e3, frame 3 all zero, the columns beyond 2 n_bins at 3e4; a random
    non-negative filter bank whose columns 2 and 100 (where they exist, and n_mels > 1) are all zero."""
    nb, nm, ld = case
    B, T = 2, 5
    g = torch.Generator().manual_seed(9300 + nb + nm)
    scale = torch.tensor([1e-6, 1.0, 1e3, 1.0, 1.0, 1e3, 1e-6, 1.0, 1e3, 1.0])
    spec = torch.randn(B * T, ld, generator=g) * scale[:, None]
    spec[3] = 0.0
    spec[:, 2 * nb:] = er.LOUD
    fb = torch.rand(nb, nm, generator=g)
    for m in (2, 100):
        if m < nm:
            fb[:, m] = 0.0
    return spec, fb, B, T, nb, nm, ld


def _mel_run(spec, fb, B, T, nb, nm, ld):
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import lib
    assert spec.shape == (B * T, ld) and fb.shape == (nb, nm) and ld >= 2 * nb and bool(torch.isfinite(spec).all())
    out = torch.full((B, nm, T), SENT, device="cuda")
    sd, fd = _dev(spec), _dev(fb)
    ops.check(lib.ua2_melspec_db(ops.ptr(out), ops.ptr(sd), ops.ptr(fd), B, T, nb, nm, ld, MEL_MEAN, MEL_STD, ops.stream()), "ua2_melspec_db")
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("case", MEL_CASES, ids=lambda c: f"bins{c[0]}-mels{c[1]}-ld{c[2]}")
def test_melspec_db_parity(case):
    spec, fb, B, T, nb, nm, ld = mel_host(case)
    got = _mel_run(spec, fb, B, T, nb, nm, ld)
    ref = er.melspec_db_ref(spec, fb, B, T, nb, MEL_MEAN, MEL_STD)
    ok, err, e, bar = er.rows_check(got, ref, er.melspec_db_ref(spec, fb, B, T, nb, MEL_MEAN, MEL_STD, dt=F32))
    _line("melspec_db", f"n_bins={nb} n_mels={nm} ld={ld} max|ref|={float(ref.abs().max()):.2f}", err, e, bar)
    assert ok
    floor = (torch.tensor(-100.0) - torch.tensor(MEL_MEAN, dtype=F32)) / torch.tensor(MEL_STD, dtype=F32)
    assert bool((got[0, :, 3] == floor).all())                                     # the all-zero frame
    if nm > 2:
        assert bool((got[:, 2, :] == floor).all())                                 # an all-zero filter column
    quiet = spec.clone()
    quiet[:, 2 * nb:] = 0.0
    assert torch.equal(_mel_run(quiet, fb, B, T, nb, nm, ld), got)                 # the unused columns of spec influence nothing


# ---- ua2_conv2d -------------------------------------------------------------------------------------------------------------------
# (B, Cin, F, T, Cout, stride, residual, ReLU, bias).  The nine cases of tests/test_gpu_bestrq.py; then either side of the small-Cin
# switch (4 | 5); Cin = 17 (a second channel group that is nearly all padding); F = T = 1; To on and past the 64-step tile edge; Cout
# on and past the 128-row block edge; the arms bias = None and residual without ReLU
_RR = lambda B, Cin, Fq, T, Cout, stride, rr: (B, Cin, Fq, T, Cout, stride, rr, rr, True)
CONV2D_CASES = [_RR(*c) for c in [
    (2, 1, 16, 48, 16, (2, 2), False), (1, 16, 8, 24, 16, (1, 1), True), (2, 16, 7, 21, 32, (2, 2), False), (1, 48, 5, 3, 16, (2, 1), False),
    (1, 20, 6, 19, 24, (1, 2), True), (1, 3, 5, 9, 7, (1, 1), True), (1, 16, 3, 150, 144, (1, 2), False), (1, 16, 4, 10, 8, (2, 2), False),
    (1, 24, 5, 17, 40, (1, 1), True),
    (1, 4, 5, 9, 16, (1, 1), False), (1, 5, 5, 9, 16, (1, 1), True), (1, 17, 4, 10, 16, (2, 2), False), (1, 16, 1, 1, 16, (1, 1), False),
    (1, 16, 3, 127, 16, (1, 2), False), (1, 16, 3, 129, 16, (1, 2), True), (1, 16, 2, 20, 128, (2, 1), False), (1, 16, 2, 20, 129, (2, 1), True)]]
CONV2D_CASES += [(1, 16, 8, 24, 16, (1, 1), True, True, False), (1, 3, 5, 9, 7, (1, 1), False, False, False), (1, 20, 6, 19, 24, (1, 2), True, False, True),
                 (1, 3, 5, 9, 7, (1, 1), True, False, True)]


def _conv2d_id(c):
    B, Cin, Fq, T, Cout, stride, resid, relu, bias = c
    return (f"{'small' if Cin <= 4 else 'mfma'}-B{B}-Cin{Cin}-F{Fq}-T{T}-Cout{Cout}-s{stride[0]}{stride[1]}" + ("-resid" if resid else "") +
            ("-relu" if relu else "") + ("" if bias else "-nobias"))


@functools.lru_cache(maxsize=None)
def conv2d_host(case):
    B, Cin, Fq, T, Cout, stride, resid, relu, bias = case
    x, w, b, r = er.conv2d_case(B, Cin, Fq, T, Cout, stride, resid, bias, 9000 + CONV2D_CASES.index(case))
    return x, w, b, r, er.conv2d_ref(x, w, b, stride, r, relu), er.conv2d_replay(x, w, b, stride, r, relu)


@pytest.mark.parametrize("case", CONV2D_CASES, ids=_conv2d_id)
def test_conv2d_parity(case):
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import lib
    B, Cin, Fq, T, Cout, stride, resid, relu, bias = case
    x, w, b, r, ref, replay = conv2d_host(case)
    assert (Cin <= ops.CONV2D_SMALL_CIN) == (Cin <= 4) and stride[0] in (1, 2) and stride[1] in (1, 2)
    y = torch.full(tuple(ref.shape), SENT, device="cuda")
    xd, wd, bd, rd = _dev(x), ops.pack_conv2d_weight(_dev(w)), _dev(b), _dev(r)
    ops.check(lib.ua2_conv2d(ops.ptr(xd), ops.ptr(wd), ops.ptr(bd), ops.ptr(rd), ops.ptr(y), B, Cin, Cout, Fq, T, stride[0], stride[1], int(relu),
                             ops.stream()), "ua2_conv2d")
    torch.cuda.synchronize()
    ok, err, e, bar = er.conv_check(y, ref, replay)
    _line("conv2d", _conv2d_id(case), err, e, bar, "E_replay")
    assert ok
