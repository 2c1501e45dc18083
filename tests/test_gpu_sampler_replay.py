"""The four sampler entry points (ua2_sample_topk / _rows, ua2_sample_topp / _rows; csrc/ua2_sample.hip) and the frame executor's
use of them against the float64 replay of tests/sampler_refs.py: WHICH id a given (logits, key, draw, row, stream) must produce.

Every kernel-level launch is one of sampler_refs.CASES, whose inputs tests/test_sampler_refs_host.py holds to 0 rows outside the exact
assertion.  A launch runs in padded buffers (ld > V, rows past M; the padding holds +3e4, which would win any race it entered),
with out_tokens wider than the written column and pre-filled, and checks besides the ids: the columns and rows of out_tokens it
must not write, its inputs bit-unchanged, and next_h == emb[id + emb_row_offset] bit for bit.  Each prints one PARITY line."""
import ctypes as C

import numpy as np
import pytest
import torch

import sampler_refs as sr

pytestmark = pytest.mark.gpu

PAD, EXTRA, FILL = 5, 2, 3e4                   # pad columns, rows past M, what both hold
OUT_LD, OUT_COL, OUT_FILL = 3, 1, -77
CE, EMB_OFF = 8, 3


def _s32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= (1 << 31) else x


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _launch(L, dtype):
    """One launch of L through ctypes.  -> ids [M] numpy.  Asserts everything about the launch that is not the ids' values."""
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import check, lib
    M, V, ld, rows = L.M, L.V, L.V + PAD, L.M + EXTRA
    host = torch.full((rows, ld), FILL, dtype=torch.float32)
    host[:M, :V] = torch.from_numpy(L.logits)
    lg = host.cuda()
    out = torch.full((rows, OUT_LD), OUT_FILL, dtype=torch.int32, device="cuda")
    emb = torch.randn(V + EMB_OFF, CE, generator=torch.Generator().manual_seed(5)).to(dtype).cuda()
    nh = torch.full((rows, CE), -5.0, device="cuda")
    fb_h = None if L.forbid is None else torch.cat([torch.from_numpy(L.forbid).int(), torch.zeros(EXTRA, dtype=torch.int32)])
    fb = None if fb_h is None else fb_h.cuda()
    ptr = lambda t: None if t is None else t.data_ptr()
    tail = (L.stream_id, out.data_ptr(), OUT_LD, OUT_COL, emb.data_ptr(), EMB_OFF, CE, nh.data_ptr())
    head = (ops.dtype_code(dtype), M, lg.data_ptr(), ld, V, L.topk, C.c_float(L.T), ptr(fb))
    nucleus = 0.0 < L.top_p < 1.0
    if L.form == "shared":
        cnt_h = torch.tensor([_s32(w) for w in L.counter], dtype=torch.int32)
        state_h = [cnt_h]
        state = [cnt_h.cuda()]
        args = head + (L.seed, state[0].data_ptr()) + tail + (L.key_shift,)
        if nucleus:
            check(lib.ua2_sample_topp(*args, C.c_float(L.top_p), None, ops.stream()), "ua2_sample_topp")
        else:
            check(lib.ua2_sample_topk(*args, ops.stream()), "ua2_sample_topk")
    else:
        pad_k = [0] * EXTRA
        state_h = [torch.tensor([[_s32(k), _s32(k >> 32)] for k in list(L.keys) + pad_k], dtype=torch.int32),
                   torch.tensor([_s32(d) for d in list(L.draws) + pad_k], dtype=torch.int32)]
        state = [t.cuda() for t in state_h]
        args = head + (state[0].data_ptr(), state[1].data_ptr()) + tail
        if nucleus:
            check(lib.ua2_sample_topp_rows(*args, C.c_float(L.top_p), None, ops.stream()), "ua2_sample_topp_rows")
        else:
            check(lib.ua2_sample_topk_rows(*args, ops.stream()), "ua2_sample_topk_rows")
    torch.cuda.synchronize()
    o = out.cpu()
    ids = o[:M, OUT_COL].clone()
    o[:M, OUT_COL] = OUT_FILL
    assert bool((o == OUT_FILL).all()), "out_tokens was written outside column out_col of rows [0, M)"
    assert torch.equal(_bits(lg.cpu()), _bits(host)), "the logits were written"
    assert fb is None or torch.equal(fb.cpu(), fb_h), "forbid was written"
    for d, h in zip(state, state_h):
        assert torch.equal(d.cpu(), h), "counter / row_key / row_draw was written"
    assert bool((ids >= 0).all()) and bool((ids < V).all())
    want_nh = emb[(ids.long() + EMB_OFF).cuda()].float()
    assert torch.equal(_bits(nh[:M]), _bits(want_nh)), "next_h is not emb[id + emb_row_offset]"
    assert bool((nh[M:] == -5.0).all()), "next_h was written past row M"
    return ids.numpy()


def _assert_replay(case, R, got):
    print(R.line(case))
    bad = R.mismatches(got)
    assert not bad, (case, [(m, int(got[m]), int(R.ids[m]), R.near[m].tolist()) for m in bad[:8]], len(bad))
    assert int((~R.exact).sum()) <= sr.CAP * len(R.ids), case


def _dtype_of(name):
    """The gather's dtype alternates over the cases: fp32 and bf16 tables both see every family."""
    return (torch.float32, torch.bfloat16)[list(sr.CASES).index(name) % 2]


@pytest.mark.parametrize("name", [n for n in sr.CASES if n != "u-edge"])
def test_launch_replays(name):
    """Shapes, counter words, per-row streams, the tie rows and the nucleus cases: every row's id is the float64 replay's."""
    L, R = sr.case(name)
    got = _launch(L, _dtype_of(name))
    _assert_replay(name, R, got)
    if name == "ctr-shift1":
        assert bool((got[0::4] == got[1::4]).all())                      # a pair that holds equal logits holds one id
    if name == "rows-tie":
        assert got.tolist() == [a for _, a, _ in L.note]                 # the lower of the two columns that tie by construction


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_u_edge_column_wins(dtype):
    """Row 0 meets a counter whose r[0] >> 8 is 0xFFFFFF at the column of its largest logit.  The contract's u = 1 - 2^-24 gives it
    the smallest Exp(1) draw there is: it wins.  RN(x + 0.5) * 2^-24 without the min is 1.0f there, q = -0.0f and the score -inf:
    before the min was added this case failed with another of the eight kept columns as row 0's id."""
    L, R = sr.case("u-edge")
    got = _launch(L, dtype)
    _assert_replay("u-edge", R, got)
    assert int(got[0]) == sr.U_EDGE["column"]


# ---- frame level: the executor's nine samplers per row -----------------------------------------------------------------------

F_TOPK, F_T, F_SEED = 20, 0.9, 0x5EED0000FFFFFFF0


def _frames(m, R, mode, n_frames, top_p=0.0, rows=False, key_shift=0, switch_at=None, tag=""):
    """Runs n_frames frames one at a time and replays all nine heads of every row of each from the logits the frame leaves behind
    (guided frames: the mixed logits), the counters / row streams and forbid read BEFORE the frame.  switch_at: before that frame
    every row's forbid is set to va - 1, so each audio head can only give va - 1 = reason_eos and the device switch sets forbid to
    reason_card for the frame after it."""
    st = m._st
    va, ncb = st["va"], st["ncb"]
    reason_card = 40
    left_out = total = 0
    for f in range(n_frames):
        if f == switch_at:
            st["forbid"][:R].fill_(va - 1)
        cnt = st["counters"].cpu().tolist()
        forbid = st["forbid"][:R].cpu().tolist()
        if rows:
            rk, rd = st["row_key"][:R].cpu().tolist(), st["row_draw"][:R].cpu().tolist()
        m.generate_frames(1, R, mode, reason_eos=va - 1, reason_card=reason_card, use_graph=(f % 2 == 0))
        out = st["out_tokens"][:R].cpu().numpy()
        tl, al = m.buffer("text_logits", R).cpu().numpy(), m.buffer("audio_logits", R).cpu().numpy()
        after = st["counters"].cpu().tolist()
        reps, got = [], []
        for r in range(R):
            if rows:
                key, draw, part = (rk[r][0] & sr.U32, rk[r][1] & sr.U32), rd[r], 0
            else:
                key, draw, part = sr.key_words(0, cnt[2], cnt[3]), cnt[1], r >> key_shift
            common = dict(T=F_T, top_p=top_p, key=key, draw=draw, row_part=part)
            reps.append(dict(common, logits=tl[r], forbid=0, topk=min(F_TOPK, tl.shape[1]), stream_id=0)); got.append(out[r, 0])
            for i in range(ncb):
                reps.append(dict(common, logits=al[r, i], forbid=forbid[r], topk=F_TOPK, stream_id=1 + i)); got.append(out[r, 1 + i])
        Rp = sr.replay_rows(reps)
        print(Rp.line(f"frame{tag}-f{f}"), f"nucleus margin {Rp.min_margin:.2e}")
        bad = Rp.mismatches(got)
        assert not bad, (tag, f, [(b // 9, b % 9, int(got[b]), int(Rp.ids[b]), Rp.near[b].tolist()) for b in bad[:8]])
        left_out += int((~Rp.exact).sum()); total += len(got)
        # exactly one draw index per sampled frame, on the stream the frame read
        if rows:
            assert st["row_draw"][:R].cpu().tolist() == [_s32(d + 1) for d in rd] and after[1] == cnt[1]
        else:
            assert after[1] == _s32(cnt[1] + 1)
        assert after[2:] == cnt[2:] and after[0] == cnt[0] + 1
        if mode == 2:
            assert np.array_equal(out[0::2], out[1::2])                   # both rows of a pair hold one id
        if f == switch_at:
            assert bool((out[:, 1:] == va - 1).all()) and st["forbid"][:R].cpu().tolist() == [reason_card] * R
        elif switch_at is not None and f > switch_at:
            assert forbid == [reason_card] * R and bool((out[:, 1:] >= reason_card).all())
    assert left_out <= sr.CAP * total, (tag, left_out, total)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("form", ["R1", "R3", "guided", "rows-topp"])
def test_frame_heads_replay(dtype, form):
    from helpers import load_golden_lm, product_decode_loop
    from row_stream_refs import model, prompt
    m = model(dtype)
    tag_dt = "bf16" if dtype == torch.bfloat16 else "fp32"
    m.set_row_seeds(None)
    m.set_top_p(0.0)
    try:
        if form == "guided":
            d, _ = load_golden_lm()
            t, k = torch.from_numpy(d["cfg2_tokens"]).long(), torch.from_numpy(d["cfg2_mask"]).bool()
            m.set_sampling(F_TOPK, F_T, seed=F_SEED + 1)
            product_decode_loop(m, t, k, 0, "audio", fast=True, cfg_scale=1.5)        # prefill and the first decode frame's rows, no frame yet
            m.set_cfg(1.5)
            _frames(m, 2, 2, 3, key_shift=1, tag=f"-{form}-{tag_dt}")
        else:
            R = 1 if form == "R1" else 3
            m.set_sampling(F_TOPK, F_T, seed=F_SEED + R)
            m.begin_ragged([prompt(b, 0) for b in range(R)])
            if form == "rows-topp":
                m.set_row_seeds([F_SEED + 31 * b for b in range(R)])
                m._st["row_draw"][:R] = torch.tensor([0, 0x7FFFFFFF, -1], dtype=torch.int32, device="cuda")    # per row, and across the int32 edges
                m.set_top_p(0.8)
            _frames(m, R, 0, 4, top_p=0.8 if form == "rows-topp" else 0.0, rows=form == "rows-topp", switch_at=2, tag=f"-{form}-{tag_dt}")
    finally:
        m.set_row_seeds(None)
        m.set_top_p(0.0)
        m.set_cfg(1.0)
        m.set_sampling(1, 1.0)
        m._st["forbid"].zero_()
