"""fp8 (OCP e4m3fn) weight-only plan of the few-row decode frame (include/ua2hip.h ua2_pack_linear_w8 / ua2_linear_w8 / ua2_stage3_set_w8).

The contract: per output row a power-of-two scale 2^e, q = RNE_e4m3fn(W 2^-e), and the model computes with W' = q 2^e, which is exactly
representable in bf16.  The defining property is therefore an identity, not a tolerance: the fp8 launch / plan gives, bit for bit, what the
bf16 launch / plan gives on W'.  No test here compares the fp8 plan with itself: the other side is always the bf16 path on W' (or the CPU
oracle on W')."""
import numpy as np
import pytest
import torch

from helpers import build_oracle, build_product_model, load_golden_lm, product_decode_loop, toy_state_dict
from toy_configs import TOY_MODEL_ARGS
from w8_ref import w8_state_dict

pytestmark = pytest.mark.gpu

RC = TOY_MODEL_ARGS["audio_reason_vocab_size"]
FP8 = torch.float8_e4m3fn
DEV = "cuda"


def _launches(name):
    from uniaudio2_amd._lib import lib
    return lib.ua2_debug_kernel_launches(name.encode())


def _unpack_q(q, N, K, rope_hs=0):
    """fp8 image [N16/16][K/64][64 lanes][16 B] -> [N16, K] uint8 in SOURCE row order (the layout stated in include/ua2hip.h)."""
    n16 = (N + 15) // 16 * 16
    img = q.cpu().view(n16 // 16, K // 64, 64, 2, 8)                 # tile, burst, lane, half, e
    lane = torch.arange(64)
    col, g = lane % 16, lane // 16
    out = torch.zeros(n16, K, dtype=torch.uint8)
    for t in range(n16 // 16):
        for b in range(K // 64):
            for half in range(2):
                k0 = (2 * b + half) * 32
                for e in range(8):
                    out[t * 16 + col, k0 + g * 8 + e] = img[t, b, :, half, e]
    return out[_rope_rows(n16, rope_hs)] if rope_hs else out


def _rope_rows(n, hs):
    """inverse view of the pack's row permutation: result[src_row] = packed column holding it"""
    packed = torch.arange(n)
    h, within = packed // hs, packed % hs
    r, c = within // 16, within % 16
    src = h * hs + torch.where(c < 8, r * 8 + c, hs // 2 + r * 8 + (c - 8))
    inv = torch.empty(n, dtype=torch.long)
    inv[src] = packed
    return inv


@pytest.mark.parametrize("N,K,transposed,rope_hs,src_dtype", [
    (256, 128, False, 0, torch.float32), (110, 128, True, 0, torch.float32), (384, 256, False, 32, torch.float32),
    (384, 256, False, 64, torch.bfloat16), (512, 192, False, 128, torch.float32)])
def test_pack_matches_the_torch_quantiser_byte_for_byte(N, K, transposed, rope_hs, src_dtype):
    from uniaudio2_amd import ops
    g = torch.Generator().manual_seed(N * 7 + K)
    W = (torch.randn(N, K, generator=g) * 0.02).to(src_dtype)
    W[3] = 0                                                       # an all-zero row
    W[5, 7] = 448 * 2.0 ** -9                                      # a row whose amax is exactly 448 x a power of two
    W[5, :7] *= 0.1
    src = (W.t().contiguous() if transposed else W).to(DEV)
    q, exp, twin = ops.pack_linear_w8(src, transposed=transposed, rope_head_size=rope_hs)
    q_ref, e_ref = ops.quant_w8(W.float())                         # CPU restatement: amax -> e -> cast
    n16 = (N + 15) // 16 * 16
    got = _unpack_q(q, N, K, rope_hs)
    assert torch.equal(got[:N], q_ref.view(torch.uint8)), "fp8 codes"
    assert int(got[N:].to(torch.int32).abs().sum()) == 0, "padding rows are zero codes"
    e_src = torch.zeros(n16, dtype=torch.int32)
    e_src[:N] = e_ref
    e_packed = exp.cpu().to(torch.int32)
    want = e_src if not rope_hs else torch.zeros_like(e_src).scatter_(0, _rope_rows(n16, rope_hs), e_src)
    assert torch.equal(e_packed, want), "exponents, packed column order"
    Wp = ops.dequant_w8(W.float())
    assert torch.equal(Wp.bfloat16().float(), Wp), "W' is a bf16 number"
    twin_ref = ops.pack_linear(Wp.bfloat16().to(DEV), torch.bfloat16, rope_head_size=rope_hs)
    assert torch.equal(twin.view(torch.int16), twin_ref.view(torch.int16)), "bf16 twin == pack_linear(W')"


def test_pack_refuses_k_not_multiple_of_64():
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import Ua2Error
    with pytest.raises(Ua2Error, match="multiple of 64"):
        ops.pack_linear_w8(torch.zeros(32, 96, device=DEV))


def test_all_256_codes_dequantise_exactly():
    """Every e4m3fn code except the two NaNs as a weight (one 448 per row pins e = 0), one-hot activations: the kernel's output
    shows each dequantised value — subnormals, both zeros, +-448 — exactly."""
    from uniaudio2_amd import ops
    N, K = 16, 128
    codes = torch.arange(256, dtype=torch.uint8)
    vals = codes.view(FP8).float()
    vals[0x7F] = vals[0xFF] = 0.0
    W = torch.zeros(N, K)
    W[:4, :64] = vals.view(4, 64)
    W[:, 64] = 448.0
    q, exp, twin = ops.pack_linear_w8(W.to(DEV))
    assert int(exp.cpu().abs().sum()) == 0
    n0 = _launches("gemv_w8")
    for k0 in range(0, K, 5):
        ks = list(range(k0, min(k0 + 5, K)))
        x = torch.zeros(len(ks), K, device=DEV)
        for m, k in enumerate(ks):
            x[m, k] = 1.0
        y = torch.full((len(ks), N), 7.0, device=DEV)
        a = ops.linear(dtype=torch.bfloat16, M=len(ks), N=N, K=K, w0=twin, x=x, y=y, launch=False)
        ops.linear_w8(a, (q, exp))
        assert torch.equal(y.cpu(), W[:, ks].t().contiguous()), ks
    assert _launches("gemv_w8") - n0 == (K + 4) // 5


# ---- kernel identity: ua2_linear_w8 against ua2_linear on the twin -------------------------------------------------------------
def _kv(M, n_head, n_kv, hs, seed):
    from uniaudio2_amd import ops
    g = torch.Generator().manual_seed(seed)
    k = (torch.randn(M, n_kv, 64, hs, generator=g) * 0.5).bfloat16().to(DEV)
    v = (torch.randn(M, n_kv, 64, hs, generator=g) * 0.5).bfloat16().to(DEV)
    pt = torch.arange(M, dtype=torch.int32, device=DEV).view(M, 1)
    return k, v, pt, ops.kv_geom(k, v, pt, n_head, n_kv, hs)


def _identity_case(pro, epi, M, N, K, heads=None, handover=False, partmax=False, seed=0):
    """Runs the launch on the twin (ua2_linear) and on the fp8 image (ua2_linear_w8); returns the two dicts of every output."""
    from uniaudio2_amd import _lib, ops
    g = torch.Generator().manual_seed(seed + N + K)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale)
    nt = 2 if epi == _lib.EPI_SWIGLU else 1
    packs = []
    for t in range(nt):
        W = rnd(N, K, scale=0.02)
        packs.append(ops.pack_linear_w8(W.to(DEV), rope_head_size=(heads[2] if epi == _lib.EPI_QKV_ROPE else 0)))
    outs = []
    for use_w8 in (False, True):
        gg = torch.Generator().manual_seed(seed + 1)
        kw = dict(dtype=torch.bfloat16, M=M, N=N, K=K, w0=packs[0][2], prologue=pro, epilogue=epi, launch=False)
        keep = {}
        if nt == 2:
            kw["w1"] = packs[1][2]
        x = torch.randn(M, K, generator=gg)
        if pro == _lib.PRO_NORM:
            kw.update(x=x.to(DEV), norm_w=(1 + 0.1 * torch.randn(K, generator=gg)).to(DEV))
        elif pro == _lib.PRO_CAST:
            kw.update(x=x.to(DEV))
        elif pro == 4:                                             # UA2_PRO_SCALED: rounded row + per-16-column sums of squares
            xh = x.bfloat16()
            kw.update(x_h=xh.to(DEV), x_ssq=(x * x).view(M, K // 16, 16).sum(-1).to(DEV).contiguous(), ldh=K)
        if pro == _lib.PRO_LOCAL_ATTN or epi == _lib.EPI_QKV_ROPE:
            n_head, n_kv, hs = heads
            k, v, pt, geom = _kv(M, n_head, n_kv, hs, seed + 5)
            keep["k_pool"], keep["v_pool"] = k, v
            pos = torch.full((M,), 5, dtype=torch.int32, device=DEV)
            kw.update(row_pos=pos, kv=geom)
            if pro == _lib.PRO_LOCAL_ATTN:
                kw.update(x=(torch.randn(M, K, generator=gg) * 0.5).to(DEV))
            else:
                ang = torch.rand(8, hs // 2, generator=gg)
                keep["q_out"] = torch.zeros(M, n_head * hs, device=DEV)
                kw.update(rope_cos=torch.cos(ang).to(DEV), rope_sin=torch.sin(ang).to(DEV), q_out=keep["q_out"])
        if epi == _lib.EPI_RESIDUAL:
            keep["y"] = torch.zeros(M, N, device=DEV)
            kw.update(resid=torch.randn(M, N, generator=gg).to(DEV), y=keep["y"])
        elif epi in (_lib.EPI_STORE, _lib.EPI_SWIGLU):
            keep["y"] = torch.zeros(M, N, device=DEV)
            kw.update(y=keep["y"])
        if handover:
            keep["y_h"] = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
            keep["y_ssq"] = torch.zeros(M, N // 16, device=DEV)
            kw.update(y_norm_w=(1 + 0.1 * torch.randn(N, generator=gg)).to(DEV), y_h=keep["y_h"], y_ssq=keep["y_ssq"], ldh=N)
        if partmax:
            nb = (N + 15) // 16
            keep["part_max"] = torch.zeros(M, nb, device=DEV)
            keep["part_idx"] = torch.zeros(M, nb, dtype=torch.int32, device=DEV)
            kw.update(part_max=keep["part_max"], part_idx=keep["part_idx"], forbid=torch.full((M,), 24, dtype=torch.int32, device=DEV))
        a = ops.linear(**kw)
        n_g, n_w = _launches("gemv"), _launches("gemv_w8")
        if use_w8:
            ops.linear_w8(a, packs[0][:2], packs[1][:2] if nt == 2 else None)
        else:
            _lib.check(_lib.lib.ua2_linear(_lib.C.byref(a), ops.stream()), "ua2_linear")
        torch.cuda.synchronize()
        d_g, d_w = _launches("gemv") - n_g, _launches("gemv_w8") - n_w
        assert (d_g, d_w) == ((0, 1) if use_w8 else (1, 0)), (use_w8, d_g, d_w)
        outs.append({k: v.cpu().clone() for k, v in keep.items()})
    return outs


def _assert_same(outs, what):
    ref, got = outs
    assert ref.keys() == got.keys() and ref
    for k in ref:
        a, b = ref[k], got[k]
        if a.dtype == torch.bfloat16:
            a, b = a.view(torch.int16), b.view(torch.int16)
        assert torch.equal(a, b), (what, k)
        assert k not in ("y", "q_out", "y_h") or float(ref[k].float().abs().max()) > 0, (what, k, "output never written")


PRO_SCALED = 4
# (N, K, (n_head, n_kv, head_size) of the q|k|v launch) at the toy and the released sizes; SwiGLU N = the intermediate width
QKV_SHAPES = [(256, 128, (4, 2, 32)), (5120, 3072, (24, 8, 128)), (3072, 2048, (32, 8, 64))]
MLP_SHAPES = [(512, 256), (8192, 3072), (8192, 2048)]
DOWN_SHAPES = [(256, 512), (3072, 8192), (2048, 8192), (3072, 3072)]


@pytest.mark.parametrize("M", [1, 2, 5])
@pytest.mark.parametrize("pro", ["norm", "scaled"])
def test_kernel_identity_qkv_rope(pro, M):
    from uniaudio2_amd import _lib
    for N, K, heads in QKV_SHAPES:
        _assert_same(_identity_case(_lib.PRO_NORM if pro == "norm" else PRO_SCALED, _lib.EPI_QKV_ROPE, M, N, K, heads=heads), (pro, N, K))


@pytest.mark.parametrize("M", [1, 2, 5])
@pytest.mark.parametrize("pro", ["norm", "scaled"])
def test_kernel_identity_swiglu(pro, M):
    from uniaudio2_amd import _lib
    for N, K in MLP_SHAPES:
        _assert_same(_identity_case(_lib.PRO_NORM if pro == "norm" else PRO_SCALED, _lib.EPI_SWIGLU, M, N, K), (pro, N, K))


@pytest.mark.parametrize("M", [1, 2, 5])
def test_kernel_identity_residual_with_handover(M):
    from uniaudio2_amd import _lib
    for N, K in DOWN_SHAPES:
        _assert_same(_identity_case(_lib.PRO_CAST, _lib.EPI_RESIDUAL, M, N, K, handover=True), (N, K))
        _assert_same(_identity_case(_lib.PRO_CAST, _lib.EPI_RESIDUAL, M, N, K), (N, K, "plain"))


@pytest.mark.parametrize("M", [1, 2, 5])
@pytest.mark.parametrize("pro", ["norm", "scaled", "cast"])
def test_kernel_identity_store_with_partial_argmax(pro, M):
    from uniaudio2_amd import _lib
    p = {"norm": _lib.PRO_NORM, "scaled": PRO_SCALED, "cast": _lib.PRO_CAST}[pro]
    shapes = [(200, 128), (12296, 2048)] if pro != "cast" else [(512, 256), (128256, 3072)]      # audio_head[i] / lm_head
    for N, K in shapes:
        _assert_same(_identity_case(p, _lib.EPI_STORE, M, N, K, partmax=True), (pro, N, K))
    if pro == "cast":                                              # projection: STORE with the hand-over emission
        for N, K in [(128, 256), (2048, 3072)]:
            _assert_same(_identity_case(p, _lib.EPI_STORE, M, N, K, handover=True), (pro, N, K, "handover"))


def test_kernel_identity_local_attention_prologue():
    from uniaudio2_amd import _lib
    for N, K, heads in [(128, 128, (4, 2, 32)), (2048, 2048, (32, 8, 64)), (3072, 3072, (24, 8, 128))]:
        _assert_same(_identity_case(_lib.PRO_LOCAL_ATTN, _lib.EPI_RESIDUAL, 1, N, K, heads=heads, handover=True), (N, K))


@pytest.mark.parametrize("M", [1, 5])
def test_kernel_identity_where_the_fp8_and_13_bit_groups_disagree(M):
    """K = 192 is 6 chunks: whole fp8 groups (2 chunks), no whole 13-bit group (4), so the one K class where the form function answers
    differently per form.  The launcher gives it 4 waves x 4 chunks in a single round, which the fp8 fall-back form serves (a load per chunk):
    one gemv_w8 launch, no gemv launch (_identity_case counts both), the twin's bits.  The 13-bit side of this K:
    test_gpu_l13.py test_no_image_for_k_not_a_multiple_of_128."""
    import ctypes as C
    from uniaudio2_amd import _lib
    w, c, mr = C.c_int32(), C.c_int32(), C.c_int32()
    assert _lib.lib.ua2_debug_gemv_geometry(_lib.UA2_BF16, 32, 192, 1, C.byref(w), C.byref(c), C.byref(mr)) == 0
    assert (w.value, c.value, mr.value) == (4, 4, 0)
    _assert_same(_identity_case(_lib.PRO_CAST, _lib.EPI_STORE, M, 32, 192), (M, 32, 192))


def test_direct_launch_refuses_what_the_fp8_kernel_does_not_serve():
    """Return codes only: more rows than the launchers give the decode kernel, an fp32 launch, a GELU epilogue."""
    from uniaudio2_amd import _lib, ops
    q, exp, twin = ops.pack_linear_w8(torch.randn(64, 128, device=DEV) * 0.02)
    n0 = _launches("gemv_w8") + _launches("gemv")
    for M, dtype, epi in [(6, torch.bfloat16, _lib.EPI_STORE), (1, torch.float32, _lib.EPI_STORE), (1, torch.bfloat16, _lib.EPI_GELU)]:
        x, y = torch.zeros(M, 128, device=DEV), torch.zeros(M, 64, device=DEV)
        a = ops.linear(dtype=dtype, M=M, N=64, K=128, w0=twin, x=x, y=y, epilogue=epi, launch=False)
        with pytest.raises(_lib.Ua2Error, match="ua2_linear_w8"):
            ops.linear_w8(a, (q, exp))
    assert _launches("gemv_w8") + _launches("gemv") == n0, "a refused call launches nothing"


# ---- plan identity (the defining property) --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return load_golden_lm()


@pytest.fixture(scope="module")
def sd(golden):
    return toy_state_dict(golden[1])


@pytest.fixture(scope="module")
def sd_w8(sd):
    return w8_state_dict(sd)


def _case(d, case):
    tokens = torch.from_numpy(d[f"{case}_tokens"]).long()
    mask = torch.from_numpy(d[f"{case}_mask"]).bool()
    if tokens.dim() == 2:
        tokens, mask = tokens[None], mask[None]
    return tokens, mask


def _pools(m):
    return [t.cpu().clone() for g in (m.audio_understanding_expert, m.backbone, m.audio_generation_expert, m.decoder)
            for t in g.kv_cache.k + g.kv_cache.v]


def _pair(sd, sd_w8, batch, **kw):
    a = build_product_model(sd, torch.bfloat16, batch=batch, weight_dtype=FP8, **kw)        # model A: the fp8 plan
    b = build_product_model(sd_w8, torch.bfloat16, batch=batch, **kw)                       # model B: today's bf16 plan loaded with W'
    assert a.weight_dtype is None and a._st["weight_dtype"] == FP8 and b._st["weight_dtype"] is None
    return a, b


def _decode_counted(m, fn):
    """fn() with the "gemv" / "gemv_w8" counters taken around its DECODE part only: the snapshot is made when the (last) forward_prefix
    of fn returns, so prefill chunks — many-row launches on the twin — are outside.  -> (result, gemv launches, gemv_w8 launches)."""
    snap = {}
    orig = m.forward_prefix

    def prefix(*a, **kw):
        r = orig(*a, **kw)
        torch.cuda.synchronize()
        snap["g"], snap["w"] = _launches("gemv"), _launches("gemv_w8")
        return r

    m.forward_prefix = prefix
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        del m.forward_prefix
    assert snap, "fn never prefilled"
    return out, _launches("gemv") - snap["g"], _launches("gemv_w8") - snap["w"]


@pytest.mark.parametrize("case,frames,feedback,switch", [("tts1", 12, "audio", 9), ("asr1", 10, "text", None), ("tts2", 12, "audio", 5)])
def test_plan_identity_per_frame_logits_ids_and_caches(golden, sd, sd_w8, case, frames, feedback, switch):
    d, _ = golden
    tokens, mask = _case(d, case)
    a, b = _pair(sd, sd_w8, tokens.size(0))
    run = lambda m: product_decode_loop(m, tokens, mask, frames, feedback, forbid_switch=switch, reason_card=RC, collect_logits=True)
    ra, ga, wa = _decode_counted(a, lambda: run(a))
    rb, gb, wb = _decode_counted(b, lambda: run(b))
    # the decode frames of model A: "gemv_w8" moved and "gemv" did not (no launch fell back to the twin); model B the other way round,
    # launch for launch except lm_head, which rides on a down-projection launch in B and is a launch of its own in A
    assert wa > 0 and ga == 0 and wb == 0 and gb > 0, (ga, wa, gb, wb)
    for k in ("samples", "text_logits", "audio_logits"):
        assert torch.equal(ra[k], rb[k]), (case, k)
    for pa, pb in zip(_pools(a), _pools(b)):
        assert torch.equal(pa.view(torch.int16), pb.view(torch.int16)), "K/V pools"


@pytest.mark.parametrize("what", ["greedy", "ngram", "topk", "cfg", "skip_text", "no_tables"])
def test_plan_identity_on_device_loops(golden, sd, sd_w8, what, monkeypatch):
    from uniaudio2_amd._lib import lib
    d, _ = golden
    if what == "no_tables":
        monkeypatch.setenv("UA2_NO_PROJ_TABLE", "1")
    tokens, mask = _case(d, "asr1" if what == "ngram" else "tts1")
    if what == "cfg":
        tokens, mask = tokens.repeat(2, 1, 1), mask.repeat(2, 1, 1)
        tokens[1, :-1, -1] = 0                                      # the unconditional row: another prompt
    B, L, _ = tokens.shape
    a, b = _pair(sd, sd_w8, B)

    def run(m):
        dev = torch.device(DEV)
        tk, mk = tokens.to(dev), mask.to(dev)
        m.reset_caches()
        pos = torch.arange(L, device=dev).unsqueeze(0).repeat(B, 1)
        m.forward_prefix(tk[:, :-1], tokens_mask=mk, input_pos=pos[:, :-1])
        m.set_sampling(8, 0.9, seed=1234) if what == "topk" else m.set_sampling(1, 1.0)
        m.set_cfg(1.5 if what == "cfg" else 1.0)
        m.set_ngram(3 if what == "ngram" else 0, fallback=7)
        m.begin_decode(tk[:, -1:], mk[:, -1:], torch.tensor([L - 1], device=dev))
        mode = 1 if what == "ngram" else (2 if what == "cfg" else 0)
        log = m.generate_frames(10, B, mode, reason_eos=-1, reason_card=RC, skip_text_head=(what == "skip_text")).cpu().clone()
        return log, m.buffer("text_logits", B).cpu().clone(), m.buffer("audio_logits", B).cpu().clone()

    (la, ta, aa), ga, wa = _decode_counted(a, lambda: run(a))
    (lb, tb, ab), gb, wb = _decode_counted(b, lambda: run(b))
    assert wa > 0 and ga == 0 and wb == 0 and gb > 0, (ga, wa, gb, wb)
    assert torch.equal(la, lb), what
    assert torch.equal(aa, ab) or what == "ngram"                  # the text loop never runs the depth decoder
    assert torch.equal(ta, tb) or what == "skip_text"
    for pa, pb in zip(_pools(a), _pools(b)):
        assert torch.equal(pa.view(torch.int16), pb.view(torch.int16)), "K/V pools"
    lib.ua2_debug_refresh_env()


def test_rows_of_a_batch_equal_their_single_runs_inside_the_fp8_plan(golden, sd, sd_w8):
    """A sequence decoded alone and as one of 2, 5 (fp8 decode kernel) and 8, 32 sequences (many-row kernels on the twin W'): identical ids
    and logits; and the single run is the bf16 plan's on W' (so nothing here is the fp8 plan against itself alone)."""
    d, _ = golden
    tokens, mask = _case(d, "tts1")
    L = tokens.size(1)
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(99)

    def prompts(B):
        tk, mk = tokens.repeat(B, 1, 1), mask.repeat(B, 1, 1)
        for r in range(1, B):
            tk[r, :, -1] = torch.randint(0, 256, (L,), generator=g)
        return tk.to(dev), mk.to(dev)

    def run(m, B):
        tk, mk = prompts(B)
        m.reset_caches()
        pos = torch.arange(L, device=dev).unsqueeze(0).repeat(B, 1)
        m.forward_prefix(tk[:, :-1], tokens_mask=mk, input_pos=pos[:, :-1])
        m.begin_decode(tk[:, -1:], mk[:, -1:], torch.tensor([L - 1], device=dev))
        log = m.generate_frames(8, B, 0, reason_eos=-1, reason_card=RC).cpu().clone()
        return log[:, 0], m.buffer("text_logits", B)[0].cpu().clone(), m.buffer("audio_logits", B)[0].cpu().clone()

    b = build_product_model(sd_w8, torch.bfloat16, batch=1)
    ref = run(b, 1)
    a = build_product_model(sd, torch.bfloat16, batch=32, weight_dtype=FP8)
    for B in (1, 2, 5, 8, 32):
        got, n_g, n_w = _decode_counted(a, lambda: run(a, B))
        assert (n_w > 0 and n_g == 0) if B <= 5 else n_w == 0, (B, n_g, n_w)
        for x, y in zip(ref, got):
            assert torch.equal(x, y), B


def test_teacher_forced_against_the_bf16_oracle_on_w_prime(golden, sd, sd_w8):
    """The fp8 plan against oracle.lm_oracle in bf16 mode built on W', with the bf16 plan's own bars (tests/test_gpu_lm.py
    _bf16_teacher_forced: text ATOL 3.5e-2, audio 2.5e-2, ids asserted where the oracle's top-2 margin >= 2 x ATOL)."""
    from oracle.lm_oracle import run_decode_loop
    TEXT_ATOL, AUDIO_ATOL = 3.5e-2, 2.5e-2
    d, _ = golden

    def margin(logits, forbid=0):
        l = logits.clone()
        if forbid > 0:
            l[:forbid] = float("-inf")
        s = l.sort(-1).values
        return float(s[-1] - s[-2])

    for case, frames, feedback, switch in [("tts1", 24, "audio", 9), ("asr1", 10, "text", None)]:
        tokens, mask = _case(d, case)
        B, L, _ = tokens.shape
        o = run_decode_loop(build_oracle(sd_w8, "bf16", B), tokens, mask, frames, feedback, forbid_switch=switch, reason_card=RC,
                            collect_logits=True, scaled=True)
        m = build_product_model(sd, torch.bfloat16, batch=B, weight_dtype=FP8)
        tk, mk = tokens.to(DEV), mask.to(DEV)
        m.reset_caches()
        pos = torch.arange(0, L, device=DEV).unsqueeze(0).repeat(B, 1)
        m.forward_prefix(tk[:, :-1], labels=tk[:, 1:, :-1], tokens_mask=mk, loss_mask=mk, input_pos=pos[:, :-1])
        ct, cm = tk[:, -1:], mk[:, -1:]
        compared = total = 0
        n_w = _launches("gemv_w8")
        for f in range(frames):
            forbid = 0 if (switch is None or f < switch) else RC
            s = m.generate_frame(ct, cm, input_pos=torch.tensor([L - 1 + f], device=DEV), input_pos_maxp1=L + f, forbid_prefix=forbid).cpu()
            tl, al = m.buffer("text_logits", B).cpu(), m.buffer("audio_logits", B).cpu()
            np.testing.assert_allclose(tl.numpy(), o["text_logits"][f].numpy(), atol=TEXT_ATOL, rtol=0)
            for r in range(B):
                total += 9
                if margin(o["text_logits"][f, r]) >= 2 * TEXT_ATOL:
                    assert int(s[r, 0]) == int(o["samples"][f, r, 0]), f"text id differs at frame {f}"
                    compared += 1
                for i in range(8):
                    np.testing.assert_allclose(al[r, i].numpy(), o["audio_logits"][f, r, i].numpy(), atol=AUDIO_ATOL, rtol=0)
                    if margin(o["audio_logits"][f, r, i], forbid) < 2 * AUDIO_ATOL:
                        break
                    assert int(s[r, 1 + i]) == int(o["samples"][f, r, 1 + i]), f"audio id {i} differs at frame {f}"
                    compared += 1
            so = o["samples"][f].to(DEV)
            text_tok, audio = so[:, 0:1].long(), so[:, 1:].long()
            if feedback == "audio":
                ct = torch.cat([audio, text_tok], dim=-1).unsqueeze(1)
                cm = torch.cat([torch.ones_like(audio).bool(), torch.zeros(B, 1, device=DEV).bool()], dim=1).unsqueeze(1)
            else:
                ct = torch.cat([torch.zeros_like(audio), text_tok], dim=-1).unsqueeze(1)
                cm = torch.cat([torch.zeros_like(audio).bool(), torch.ones(B, 1, device=DEV).bool()], dim=1).unsqueeze(1)
        assert _launches("gemv_w8") > n_w
        assert compared >= total // 4, f"only {compared}/{total} tokens had a defined arg-max"


def test_clearing_and_attaching_the_fp8_images_recaptures(golden, sd, sd_w8):
    d, _ = golden
    tokens, mask = _case(d, "tts1")
    a, b = _pair(sd, sd_w8, 1)
    run = lambda m: product_decode_loop(m, tokens, mask, 8, "audio", fast=True)["samples"]
    ref = run(b)
    r1, g1, w1 = _decode_counted(a, lambda: run(a))
    a.set_w8(False)
    r2, g2, w2 = _decode_counted(a, lambda: run(a))
    a.set_w8(True)
    r3, g3, w3 = _decode_counted(a, lambda: run(a))
    assert w1 > 0 and g1 == 0 and w2 == 0 and g2 > 0 and (g3, w3) == (g1, w1), (g1, w1, g2, w2, g3, w3)
    assert torch.equal(r1, ref) and torch.equal(r2, ref) and torch.equal(r3, ref)


def test_bad_arguments_are_refused_by_return_code(golden, sd):
    from uniaudio2_amd import _lib
    from uniaudio2_amd._lib import W8Entry, lib
    with pytest.raises(ValueError, match="bf16"):
        build_product_model(sd, torch.float32, batch=1, weight_dtype=FP8)
    m = build_product_model(sd, torch.bfloat16, batch=1, weight_dtype=FP8)
    t, q, e = m._st["w8"][0]
    foreign = torch.zeros(16, device=DEV)
    tab = (W8Entry * 1)(W8Entry(foreign.data_ptr(), q.data_ptr(), e.data_ptr()))
    assert lib.ua2_stage3_set_w8(m._h, tab, 1) != 0 and b"not a weight of this plan" in lib.ua2_last_error()
    f32 = build_product_model(sd, torch.float32, batch=1)
    tab = (W8Entry * 1)(W8Entry(f32._st["lm_head"].data_ptr(), q.data_ptr(), e.data_ptr()))
    assert lib.ua2_stage3_set_w8(f32._h, tab, 1) != 0 and b"UA2_BF16" in lib.ua2_last_error()
    with pytest.raises(ValueError, match="without fp8"):
        f32.set_w8(True)
