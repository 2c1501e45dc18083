"""bf16 operand rows into the one-row-tile UA2_PRO_CAST launches of the decode kernel (include/ua2hip.h, beside y_norm_w; the plan's
opt-out UA2_NO_ROW_OPERAND=1 is read when a plan is created).

The producer rounds its fp32 result to bf16 once (UA2_EPI_SWIGLU with y_h, ua2_attn with y_h); the consumer (UA2_PRO_CAST with x_h)
copies 16-byte pieces into its LDS operand row instead of loading the fp32 row and rounding it in every workgroup.  The same RNE of
the same value, so every comparison here is torch.equal.

Op level: a CAST launch fed x_h against the same launch fed fp32 x; a SWIGLU launch's y_h and the attention's y_h against RNE_bf16 of
their y; one row more than the decode kernel's tile is refused (the plan then hands over the packed operand as before) and the fp32
route still gives the rows their bits.  Frame level: two plans in one process, switch on and off, agree on everything 12 frames leave
behind at one and at two rows, and teacher-forced scoring (it shares run_gpt) does not change."""
import pytest
import torch

from helpers import build_product_model, load_golden_lm, toy_state_dict

pytestmark = pytest.mark.gpu

FRAMES = 12
TILE_ROWS = 5          # rows the launchers give the decode kernel on bf16 (ua2_gemv_rows_preferred; UA2_GEMV_MAX_ROWS unset)
# (K, N): K = 128 / 256 — one and two chunks per wave of the small fall-back geometries; K = 8192, N = 32 — 16 waves x 16 chunks, one burst
SHAPES = [(128, 48), (256, 512), (8192, 32)]
FORMS = ["bf16", "l13", "fp8"]


def _rne_bf16(t):
    return t.to(torch.bfloat16)          # torch rounds fp32 -> bf16 to nearest even, as f2bf does (no NaN in these inputs)


def _weight(form, N, K, g, dev):
    """One [N, K] Linear in `form` -> (the packed bf16 weight a launch names as w0 / w1, its image for linear_l13 / linear_w8 or None)"""
    from uniaudio2_amd import ops
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(dev)
    if form == "fp8":
        q, exp, twin = ops.pack_linear_w8(w)
        return twin, (q, exp)
    packed = ops.pack_linear(w, torch.bfloat16)
    if form == "l13":
        image, base, esc = ops.pack_linear_l13(packed, N, K)
        assert int(esc[0]) == 0                                               # an image with escapes is never used
        return packed, (image, base)
    return packed, None


def _go(form, args, i0, i1=None):
    """the launch `args` (ops.linear(..., launch=False)) on bf16 weights, their 13-bit images or their fp8 twins"""
    import ctypes as C
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import check, lib
    if form == "fp8":
        ops.linear_w8(args, i0, i1)
    elif form == "l13":
        ops.linear_l13(args, i0, i1)
    else:
        check(lib.ua2_linear(C.byref(args), ops.stream()), "ua2_linear")


def _operand(M, K, g, dev):
    x = torch.randn(M, K, generator=g)
    x[0, 0], x[0, 1], x[-1, K - 1] = -0.0, 1e30, 1e-30                       # a signed zero, a large and a small magnitude
    x[0, 2], x[0, 3] = 1.00390625, 1.01171875                                # ties of the bf16 rounding (1 + 2^-8, 1 + 3 2^-8): to even
    return x.to(dev)


@pytest.mark.parametrize("M", [1, 2, TILE_ROWS])
@pytest.mark.parametrize("K,N", SHAPES)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("epi", ["residual", "store"])
def test_cast_launch_on_bf16_rows_equals_launch_on_fp32_rows(epi, form, K, N, M):
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import EPI_RESIDUAL, EPI_STORE, PRO_CAST
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(K + N + M)
    w0, image = _weight(form, N, K, g, dev)
    x = _operand(M, K, g, dev)
    xh = _rne_bf16(x)
    resid = torch.randn(M, N, generator=g).to(dev)

    def launch(**operand):
        y = torch.full((M, N), float("nan"), device=dev)
        kw = dict(resid=resid, epilogue=EPI_RESIDUAL) if epi == "residual" else dict(epilogue=EPI_STORE)
        _go(form, ops.linear(dtype=torch.bfloat16, M=M, N=N, K=K, w0=w0, prologue=PRO_CAST, y=y, launch=False, **kw, **operand), image)
        torch.cuda.synchronize()
        return y

    ref = launch(x=x)
    got = launch(x_h=xh)
    assert bool(torch.isfinite(ref).all()) and torch.equal(got, ref)
    # a padded row stride: the rows are found by ldx, the padding is not read into the sum
    pad = torch.full((M, K + 8), float("nan"), dtype=torch.bfloat16, device=dev)
    pad[:, :K] = xh
    got2 = launch(x_h=pad, ldx=K + 8)
    assert torch.equal(got2, ref)


@pytest.mark.parametrize("K,N", SHAPES)
def test_one_row_more_than_the_tile_takes_the_old_route(K, N):
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import EPI_STORE, PRO_CAST, Ua2Error
    dev = torch.device("cuda")
    M = TILE_ROWS + 1
    g = torch.Generator().manual_seed(K + N)
    packed = ops.pack_linear((torch.randn(N, K, generator=g) * K ** -0.5).to(dev), torch.bfloat16)
    x = torch.randn(M, K, generator=g).to(dev)
    xh = _rne_bf16(x)

    def launch(rows, **operand):
        y = torch.full((rows, N), float("nan"), device=dev)
        ops.linear(dtype=torch.bfloat16, M=rows, N=N, K=K, w0=packed, prologue=PRO_CAST, epilogue=EPI_STORE, y=y,
                   workspace=ops.linear_workspace(torch.bfloat16, rows, K, dev), **operand)
        torch.cuda.synchronize()
        return y

    with pytest.raises(Ua2Error, match="x_h"):                               # never a silent launch that ignores the rows
        launch(M, x_h=xh)
    old = launch(M, x=x)                                                     # the many-row route on fp32 rows
    new = launch(TILE_ROWS, x_h=xh[:TILE_ROWS].contiguous())
    assert torch.equal(old[:TILE_ROWS], new)                                 # row invariance: a row's bits whatever the route


@pytest.mark.parametrize("M", [1, 2, TILE_ROWS])
@pytest.mark.parametrize("K,N", [(128, 48), (256, 512), (256, 8192)])
@pytest.mark.parametrize("form", FORMS)
def test_swiglu_bf16_rows_are_the_rounded_fp32_rows(form, K, N, M):
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import EPI_SWIGLU, PRO_NORM, Ua2Error
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(K + N + M)
    (w0, i0), (w1, i1) = _weight(form, N, K, g, dev), _weight(form, N, K, g, dev)
    x = torch.randn(M, K, generator=g).to(dev)
    norm_w = torch.randn(K, generator=g).to(dev)

    def launch(want_y, want_h, ldy=None):
        y = torch.full((M, N), float("nan"), device=dev) if want_y else None
        yh = torch.full((M, ldy or N), 7.0, dtype=torch.bfloat16, device=dev) if want_h else None
        _go(form, ops.linear(dtype=torch.bfloat16, M=M, N=N, K=K, w0=w0, w1=w1, prologue=PRO_NORM, epilogue=EPI_SWIGLU, x=x, norm_w=norm_w,
                             y=y, y_h=yh, ldy=ldy, launch=False), i0, i1)
        torch.cuda.synchronize()
        return y, yh

    y_ref, _ = launch(True, False)
    y, yh = launch(True, True)
    assert torch.equal(y, y_ref) and torch.equal(yh, _rne_bf16(y_ref))
    _, only = launch(False, True)                                            # y == NULL: the fp32 store is gone, the rows are the same
    assert torch.equal(only, yh)
    _, wide = launch(False, True, ldy=N + 8)                                 # rows on y's stride, nothing written past N
    assert torch.equal(wide[:, :N], yh) and bool((wide[:, N:] == 7.0).all())
    with pytest.raises(Ua2Error, match="y_h"):                               # more rows than the tile: refused
        ops.linear(dtype=torch.bfloat16, M=TILE_ROWS + 1, N=N, K=K, w0=w0, w1=w1, prologue=PRO_NORM, epilogue=EPI_SWIGLU,
                   x=torch.zeros(TILE_ROWS + 1, K, device=dev), norm_w=norm_w, y_h=torch.zeros(TILE_ROWS + 1, N, dtype=torch.bfloat16, device=dev),
                   workspace=ops.linear_workspace(torch.bfloat16, TILE_ROWS + 1, K, dev))


@pytest.mark.parametrize("R", [1, 2, TILE_ROWS])
@pytest.mark.parametrize("nh,nkv,hs", [(4, 2, 32), (3, 1, 64), (6, 2, 128)])
def test_attention_bf16_rows_are_the_rounded_fp32_rows(nh, nkv, hs, R):
    from uniaudio2_amd import ops
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(nh * hs + R)
    qn, pages = nh * hs, 3
    kp = torch.randn(R * pages, nkv, 64, hs, generator=g).to(device=dev, dtype=torch.bfloat16)
    vp = torch.randn(R * pages, nkv, 64, hs, generator=g).to(device=dev, dtype=torch.bfloat16)
    pt = torch.randperm(R * pages, generator=g).to(torch.int32).view(R, pages).to(dev)
    pos = torch.tensor([0, 63, 64, 130, 191][:R], dtype=torch.int32, device=dev)        # one key, a page edge, several pages
    q = torch.randn(R, qn, generator=g).to(dev)
    kv = ops.kv_geom(kp, vp, pt, nh, nkv, hs)

    def launch(want_y, ldh=None):
        y = torch.full((R, qn), float("nan"), device=dev) if want_y else None
        yh = torch.full((R, ldh or qn), 7.0, dtype=torch.bfloat16, device=dev)
        ops.attn(dtype=torch.bfloat16, R=R, q=q, row_pos=pos, row_seq=None, kv=kv, y=y, y_h=yh)
        torch.cuda.synchronize()
        return y, yh

    y_ref = torch.full((R, qn), float("nan"), device=dev)
    ops.attn(dtype=torch.bfloat16, R=R, q=q, row_pos=pos, row_seq=None, kv=kv, y=y_ref)
    torch.cuda.synchronize()
    y, yh = launch(True)
    assert torch.equal(y, y_ref) and torch.equal(yh, _rne_bf16(y_ref))
    _, only = launch(False)
    assert torch.equal(only, yh)
    _, wide = launch(False, ldh=qn + 8)
    assert torch.equal(wide[:, :qn], yh) and bool((wide[:, qn:] == 7.0).all())


# ---- frame level ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return load_golden_lm()


@pytest.fixture(scope="module")
def sd(golden):
    return toy_state_dict(golden[1])


def _prompt(d, case, rows):
    tokens = torch.from_numpy(d[f"{case}_tokens"]).long()
    mask = torch.from_numpy(d[f"{case}_mask"]).bool()
    if tokens.dim() == 2:
        tokens, mask = tokens[None], mask[None]
    return tokens[rows].cuda(), mask[rows].cuda()


def _gemv_launches():
    from uniaudio2_amd._lib import lib
    return lib.ua2_debug_kernel_launches(b"gemv")


def _model(sd, tokens, monkeypatch, on):
    monkeypatch.delenv("UA2_NO_ROW_OPERAND", raising=False)
    if not on:
        monkeypatch.setenv("UA2_NO_ROW_OPERAND", "1")
    return build_product_model(sd, torch.bfloat16, batch=tokens.shape[0])        # the switch is read by ua2_stage3_create


def _run(sd, tokens, mask, monkeypatch, on, use_graph=False, **frame_kw):
    """FRAMES greedy audio-feedback frames, one generate_frames call per frame: the frame log, audio_logits and h_final after every
    frame, every GPT's cache pools after the last, and the decode-kernel launches the frames issued."""
    B, L, _ = tokens.shape
    m = _model(sd, tokens, monkeypatch, on)
    m.reset_caches()
    pos = torch.arange(0, L, device="cuda").unsqueeze(0).repeat(B, 1)
    m.forward_prefix(tokens[:, :-1], labels=tokens[:, 1:, :-1], tokens_mask=mask, loss_mask=mask, input_pos=pos[:, :-1])
    m.begin_decode(tokens[:, -1:], mask[:, -1:], torch.tensor([L - 1], device="cuda"))
    log, logits, hfin = [], [], []
    n0 = _gemv_launches()
    for _ in range(FRAMES):
        log.append(m.generate_frames(1, B, 0, use_graph=use_graph, **frame_kw).cpu().clone())
        logits.append(m.buffer("audio_logits", B).cpu().clone())
        hfin.append(m.buffer("h_final", B).cpu().clone())
    n = _gemv_launches() - n0
    pools = []
    for gpt in (m.audio_understanding_expert, m.backbone, m.audio_generation_expert, m.decoder):
        pools += [t.cpu().clone() for t in list(gpt.kv_cache.k) + list(gpt.kv_cache.v)]
    return dict(log=torch.cat(log), logits=logits, hfin=hfin, pools=pools, launches=n)


def _same(a, b):
    assert torch.equal(a["log"], b["log"])
    for f in range(FRAMES):
        assert torch.equal(a["logits"][f], b["logits"][f]), f
        assert torch.equal(a["hfin"][f], b["hfin"][f]), f
    for x, y in zip(a["pools"], b["pools"]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("case,rows", [("tts1", 1), ("tts2", 2)])
def test_frames_agree_with_the_switch_on_and_off(golden, sd, case, rows, monkeypatch):
    d, _ = golden
    tokens, mask = _prompt(d, case, slice(0, rows))
    on = _run(sd, tokens, mask, monkeypatch, on=True)
    off = _run(sd, tokens, mask, monkeypatch, on=False)
    _same(on, off)
    assert int(on["log"][:, :, 1:].min()) >= 0                                  # every audio id of every frame was written
    assert on["launches"] == off["launches"]                                    # the same launches: only their operands changed form
    rep = _run(sd, tokens, mask, monkeypatch, on=True, use_graph=True)          # the captured frame (what the generators replay)
    _same(rep, off)
    skip = _run(sd, tokens, mask, monkeypatch, on=True, skip_text_head=True)    # no riders: the down-projections are plain launches
    skip_off = _run(sd, tokens, mask, monkeypatch, on=False, skip_text_head=True)
    _same(skip, skip_off)


def test_teacher_forced_scoring_is_unchanged(golden, sd, monkeypatch):
    d, _ = golden
    tokens, mask = _prompt(d, "tts2", slice(0, 2))
    out = []
    for on in (True, False):
        m = _model(sd, tokens, monkeypatch, on)
        m.reset_caches()
        r = m.score_sequence(tokens, mask)
        out.append((r["nll"].cpu().clone(), r["pred"].cpu().clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
