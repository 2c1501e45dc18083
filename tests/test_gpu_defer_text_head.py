"""Deferred text head of the audio-feedback loop (include/ua2hip.h UA2_FRAME_DEFER_TEXT_HEAD / ua2_stage3_text_flush): the frames keep
their h_final rows and lm_head runs once per up to 64 kept rows.  Everything a caller can observe — the id log (text column
included), the logits buffers, the fed-back state, what a continued run produces — is bit-identical to running lm_head in every frame."""
import pytest
import torch

from helpers import build_product_model, load_golden_lm, toy_state_dict
from toy_configs import TOY_MODEL_ARGS

gpu = pytest.mark.gpu
RC = TOY_MODEL_ARGS["audio_reason_vocab_size"]
DEFER_ROWS = (5, 6, 16, 17, 33, None)          # UA2_DEFER_ROWS: the launcher's kernel-form steps (decode kernel up to 5 rows, one / two / three row tiles); None = the default 64


@pytest.fixture(scope="module")
def golden():
    return load_golden_lm()


@pytest.fixture(scope="module")
def sd(golden):
    return toy_state_dict(golden[1])


def _refresh():
    from uniaudio2_amd._lib import lib
    lib.ua2_debug_refresh_env()


def _flushes():
    from uniaudio2_amd._lib import lib
    return lib.ua2_debug_kernel_launches(b"text_flush")


def _prompt(d, B):
    """B = 1: the golden's tts1 prompt; B = 2: its two tts2 prompts; more rows: those two and copies with other text ids."""
    case = "tts1" if B == 1 else "tts2"
    tokens, mask = torch.from_numpy(d[f"{case}_tokens"]).long(), torch.from_numpy(d[f"{case}_mask"]).bool()
    if tokens.dim() == 2:
        tokens, mask = tokens[None], mask[None]
    reps = -(-B // tokens.size(0))
    tokens, mask = tokens.repeat(reps, 1, 1)[:B].clone(), mask.repeat(reps, 1, 1)[:B].clone()
    for b in range(2, B):                        # other text ids (below the largest the golden uses): distinct rows
        tokens[b, :, -1] = (tokens[b, :, -1] + 7 * b) % (int(tokens[:, :, -1].max()) + 1)
    return case, tokens, mask


def _start(m, tokens, mask, mode=0, topk=1, cfg=1.0):
    dev = "cuda"
    B, L, _ = tokens.shape
    tokens, mask = tokens.to(dev), mask.to(dev)
    m.reset_caches()
    pos = torch.arange(0, L, device=dev).unsqueeze(0).repeat(B, 1)
    m.forward_prefix(tokens[:, :-1], tokens_mask=mask, input_pos=pos[:, :-1])
    m.set_cfg(cfg)
    m.set_sampling(1, 1.0, seed=0)               # a new key rewinds the draw index: every run draws the same numbers
    m.set_sampling(topk, 0.9, seed=77)
    m.begin_decode(tokens[:, -1:], mask[:, -1:], torch.tensor([L - 1], device=dev))


def _observe(m, B, frames, defer, more=3):
    """`frames` frames, everything observable afterwards, and `more` frames continued from there."""
    log = m.generate_frames(frames, B, 0, reason_eos=-1, reason_card=RC, defer_text_head=defer).cpu().clone()
    st = m._st
    out = dict(log=log, text_logits=m.buffer("text_logits", B).cpu().clone(), audio_logits=m.buffer("audio_logits", B).cpu().clone(),
               tokens=st["tokens"][:B].cpu().clone(), mask=st["mask"][:B].cpu().clone(), row_pos=st["row_pos"][:B].cpu().clone())
    out["more"] = m.generate_frames(more, B, 0, reason_eos=-1, reason_card=RC, defer_text_head=defer).cpu().clone()
    return out


@gpu
@pytest.mark.parametrize("B", [1, 2, 5])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_every_bit_equals_the_undeferred_path(golden, sd, dtype, B, monkeypatch):
    from uniaudio2_amd.llm_models.model_new import defer_windows
    d, _ = golden
    case, tokens, mask = _prompt(d, B)
    frames = 20 if B == 5 else 14
    m = build_product_model(sd, dtype, batch=B)
    _start(m, tokens, mask)
    n0 = _flushes()
    ref = _observe(m, B, frames, defer=False)
    assert _flushes() == n0
    assert ref["log"].shape == (frames, B, 9) and int((ref["log"][:, :, 0] < 0).sum()) == 0
    for rows in DEFER_ROWS:
        if rows is None:
            monkeypatch.delenv("UA2_DEFER_ROWS", raising=False)
        else:
            monkeypatch.setenv("UA2_DEFER_ROWS", str(rows))
        _refresh()
        _start(m, tokens, mask)
        n0 = _flushes()
        got = _observe(m, B, frames, defer=True)
        cap = rows or 64
        assert _flushes() - n0 == len(defer_windows(0, frames, B, cap)) + len(defer_windows(frames, 3, B, cap)), rows   # it did defer
        assert int((got["log"][:, :, 0] < 0).sum()) == 0 and int((got["more"][:, :, 0] < 0).sum()) == 0, rows
        for k in ref:
            assert torch.equal(got[k], ref[k]), (rows, k)
    if dtype == torch.float32:                                     # and the ids are the reference's own
        gold = torch.from_numpy(d[f"{case}_samples"]).long()
        n = int((d[f"{case}_forbid"] == 0).sum())                  # the golden raises forbid_prefix by hand from there on
        rows_g = min(B, gold.shape[1])
        assert n >= 4 and torch.equal(got["log"][:n, :rows_g].long(), gold[:n, :rows_g])


@gpu
def test_eligible_calls_flush_and_ineligible_calls_do_not(golden, sd, monkeypatch):
    from uniaudio2_amd.llm_models.model_new import defer_windows
    d, _ = golden
    _, tokens, mask = _prompt(d, 2)

    def run(m, frames, mode=0, defer=True, topk=1, cfg=1.0, **kw):
        _start(m, tokens, mask, mode, topk, cfg)
        n0 = _flushes()
        log = m.generate_frames(frames, 2, mode, reason_eos=-1, reason_card=RC, defer_text_head=defer, **kw).cpu().clone()
        return log, _flushes() - n0

    m = build_product_model(sd, torch.bfloat16, batch=2)
    log, n = run(m, 12)
    assert n == len(defer_windows(0, 12, 2, 64)) == 1
    assert torch.equal(log, run(m, 12, defer=False)[0])
    monkeypatch.setenv("UA2_DEFER_ROWS", "8")
    _refresh()
    log8, n = run(m, 12)
    assert n == len(defer_windows(0, 12, 2, 8)) == 3 and torch.equal(log8, log)
    monkeypatch.delenv("UA2_DEFER_ROWS")
    _refresh()

    def same_and_unflushed(what, mm=m, **kw):
        a, na = run(mm, kw.pop("frames", 6), **kw)
        b, nb = run(mm, a.shape[0], defer=False, **kw)
        assert na == 0 and nb == 0, what
        assert torch.equal(a, b), what

    same_and_unflushed("one frame", frames=1)
    same_and_unflushed("text feedback", mode=1)
    same_and_unflushed("guided pair", mode=2, cfg=1.5)
    same_and_unflushed("top-k", topk=5)
    same_and_unflushed("skip_text_head", skip_text_head=True)
    m.set_order_free_rows(2)
    same_and_unflushed("order-free rows")
    m.set_order_free_rows(0)
    monkeypatch.setenv("UA2_NO_DEFER_TEXT_HEAD", "1")
    _refresh()
    same_and_unflushed("environment opt-out")
    monkeypatch.delenv("UA2_NO_DEFER_TEXT_HEAD")
    _refresh()
    assert run(m, 6)[1] == 1                                       # ... and eligible again
    try:
        from test_gpu_w8 import FP8
    except ImportError:
        FP8 = None
    if FP8 is not None:
        m8 = build_product_model(sd, torch.bfloat16, batch=2, weight_dtype=FP8)
        same_and_unflushed("fp8 plan", mm=m8)


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_two_calls_back_to_back_equal_one(golden, sd, dtype):
    d, _ = golden
    _, tokens, mask = _prompt(d, 2)
    m = build_product_model(sd, dtype, batch=2)
    _start(m, tokens, mask)
    one = m.generate_frames(16, 2, 0, reason_eos=-1, reason_card=RC).cpu().clone()
    _start(m, tokens, mask)
    n0 = _flushes()
    a = m.generate_frames(8, 2, 0, reason_eos=-1, reason_card=RC).cpu().clone()
    b = m.generate_frames(8, 2, 0, reason_eos=-1, reason_card=RC).cpu().clone()
    assert _flushes() - n0 == 2                                    # one window per call: nothing is carried between calls
    assert torch.equal(torch.cat([a, b]), one) and int((one[:, :, 0] < 0).sum()) == 0


@gpu
def test_recorded_frames_replay_until_the_environment_is_refreshed(golden, sd):
    """The executor's graph cache (ua2_stage3.hip FrameKey / drop_graphs).  Captured frames count their launches at capture only, so the
    rise of a family counter over a call says whether a frame was recorded or replayed: a frame is recorded once per key, replayed
    after that, and recorded again after ua2_debug_refresh_env (the launch-time knobs are baked into it) — with the ids of the ungraphed
    path throughout.  The guidance scale is part of the key: another scale records another frame, the first one's stays."""
    from uniaudio2_amd._lib import lib
    d, _ = golden

    def frames(m, n, B=1, mode=0, use_graph=True):
        n0 = lib.ua2_debug_kernel_launches(b"gemv")
        log = m.generate_frames(n, B, mode, reason_eos=-1, reason_card=RC, use_graph=use_graph, defer_text_head=False).cpu().clone()
        return log, lib.ua2_debug_kernel_launches(b"gemv") - n0

    _, tokens, mask = _prompt(d, 1)
    m = build_product_model(sd, torch.bfloat16, batch=1)
    _start(m, tokens, mask)
    a, per_frame = frames(m, 2)
    assert per_frame > 0                                           # recorded once; the call's second frame replayed it
    b, n = frames(m, 1)
    assert n == 0                                                  # replayed
    _refresh()                                                     # the environment itself is unchanged
    c, n = frames(m, 1)
    assert n == per_frame                                          # recorded again
    ref = build_product_model(sd, torch.bfloat16, batch=1)
    _start(ref, tokens, mask)
    assert torch.equal(torch.cat([a, b, c]), frames(ref, 4, use_graph=False)[0])

    _, tokens, mask = _prompt(d, 2)
    m = build_product_model(sd, torch.bfloat16, batch=2)
    _start(m, tokens, mask, mode=2, cfg=2.0)
    per_frame = frames(m, 2, 2, 2)[1]
    assert per_frame > 0
    m.set_cfg(2.0)
    assert frames(m, 1, 2, 2)[1] == 0                              # the same scale: the same key
    m.set_cfg(1.5)
    assert frames(m, 1, 2, 2)[1] == per_frame                      # another scale: recorded anew
    m.set_cfg(2.0)
    assert frames(m, 1, 2, 2)[1] == 0                              # ... and the first frame is still there


@pytest.fixture(scope="module")
def full_model():
    import bench
    return bench.build_model(torch.device("cuda"), seed=0), bench


@gpu
def test_fullsize_windows_of_64_and_2_rows(full_model):
    """The real N = 128 256, K = 3072 instantiations of lm_head at 64 rows and at 2 rows, and the undeferred last frame: 67 frames."""
    m, bench = full_model
    dev = torch.device("cuda")
    tokens, mask = bench.make_prompt(dev, seed=4242)
    m.setup_caches(1, dtype=torch.bfloat16, max_seq_length=256, max_rows=64, log_frames=80)
    outs = []
    for defer in (False, True):
        L = tokens.size(1)
        m.reset_caches()
        pos = torch.arange(L, device=dev).unsqueeze(0)
        m.forward_prefix(tokens[:, :-1], tokens_mask=mask, input_pos=pos[:, :-1])
        m.begin_decode(tokens[:, -1:], mask[:, -1:], torch.tensor([L - 1], device=dev))
        n0 = _flushes()
        log = m.generate_frames(67, 1, 0, reason_eos=-1, reason_card=bench.REASON_CARD, defer_text_head=defer).cpu().clone()
        assert _flushes() - n0 == (2 if defer else 0)
        outs.append((log, m.buffer("text_logits", 1).cpu().clone()))
    assert int((outs[0][0][:, :, 0] < 0).sum()) == 0
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("R", [1, 2, 5, 32])
@pytest.mark.parametrize("n_frames", [2, 64, 65, 74, 129])
@pytest.mark.parametrize("start", [0, 5, 63, 64])
def test_windows_tile_the_deferred_frames(start, n_frames, R):
    from uniaudio2_amd.llm_models.model_new import defer_windows
    for cap_rows in (64, 33, 32 if R == 32 else 5 * R):
        cap_frames = cap_rows // R
        win = defer_windows(start, n_frames, R, cap_rows)
        covered = [f for f0, n in win for f in range(f0, f0 + n)]
        assert covered == list(range(start, start + n_frames - 1))          # exactly the deferred frames, in order; never the last frame
        for f0, n in win:
            assert n >= 1 and n * R <= cap_rows
            assert f0 // cap_frames == (f0 + n - 1) // cap_frames            # never across a multiple of cap_frames: the ring does not wrap
    with pytest.raises(ValueError):
        defer_windows(0, 4, 5, 4)
