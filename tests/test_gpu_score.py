"""Teacher-forced scoring on the device (include/ua2hip.h ua2_xent_embed / ua2_stage3_score; Model_stage3.score / score_sequence /
forward): the cross-entropy tail against float64, the fp32 plan against the reference's own forward (tests/golden/lm_score.npz), the
tie to generation (a greedy sequence scored teacher-forced reproduces the ids and logits generation saw: lm_toy_fp32.npz), the bf16
plan against the oracle restatement (tests/score_ref.py), row / batch / chunking invariance, the fp8 plan's contract, the absence of
side effects on the decode state, and one chunk at the released sizes."""
import json
import os

import numpy as np
import pytest
import torch

import score_ref
from helpers import GOLDEN, build_oracle, build_product_model, load_golden_lm, product_decode_loop, toy_state_dict

pytestmark = pytest.mark.gpu

# Bar of the kernel's finite nll against float64.  HOST_FP32_ERR: the worst |error| against float64 of an fp32 numpy restatement of the
# kernel's formula (score_ref.xent32: max-subtracted, every operation rounded to fp32, numpy's pairwise sums) on the very inputs of
# test_xent_embed_against_float64 — measured 8.22e-7 (V = 128256, M = 67; nll up to 17.3, where half an fp32 ulp is 9.5e-7), and
# re-measured on the host by tests/test_score_host.py.  The bar is 8 x that: room for another summation order and for the ulps of the
# device's expf / logf.
HOST_FP32_ERR = 8.3e-7
NLL_BAR = 8 * HOST_FP32_ERR
TEXT_ATOL, AUDIO_ATOL = 3.5e-2, 2.5e-2       # the bf16 plan's logit bars of tests/test_gpu_lm.py (teacher-forced frames against the bf16 oracle)


def _lib():
    from uniaudio2_amd._lib import check, lib
    return lib, check


def _launches(family="score"):
    return _lib()[0].ua2_debug_kernel_launches(family.encode())


def run_xent(x, y, V, emb=None, emb_row0=0):
    """ua2_xent_embed on logits x (M, ld) float32 / labels y (M,) (numpy), labels and outputs in column 1 of 3-wide buffers.  emb: a
    device table (rows, C) float32 or bfloat16.  -> nll (M,), pred (M,), gathered rows (M, C) or None, all numpy / torch cpu."""
    from uniaudio2_amd import ops
    lib, check = _lib()
    M, ld = x.shape
    dev = torch.device("cuda")
    xd = torch.from_numpy(x).to(dev)
    lab = torch.full((M, 3), 12345, dtype=torch.int32, device=dev)
    lab[:, 1] = torch.from_numpy(y).to(dev)
    nll = torch.full((M, 3), -7.0, dtype=torch.float32, device=dev)
    pred = torch.full((M, 3), -7, dtype=torch.int32, device=dev)
    out, dt, Cw = None, ops.dtype_code(torch.float32), 0
    if emb is not None:
        Cw = emb.shape[1]
        out = torch.full((M, Cw), -7.0, dtype=torch.float32, device=dev)
        dt = ops.dtype_code(emb.dtype)
    check(lib.ua2_xent_embed(dt, M, xd.data_ptr(), ld, V, lab.data_ptr(), 3, 1, nll.data_ptr(), pred.data_ptr(), 3, 1,
                             emb.data_ptr() if emb is not None else None, emb_row0, Cw, out.data_ptr() if out is not None else None,
                             ops.stream()), "ua2_xent_embed")
    torch.cuda.synchronize()
    assert bool((nll[:, [0, 2]] == -7.0).all()) and bool((pred[:, [0, 2]] == -7).all()), "wrote outside its output column"
    return nll[:, 1].cpu().numpy(), pred[:, 1].cpu().numpy(), None if out is None else out.cpu()


@pytest.mark.parametrize("V,ld", score_ref.XENT_SHAPES)
def test_xent_embed_against_float64(V, ld):
    g = torch.Generator().manual_seed(V)
    Cw, row0 = 40, 3
    tables = [torch.randn(V + row0, Cw, generator=g).to("cuda"), torch.randn(V + row0, Cw, generator=g).to("cuda", torch.bfloat16)]
    worst = 0.0
    for M in score_ref.XENT_ROWS:
        x, y = score_ref.xent_rows(V, ld, M)
        want = score_ref.xent64_stable(x[:, :V], y)
        with np.errstate(all="ignore"):
            want_pred = np.where(np.isnan(x[:, :V]), -np.inf, x[:, :V]).argmax(axis=-1)     # numpy's first arg-max; a NaN never wins
        for emb in tables + [None]:
            nll, pred, rows = run_xent(x, y, V, emb, row0)
            assert np.array_equal(pred, want_pred), (V, M)
            assert np.array_equal(np.isnan(nll), np.isnan(want)), "a row of -inf, or one that holds a NaN, gives NaN"
            assert np.array_equal(np.isposinf(nll), np.isposinf(want)), "a -inf target gives +inf"
            assert not np.isneginf(nll).any()
            assert (nll[y < 0] == 0).all(), "label -1 gives 0"
            fin = np.isfinite(want)
            if fin.any():
                err = float(np.abs(nll[fin].astype(np.float64) - want[fin]).max())
                worst = max(worst, err)
                assert err <= NLL_BAR, (V, M, err)
            if emb is not None:
                src = emb.float().cpu()[row0 + np.clip(y, 0, None).astype(np.int64)]         # the LABEL's row (label -1: row emb_row0)
                assert torch.equal(rows, src), "gather is not the label's table row bit for bit"
        if M == 67:   # a row's bits do not depend on the rows beside it
            nll67, pred67, _ = run_xent(x, y, V)
            for m in (0, 2, 6, 13, 66):
                n1, p1, _ = run_xent(x[m:m + 1], y[m:m + 1], V)
                assert n1.view(np.int32)[0] == nll67.view(np.int32)[m] and p1[0] == pred67[m], (V, m)
    print(f"ua2_xent_embed V={V}: worst finite |nll - float64| {worst:.3e} (bar {NLL_BAR:.3e})")


def test_xent_embed_rejects_bad_arguments():
    lib, _ = _lib()
    x = torch.zeros(2, 8, device="cuda")
    lab = torch.zeros(2, dtype=torch.int32, device="cuda")
    nll, pred = torch.zeros(2, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    assert lib.ua2_xent_embed(0, 2, x.data_ptr(), 4, 8, lab.data_ptr(), 1, 0, nll.data_ptr(), pred.data_ptr(), 1, 0, None, 0, 0, None, None) != 0  # ld < V
    assert lib.ua2_xent_embed(0, 2, x.data_ptr(), 8, 8, lab.data_ptr(), 1, 1, nll.data_ptr(), pred.data_ptr(), 1, 0, None, 0, 0, None, None) != 0  # label column
    assert lib.ua2_xent_embed(0, 2, x.data_ptr(), 8, 8, lab.data_ptr(), 1, 0, nll.data_ptr(), pred.data_ptr(), 1, 0, x.data_ptr(), 0, 4, None, None) != 0  # gather without emb_out


# ---- plans ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "lm_score.npz")), json.load(open(os.path.join(GOLDEN, "lm_score.json")))


@pytest.fixture(scope="module")
def golden_lm():
    return load_golden_lm()


@pytest.fixture(scope="module")
def sd(golden_lm):
    return toy_state_dict(golden_lm[1])


@pytest.fixture(scope="module")
def fp32_plan(sd):
    return build_product_model(sd, torch.float32, batch=2)


@pytest.fixture(scope="module")
def bf16_plan(sd):
    return build_product_model(sd, torch.bfloat16, batch=4)


def case_inputs(d, case, dev="cuda"):
    t = lambda k, dt: torch.from_numpy(d[f"{case}_{k}"]).to(dev, dt)
    return t("tokens", torch.long), t("mask", torch.bool), t("loss_mask", torch.bool), t("text_labels", torch.long)


def golden_nll_pred(d, case):
    """lse - logit and arg-max of the reference's logits in the layout of Model_stage3.score, and the margins: (B, S, 9) each."""
    mask = d[f"{case}_mask"]
    B, L, W = mask.shape
    sel = mask[:, 1:, 0]
    nll, pred, margin = np.zeros((B, L - 1, W)), np.full((B, L - 1, W), -1, dtype=np.int64), np.full((B, L - 1, W), np.inf)
    nll[..., -1] = score_ref.xent64(d[f"{case}_text_logits"], d[f"{case}_text_labels"])
    pred[..., -1] = d[f"{case}_text_logits"].argmax(-1)
    margin[..., -1] = d[f"{case}_text_margin"]
    nll[..., :-1][sel] = score_ref.xent64(d[f"{case}_ci_logits"], d[f"{case}_choosed_label"])
    pred[..., :-1][sel] = d[f"{case}_ci_logits"].argmax(-1)
    margin[..., :-1][sel] = d[f"{case}_ci_margin"]
    return nll, pred, margin


@pytest.mark.parametrize("case", ["mix1", "pair2"])
def test_fp32_plan_against_the_reference_forward(golden, fp32_plan, case):
    d, meta = golden
    tokens, mask, loss_mask, text_labels = case_inputs(d, case)
    labels = tokens[:, 1:, :-1]
    text_logits, ci_logits, label, cmask = fp32_plan.forward(tokens[:, :-1], labels, mask, loss_mask)
    e_t = float(np.abs(text_logits.cpu().numpy() - d[f"{case}_text_logits"]).max())
    e_a = float(np.abs(ci_logits.cpu().numpy() - d[f"{case}_ci_logits"]).max())
    print(f"fp32 forward {case}: text logits off by {e_t:.2e}, ci logits by {e_a:.2e}")
    assert ci_logits.shape == d[f"{case}_ci_logits"].shape
    assert e_t < 5e-5 and e_a < 5e-5
    assert np.array_equal(label.cpu().numpy(), d[f"{case}_choosed_label"])
    assert np.array_equal(cmask.cpu().numpy(), d[f"{case}_choosed_mask"])
    out = fp32_plan.score(tokens[:, :-1], labels, mask, loss_mask, text_labels=text_labels)
    want_nll, want_pred, margin = golden_nll_pred(d, case)
    nll, pred = out["nll"].cpu().numpy(), out["pred"].cpu().numpy()
    assert out["nll"].dtype == torch.float32 and out["pred"].dtype == torch.int32 and nll.shape == want_nll.shape
    e_n = float(np.abs(nll - want_nll).max())
    print(f"fp32 score {case}: nll off by {e_n:.2e}")
    assert e_n < 1e-4
    sure = margin > 1e-4
    assert np.array_equal(pred[sure], want_pred[sure])
    sel = d[f"{case}_mask"][:, 1:, 0]
    assert (pred[..., :-1][~sel] == -1).all() and (nll[..., :-1][~sel] == 0).all()
    want = {**meta["metrics"][case]["text"], **meta["metrics"][case]["residual8"]}
    assert set(out["metrics"]) == set(want)
    for k, v in want.items():
        assert out["metrics"][k].dtype == torch.float64 and out["metrics"][k].is_cuda
        assert abs(float(out["metrics"][k]) - v) < 1e-4, (k, float(out["metrics"][k]), v)
    three = fp32_plan.score(tokens[:, :-1], labels, mask, loss_mask, text_labels=text_labels, loss_weights=[1, 1, 1])["metrics"]
    assert set(three) == set(meta["metrics"][case]["text"]) | set(meta["metrics"][case]["residual3"])


def _generated_sequence(d, case, frames, feedback):
    """prompt + the reference's sampled ids of frames 0 .. frames - 1 as the feedback protocol lays them out -> (1, L + frames, 9)."""
    tokens = torch.from_numpy(d[f"{case}_tokens"]).long()
    mask = torch.from_numpy(d[f"{case}_mask"]).bool()
    s = torch.from_numpy(d[f"{case}_samples"][:frames, 0]).long()                  # (F, 9) [text, a0 .. a7]
    cont = torch.zeros(frames, 9, dtype=torch.long)
    cmask = torch.zeros(frames, 9, dtype=torch.bool)
    cont[:, -1] = s[:, 0]
    if feedback == "audio":
        cont[:, :-1] = s[:, 1:]
        cmask[:, :-1] = True
    else:
        cmask[:, -1] = True
    return torch.cat([tokens, cont])[None].cuda(), torch.cat([mask, cmask])[None].cuda(), s


def test_scored_greedy_sequence_reproduces_generation(golden_lm, sd):
    d, _ = golden_lm
    m = build_product_model(sd, torch.float32, batch=1)
    F_ = 9                                                                           # tts1 frames 0 .. 8: before its forbid_prefix switch
    tokens, mask, s = _generated_sequence(d, "tts1", F_, "audio")
    L = tokens.shape[1] - F_
    rows = slice(L - 1, L - 1 + F_)                                                  # row r scores step r + 1
    out = m.score_sequence(tokens, mask)
    pred = out["pred"][0, rows].cpu()
    assert torch.equal(pred[:, :-1].long(), s[:, 1:]) and torch.equal(pred[:, -1].long(), s[:, 0])
    want_nll = score_ref.xent64(d["tts1_audio_logits"][:F_, 0], s[:, 1:].numpy())         # row L - 1 + f is labelled with the audio ids of frame f
    assert float(np.abs(out["nll"][0, rows, :-1].cpu().numpy() - want_nll).max()) < 1e-4
    text_logits, ci_logits, _, _ = m.forward(tokens[:, :-1], tokens[:, 1:, :-1], mask, mask)
    tl, al = text_logits[0, rows].cpu(), ci_logits.cpu()
    assert al.shape[0] == F_
    assert float(np.abs(tl.numpy() - d["tts1_text_logits"][:F_, 0]).max()) < 5e-5
    assert float(np.abs(al.numpy() - d["tts1_audio_logits"][:F_, 0]).max()) < 5e-5
    gen = product_decode_loop(m, tokens[:, :L].cpu(), mask[:, :L].cpu(), F_, "audio", collect_logits=True)
    assert torch.equal(gen["samples"][:, 0].long().cpu(), s)
    assert torch.equal(gen["text_logits"][:, 0], tl), "teacher-forced text logits are not the bits generation saw"
    assert torch.equal(gen["audio_logits"][:, 0], al), "teacher-forced audio logits are not the bits generation saw"
    # asr1: the text stream of a text-feedback loop
    F_ = 10
    tokens, mask, s = _generated_sequence(d, "asr1", F_, "text")
    L = tokens.shape[1] - F_
    rows = slice(L - 1, L - 1 + F_)
    out = m.score_sequence(tokens, mask)
    assert torch.equal(out["pred"][0, rows, -1].cpu().long(), s[:, 0])
    want_nll = score_ref.xent64(d["asr1_text_logits"][:F_, 0], s[:, 0].numpy())        # row L - 1 + f is labelled with the text id of frame f
    assert float(np.abs(out["nll"][0, rows, -1].cpu().numpy() - want_nll).max()) < 1e-4
    text_logits = m.forward(tokens[:, :-1], tokens[:, 1:, :-1], mask, mask)[0]
    tl = text_logits[0, rows].cpu()
    assert float(np.abs(tl.numpy() - d["asr1_text_logits"][:F_, 0]).max()) < 5e-5
    gen = product_decode_loop(m, tokens[:, :L].cpu(), mask[:, :L].cpu(), F_, "text", collect_logits=True)
    assert torch.equal(gen["text_logits"][:, 0], tl)


@pytest.mark.parametrize("case", ["mix1", "pair2"])
def test_bf16_plan_against_the_bf16_oracle(golden, sd, bf16_plan, case):
    d, _ = golden
    tokens, mask, loss_mask, text_labels = case_inputs(d, case)
    labels = tokens[:, 1:, :-1]
    o_text, o_audio = score_ref.teacher_forced(build_oracle(sd, "bf16", batch=tokens.shape[0]), tokens[:, :-1].cpu(), labels.cpu(), mask.cpu())
    sel = mask[:, 1:, 0].cpu()
    text_logits, ci_logits, _, _ = bf16_plan.forward(tokens[:, :-1], labels, mask, loss_mask)
    e_t = float((text_logits.cpu() - o_text).abs().max())
    e_a = float((ci_logits.cpu() - o_audio[sel]).abs().max())
    print(f"bf16 forward {case}: text logits off by {e_t:.2e} (bar {TEXT_ATOL}), ci logits by {e_a:.2e} (bar {AUDIO_ATOL})")
    assert e_t < TEXT_ATOL and e_a < AUDIO_ATOL
    out = bf16_plan.score(tokens[:, :-1], labels, mask, loss_mask, text_labels=text_labels)
    nll, pred = out["nll"].cpu().numpy(), out["pred"].cpu().numpy()
    lab_a = np.where(sel.numpy()[..., None], labels.cpu().numpy(), -1)
    want_t, want_a = score_ref.xent64(o_text.numpy(), text_labels.cpu().numpy()), score_ref.xent64(o_audio.numpy(), lab_a)
    assert float(np.abs(nll[..., -1] - want_t).max()) < 2 * TEXT_ATOL
    assert float(np.abs(nll[..., :-1] - want_a).max()) < 2 * AUDIO_ATOL
    top2 = torch.topk(o_text, 2, dim=-1).values
    sure = ((top2[..., 0] - top2[..., 1]) > TEXT_ATOL).numpy()
    assert np.array_equal(pred[..., -1][sure], o_text.argmax(-1).numpy()[sure])
    top2 = torch.topk(o_audio, 2, dim=-1).values
    sure = ((top2[..., 0] - top2[..., 1]) > AUDIO_ATOL).numpy() & sel.numpy()[..., None]
    assert np.array_equal(pred[..., :-1][sure], o_audio.argmax(-1).numpy()[sure])


def _three(d):
    """pair2's two sequences and the first 14 frames of mix1: three aligned sequences with different contents."""
    t2, m2, l2, _ = case_inputs(d, "pair2")
    t1, m1, l1, _ = case_inputs(d, "mix1")
    n = t2.shape[1]
    return torch.cat([t2, t1[:, :n]]), torch.cat([m2, m1[:, :n]]), torch.cat([l2, l1[:, :n]])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_a_sequence_scores_the_same_bits_alone_and_in_a_batch(golden, sd, bf16_plan, dtype):
    d, _ = golden
    tokens, mask, loss_mask = _three(d)
    m = bf16_plan if dtype == torch.bfloat16 else build_product_model(sd, dtype, batch=4)
    together = m.score_sequence(tokens, mask, loss_mask)
    for b in range(3):
        alone = m.score_sequence(tokens[b:b + 1], mask[b:b + 1], loss_mask[b:b + 1])
        assert torch.equal(alone["nll"][0], together["nll"][b]) and torch.equal(alone["pred"][0], together["pred"][b]), b
    if dtype == torch.float32:                       # ... and under another chunking of the same rows
        m16 = build_product_model(sd, dtype, batch=16)
        other = m16.score_sequence(tokens, mask, loss_mask)
        assert torch.equal(other["nll"], together["nll"]) and torch.equal(other["pred"], together["pred"])


def test_fp8_plan_scores_the_bits_of_the_bf16_plan_on_the_dequantised_weights(golden, sd):
    from w8_ref import w8_state_dict
    d, _ = golden
    tokens, mask, loss_mask = _three(d)
    a = build_product_model(sd, torch.bfloat16, batch=4, weight_dtype=torch.float8_e4m3fn)
    b = build_product_model(w8_state_dict(sd), torch.bfloat16, batch=4)
    ra, rb = a.score_sequence(tokens, mask, loss_mask), b.score_sequence(tokens, mask, loss_mask)
    assert torch.equal(ra["nll"], rb["nll"]) and torch.equal(ra["pred"], rb["pred"])
    assert bool((ra["nll"] > 0).any())


def test_score_leaves_the_decode_state_alone(golden, golden_lm, sd, bf16_plan):
    d, _ = golden
    dl, _ = golden_lm
    m = bf16_plan
    lib, _ = _lib()
    tokens = torch.from_numpy(dl["tts1_tokens"]).long()[None]
    mask = torch.from_numpy(dl["tts1_mask"]).bool()[None]

    def generate():
        m.set_sampling(1)                            # another key, then the seeded one: the draw index is rewound
        m.set_sampling(5, 1.0, seed=123)
        ids = product_decode_loop(m, tokens, mask, 6, "audio", fast=True)["samples"].clone()
        m.set_sampling(1)
        return ids

    ids = generate()
    st = m._st
    before = {k: st[k].clone() for k in ("frame_log", "counters", "out_tokens", "forbid")}
    n0 = _launches()
    st_tokens, st_mask, st_loss = _three(d)
    out = m.score_sequence(st_tokens, st_mask, st_loss)
    torch.cuda.synchronize()
    rows = st_tokens.shape[0] * (st_tokens.shape[1] - 1)
    assert _launches() - n0 == -(-rows // st["B"]), "one ua2_stage3_score per chunk of max_batch rows"
    for k, v in before.items():
        assert torch.equal(st[k], v), f"score changed {k}"
    assert torch.equal(generate(), ids), "the same seeded generation after a score gives other ids"
    # while a beam is attached: refused by the method and by the executor
    m.begin_beams(tokens[0].cuda(), mask[0].cuda(), beam_width=2, max_length=4)
    try:
        with pytest.raises(ValueError, match="beam"):
            m.score_sequence(st_tokens, st_mask, st_loss)
        lab = torch.zeros(1, 9, dtype=torch.int32, device="cuda")
        nll, pred = torch.zeros(1, 9, device="cuda"), torch.zeros(1, 9, dtype=torch.int32, device="cuda")
        assert lib.ua2_stage3_score(m._h, 1, lab.data_ptr(), nll.data_ptr(), pred.data_ptr(), None) != 0
        assert b"beam" in lib.ua2_last_error()
    finally:
        m.end_beams()
    again = m.score_sequence(st_tokens, st_mask, st_loss)
    assert torch.equal(again["nll"], out["nll"]) and torch.equal(again["pred"], out["pred"])


def test_one_chunk_at_the_released_sizes():
    """The random-weight model of tests/test_gpu_fullsize.py (bench.build_model), 16 positions of mixed text / audio, bf16 plan: V =
    128256 through the executor."""
    import bench
    dev = torch.device("cuda")
    m = bench.build_model(dev, seed=0)
    m.setup_caches(16, dtype=torch.bfloat16, max_seq_length=64, max_rows=64, log_frames=8)
    va, vt = bench.SEM_CARD + bench.REASON_CARD, m.backbone.config.padded_vocab_size
    assert vt == 128256
    g = torch.Generator().manual_seed(11)
    L = 17
    tokens = torch.zeros(1, L, 9, dtype=torch.long)
    mask = torch.zeros(1, L, 9, dtype=torch.bool)
    for a, b, audio in ((0, 6, False), (6, 14, True), (14, 17, False)):
        if audio:
            tokens[0, a:b, :-1] = torch.randint(0, va, (b - a, 8), generator=g)
            mask[0, a:b, :-1] = True
        else:
            tokens[0, a:b, -1] = torch.randint(0, 128000, (b - a,), generator=g)
            mask[0, a:b, -1] = True
    n0 = _launches()
    out = m.score_sequence(tokens.to(dev), mask.to(dev))
    assert _launches() - n0 == 1                                                     # 16 rows: one chunk
    nll, pred = out["nll"][0].cpu().numpy(), out["pred"][0].cpu().numpy()
    assert np.isfinite(nll).all()
    text = m.buffer("text_logits", 16).cpu().numpy()                                 # B = 1: the chunk's rows are the sequence's, in order
    audio = m.buffer("audio_logits", 16).cpu().numpy()
    sel = mask[0, 1:, 0].numpy()
    text_labels = np.where(mask[0, 1:, -1].numpy(), tokens[0, 1:, -1].numpy(), -1)
    assert np.array_equal(pred[:, -1], text.argmax(-1))
    assert np.array_equal(pred[sel, :-1], audio[sel].argmax(-1)) and (pred[~sel, :-1] == -1).all()
    e_t = float(np.abs(nll[:, -1] - score_ref.xent64(text, text_labels)).max())
    e_a = float(np.abs(nll[sel, :-1] - score_ref.xent64(audio[sel], tokens[0, 1:, :-1].numpy()[sel])).max())
    print(f"released sizes: nll against float64 of the plan's own logits: text {e_t:.2e}, audio {e_a:.2e} (bar {NLL_BAR:.2e})")
    assert e_t <= NLL_BAR and e_a <= NLL_BAR
    assert (nll[sel, :-1] > 0).all() and (nll[text_labels >= 0, -1] > 0).all() and (nll[text_labels < 0, -1] == 0).all()
