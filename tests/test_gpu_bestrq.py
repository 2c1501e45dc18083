"""BEST-RQ (MusicFM 25 Hz) encoder on the device: ua2_conv2d against F.conv2d in float64, the MusicFM25Hz mirror against goldens from the
reference's own modules (tests/golden/make_golden_bestrq.py), the mel front end against its float64 restatement, and a toy
fetch_codes_batch with the encoder inside.

Tolerances are measured, not picked (bestrq_toy.json, produced on the CPU by the golden generator; max |difference|):
  ua2_conv2d    DESIGN.md §2's exact-conv contract: 2e-5 x max |reference|, the reference being F.conv2d in float64.
  stem          gap between the reference Conv2dSubsampling and bestrq_ref.stem_ref (both fp32): gap_stem_fp32 = 1.401e-06 on values up
                to 4.1.  The kernels sum in yet another order: bound 2 x gap = 2.801e-06.
  fp32 taps     gap between transformers' conformer and bestrq_ref.conformer_ref: gap_enc_fp32 = 1.401e-06; bound 2 x gap.
  bf16 taps     the reference under torch.autocast("cpu", bfloat16) against itself in fp32: gap_enc_bf16 = 2.426e-02; bound 2 x gap.
  mel           bestrq_ref.mel_ref in fp32 against float64: gap_mel = 9.230e-06; the device gets 2 x gap against float64.  The all-zero
                clip is exact.  torchaudio is not installed where the goldens are made: the front end is not pinned on it.
The bounds are read from the json, so regenerating the goldens moves them with the measurement.
"""
import json
import os
from functools import lru_cache

import numpy as np
import pytest
import torch

import bestrq_ref as br
from weights import seeded_tensor

pytestmark = pytest.mark.gpu
HERE = os.path.join(os.path.dirname(__file__), "golden")


@lru_cache(maxsize=None)
def _gold():
    return np.load(os.path.join(HERE, "bestrq_toy.npz")), json.load(open(os.path.join(HERE, "bestrq_toy.json")))


# ---- ua2_conv2d ----------------------------------------------------------------------------------------------------------
def _conv_case(B, Cin, F, T, Cout, stride, res_relu, seed):
    x = seeded_tensor((B, Cin, F, T), seed, std=1.0)
    w = seeded_tensor((Cout, Cin, 3, 3), seed + 1, std=1.0) / (9 * Cin) ** 0.5
    b = seeded_tensor((Cout,), seed + 2, std=0.3)
    Fo, To = (F - 1) // stride[0] + 1, (T - 1) // stride[1] + 1
    r = seeded_tensor((B, Cout, Fo, To), seed + 3, std=1.0) if res_relu else None
    ref = torch.nn.functional.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=1)
    if res_relu:
        ref = torch.relu(ref + r.double())
    return x, w, b, r, ref


def _conv_run(x, w, b, r, stride, relu):
    from uniaudio2_amd import ops
    return ops.conv2d(x.cuda(), ops.pack_conv2d_weight(w.cuda()), w.shape[0], stride=stride, bias=b.cuda(),
                      residual=r.cuda() if r is not None else None, relu=relu).cpu()


# (B, Cin, F, T, Cout, stride, residual + ReLU): the first layer's vector form; a stride-1 block tail; odd F and T; T below any tile
# with three channel groups; Cin and Cout that are no multiples of 16 (handled: padded channels, masked rows); more than one time
# tile, more than one 128-channel row block and a partial one; on the matrix-pipe kernel a Cout below one 16-row tile and a Cout that
# leaves a lone partial tile past a wave's first (40 = 16 + 16 + 8: wave 1 holds rows 32 .. 39 and a clamped, fully masked second tile)
CONV_CASES = [(2, 1, 16, 48, 16, (2, 2), False), (1, 16, 8, 24, 16, (1, 1), True), (2, 16, 7, 21, 32, (2, 2), False),
              (1, 48, 5, 3, 16, (2, 1), False), (1, 20, 6, 19, 24, (1, 2), True), (1, 3, 5, 9, 7, (1, 1), True),
              (1, 16, 3, 150, 144, (1, 2), False), (1, 16, 4, 10, 8, (2, 2), False), (1, 24, 5, 17, 40, (1, 1), True)]


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(str(v) for v in c[:5]) + f"s{c[5][0]}{c[5][1]}" + ("rr" if c[6] else ""))
def test_conv2d_vs_float64(case):
    B, Cin, F, T, Cout, stride, rr = case
    x, w, b, r, ref = _conv_case(B, Cin, F, T, Cout, stride, rr, 9000 + 10 * CONV_CASES.index(case))
    got = _conv_run(x, w, b, r, stride, rr)
    assert got.shape == ref.shape and got.dtype == torch.float32
    err, bound = float((got.double() - ref).abs().max()), 2e-5 * float(ref.abs().max())
    print(f"conv2d {case}: max |device - float64| {err:.3e} (bound {bound:.3e})")
    assert err <= bound


@pytest.mark.parametrize("case", [CONV_CASES[0], CONV_CASES[2]], ids=["cin1", "cin16"])
def test_conv2d_row_of_a_batch_is_the_row_alone(case):
    B, Cin, F, T, Cout, stride, rr = case
    x, w, b, r, _ = _conv_case(B, Cin, F, T, Cout, stride, rr, 9100)
    both = _conv_run(x, w, b, r, stride, rr)
    alone = _conv_run(x[:1].contiguous(), w, b, None, stride, rr)
    assert torch.equal(both[0], alone[0])


def test_conv2d_refuses_bad_strides():
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import Ua2Error
    x, w = torch.zeros(1, 16, 4, 4).cuda(), torch.zeros(16, 16, 3, 3).cuda()
    with pytest.raises(Ua2Error, match="stride"):
        ops.conv2d(x, ops.pack_conv2d_weight(w), 16, stride=(3, 1))


# ---- rotary glue ----------------------------------------------------------------------------------------------------------
def test_layernorm_rope_rows_vs_restatement():
    from uniaudio2_amd import ops
    R, C, hs, P = 37, 64, 32, 40
    x = seeded_tensor((R, C), 9200, std=1.5)
    w, b = 1.0 + 0.1 * seeded_tensor((C,), 9201, std=1.0), seeded_tensor((C,), 9202, std=0.1)
    cos, sin = br.rotary_tables(P, hs, 10000)
    pos = (torch.arange(R) * 7 % P).to(torch.int32)
    got = ops.layernorm_rope_rows(x.cuda(), w.cuda(), b.cuda(), 1e-5, cos.contiguous().cuda(), sin.contiguous().cuda(), pos.cuda(), hs).cpu()
    n = br._ln(x.double(), w.double(), b.double(), 1e-5)
    nh = n.view(R, C // hs, hs)
    c, s = cos.double()[pos.long()][:, None, :], sin.double()[pos.long()][:, None, :]
    rot = (nh * c + torch.cat([-nh[..., hs // 2:], nh[..., :hs // 2]], -1) * s).reshape(R, C)
    plain = ops.layernorm_rows(x.cuda(), w.cuda(), b.cuda(), 1e-5).cpu()
    assert torch.equal(got[:, C:], plain)                              # the un-rotated half is ua2_layernorm_rows, bit for bit
    err = float((got[:, :C].double() - rot).abs().max())
    print(f"layernorm_rope_rows: max |device - float64| {err:.3e}")
    # fp32 unit roundoff u = 2^-24: the LayerNorm value carries <= 8 u (mean and rstd, each amplified by <= 2, then sub, two products, add);
    # the rotation adds three roundings over two such terms: <= 16 u x max |value|
    assert err <= 16 * 2.0 ** -24 * float(rot.abs().max())


# ---- mirror vs golden -------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _encoder(dtype):
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.modules.our_MERT_BESTRQ.mert_fairseq.models.musicfm.model.musicfm_25hz import MusicFM25Hz
    enc = MusicFM25Hz(br.TOY, taps=br.TAPS)
    enc.load_state_dict(br.state_dict(br.TOY, n_layers=max(br.TAPS)), strict=True)
    return enc.cuda().prepare(dtype)


@pytest.mark.parametrize("name", list(br.CASES))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_encoder_vs_reference_golden(name, dtype):
    d, meta = _gold()
    T25 = br.CASES[name]
    enc = _encoder(dtype)
    x = br.stem_input(T25).cuda()
    stem, P = enc.stem(x)
    assert P == T25
    serr = float((stem.view(br.BATCH, P, -1).cpu() - torch.from_numpy(d[f"stem_{name}"])).abs().max())
    print(f"bestrq {name} {dtype}: stem max |device - reference| {serr:.3e} (bound {2 * meta['gap_stem_fp32']:.3e})")
    taps = enc.encode(x)
    bound = 2 * (meta["gap_enc_fp32"] if dtype == torch.float32 else meta["gap_enc_bf16"])
    errs = []
    for t, got in zip(br.TAPS, taps):
        assert got.shape == (br.BATCH, T25, br.TOY["encoder_dim"])
        errs.append(float((got.cpu() - torch.from_numpy(d[f"tap{t}_{name}"])).abs().max()))
    print(f"bestrq {name} {dtype}: taps max |device - reference| {errs} (bound {bound:.3e})")
    alone = enc.encode(x[:1].contiguous())
    for a, g in zip(alone, taps):
        assert torch.equal(a[0], g[0]), "row 0 of B = 2 differs from the row run alone"
    assert serr <= 2 * meta["gap_stem_fp32"], serr                     # the stem is exact fp32 under both plans
    assert max(errs) <= bound, errs


# ---- mel front end ----------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _mel_single(name):
    from uniaudio2_amd import ops
    return ops.melspec(torch.from_numpy(br.clips()[name])[None].cuda(), br.MEL_N_MELS)[0].cpu()


@pytest.mark.parametrize("name", ["a", "b", "z"])
def test_mel_vs_float64_restatement(name):
    _, meta = _gold()
    clip = br.clips()[name]
    got = _mel_single(name)
    ref = br.mel_ref(torch.from_numpy(clip)[None], br.MEL_N_MELS, torch.float64)[0]
    assert got.shape == ref.shape == (128, 4 * (len(clip) // 960)) and got.dtype == torch.float32
    err = float((got.double() - ref).abs().max())
    print(f"mel {name}: max |device - float64| {err:.3e} (bound {2 * meta['gap_mel']:.3e})")
    if name == "z":
        assert torch.equal(got, torch.full_like(got, float((torch.tensor(-100.0) - br.MEL_MEAN) / br.MEL_STD)))
        return
    assert err <= 2 * meta["gap_mel"], err


def test_mel_batch_is_bitwise_the_single_clips():
    from uniaudio2_amd import ops
    clips = br.clips()
    batch = torch.stack([torch.from_numpy(clips["b"]), torch.from_numpy(clips["z"])]).cuda()
    got = ops.melspec(batch, br.MEL_N_MELS).cpu()
    assert torch.equal(got[0], _mel_single("b")) and torch.equal(got[1], _mel_single("z"))


# ---- fetch_codes_batch ------------------------------------------------------------------------------------------------------
def test_fetch_codes_batch_with_the_encoder_inside():
    """Toy fetch_codes_batch with the BEST-RQ and Whisper encoders set and a callable that supplies WavLM only: the codes equal those of
    the same model with bestrq_ref's features (the fp32 restatement on the device's own mel) injected."""
    import test_gpu_codec_model as tcm
    import whisper_ref as wr
    from codec_model_stub import CFG, fetch_inputs
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models.modeling_whisper import WhisperEncoder
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models.PretrainedModel import BESTRQ_Model
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.modules.our_MERT_BESTRQ.mert_fairseq.models.musicfm.model.musicfm_25hz import MusicFM25Hz
    _, meta = tcm._gold()
    model, _ = tcm._toy_model(meta)
    B, T25, P = CFG["B"], CFG["T25"], 72
    cfg = br.config(encoder_dim=CFG["Cb"], num_attention_heads=16, intermediate_size=64, encoder_depth=2)
    sd = br.state_dict(cfg, seed=8300)
    mus = MusicFM25Hz(cfg, taps=(1, 2))
    mus.load_state_dict(sd, strict=True)
    bq = BESTRQ_Model(model=mus, layers=(1, 2), dtype=torch.float32)
    wcfg = dict(d_model=CFG["Cw"], encoder_layers=2, encoder_attention_heads=1, encoder_ffn_dim=128, num_mel_bins=80, max_source_positions=P)
    wenc = WhisperEncoder(wcfg)
    wenc.load_state_dict(wr.encoder_state_dict(wcfg, seed=7300), strict=True)
    object.__setattr__(model, "whisper_encoder", wenc.cuda().prepare(torch.float32))
    object.__setattr__(model, "bestrq_encoder", bq)
    f = {k: v.cuda() for k, v in fetch_inputs().items()}
    mels = torch.stack([wr.encoder_mels(P, seed=7400 + i)[0] for i in range(B)]).cuda()
    audios = (0.1 * seeded_tensor((B, 1, T25 * 960), 8400, std=1.0)).cuda()
    masks = torch.zeros(3, B, dtype=torch.bool)
    with pytest.raises(NotImplementedError, match=r"frozen WavLM encoder \("):
        model.fetch_codes_batch(audios, mels, film_masks=masks)
    model.ssl_features = lambda a, m: dict(wavlm=f["wavlm"])
    rc, mc, _ = model.fetch_codes_batch(audios, mels, film_masks=masks)
    ac, sem = bq.extract_continous_embeds_multiple(audios)
    assert ac.shape == sem.shape == (B, CFG["Cb"], T25)
    mel = mus.preprocess(audios[:, 0]).cpu()
    _, (r_ac, r_sem) = br.encoder_ref(sd, cfg, mel, taps=(1, 2))
    print(f"toy fetch: max |device bestrq feature - bestrq_ref| {float((ac.cpu() - r_ac.transpose(1, 2)).abs().max()):.3e} / "
          f"{float((sem.cpu() - r_sem.transpose(1, 2)).abs().max()):.3e}")
    model.ssl_features = lambda a, m: dict(wavlm=f["wavlm"], bestrq_acoustic=r_ac.transpose(1, 2).contiguous().cuda(),
                                           bestrq_semantic=r_sem.transpose(1, 2).contiguous().cuda())
    rc2, mc2, _ = model.fetch_codes_batch(audios, mels, film_masks=masks)
    assert rc[0].shape == rc2[0].shape and mc[0].shape == (B, 15, 8)
    assert torch.equal(rc[0], rc2[0]) and torch.equal(mc[0], mc2[0])
