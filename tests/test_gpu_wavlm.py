"""WavLM encoder on the device: the four new kernels against float64 restatements (tests/wavlm_ref.py), the WavLMEncoder mirror
against goldens from transformers' WavLMModel (tests/golden/make_golden_wavlm.py), and a toy fetch_codes_batch / tokenize(path) with
all three frozen encoders inside and no callable.

Tolerances (wavlm_toy.json is produced on the CPU by the golden generator; the bounds are read from it, so regenerating moves them):
  ua2_wavlm_conv0     2 x gap_front_fp32 (transformers' feature extractor vs the restatement, both fp32, measured on outputs of
                      max |front|), scaled by max |reference| / max |front|: the same relative bar on this case's output range.
  ua2_conv1d_grouped  DESIGN.md §2's exact-conv contract: 2e-5 x max |reference|, the reference being F.conv1d in float64.
  ua2_relpos_gate     2 x gap_gate (the restatement in fp32 vs float64 on the same inputs).
  ua2_attn_relbias    fp32 2e-4, bf16 1e-2 on unit-scale outputs: the bars tests/test_gpu_attn.py holds for the same two arithmetic
                      classes; the reference reads the K / V values the cache holds (bf16-rounded under the bf16 plan).
  encoder             2 x gap_enc_fp32 / 2 x gap_enc_bf16 (hidden_states[0], every tap, the tap mean), front end 2 x gap_front_fp32.
"""
import json
import os
from functools import lru_cache

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wavlm_ref as wr
from weights import seeded_tensor

pytestmark = pytest.mark.gpu
HERE = os.path.join(os.path.dirname(__file__), "golden")


@lru_cache(maxsize=None)
def _gold():
    d = dict(np.load(os.path.join(HERE, "wavlm_toy.npz")))
    d.update(np.load(os.path.join(HERE, "wavlm_toy_a.npz")))
    return d, json.load(open(os.path.join(HERE, "wavlm_toy.json")))


def _mw():
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models import modeling_wavlm
    return modeling_wavlm


# ---- ua2_wavlm_conv0 ----------------------------------------------------------------------------------------------------------
# (B, N, C, K, stride): the toy first layer; one frame (variance 0); 4 099 frames = 16 statistic chunks of 256 + a partial one, C no power of two
CONV0_CASES = [(2, 4000, 32, 10, 5), (1, 10, 16, 10, 5), (2, 5 * 4099 + 5, 48, 10, 5)]


def _conv0_case(B, N, C, K, seed):
    t = torch.arange(N, dtype=torch.float32)
    x = torch.stack([0.3 * torch.sin(0.05 * (b + 1) * t) + seeded_tensor((N,), seed + b, std=0.1) for b in range(B)])
    return x, seeded_tensor((C, K), seed + 10, std=1.0) / K ** 0.5, 1.0 + 0.1 * seeded_tensor((C,), seed + 11, std=1.0), seeded_tensor((C,), seed + 12, std=0.1)


def _conv0_run(x, w, gw, gb, stride):
    from uniaudio2_amd import ops
    return ops.wavlm_conv0(x.cuda(), w.cuda(), gw.cuda(), gb.cuda(), stride).cpu()


@pytest.mark.parametrize("case", CONV0_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_conv0_vs_float64(case):
    d, meta = _gold()
    B, N, C, K, stride = case
    x, w, gw, gb = _conv0_case(B, N, C, K, 6600 + 20 * CONV0_CASES.index(case))
    got = _conv0_run(x, w, gw, gb, stride)
    ref = wr.conv0_ref(x.double(), w.double(), gw.double(), gb.double(), stride)
    assert got.shape == ref.shape == (B, (N - K) // stride + 1, C) and got.dtype == torch.float32
    front_max = max(float(np.abs(d[f"front_{n}"]).max()) for n in wr.CASES)
    err, bound = float((got.double() - ref).abs().max()), 2 * meta["gap_front_fp32"] * float(ref.abs().max()) / front_max
    print(f"conv0 {case}: max |device - float64| {err:.3e} (bound {bound:.3e}, max |ref| {float(ref.abs().max()):.3f})")
    if got.shape[1] == 1:
        # one frame: mean = the value, variance exactly 0 -> (v - mean) = 0 and the output is GELU(gn_b), whatever the filter
        expect = wr.gelu(gb.double())[None, None, :].expand_as(ref)
        assert float((ref - expect).abs().max()) == 0.0
        assert float((got.double() - expect).abs().max()) <= 2.0 ** -22 * float(expect.abs().max())      # fp32: b c, 1 + erf and the product round once each, erf to 2 ulp of a value < 0.2
    assert err <= bound


def test_conv0_row_of_a_batch_is_the_row_alone_and_zero_clip_is_exact():
    B, N, C, K, stride = CONV0_CASES[2]
    x, w, gw, gb = _conv0_case(B, N, C, K, 6700)
    x[1] = 0.0
    both = _conv0_run(x, w, gw, gb, stride)
    alone = _conv0_run(x[:1].contiguous(), w, gw, gb, stride)
    assert torch.equal(both[0], alone[0])
    # the all-zero clip: every conv value, the mean and the variance are exactly 0: every frame is GELU(gn_b), the bits of the
    # one-frame case (the same device expression on the same operand)
    one = _conv0_run(torch.zeros(1, K), w, gw, gb, stride)
    assert torch.equal(both[1], one[0].expand_as(both[1]))
    assert float((both[1].double() - wr.gelu(gb.double())[None, :]).abs().max()) <= 2.0 ** -22 * float(wr.gelu(gb.double()).abs().max())


def test_conv0_refuses_bad_arguments():
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import Ua2Error
    with pytest.raises(Ua2Error, match="multiple of 4"):
        ops.wavlm_conv0(torch.zeros(1, 100).cuda(), torch.zeros(6, 10).cuda(), torch.ones(6).cuda(), torch.zeros(6).cuda(), 5)


# ---- ua2_conv1d_grouped ---------------------------------------------------------------------------------------------------------
# (B, T, C, groups, K, GELU, residual): toy-like; the released geometry with T < K / 2; the same with two time blocks, plain; odd K (nothing
# dropped) with two row tiles per group; a single step
GCONV_CASES = [(2, 37, 64, 4, 16, True, True), (1, 50, 768, 16, 128, True, True), (1, 200, 768, 16, 128, False, False),
               (2, 19, 32, 2, 5, False, False), (1, 1, 64, 4, 16, True, True)]


def _gconv_case(B, T, C, groups, K, resid, seed):
    x = seeded_tensor((B, T, C), seed, std=1.0)
    w = seeded_tensor((C, C // groups, K), seed + 1, std=1.0) / (K * C // groups) ** 0.5
    return x, w, seeded_tensor((C,), seed + 2, std=0.3), (seeded_tensor((B, T, C), seed + 3, std=1.0) if resid else None)


def _gconv_run(x, w, b, r, groups, act):
    from uniaudio2_amd import ops
    B, T, C = x.shape
    y = ops.conv1d_grouped(x.cuda().view(B * T, C), ops.pack_conv1d_grouped_weight(w.cuda(), groups), B, T, groups, w.shape[-1], bias=b.cuda(),
                           resid=r.cuda().view(B * T, C) if r is not None else None, gelu=act)
    return y.cpu().view(B, T, C)


@pytest.mark.parametrize("case", GCONV_CASES, ids=lambda c: "x".join(str(int(v)) for v in c))
def test_conv1d_grouped_vs_float64(case):
    B, T, C, groups, K, act, resid = case
    x, w, b, r = _gconv_case(B, T, C, groups, K, resid, 6800 + 10 * GCONV_CASES.index(case))
    got = _gconv_run(x, w, b, r, groups, act)
    ref = wr.grouped_conv_ref(x.double(), w.double(), b.double(), groups, act, r.double() if resid else None)
    assert got.shape == ref.shape and got.dtype == torch.float32
    err, bound = float((got.double() - ref).abs().max()), 2e-5 * float(ref.abs().max())
    print(f"conv1d_grouped {case}: max |device - float64| {err:.3e} (bound {bound:.3e})")
    assert err <= bound


def test_conv1d_grouped_row_of_a_batch_is_the_row_alone():
    B, T, C, groups, K, act, resid = GCONV_CASES[0]
    x, w, b, r = _gconv_case(B, T, C, groups, K, resid, 6900)
    both = _gconv_run(x, w, b, r, groups, act)
    alone = _gconv_run(x[:1].contiguous(), w, b, r[:1].contiguous(), groups, act)
    assert torch.equal(both[0], alone[0])


def test_conv1d_grouped_refuses_24_channels_per_group():
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import Ua2Error
    x = torch.zeros(4, 48).cuda()
    with pytest.raises(Ua2Error, match="groups"):
        ops.conv1d_grouped(x, torch.zeros(48 * 24 * 4).cuda(), 1, 4, 2, 4)


# ---- ua2_relpos_gate ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", wr.GATE_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_relpos_gate_vs_float64(case):
    from uniaudio2_amd import ops
    _, meta = _gold()
    R, H, hs = case
    h, w, b, c = wr.gate_case(R, H, hs)
    got = ops.relpos_gate(h.cuda(), w.cuda().contiguous(), b.cuda(), c.cuda(), H).cpu()
    ref = wr.gate_ref(h.double(), w.double(), b.double(), c.double(), H)
    err = float((got.double() - ref).abs().max())
    print(f"relpos_gate {case}: max |device - float64| {err:.3e} (bound {2 * meta['gap_gate']:.3e})")
    assert got.shape == (R, H) and err <= 2 * meta["gap_gate"]


# ---- ua2_attn_relbias -----------------------------------------------------------------------------------------------------------
def _paged(k, v, dtype):
    """k, v [B, H, T, hs] -> (pools in the DenseKV layout, page table, the values the cache holds as float64)."""
    B, H, T, hs = k.shape
    mp = (T + 63) // 64
    kp, vp = torch.zeros(B * mp, H, 64, hs, dtype=dtype), torch.zeros(B * mp, H, 64, hs, dtype=dtype)
    for b in range(B):
        for pg in range(mp):
            n = min(64, T - pg * 64)
            kp[b * mp + pg, :, :n] = k[b, :, pg * 64:pg * 64 + n].to(dtype)
            vp[b * mp + pg, :, :n] = v[b, :, pg * 64:pg * 64 + n].to(dtype)
    table = torch.arange(B * mp, dtype=torch.int32).view(B, mp)
    return kp.cuda(), vp.cuda(), table.cuda(), k.to(dtype).double(), v.to(dtype).double()


def _attn_setup(case, dtype):
    from uniaudio2_amd import ops
    B, H, hs, T = case
    q, k, v, gate, embed = wr.attn_case(B, H, hs, T)
    kp, vp, table, k64, v64 = _paged(k, v, dtype)
    s = dict(B=B, H=H, hs=hs, T=T, keep=(kp, vp, table), geom=ops.kv_geom(kp, vp, table, H, H, hs),
             q=q.permute(0, 2, 1, 3).reshape(B * T, H * hs).contiguous().cuda(), gate=gate.permute(0, 2, 1).reshape(B * T, H).contiguous().cuda(),
             all_pos=torch.full((B * T,), T - 1, dtype=torch.int32).cuda(), seq=torch.arange(B, dtype=torch.int32).repeat_interleave(T).cuda(),
             q_pos=torch.arange(T, dtype=torch.int32).repeat(B).cuda(), embed=embed, q64=q.double(), k64=k64, v64=v64, gate64=gate.double())
    s["tab"] = _mw().bias_table(embed, T, 320, 800).cuda()
    return s


def _rows(x):                               # [B, H, T, hs] -> [B * T, H * hs]
    B, H, T, hs = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * T, H * hs)


def _groups(s, qt, reverse=False):
    """Row groups of qt * 16 rows; reverse: the rows of a sequence dealt in descending order (another composition of every group)."""
    from uniaudio2_amd import ops
    B, T = s["B"], s["T"]
    if not reverse:
        return ops.attn_groups(np.full(B * T, T - 1), np.repeat(np.arange(B), T), s["H"], s["H"], "cuda", q_tiles=qt)
    per, rows, gseq = qt * 16, [], []
    for b in range(B):
        order = np.arange(b * T, (b + 1) * T)[::-1]
        for c in range(0, T, per):
            idx = order[c:c + per]
            rows.append(np.concatenate([idx, np.full(per - len(idx), -1)]))
            gseq.append(b)
    to = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int32)).cuda()
    return to(np.stack(rows)).contiguous(), to(gseq), to(np.full(len(gseq), T)), qt


def _relbias(s, dtype, groups=None, tab=None, q_pos=None):
    from uniaudio2_amd import ops
    y = torch.full((s["B"] * s["T"], s["H"] * s["hs"]), float("nan"), device="cuda")
    tab = s["tab"] if tab is None else tab
    ops.attn_relbias(dtype=dtype, R=y.shape[0], q=s["q"], row_pos=s["all_pos"], row_seq=s["seq"], kv=s["geom"], q_pos=s["q_pos"] if q_pos is None else q_pos,
                     gate=s["gate"], rel_tab=tab, y=y, groups=groups)
    return y.cpu()


@pytest.mark.parametrize("case", wr.ATTN_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_attn_relbias_fp32_vs_float64(case):
    s = _attn_setup(case, torch.float32)
    got = _relbias(s, torch.float32)
    ref = _rows(wr.attn_ref(s["q64"], s["k64"], s["v64"], s["gate64"], wr.bias_table(s["embed"], s["T"], 320, 800).double()))
    err = float((got.double() - ref).abs().max())
    print(f"attn_relbias fp32 {case}: max |device - float64| {err:.3e} (bound 2e-4); max |gate * table| "
          f"{float((s['gate64'].max() * s['embed'].abs().max())):.2f}")
    assert err <= 2e-4


@pytest.mark.parametrize("case", wr.ATTN_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_attn_relbias_bf16_vs_float64_and_grouping(case):
    s = _attn_setup(case, torch.bfloat16)
    ref = _rows(wr.attn_ref(s["q64"], s["k64"], s["v64"], s["gate64"], wr.bias_table(s["embed"], s["T"], 320, 800).double()))
    outs = [_relbias(s, torch.bfloat16, _groups(s, 4)), _relbias(s, torch.bfloat16, _groups(s, 4, reverse=True))]
    if s["hs"] == 64:
        outs.append(_relbias(s, torch.bfloat16, _groups(s, 8)))
    err = float((outs[0].double() - ref).abs().max())
    print(f"attn_relbias bf16 {case}: max |device - float64| {err:.3e} (bound 1e-2)")
    for o in outs[1:]:
        assert torch.equal(o, outs[0]), "a row's result depends on how the rows are grouped"
    assert err <= 1e-2


def test_attn_relbias_zero_table_is_ops_attn():
    """fp32: with an all-zero table the parity form is ua2_attn's fp32 row kernel term for term (score + gate * 0): torch.equal, given q
    scaled by head_size^-0.5 = 2^-3 exactly (ua2_attn multiplies by the same power of two itself).  bf16: the flash form is a second
    kernel compiled on its own; its scores are (q 2^-3) log2 e against ua2_attn's q (log2 e 2^-3) — the same bits — but equality of two
    separately compiled softmax bodies does not hold by construction, so only the 1e-2 bar is asserted there."""
    from uniaudio2_amd import ops
    case = (2, 2, 64, 50)
    for dtype in (torch.float32, torch.bfloat16):
        s = _attn_setup(case, dtype)
        groups = _groups(s, 4) if dtype == torch.bfloat16 else None
        got = _relbias(s, dtype, groups, tab=torch.zeros_like(s["tab"]))
        y = torch.empty_like(got).cuda()
        ops.attn(dtype=dtype, R=y.shape[0], q=(s["q"] * 8.0).contiguous(), row_pos=s["all_pos"], row_seq=s["seq"], kv=s["geom"], y=y, groups=groups)
        diff = float((got - y.cpu()).abs().max())
        print(f"zero table vs ops.attn {dtype}: max |difference| {diff:.3e}")
        if dtype == torch.float32:
            assert torch.equal(got, y.cpu())
        else:
            assert diff <= 1e-2


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_attn_relbias_clamps_the_table_index(dtype):
    """A table shorter than the sequence (tab_half = 10 < T - 1) on a legal buffer: relative positions beyond +-10 read the end entries;
    a q_pos far outside reads entry 0 for every key."""
    case = (1, 2, 64, 50)
    s = _attn_setup(case, dtype)
    T, half = s["T"], 10
    groups = _groups(s, 4) if dtype == torch.bfloat16 else None
    short = s["tab"][:, T - 1 - half:T + half].contiguous()
    pos = torch.arange(T)
    rel = (pos[None, :] - pos[:, None]).clamp(-half, half) + half
    bound = 2e-4 if dtype == torch.float32 else 1e-2
    got = _relbias(s, dtype, groups, tab=short)
    ref = _rows(wr.attn_ref(s["q64"], s["k64"], s["v64"], s["gate64"], short.cpu().double()[:, rel]))
    assert float((got.double() - ref).abs().max()) <= bound
    far = _relbias(s, dtype, groups, tab=short, q_pos=(s["q_pos"] + 100000).contiguous())
    ref_far = _rows(wr.attn_ref(s["q64"], s["k64"], s["v64"], s["gate64"], short.cpu().double()[:, torch.zeros(T, T, dtype=torch.long)]))
    assert float((far.double() - ref_far).abs().max()) <= bound


def test_attn_relbias_refuses_other_head_sizes():
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import Ua2Error
    kp = torch.zeros(1, 2, 64, 32).cuda()
    table = torch.zeros(1, 1, dtype=torch.int32).cuda()
    z = lambda *shape: torch.zeros(*shape).cuda()
    with pytest.raises(Ua2Error, match="head_size 32"):
        ops.attn_relbias(dtype=torch.float32, R=1, q=z(1, 64), row_pos=table.view(-1), row_seq=table.view(-1), kv=ops.kv_geom(kp, kp, table, 2, 2, 32),
                         q_pos=table.view(-1), gate=z(1, 2), rel_tab=z(2, 1), y=z(1, 64))


# ---- mirror vs golden -------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _encoder(dtype):
    enc = _mw().WavLMEncoder(wr.TOY, taps=wr.TAPS)
    enc.load_state_dict(wr.state_dict(wr.TOY), strict=True)
    return enc.cuda().prepare(dtype)


@pytest.mark.parametrize("name", list(wr.CASES))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_encoder_vs_transformers_golden(name, dtype):
    d, meta = _gold()
    enc = _encoder(dtype)
    wav = wr.clips(name).cuda()
    rows, T = enc.front_end(wav)
    assert T == enc.frames(wr.CASES[name])
    ferr = float((rows.view(wr.BATCH, T, -1).cpu() - torch.from_numpy(d[f"front_{name}"])).abs().max())
    hs = enc.hidden_states(wav)
    mean = enc(wav)
    bound = 2 * (meta["gap_enc_fp32"] if dtype == torch.float32 else meta["gap_enc_bf16"])
    errs = {i: float((hs[i].cpu() - torch.from_numpy(d[f"hs{i}_{name}"])).abs().max()) for i in (0,) + wr.TAPS}
    errs["mean"] = float((mean.cpu() - torch.from_numpy(d[f"mean_{name}"])).abs().max())
    print(f"wavlm {name} {dtype}: front max |device - transformers| {ferr:.3e} (bound {2 * meta['gap_front_fp32']:.3e}); "
          f"hidden_states / mean {errs} (bound {bound:.3e})")
    assert mean.shape == (wr.BATCH, T, wr.TOY["hidden_size"])
    alone = enc.hidden_states(wav[:1].contiguous())
    for a, g in zip(alone, hs):
        assert torch.equal(a[0], g[0]), "row 0 of B = 2 differs from the row run alone"
    assert ferr <= 2 * meta["gap_front_fp32"], ferr                    # the feature extractor is fp32 under both plans
    assert max(errs.values()) <= bound, errs


# ---- fetch_codes_batch / tokenize with the three encoders inside --------------------------------------------------------------------
# WavLM at the released convolution geometry (320 samples per frame) and a toy width of 128 = 2 heads x 64
FETCH_WAVLM = dict(wr.TOY, conv_dim=(32,) * 7, conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2), num_hidden_layers=2)


@lru_cache(maxsize=None)
def _codec_with_encoders(P):
    """Toy AudioDiffusion1D (wavlm_fea_dim 128) carrying toy Whisper (P positions), BEST-RQ and WavLM encoders, ssl_features None."""
    import zlib
    import bestrq_ref as br
    import whisper_ref as whr
    from codec_model_stub import CFG, module_state_dict
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models.AudioDiffusion1D import AudioDiffusion1D
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models.modeling_whisper import WhisperEncoder
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models.PretrainedModel import BESTRQ_Model
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.modules.our_MERT_BESTRQ.mert_fairseq.models.musicfm.model.musicfm_25hz import MusicFM25Hz
    c = CFG
    m = AudioDiffusion1D(whisper_fea_dim=c["Cw"], wavlm_fea_dim=128, codec_dim=c["D"], encoder_depth=c["depth"], unet_model_config_path=None)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    new = module_state_dict(shapes, 305)
    for k in shapes:
        if k.endswith("_codebook.embed"):
            lvl = int(k.split("layers.")[1].split(".")[0])
            new[k] = seeded_tensor(shapes[k], zlib.crc32(k.encode()) % 100000, std=0.7 ** lvl)
    m.load_state_dict(new)
    m = m.cuda().prepare()
    cfg = br.config(encoder_dim=c["Cb"], num_attention_heads=16, intermediate_size=64, encoder_depth=2)
    mus = MusicFM25Hz(cfg, taps=(1, 2))
    mus.load_state_dict(br.state_dict(cfg, seed=8300), strict=True)
    wcfg = dict(d_model=c["Cw"], encoder_layers=2, encoder_attention_heads=1, encoder_ffn_dim=128, num_mel_bins=80, max_source_positions=P)
    wenc = WhisperEncoder(wcfg)
    wenc.load_state_dict(whr.encoder_state_dict(wcfg, seed=7300), strict=True)
    lenc = _mw().WavLMEncoder(FETCH_WAVLM, taps=(1, 2))
    lenc.load_state_dict(wr.state_dict(FETCH_WAVLM, seed=6050), strict=True)
    object.__setattr__(m, "whisper_encoder", wenc.cuda().prepare(torch.float32))
    object.__setattr__(m, "bestrq_encoder", BESTRQ_Model(model=mus, layers=(1, 2), dtype=torch.float32))
    object.__setattr__(m, "wavlm_encoder", lenc.cuda().prepare(torch.float32))
    return m


def test_fetch_codes_batch_with_all_three_encoders_and_no_callable():
    """Plumbing identity: the codes of fetch_codes_batch(ssl_features=None) are those of the same model with the encoder's own
    get_wavlm_feature output injected through ssl_features (the same device values on both routes: no near-tie can flip a code)."""
    import whisper_ref as whr
    from codec_model_stub import CFG
    B, T25, P = CFG["B"], CFG["T25"], 72
    m = _codec_with_encoders(P)
    mels = torch.stack([whr.encoder_mels(P, seed=7400 + i)[0] for i in range(B)]).cuda()
    audios = (0.1 * seeded_tensor((B, 1, T25 * 960), 8400, std=1.0)).cuda()
    masks = torch.zeros(3, B, dtype=torch.bool)
    m.ssl_features = None
    rc, mc, _ = m.fetch_codes_batch(audios, mels, film_masks=masks)
    feat = m.get_wavlm_feature(audios, T25)
    assert feat.shape == (B, 128, 2 * T25)                               # 28 800 samples at 24 kHz -> 19 360 at 16 kHz -> 60 frames
    m.ssl_features = lambda a, s: dict(wavlm=feat)
    rc2, mc2, _ = m.fetch_codes_batch(audios, mels, film_masks=masks)
    m.ssl_features = None
    assert mc[0].shape == (B, 15, 8) and torch.equal(rc[0], rc2[0]) and torch.equal(mc[0], mc2[0])


def test_tokenize_path_equals_audio2token(tmp_path):
    """tokenize(path) of a 16-bit wav written with scipy = audio2token of the loaded tensor: one 30-s segment through the three
    encoders (Whisper at its 1 500 positions, WavLM 480 160 samples -> 1 500 frames), no callable anywhere."""
    from scipy.io import wavfile
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.reason_tokenizer import ReasoningTokenizer, load_wav
    m = _codec_with_encoders(1500)
    m.ssl_features = None
    tok = ReasoningTokenizer(model=m, device="cuda")
    x = (0.2 * seeded_tensor((26000,), 78, std=1.0)).clamp(-1, 1)
    path = str(tmp_path / "x.wav")
    wavfile.write(path, 24000, (x * 32767).to(torch.int16).numpy())
    torch.manual_seed(5); torch.cuda.manual_seed(5)
    reason, rec = tok.tokenize(path)
    audio, fs = load_wav(path)
    assert fs == 24000
    torch.manual_seed(5); torch.cuda.manual_seed(5)
    reason2, rec2 = tok.audio2token(audio.cuda(), 24000)
    assert reason.shape[0] == 8 and rec.shape == (8, int(26000 / 24000 * 12.5) + 1)
    assert torch.equal(reason, reason2.squeeze(0)) and torch.equal(rec, rec2.squeeze(0))
