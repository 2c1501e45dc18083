"""GPU side of the reasoning-conditioned decode (ReasoningTokenizer.detokenize / token2audio / detokenize_batch, the two-stream
AudioDiffusion1D.inference_codes, csrc/ua2_codec_join.hip) and of the 30-s window shape on the existing kernels.
Goldens: tests/golden/reason_decode.npz (the reference's own token2audio on stand-ins and its two-stream inference_codes at
toy size, tests/golden/make_golden_reason_decode.py); oracles: oracle/codec_model_oracle.py (DiT), oracle/codec_oracle.py
(ScalarModel)."""
import json
import os
import time

import numpy as np
import pytest
import torch

from codec_model_stub import CFG, StubEstimator, module_state_dict
from reason_decode_stub import INFER, infer_reason_inputs, make_reason_codes, reason_len
from weights import seeded_tensor

pytestmark = pytest.mark.gpu
HERE = os.path.join(os.path.dirname(__file__), "golden")
G = np.load(os.path.join(HERE, "reason_decode.npz"))


class _Table(torch.nn.Module):
    def __init__(self, t):
        super().__init__()
        self.t = t.cuda()

    def get_output_from_indices(self, idx):
        return sum(self.t[l][idx[..., l]] for l in range(idx.shape[-1]))


def _two_stream_toy_model():
    from test_gpu_codec_model import _gold, _toy_model
    _, meta = _gold()
    m, _ = _toy_model(meta, dit=True)
    i = infer_reason_inputs()
    rmeta = json.load(open(os.path.join(HERE, "reason_decode.json")))
    w = module_state_dict({k: tuple(s) for k, s in rmeta["keys"]}, 503)
    with torch.no_grad():
        for name in ("cond_feature_emb", "reason_adaptor"):
            getattr(m, name).weight.copy_(w[name + ".weight"]); getattr(m, name).bias.copy_(w[name + ".bias"])
        m.zero_cond_embedding1.copy_(i["zero_cond"])
    m.prepare()
    m.vq_pronunciation_semantic, m.vq_structure_semantic, m.vq_acoustic = _Table(i["tab_phone"]), _Table(i["tab_sem"]), _Table(i["tab_ac"])
    m.audio_thinking.reasoning_vq = _Table(i["tab_reason"])
    return m, i


@pytest.mark.parametrize("tag", ["infer2_first", "infer2_other"])
def test_two_stream_inference_codes_vs_reference_golden(tag):
    """codes = [reason (1, 8, 11), rec (1, 8, 25)]: reasoning_vq look-up, reason_adaptor, x2.5 nearest (27 rows) cropped to 25 and
    added to the look-up sum (ua2_reason_merge), then the one-stream path, against the reference's own inference_codes."""
    from test_gpu_codec_model import _close
    m, i = _two_stream_toy_model()
    est = StubEstimator("cuda")
    true_lat, n_inc = (i["first_latent"], 0) if tag == "infer2_first" else (i["true_latent"], i["incontext"])
    lat = m.inference_codes([i["reason"].cuda(), i["codes"].cuda()], None, true_lat.cuda(), i["latent_length"], n_inc, additional_feats=[],
                            guidance_scale=1.5, num_steps=CFG["steps"], scenario="other_seg", noise=i["noise"].cuda(),
                            estimator=lambda x, t: est(x, timestep=torch.full((2,), t, device="cuda")).sample, return_reasoning_text=False)
    _close(lat.cpu().numpy(), G[tag], 2e-4, tag)
    # the x2.5 table the merge used is F.interpolate's, as the reference host computed it
    src = m.reason_rows(INFER["T_q"], INFER["T"], 1, "cuda")
    np.testing.assert_array_equal(src.cpu().numpy(), G["up_11"][:INFER["T"]])
    # a reason stream too short for the rec window: the reference's feature_combine fails on the shapes; here a ValueError
    with pytest.raises(ValueError, match="reasoning codes"):
        m.inference_codes([i["reason"][:, :, :9].cuda(), i["codes"].cuda()], None, true_lat.cuda(), i["latent_length"], n_inc,
                          additional_feats=[], guidance_scale=1.5, num_steps=CFG["steps"], scenario="other_seg", noise=i["noise"].cuda(),
                          estimator=lambda x, t: est(x, timestep=torch.full((2,), t, device="cuda")).sample)
    with pytest.raises(NotImplementedError):
        m.inference_codes([i["reason"].cuda(), i["codes"].cuda()], None, true_lat.cuda(), i["latent_length"], n_inc, return_reasoning_text=True)


def test_reason_merge_equals_torch_in_and_out_of_place():
    from uniaudio2_amd import ops
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models._dense import nearest_indices
    g = torch.Generator().manual_seed(3)
    up = nearest_indices(150, 2.5, "cpu")[:375]
    np.testing.assert_array_equal(up.numpy(), G["up_150"][:375])
    for B in (1, 3):
        rec = torch.randn(B * 375, 768, generator=g).cuda()
        reason = torch.randn(B * 150, 768, generator=g).cuda()
        src = torch.cat([up + b * 150 for b in range(B)]).to(torch.int32).cuda()
        want = rec + reason[src.long()]
        got = ops.reason_merge(rec, reason, src)
        assert torch.equal(got, want)
        ops.reason_merge(rec, reason, src, out=rec)
        assert torch.equal(rec, want)
    with pytest.raises(ValueError):
        ops.reason_merge(rec, reason[:10], src)


@pytest.mark.parametrize("win,ovlp", [(480000, 120000), (720000, 180000)])
def test_crossfade_equals_host_crossfade_concat(win, ovlp):
    from uniaudio2_amd import ops
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.reason_tokenizer import crossfade_concat
    g = torch.Generator().manual_seed(win)
    hop = win - ovlp
    for n in range(1, 6):
        seg = (torch.rand(n, win + 960, generator=g) - 0.5)      # decoded windows may be longer than `win`: the extra is ignored
        full = (n - 1) * hop + win
        for target in (full, full - win // 3, (n - 1) * hop + ovlp // 2 + 1):
            want = crossfade_concat([seg[k:k + 1].clone() for k in range(n)], win, ovlp, target)
            got = ops.crossfade(seg.cuda(), win, ovlp, target).cpu()
            assert got.shape == (target,)
            assert torch.equal(got, want[0]), (n, target, float((got - want[0]).abs().max()))


@pytest.mark.parametrize("T", (376, 1200))
def test_token2audio_on_device_stand_ins_vs_reference_golden(T):
    """The host logic with device tensors: stand-ins on cuda:0, the windows joined by ua2_crossfade."""
    from test_reason_decode import check_t2a, product_t2a
    model, wave = product_t2a(T, "cuda")
    check_t2a(T, model, wave, exact=False)


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-3), (torch.bfloat16, 6e-2)])
def test_dit_forward_at_the_30s_window_vs_oracle(dtype, tol):
    """The DiT mirror at a 30-s window's length (B = 2 guided rows x 750 frames: 11 full 64-key pages + a 46-key tail) at toy
    width against the oracle, at the bars of test_dit_forward_vs_oracle."""
    from oracle.codec_model_oracle import dit_forward
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models.transformer_1d_flow import Transformer1DModel
    import dit_toy
    c = dit_toy.CFG
    m = Transformer1DModel(num_attention_heads=c["heads"], attention_head_dim=c["head_dim"], in_channels=c["in_channels"],
                           out_channels=c["out_channels"], num_layers=c["layers"])
    sd = dit_toy.state_dict(5)
    m.load_state_dict(sd)
    m = m.cuda().prepare(dtype)
    x = seeded_tensor((2, 750, c["in_channels"]), 29, std=1.0)
    ref = dit_forward(sd, x, torch.tensor([0.45, 0.45]), c["heads"], c["head_dim"]).numpy()
    got = m(x.cuda(), 0.45).cpu().numpy()
    assert got.shape == ref.shape
    err = np.sqrt(np.mean((got - ref) ** 2)) / max(1e-6, np.sqrt(np.mean(ref ** 2)))
    print(f"DiT {dtype} at 2 x 750: relative rms error {err:.3e}")
    assert err < tol, err


def test_scalar_decode_30s_window_vs_cpu_oracle_and_batched_equals_per_window():
    from test_gpu_codec import _bench_scalar_model, _rms
    m, o = _bench_scalar_model()
    lat = torch.tanh(seeded_tensor((3, 136, 750), 98, std=1.0))
    got = m.decode(lat[:1].cuda()).cpu().numpy()
    ref = o.decode(lat[:1]).numpy()
    assert got.shape == ref.shape == (1, 1, 720000)
    scale = max(1.0, float(np.sqrt(np.mean(ref ** 2))))
    print("30-s window decode: rms err %.3e (ref rms %.3e)" % (_rms(got, ref), np.sqrt(np.mean(ref ** 2))))
    assert _rms(got, ref) < 1e-4 * scale
    batched = m.decode(lat.cuda())
    for k in range(3):
        assert torch.equal(batched[k:k + 1], m.decode(lat[k:k + 1].cuda())), k


def _released_size_tokenizer():
    from test_gpu_codec import BENCH_SCALAR_CFG
    from make_golden_codec import codec_state_dict
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models.AudioDiffusion1D import AudioDiffusion1D
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models.scalar24k import ScalarModel
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.models.transformer_1d_flow import RELEASED_CONFIG
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.reason_tokenizer import ReasoningTokenizer
    torch.manual_seed(0)
    model = AudioDiffusion1D(unet_model_config_path=dict(RELEASED_CONFIG), encoder_depth=1, device="cuda")
    with torch.no_grad():
        for _, p_ in model.named_parameters():
            if p_.dim() > 1:
                p_.normal_(0, 0.02)
        for n_, b_ in model.named_buffers():
            if n_.endswith("_codebook.embed"):
                b_.normal_(0, 0.5)
    model = model.cuda().prepare()
    sq = ScalarModel(**BENCH_SCALAR_CFG)
    sq.load_state_dict(codec_state_dict({k: tuple(v.shape) for k, v in sq.state_dict().items()}, 77))
    return ReasoningTokenizer(sq_codec=sq.cuda().prepare(), model=model, device="cuda")


def test_detokenize_runs_at_the_released_dit_size():
    """detokenize(reason, rec) with the released DiT's shape (seeded weights), 2 Euler steps: one 30-s window (T = 375) and three
    (T = 700).  Times it (information)."""
    tok = _released_size_tokenizer()
    g = torch.Generator().manual_seed(8)
    for T in (375, 700):
        rec = torch.randint(0, 8192, (8, T), generator=g)
        reason = torch.randint(0, 4096, (8, reason_len(T)), generator=g)
        wav = tok.detokenize(reason, rec, steps=2)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        wav = tok.detokenize(reason, rec, steps=2)
        dt = time.perf_counter() - t0
        assert wav.shape == (1, int(T / 12.5 * 24000)) and wav.dtype == torch.float32 and wav.device.type == "cpu"
        assert torch.isfinite(wav).all() and wav.abs().max() > 0
        print(f"detokenize T = {T} ({T / 12.5:.1f} s, {len(tok.model.cfm_wrapper._graphs)} recorded solves), 2 Euler steps: {dt * 1e3:.1f} ms")


@pytest.mark.parametrize("max_batch", [1, 3])
def test_detokenize_batch_equals_the_detokenize_loop_under_the_invariant_contract(max_batch, monkeypatch):
    from test_gpu_codec_model import _stage2_tokenizer
    monkeypatch.setenv("UA2_GEMM_NO_KSPLIT", "1")
    L = 136
    dit = dict(num_attention_heads=4, attention_head_dim=64, in_channels=2 * L + 768, out_channels=L, num_layers=2)
    tok = _stage2_tokenizer(dit, sum_order=0)
    g = torch.Generator().manual_seed(13)
    Ts = (700, 100, 376, 375)
    rec = [torch.randint(0, 8192, (8, T), generator=g) for T in Ts]
    reason = [torch.randint(0, 4096, (8, reason_len(T)), generator=g) for T in Ts]
    torch.manual_seed(77)
    single = [tok.detokenize(q, c, steps=3) for q, c in zip(reason, rec)]
    torch.manual_seed(77)
    batch = tok.detokenize_batch(reason, rec, steps=3, max_batch=max_batch)
    for T, a, b in zip(Ts, single, batch):
        assert a.shape == b.shape == (1, int(T / 12.5 * 24000)) and torch.isfinite(a).all() and a.abs().max() > 0
        assert torch.equal(a, b), (T, float((a - b).abs().max()))
    # the reason stream conditions the result: another reason stream, same seed, another wave
    torch.manual_seed(77)
    other = tok.detokenize(torch.roll(reason[0], 1, -1), rec[0], steps=3)
    assert not torch.equal(other, single[0])
