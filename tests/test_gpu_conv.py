"""GPU parity of the conv kernel against the PyTorch fp32 ops the reference calls (F.conv1d /
F.conv_transpose1d on CPU), tolerance 2e-5 relative to the output scale (fp32, different summation order).

The anchor of the conv family is tests/test_gpu_conv_parity.py: every kernel of ua2_conv1d / ua2_conv1d_tc against float64
restatements (tests/conv_refs.py) under derived bars, with guard margins around every buffer.  The global tolerances here are
kept as they were; the bit-identity tests below (pipelined == plain) hang from that anchor."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _close(got, ref, tol=2e-5):
    scale = float(ref.abs().max()) + 1e-6
    err = float((got.cpu() - ref).abs().max())
    assert err <= tol * scale, f"max err {err:.3e} vs scale {scale:.3e}"


CONV_CASES = [
    # Cin, Cout, K, stride, dil, causal, T
    (1, 32, 7, 1, 1, True, 1000), (32, 32, 7, 1, 9, True, 777), (48, 48, 7, 1, 5, False, 300), (64, 64, 1, 1, 1, True, 130),
    (32, 64, 4, 2, 1, True, 1001), (136, 512, 7, 1, 1, False, 100), (64, 128, 10, 5, 1, True, 640), (1024, 768, 2, 2, 1, False, 64),
    (64, 128, 16, 8, 1, True, 803), (128, 64, 3, 1, 2, True, 97), (17, 19, 5, 1, 3, False, 70),
]


# fast = the bf16 x 3 form of the kernel (16-bit split operands on the bf16 MFMA, fp32 accumulate): ~2^-16 relative per
# product instead of exact fp32; tolerance 1e-4 of the output scale (measured 1e-5), the exact form keeps 2e-5
@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("Cin,Cout,K,stride,dil,causal,T", CONV_CASES)
def test_conv1d_matches_torch(Cin, Cout, K, stride, dil, causal, T, fast):
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import ACT_PRELU
    g = torch.Generator().manual_seed(Cin * 7 + K)
    x = torch.randn(2, Cin, T, generator=g)
    w = torch.randn(Cout, Cin, K, generator=g) / (Cin * K) ** 0.5
    b = torch.randn(Cout, generator=g)
    alpha = torch.tensor([0.2])
    if causal:                                   # scalar24k.py:70-74 (stride 1) / conv.py:239-243 (left pad k_eff - stride, extra right pad)
        pad_l = dil * (K - 1) - (stride - 1)
        n_frames = -(-(T - (dil * (K - 1) + 1) + pad_l) // stride) + 1
        extra = (n_frames - 1) * stride + (dil * (K - 1) + 1) - pad_l - T
        xp = F.pad(x, (pad_l, max(extra, 0)))
    else:                                        # scalar24k.py:17,47 symmetric
        pad_l = (K * dil - dil) // 2
        xp = F.pad(x, (pad_l, pad_l))
    ref = F.prelu(F.conv1d(xp, w, b, stride=stride, dilation=dil), alpha)
    res = torch.randn(ref.shape, generator=g)
    ref = ref + res
    wp, wlo = ops.pack_conv_weight_x3(w.cuda()) if fast else (ops.pack_conv_weight(w.cuda())[0], None)
    y = ops.conv1d(x.cuda(), wp, K, Cout, stride=stride, dilation=dil, pad_left=pad_l, Tout=ref.shape[-1], bias=b.cuda(),
                   post_act=ACT_PRELU, post_alpha=alpha.cuda(), residual=res.cuda(), w_lo=wlo)
    _close(y, ref, tol=1e-4 if fast else 2e-5)


@pytest.mark.parametrize("Cin,Cout,stride,K,causal,T", [(64, 32, 2, 4, True, 333), (128, 64, 5, 10, True, 64), (32, 32, 3, 6, True, 200),
                                                        (64, 64, 4, 8, False, 100), (512, 256, 8, 16, True, 25), (16, 16, 2, 2, False, 50)])
@pytest.mark.parametrize("fast", [False, True])
def test_conv_transpose1d_matches_torch(Cin, Cout, stride, K, causal, T, fast):
    from uniaudio2_amd import ops
    g = torch.Generator().manual_seed(Cin + stride)
    x = torch.randn(2, Cin, T, generator=g)
    w = torch.randn(Cin, Cout, K, generator=g) / (Cin * K / stride) ** 0.5
    b = torch.randn(Cout, generator=g)
    if causal:                                   # scalar24k.py:91-93,108-112: padding 0, drop the last `stride` samples
        ref = F.conv_transpose1d(x, w, b, stride=stride)[:, :, :-stride]
        trim = 0
    else:                                        # padding = (k - s) // 2
        trim = (K - stride) // 2
        ref = F.conv_transpose1d(x, w, b, stride=stride, padding=trim)
    rows, M = ops.convtr_phase_rows(w.cuda(), stride)
    wp, wlo = ops.pack_conv_weight_x3(rows) if fast else (ops.pack_convtr_weight(w.cuda(), stride)[0], None)
    y = ops.conv1d(x.cuda(), wp, M, Cout, pad_left=M - 1, Tout=ref.shape[-1], bias=b.cuda(), out_phases=stride, out_trim_left=trim, w_lo=wlo)
    _close(y, ref, tol=1e-4 if fast else 2e-5)


def test_conv1d_pre_activation_repeat_and_pool():
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import ACT_ELU, ACT_ROUND9, ACT_TANH
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 64, 150, generator=g)
    w = torch.randn(64, 64, 3, generator=g) / 14
    wp, _ = ops.pack_conv_weight(w.cuda())
    # SEANet resblock step: ELU -> conv(k=3, dilation 2), causal (seanet.py:92-94)
    ref = F.conv1d(F.pad(F.elu(x), (4, 0)), w, dilation=2)
    _close(ops.conv1d(x.cuda(), wp, 3, 64, dilation=2, pad_left=4, Tout=150, pre_act=ACT_ELU), ref)
    # PostProcessor: repeat each step twice, then conv (scalar24k.py:136-140); tanh epilogue (scalar24k.py:385)
    xr = x.transpose(1, 2).repeat(1, 1, 2).view(1, -1, 64).transpose(1, 2)
    ref = torch.tanh(F.conv1d(F.pad(xr, (2, 0)), w))
    _close(ops.conv1d(x.cuda(), wp, 3, 64, pad_left=2, Tout=300, in_repeat=2, post_act=ACT_TANH), ref)
    # decode entry: round(9x)/9 on the input (scalar24k.py:404)
    ref = F.conv1d(F.pad(torch.round(9 * x) / 9, (1, 1)), w)
    _close(ops.conv1d(x.cuda(), wp, 3, 64, pad_left=1, Tout=150, pre_act=ACT_ROUND9), ref)
    # the same three through the bf16 x 3 form
    wh, wl = ops.pack_conv_weight_x3(w.cuda())
    _close(ops.conv1d(x.cuda(), wh, 3, 64, pad_left=1, Tout=150, pre_act=ACT_ROUND9, w_lo=wl), ref, tol=1e-4)
    ref = torch.tanh(F.conv1d(F.pad(xr, (2, 0)), w))
    _close(ops.conv1d(x.cuda(), wh, 3, 64, pad_left=2, Tout=300, in_repeat=2, post_act=ACT_TANH, w_lo=wl), ref, tol=1e-4)
    ref = F.conv1d(F.pad(F.elu(x), (4, 0)), w, dilation=2)
    _close(ops.conv1d(x.cuda(), wh, 3, 64, dilation=2, pad_left=4, Tout=150, pre_act=ACT_ELU, w_lo=wl), ref, tol=1e-4)
    _close(ops.avgpool1d(x.cuda(), 2), F.avg_pool1d(x, 2), tol=1e-6)


def test_streaming_convs_match_whole_sequence_reference_self_test():
    """Port of the reference's own self-test (tools/tokenizer/MimiCodec/model/modules/streaming.py:306-358 `test()`):
    RawStreamingConv1d / RawStreamingConvTranspose1d fed chunk by chunk inside `streaming()` reproduce their
    whole-sequence outputs (relative L2 <= 1e-6) over the same grid of kernel sizes, strides, lengths and chunk sizes
    (the 1043-sample case only with the two larger chunk sizes, to bound the launch count)."""
    import itertools
    from uniaudio2_amd.tools.tokenizer.MimiCodec.model.modules.streaming import RawStreamingConv1d, RawStreamingConvTranspose1d
    torch.manual_seed(1234)
    device = "cuda"
    kernel_sizes = [1, 3, 4, 8, 15, 16]
    strides = [1, 2, 3, 4, 5, 6, 7, 8, 9]
    chin, chout = 6, 12
    checked = 0
    for kernel, stride in itertools.product(kernel_sizes, strides):
        if stride > kernel:
            continue
        conv = RawStreamingConv1d(chin, chout, kernel, stride).to(device)
        convtr = RawStreamingConvTranspose1d(chout, chin, kernel, stride).to(device)
        for length in [4, 8, 32, 54, 65, 128, 1043]:
            if length < kernel:
                continue
            batch_size = 3
            x = torch.randn(batch_size, chin, length).to(device)
            y = conv(x)
            z = convtr(y)
            # the whole-sequence results themselves against torch on the CPU, like every other reference of this file (on the GPU
            # these ~270 small shapes each went through MIOpen's kernel search: 13 s of the suite, and third-party native code
            # that has nothing to do with what is tested)
            yt = torch.nn.functional.conv1d(x.cpu(), conv.weight.detach().cpu(), conv.bias.detach().cpu(), stride=stride)
            zt = torch.nn.functional.conv_transpose1d(yt, convtr.weight.detach().cpu(), convtr.bias.detach().cpu(), stride=stride)
            assert (y.cpu() - yt).norm() / yt.norm() <= 1e-5 and (z.cpu() - zt).norm() / zt.norm() <= 1e-5
            for chunk_size in ([5, 8] if length > 200 else [1, 3, 5, 8]):
                ys, zs = [], []
                with conv.streaming(batch_size), convtr.streaming(batch_size):
                    for offset in range(0, length, chunk_size):
                        chunk = x[..., offset:offset + chunk_size]
                        ys.append(conv(chunk))
                        zs.append(convtr(ys[-1]))
                y_stream = torch.cat(ys, dim=-1)
                z_stream = torch.cat(zs, dim=-1)
                yy = y[..., :y_stream.shape[-1]]
                zz = z[..., :z_stream.shape[-1]]
                assert yy.shape == y_stream.shape, (yy.shape, y_stream.shape)
                assert (y_stream - yy).norm() / yy.norm() <= 1e-6
                assert int((length - kernel) / stride) + 1 == y_stream.shape[-1]
                assert zz.shape == z_stream.shape, (zz.shape, z_stream.shape)
                assert (z_stream - zz).norm() / zz.norm() <= 1e-6, (kernel, stride, length, chunk_size)
                checked += 1
            assert not conv.is_streaming and not convtr.is_streaming          # state dropped on exit
    assert checked > 500


def test_seanet_streaming_equals_whole_sequence():
    """The causal SEANet decoder / encoder run frame by frame under `streaming()` (how low-latency decoding uses them,
    SURVEY.md §8f rank 4) give the whole-sequence waveform / latent: conv.py:245-252 (left padding added once),
    :306-329 (no trims while streaming) on top of the state machines above."""
    from uniaudio2_amd.tools.tokenizer.MimiCodec.model.modules.seanet import SEANetDecoder, SEANetEncoder
    import json
    import os
    import sys
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    sys.path.insert(0, here)
    from make_golden_codec import SEANET_CFG, codec_state_dict
    meta = json.load(open(os.path.join(here, "codec_toy.json")))
    cfg = dict(SEANET_CFG)
    dec, enc = SEANetDecoder(**cfg), SEANetEncoder(**cfg)
    dec.load_state_dict(codec_state_dict({k: tuple(s) for k, s in meta["seanet_dec_keys"]}, 42))
    enc.load_state_dict(codec_state_dict({k: tuple(s) for k, s in meta["seanet_enc_keys"]}, 41))
    dec, enc = dec.cuda().eval(), enc.cuda().eval()
    hop = dec.hop_length
    z = torch.randn(2, cfg["dimension"], 12, device="cuda")
    whole = dec(z)
    outs = []
    with dec.streaming(2):
        for t in range(z.shape[-1]):
            outs.append(dec(z[..., t:t + 1]))
    stream = torch.cat(outs, dim=-1)
    assert stream.shape[-1] == z.shape[-1] * hop
    assert (stream - whole[..., :stream.shape[-1]]).norm() / whole.norm() <= 1e-5
    wav = torch.randn(2, 1, hop * 10, device="cuda")
    lat = enc(wav)
    outs = []
    with enc.streaming(2):
        for t in range(0, wav.shape[-1], hop):
            outs.append(enc(wav[..., t:t + hop]))
    lat_s = torch.cat(outs, dim=-1)
    assert lat_s.shape == lat.shape
    assert (lat_s - lat).norm() / lat.norm() <= 1e-5


@pytest.mark.parametrize("C,dil,T", [(32, 9, 1000), (64, 1, 333), (128, 5, 257), (32, 3, 70)])
def test_fused_residual_unit_matches_torch(C, dil, T):
    """The fused residual unit of the bf16 x 3 conv kernel (scalar24k.py:143-151): y = x + prelu2(W2 prelu1(conv1(x) + b1) + b2)
    in one launch, against the torch composition; and against the two-launch route through the same kernel (1e-4 of scale:
    the fused route rounds h to 16 bits through the same hi / lo split the unfused route applies when it re-stages h)."""
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import ACT_PRELU
    g = torch.Generator().manual_seed(C + dil)
    x = torch.randn(2, C, T, generator=g)
    w1 = torch.randn(C, C, 7, generator=g) / (7 * C) ** 0.5
    w2 = torch.randn(C, C, 1, generator=g) / C ** 0.5
    b1, b2 = torch.randn(C, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1
    a1, a2 = torch.tensor([0.2]), torch.tensor([0.3])
    h = F.prelu(F.conv1d(F.pad(x, (dil * 6, 0)), w1, b1, dilation=dil), a1)
    ref = F.prelu(F.conv1d(h, w2, b2), a2) + x
    w1h, w1l = ops.pack_conv_weight_x3(w1.cuda())
    w2h, w2l = ops.pack_conv_weight_x3(w2.cuda())
    xc = x.cuda()
    y = ops.conv1d(xc, w1h, 7, C, dilation=dil, pad_left=dil * 6, Tout=T, bias=b1.cuda(), post_act=ACT_PRELU, post_alpha=a1.cuda(),
                   residual=xc, w_lo=w1l, fused2=(w2h, w2l, b2.cuda(), a2.cuda()))
    _close(y, ref, tol=1e-4)
    hh = ops.conv1d(xc, w1h, 7, C, dilation=dil, pad_left=dil * 6, Tout=T, bias=b1.cuda(), post_act=ACT_PRELU, post_alpha=a1.cuda(), w_lo=w1l)
    y2 = ops.conv1d(hh, w2h, 1, C, Tout=T, bias=b2.cuda(), post_act=ACT_PRELU, post_alpha=a2.cuda(), residual=xc, w_lo=w2l)
    _close(y, y2.cpu(), tol=1e-5)


PIPE_CASES = [
    # Cin, Cout, K, dil, T, residual, fused, in_repeat: (K, channel-group run, position-group) instantiation families of the
    # pipelined kernel, windows that end inside a tile, ragged channel counts, one and many units per tile.  That EVERY arm of the
    # launcher is reached is proved elsewhere: tests/test_conv_refs_host.py::test_table_reaches_every_arm_of_the_launcher asks
    # ua2_debug_conv1d_plan which instantiation each case of tests/conv_refs.py takes (at B = 2 a fused 128-channel unit of
    # 700 steps, as below, runs the plain kernel on both sides: the 8-wave arm needs ntt = 4)
    (32, 32, 7, 9, 1000, True, True, 1), (64, 64, 7, 1, 4097, True, True, 1), (128, 128, 7, 5, 700, True, True, 1),
    (512, 512, 7, 3, 150, False, False, 1), (256, 256, 1, 1, 777, True, False, 1), (17, 19, 7, 3, 70, False, False, 1),
    (48, 40, 1, 1, 333, True, False, 1), (64, 32, 7, 1, 2049, False, False, 2), (1, 32, 7, 1, 5000, False, False, 1),
    (136, 512, 7, 1, 100, False, False, 1), (32, 32, 7, 7, 24000, True, True, 1), (128, 64, 2, 1, 513, False, False, 1),
    # several tiles per workgroup (tpw > 1) through the fused epilogue, 4- and 8-wave forms
    (64, 64, 7, 9, 120000, True, True, 1), (128, 128, 7, 9, 30000, True, True, 1), (32, 32, 7, 1, 240000, True, True, 1),
]


@pytest.mark.parametrize("Cin,Cout,K,dil,T,residual,fused,rep", PIPE_CASES)
def test_pipelined_conv_kernel_is_bit_identical_to_plain(Cin, Cout, K, dil, T, residual, fused, rep, monkeypatch):
    """conv1d_x3p_kernel (software-pipelined: x window one unit ahead in registers, weights refilled in place, hardware
    bf16 pack conversion) against conv1d_x3_kernel (UA2_CONV_PIPE=off): same split, same products, same summation order —
    torch.equal, not a tolerance."""
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import ACT_PRELU
    g = torch.Generator().manual_seed(Cin * 3 + K + dil)
    x = torch.randn(2 if T < 100000 else 1, Cin, T, generator=g).cuda()
    w = (torch.randn(Cout, Cin, K, generator=g) / (Cin * K) ** 0.5).cuda()
    hi, lo = ops.pack_conv_weight_x3(w)
    b = torch.randn(Cout, generator=g).cuda()
    a1, a0 = torch.tensor([0.2]).cuda(), torch.tensor([0.1]).cuda()
    Tout = T * rep
    pre = ACT_PRELU if (Cin + dil) % 2 else 0                       # both pre-activations of the split kernels (PReLU, none)
    kw = dict(dilation=dil, pad_left=dil * (K - 1), Tout=Tout, bias=b, pre_act=pre, pre_alpha=a0, post_act=ACT_PRELU, post_alpha=a1,
              w_lo=lo, in_repeat=rep)
    if fused:
        w2 = (torch.randn(Cout, Cout, 1, generator=g) / Cout ** 0.5).cuda()
        w2h, w2l = ops.pack_conv_weight_x3(w2)
        kw.update(residual=x, fused2=(w2h, w2l, torch.randn(Cout, generator=g).cuda(), torch.tensor([0.3]).cuda()))
    elif residual:
        kw.update(residual=torch.randn(x.shape[0], Cout, Tout, generator=g).cuda())
    monkeypatch.setenv("UA2_CONV_PIPE", "off")
    ref = ops.conv1d(x, hi, K, Cout, **kw)
    monkeypatch.delenv("UA2_CONV_PIPE")
    got = ops.conv1d(x, hi, K, Cout, **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(ref).all()
    assert torch.equal(got, ref), f"max diff {(got - ref).abs().max().item():.3e}"


def test_pipelined_conv_kernel_fuzz_bit_identical():
    """40 seeded random geometries through both bf16 x 3 kernels (UA2_CONV_PIPE=off vs default): channel counts that are not
    multiples of the 32-channel group, K in {1, 2, 7}, dilations, repeat-upsampled inputs, transposed-conv phase outputs with a
    left trim, batch 1-3, lengths that end inside a tile.  torch.equal on every case."""
    import os
    import random
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import ACT_PRELU
    rnd = random.Random(20260927)
    for case in range(40):
        K = rnd.choice([1, 2, 7, 7])
        Cin = rnd.choice([1, 17, 32, 48, 64, 96, 128, 136, 256])
        Cout = rnd.choice([16, 19, 32, 40, 64, 128, 200])
        dil = rnd.choice([1, 3, 5, 9]) if K == 7 else 1
        T = rnd.choice([37, 64, 333, 1000, 2049, 5000])
        B = rnd.choice([1, 2, 3])
        rep = rnd.choice([1, 1, 2]) if K != 2 else 1
        phases = rnd.choice([2, 4, 5]) if K == 2 else 1             # K = 2: the phase form of ConvTranspose1d(k = 2 s)
        g = torch.Generator().manual_seed(case)
        x = torch.randn(B, Cin, T, generator=g).cuda()
        rows = Cout * phases
        w = (torch.randn(rows, Cin, K, generator=g) / (Cin * K) ** 0.5).cuda()
        hi, lo = ops.pack_conv_weight_x3(w)
        trim = rnd.choice([0, 1]) if phases > 1 else 0
        Tout = T * rep * phases - trim * 2 if phases > 1 else T * rep
        kw = dict(dilation=dil, pad_left=dil * (K - 1), Tout=Tout, bias=torch.randn(Cout, generator=g).cuda(), w_lo=lo, in_repeat=rep,
                  out_phases=phases, out_trim_left=trim)
        if rnd.random() < 0.5:
            kw.update(pre_act=ACT_PRELU, pre_alpha=torch.tensor([0.1]).cuda())
        if rnd.random() < 0.5:
            kw.update(post_act=ACT_PRELU, post_alpha=(torch.rand(Cout, generator=g) if rnd.random() < 0.5 else torch.tensor([0.2])).cuda())
        if rnd.random() < 0.5:
            kw.update(residual=torch.randn(B, Cout, Tout, generator=g).cuda())
        os.environ["UA2_CONV_PIPE"] = "off"
        try:
            ref = ops.conv1d(x, hi, K, Cout, **kw)
        finally:
            os.environ.pop("UA2_CONV_PIPE", None)
        got = ops.conv1d(x, hi, K, Cout, **kw)
        torch.cuda.synchronize()
        assert torch.isfinite(ref).all(), case
        assert torch.equal(got, ref), (case, K, Cin, Cout, dil, T, B, rep, phases, trim, (got - ref).abs().max().item())
