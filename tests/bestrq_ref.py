"""Plain-torch restatement of the BEST-RQ (MusicFM 25 Hz) encoder — mel front end, 2-D convolution stem, conformer — and the seeded
inputs of its parity cases, shared by tests/golden/make_golden_bestrq.py (which runs the reference's own modules and transformers'
Wav2Vec2ConformerEncoder against it), the host tests that pin it on the goldens, the GPU tests and tools/ubench/bestrq_encoder.py.
Our own code: nothing of the reference or of transformers is imported.

The parts are written the way the device computes them, not the way the reference spells them — the DFT as a matrix product against a
windowed basis, BatchNorm folded into the convolutions' weights and biases, hand-written LayerNorm / softmax / swish, the rotary step
on the LayerNorm-ed rows in front of one [rot | plain] projection — so that the gap between this file and the reference on the golden
cases measures what fp32 re-ordering costs.  That gap is the yardstick of the GPU tests' tolerances (tests/test_gpu_bestrq.py).
torchaudio is not available where the goldens are made: the mel front end is measured against its own float64 evaluation instead.
"""
import math
from collections import OrderedDict

import numpy as np
import torch

from weights import seeded_tensor

SR, N_FFT, HOP, N_BINS, CUT = 24000, 2048, 240, 1025, 960
MEL_MEAN, MEL_STD = 6.768444971712967, 18.417922652295623

# The toy encoder is 64 wide with 2 heads (head size 32), not 32 wide with head size 16: ua2_attn is built for head sizes 32, 64 and 128,
# and 32 is the smallest at which the attention kernels (fp32 and the bf16 grouped form) run.
TOY = dict(n_mels=16, conv_dim=16, encoder_dim=64, encoder_depth=4, num_attention_heads=2, intermediate_size=128,
           conv_depthwise_kernel_size=31, rotary_embedding_base=10000, layer_norm_eps=1e-5)
TAPS = (1, 3)
# T25 (frames at 25 Hz): 12 is shorter than the 31-tap depthwise window; 37 is odd and crosses a 16-row tile
CASES = OrderedDict(t12=12, t37=37)
BATCH = 2
MEL_N_MELS = 128


# ---- mel front end -----------------------------------------------------------------------------------------------------
def clips():
    """Seeded 24-kHz clips, fp32 numpy: (a) 37 * 960 + 500 samples (the cut to a multiple of 960 drops 500) of two tones + noise with a
    stretch of digital silence longer than a frame, (b) 12 * 960 samples of noise + a tone, (z) all zero."""
    g = torch.Generator().manual_seed(8001)
    n = 37 * CUT + 500
    t = torch.arange(n, dtype=torch.float64) / SR
    a = 0.4 * torch.sin(2 * math.pi * 440.0 * t) + 0.2 * torch.sin(2 * math.pi * 5200.0 * t) + 0.05 * torch.randn(n, generator=g, dtype=torch.float64)
    a[9000:14000] = 0.0
    g = torch.Generator().manual_seed(8002)
    n = 12 * CUT
    t = torch.arange(n, dtype=torch.float64) / SR
    b = 0.3 * torch.sin(2 * math.pi * 1000.0 * t) + 0.1 * torch.randn(n, generator=g, dtype=torch.float64)
    return OrderedDict(a=a.float().numpy(), b=b.float().numpy(), z=np.zeros(12 * CUT, dtype=np.float32))


def mel_tables(n_mels):
    """(basis [2048, 2050], mel_fb [1025, n_mels]) float64: periodic Hann window folded into the cos | sin DFT basis; triangular HTK
    filters over 0 .. 12 kHz without normalisation (torchaudio melscale_fbanks(norm=None, mel_scale="htk"), restated)."""
    n = torch.arange(N_FFT, dtype=torch.float64)
    hann = 0.5 - 0.5 * torch.cos(2 * math.pi * n / N_FFT)
    k = torch.arange(N_BINS, dtype=torch.float64)
    ang = 2 * math.pi * ((n[:, None] * k[None, :]) % N_FFT) / N_FFT
    basis = torch.cat([hann[:, None] * torch.cos(ang), hann[:, None] * torch.sin(ang)], 1)
    hz2mel = lambda f: 2595.0 * math.log10(1.0 + f / 700.0)
    edges = torch.tensor([700.0 * (10.0 ** (m / 2595.0) - 1.0) for m in np.linspace(hz2mel(0.0), hz2mel(SR / 2), n_mels + 2)], dtype=torch.float64)
    freqs = torch.linspace(0.0, SR // 2, N_BINS, dtype=torch.float64)
    fb = torch.zeros(N_BINS, n_mels, dtype=torch.float64)
    for m in range(n_mels):
        lo, c, hi = edges[m], edges[m + 1], edges[m + 2]
        fb[:, m] = torch.minimum((freqs - lo) / (c - lo), (hi - freqs) / (hi - c)).clamp(min=0.0)
    return basis, fb


def mel_ref(wav, n_mels=128, dtype=torch.float32):
    """wav [B, N] -> normalised dB mel [B, n_mels, 4 (N // 960)] in `dtype` arithmetic: cut to a multiple of 960, center=True reflect
    padding, frames of 2048 at hop 240, power, mel bank, 10 log10(max(., 1e-10)), the last frame dropped, (x - mean) / std."""
    basis, fb = (t.to(dtype) for t in mel_tables(n_mels))
    n = wav.shape[1] // CUT * CUT
    x = wav.to(dtype)[:, :n]
    h = N_FFT // 2
    x = torch.cat([x[:, 1:h + 1].flip(1), x, x[:, -h - 1:-1].flip(1)], 1)
    frames = x.unfold(1, N_FFT, HOP)[:, :n // HOP]
    spec = frames @ basis
    power = spec[..., :N_BINS] ** 2 + spec[..., N_BINS:] ** 2
    db = 10.0 * torch.log10((power @ fb).clamp(min=1e-10)).transpose(1, 2)
    mean, std = torch.tensor(MEL_MEAN, dtype=dtype), torch.tensor(MEL_STD, dtype=dtype)
    return (db - mean) / std


# ---- weights -----------------------------------------------------------------------------------------------------------
def config(**kw):
    return dict(TOY, **kw)


def shapes(cfg, n_layers=None):
    """Ordered name -> shape of the used part of the reference MusicFM25Hz's state dict (`conv.*`, `conformer.layers.N.*`)."""
    c, d, f, k = cfg["conv_dim"], cfg["encoder_dim"], cfg["intermediate_size"], cfg["conv_depthwise_kernel_size"]
    s = OrderedDict()

    def bn(p, n):
        s[p + ".weight"], s[p + ".bias"], s[p + ".running_mean"], s[p + ".running_var"], s[p + ".num_batches_tracked"] = (n,), (n,), (n,), (n,), ()

    for blk, cin in ((0, 1), (1, c)):
        for i, ci in ((1, cin), (2, c), (3, cin)):
            p = f"conv.conv.{blk}."
            s[p + f"conv{i}.weight"], s[p + f"conv{i}.bias"] = (c, ci, 3, 3), (c,)
            bn(p + f"bn{i}", c)
    s["conv.linear.weight"], s["conv.linear.bias"] = (d, c * cfg["n_mels"] // 4), (d,)
    for l in range(n_layers if n_layers is not None else cfg["encoder_depth"]):
        p = f"conformer.layers.{l}."
        for n in ("ffn1_layer_norm",):
            s[p + n + ".weight"], s[p + n + ".bias"] = (d,), (d,)
        s[p + "ffn1.intermediate_dense.weight"], s[p + "ffn1.intermediate_dense.bias"] = (f, d), (f,)
        s[p + "ffn1.output_dense.weight"], s[p + "ffn1.output_dense.bias"] = (d, f), (d,)
        s[p + "self_attn_layer_norm.weight"], s[p + "self_attn_layer_norm.bias"] = (d,), (d,)
        for n in ("linear_q", "linear_k", "linear_v", "linear_out"):
            s[p + f"self_attn.{n}.weight"], s[p + f"self_attn.{n}.bias"] = (d, d), (d,)
        s[p + "conv_module.layer_norm.weight"], s[p + "conv_module.layer_norm.bias"] = (d,), (d,)
        s[p + "conv_module.pointwise_conv1.weight"] = (2 * d, d, 1)
        s[p + "conv_module.depthwise_conv.weight"] = (d, 1, k)
        bn(p + "conv_module.batch_norm", d)
        s[p + "conv_module.pointwise_conv2.weight"] = (d, d, 1)
        s[p + "ffn2_layer_norm.weight"], s[p + "ffn2_layer_norm.bias"] = (d,), (d,)
        s[p + "ffn2.intermediate_dense.weight"], s[p + "ffn2.intermediate_dense.bias"] = (f, d), (f,)
        s[p + "ffn2.output_dense.weight"], s[p + "ffn2.output_dense.bias"] = (d, f), (d,)
        s[p + "final_layer_norm.weight"], s[p + "final_layer_norm.bias"] = (d,), (d,)
    return s


def state_dict(cfg, seed=8100, n_layers=None):
    """Seeded checkpoint: fan-in scaled matrices, LayerNorm / BatchNorm gains around 1, small biases, BatchNorm running statistics
    away from (0, 1) — mean ~ N(0, 0.3), variance in [0.5, 1.5] — so that a wrong folding shows."""
    out = OrderedDict()
    for i, (k, shp) in enumerate(shapes(cfg, n_layers).items()):
        if k.endswith("num_batches_tracked"):
            out[k] = torch.tensor(100, dtype=torch.int64)
            continue
        t = seeded_tensor(shp, seed * 7919 + i, std=1.0)
        if k.endswith("running_var"):
            t = 0.5 + torch.sigmoid(t)
        elif k.endswith("running_mean"):
            t = 0.3 * t
        elif ("norm" in k or ".bn" in k) and k.endswith("weight"):
            t = 1.0 + 0.1 * t
        elif k.endswith("bias"):
            t = 0.1 * t
        else:
            t = t / math.prod(shp[1:]) ** 0.5
        out[k] = t
    return out


def stem_input(T25, cfg=TOY, seed=8200, batch=BATCH):
    """[batch, n_mels, 4 T25] seeded inputs in the normalised mel's range, every row different."""
    return seeded_tensor((batch, cfg["n_mels"], 4 * T25), seed + T25, std=1.0)


# ---- stem ---------------------------------------------------------------------------------------------------------------
def _fold(sd, p, i, eps=1e-5):
    g = sd[p + f"bn{i}.weight"] / torch.sqrt(sd[p + f"bn{i}.running_var"] + eps)
    return sd[p + f"conv{i}.weight"] * g.view(-1, 1, 1, 1), (sd[p + f"conv{i}.bias"] - sd[p + f"bn{i}.running_mean"]) * g + sd[p + f"bn{i}.bias"]


def stem_ref(sd, x):
    """x [B, n_mels, T] -> [B, T // 4, encoder_dim]: Conv2dSubsampling with the BatchNorm folding of the device path."""
    F = torch.nn.functional
    h = x.unsqueeze(1)
    for blk in (0, 1):
        p = f"conv.conv.{blk}."
        (w1, b1), (w2, b2), (w3, b3) = (_fold(sd, p, i) for i in (1, 2, 3))
        a = torch.relu(F.conv2d(h, w1, b1, stride=2, padding=1))
        h = torch.relu(F.conv2d(a, w2, b2, padding=1) + F.conv2d(h, w3, b3, stride=2, padding=1))
    B, C, Fo, To = h.shape
    rows = h.permute(0, 3, 1, 2).reshape(B, To, C * Fo)
    return rows @ sd["conv.linear.weight"].t() + sd["conv.linear.bias"]


# ---- conformer -------------------------------------------------------------------------------------------------------------
def _ln(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    xc = x - mu
    return xc * torch.rsqrt((xc * xc).mean(-1, keepdim=True) + eps) * w + b


def _swish(x):
    return x / (1.0 + torch.exp(-x))


def rotary_tables(P, hs, base):
    inv_freq = 1.0 / (base ** (torch.arange(0, hs, 2, dtype=torch.int64).float() / hs))
    emb = torch.cat([torch.arange(P).float()[:, None] * inv_freq[None, :]] * 2, -1)
    return emb.cos(), emb.sin()


def conformer_ref(sd, cfg, h, taps=TAPS):
    """h [B, P, d] (the stem's output) -> tuple of hidden_states[k] for k in taps (entry k = the input of layer k = the output of
    layer k - 1); layers past the last tap are not run."""
    d, heads, eps = cfg["encoder_dim"], cfg["num_attention_heads"], cfg["layer_norm_eps"]
    hs, k = d // heads, cfg["conv_depthwise_kernel_size"]
    B, P, _ = h.shape
    cos, sin = (t.to(h.dtype) for t in rotary_tables(P, hs, cfg["rotary_embedding_base"]))
    out = []
    for l in range(max(taps)):
        p = f"conformer.layers.{l}."
        g = lambda n: sd[p + n]
        ln = lambda x, n: _ln(x, g(n + ".weight"), g(n + ".bias"), eps)

        def ffn(x, n, norm):
            t = _swish(ln(x, norm) @ g(n + ".intermediate_dense.weight").t() + g(n + ".intermediate_dense.bias"))
            return x + (t @ (0.5 * g(n + ".output_dense.weight")).t() + 0.5 * g(n + ".output_dense.bias"))

        h = ffn(h, "ffn1", "ffn1_layer_norm")
        x = ln(h, "self_attn_layer_norm")
        xh = x.view(B, P, heads, hs)
        rot = (xh * cos[None, :, None, :] + torch.cat([-xh[..., hs // 2:], xh[..., :hs // 2]], -1) * sin[None, :, None, :]).reshape(B, P, d)
        q = (rot @ g("self_attn.linear_q.weight").t() + g("self_attn.linear_q.bias")).view(B, P, heads, hs).transpose(1, 2)
        kk = (rot @ g("self_attn.linear_k.weight").t() + g("self_attn.linear_k.bias")).view(B, P, heads, hs).transpose(1, 2)
        v = (x @ g("self_attn.linear_v.weight").t() + g("self_attn.linear_v.bias")).view(B, P, heads, hs).transpose(1, 2)
        o = (torch.softmax((q @ kk.transpose(-1, -2)) * (1.0 / math.sqrt(hs)), dim=-1) @ v).transpose(1, 2).reshape(B, P, d)
        h = h + (o @ g("self_attn.linear_out.weight").t() + g("self_attn.linear_out.bias"))
        x = ln(h, "conv_module.layer_norm") @ g("conv_module.pointwise_conv1.weight")[:, :, 0].t()
        x = x[..., :d] * torch.sigmoid(x[..., d:])
        gs = g("conv_module.batch_norm.weight") / torch.sqrt(g("conv_module.batch_norm.running_var") + 1e-5)
        dw = g("conv_module.depthwise_conv.weight") * gs.view(-1, 1, 1)
        db = g("conv_module.batch_norm.bias") - g("conv_module.batch_norm.running_mean") * gs
        x = _swish(torch.nn.functional.conv1d(x.transpose(1, 2), dw, db, padding=(k - 1) // 2, groups=d)).transpose(1, 2)
        h = h + x @ g("conv_module.pointwise_conv2.weight")[:, :, 0].t()
        h = ffn(h, "ffn2", "ffn2_layer_norm")
        h = ln(h, "final_layer_norm")
        if l + 1 in taps:
            out.append(h)
    return tuple(out)


def encoder_ref(sd, cfg, x, taps=TAPS):
    """x [B, n_mels, T] -> (stem output [B, T // 4, d], taps)."""
    stem = stem_ref(sd, x)
    return stem, conformer_ref(sd, cfg, stem, taps)
