"""Plain-torch restatement of the Whisper front end (log-mel + encoder) and the seeded inputs of its parity cases, shared by
tests/golden/make_golden_whisper.py (which runs the reference's own code against it), the host tests that pin it on the goldens,
the GPU tests and tools/ubench/whisper_frontend.py.  Our own code: nothing of the reference or of transformers is imported.

Both parts are written the way the device computes them, not the way the reference spells them — fp32 DFT as a matrix product
against a windowed basis, convolutions as products over gathered taps, hand-written LayerNorm / softmax / erf-GELU, the
1/sqrt(hd) on the scores instead of on q — so that the gap between this file and the reference on the golden cases is a
measurement of what fp32 re-ordering costs.  That gap is the yardstick of the GPU tests' tolerances (tests/test_gpu_whisper.py).
"""
import math
from collections import OrderedDict

import numpy as np
import torch

from weights import seeded_tensor

N_SAMPLES, N_FFT, HOP, N_BINS, N_MELS, N_FRAMES = 480000, 400, 160, 201, 80, 3000
# frames of the log-mel whose values the golden stores: the first 8, the last 8, every 37th
FRAME_SUBSET = sorted(set(range(8)) | set(range(N_FRAMES - 8, N_FRAMES)) | set(range(0, N_FRAMES, 37)))

TOY = dict(d_model=128, encoder_layers=2, encoder_attention_heads=2, encoder_ffn_dim=256, num_mel_bins=80)
ENCODER_CASES = OrderedDict(p72=72, p200=200)          # max_source_positions: one partial query tile + two KV pages; no multiple of 64 / 128
ENCODER_BATCH = 2


# ---- log-mel ---------------------------------------------------------------------------------------------------------
def clips():
    """The three log-mel cases, fp32 numpy at 16 kHz: (a) 480 160 samples of two chirps + noise with a silent stretch (the
    max - 8 clamp is active), (b) 16 000 samples (zero padding and the 1e-10 floor), (c) all zero."""
    g = torch.Generator().manual_seed(7001)
    n = N_SAMPLES + 160
    t = torch.arange(n, dtype=torch.float64) / 16000.0
    up = torch.sin(2 * math.pi * (200.0 * t + 0.5 * (3800.0 / 30.0) * t * t))            # 200 Hz -> 4 kHz over 30 s
    down = torch.sin(2 * math.pi * (7000.0 * t - 0.5 * (5000.0 / 30.0) * t * t))         # 7 kHz -> 2 kHz
    a = 0.4 * up + 0.2 * down + 0.02 * torch.randn(n, generator=g, dtype=torch.float64)
    a[16000 * 11:16000 * 14] = 0.0                                                       # 3 s of digital silence
    g = torch.Generator().manual_seed(7002)
    tb = torch.arange(16000, dtype=torch.float64) / 16000.0
    b = 0.3 * torch.sin(2 * math.pi * 440.0 * tb) + 0.05 * torch.randn(16000, generator=g, dtype=torch.float64)
    return OrderedDict(a=a.float().numpy(), b=b.float().numpy(), c=np.zeros(16000 * 5, dtype=np.float32))


def logmel_tables():
    """(basis [400, 402], mel_fb [201, 80]) float64: periodic Hann window folded into the cos | sin DFT basis, and the Slaney-scale,
    Slaney-normalised triangular filter bank of 80 filters over 0 .. 8 kHz on the 201 bins of a 400-point DFT at 16 kHz."""
    n = torch.arange(N_FFT, dtype=torch.float64)
    hann = 0.5 - 0.5 * torch.cos(2 * math.pi * n / N_FFT)
    k = torch.arange(N_BINS, dtype=torch.float64)
    ang = 2 * math.pi * ((n[:, None] * k[None, :]) % N_FFT) / N_FFT
    basis = torch.cat([hann[:, None] * torch.cos(ang), hann[:, None] * torch.sin(ang)], 1)
    step = math.log(6.4) / 27.0
    hz2mel = lambda f: 15.0 + math.log(f / 1000.0) / step if f >= 1000.0 else 3.0 * f / 200.0
    mel2hz = lambda m: 1000.0 * math.exp(step * (m - 15.0)) if m >= 15.0 else 200.0 * m / 3.0
    mels = np.linspace(hz2mel(0.0), hz2mel(8000.0), N_MELS + 2)
    edges = torch.tensor([mel2hz(float(m)) for m in mels], dtype=torch.float64)
    freqs = torch.linspace(0.0, 8000.0, N_BINS, dtype=torch.float64)
    fb = torch.zeros(N_BINS, N_MELS, dtype=torch.float64)
    for m in range(N_MELS):
        lo, c, hi = edges[m], edges[m + 1], edges[m + 2]
        tri = torch.minimum((freqs - lo) / (c - lo), (hi - freqs) / (hi - c)).clamp(min=0.0)
        fb[:, m] = tri * 2.0 / (hi - lo)
    return basis, fb


def logmel_ref(wav, dtype=torch.float32):
    """wav [B, N] -> log-mel [B, 80, 3000] in `dtype` arithmetic (fp32: the restatement the kernel is measured against)."""
    basis, fb = (t.to(dtype).to(wav.device) for t in logmel_tables())
    x = wav.to(dtype)[:, :N_SAMPLES]
    x = torch.nn.functional.pad(x, (0, N_SAMPLES - x.shape[1]))
    x = torch.cat([x[:, 1:N_FFT // 2 + 1].flip(1), x, x[:, -N_FFT // 2 - 1:-1].flip(1)], 1)           # reflect, center=True
    frames = x.unfold(1, N_FFT, HOP)[:, :N_FRAMES]                                                       # the last of the 3001 is dropped
    spec = frames @ basis
    power = spec[..., :N_BINS] ** 2 + spec[..., N_BINS:] ** 2
    logm = torch.log10((power @ fb).clamp(min=1e-10)).transpose(1, 2)
    logm = torch.maximum(logm, logm.amax(dim=(1, 2), keepdim=True) - 8.0)
    return (logm + 4.0) / 4.0


# ---- encoder ---------------------------------------------------------------------------------------------------------
def encoder_config(P):
    return dict(TOY, max_source_positions=P)


def encoder_shapes(cfg):
    """Ordered name -> shape of the reference WhisperEncoder's state dict."""
    d, f, s = cfg["d_model"], cfg["encoder_ffn_dim"], OrderedDict()
    s["conv1.weight"], s["conv1.bias"] = (d, cfg["num_mel_bins"], 3), (d,)
    s["conv2.weight"], s["conv2.bias"] = (d, d, 3), (d,)
    s["embed_positions.weight"] = (cfg["max_source_positions"], d)
    for l in range(cfg["encoder_layers"]):
        p = f"layers.{l}."
        s[p + "self_attn.k_proj.weight"] = (d, d)
        for n in ("v_proj", "q_proj", "out_proj"):
            s[p + f"self_attn.{n}.weight"], s[p + f"self_attn.{n}.bias"] = (d, d), (d,)
        s[p + "self_attn_layer_norm.weight"], s[p + "self_attn_layer_norm.bias"] = (d,), (d,)
        s[p + "fc1.weight"], s[p + "fc1.bias"] = (f, d), (f,)
        s[p + "fc2.weight"], s[p + "fc2.bias"] = (d, f), (d,)
        s[p + "final_layer_norm.weight"], s[p + "final_layer_norm.bias"] = (d,), (d,)
    s["layer_norm.weight"], s["layer_norm.bias"] = (d,), (d,)
    return s


def encoder_state_dict(cfg, seed=7100):
    """Seeded checkpoint: fan-in scaled matrices, LayerNorm gains around 1, small biases, a SEEDED positional table (the
    sinusoid of a real checkpoint is smooth: a shifted or transposed add would hardly show)."""
    out = OrderedDict()
    for i, (k, shp) in enumerate(encoder_shapes(cfg).items()):
        t = seeded_tensor(shp, seed * 7919 + i, std=1.0)
        if k.endswith("layer_norm.weight"):
            t = 1.0 + 0.1 * t
        elif k.endswith("bias"):
            t = 0.1 * t
        elif k == "embed_positions.weight":
            t = 0.5 * t
        else:
            t = t / math.prod(shp[1:]) ** 0.5
        out[k] = t
    return out


def encoder_mels(P, seed=7200):
    """[ENCODER_BATCH, 80, 2 P] seeded inputs in the log-mel's range, every row different."""
    return seeded_tensor((ENCODER_BATCH, TOY["num_mel_bins"], 2 * P), seed + P, std=0.6)


def _taps(rows_btc, stride):
    """[B, T, C] -> [B, Tout, 3 C]: frames stride t - 1 .. stride t + 1 (zero beyond both ends), taps outermost."""
    xp = torch.nn.functional.pad(rows_btc, (0, 0, 1, 1))
    return xp.unfold(1, 3, stride).permute(0, 1, 3, 2).reshape(rows_btc.shape[0], -1, 3 * rows_btc.shape[2])


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


def _ln(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    xc = x - mu
    return xc * torch.rsqrt((xc * xc).mean(-1, keepdim=True) + eps) * w + b


def encoder_ref(sd, cfg, mels, plain=False, rnd=None):
    """mels [B, 80, T] -> (last_hidden_state [B, P, d], stem output [B, P, d] after the positional add), P = (T - 1) // 2 + 1, computed
    in the dtype of `sd` / `mels`.  plain=True: the same network through torch's own fused ops (F.conv1d, F.layer_norm, F.gelu, SDPA) —
    the form a PyTorch user would write, for timing comparisons.  rnd (default off; not with plain): a rounding applied to both
    operands of every matrix product and to the cached k, v — kernel_refs.bf16_once makes this the model of the bf16 plan (bf16
    operands, wide accumulation, everything between the products left in the working dtype)."""
    F = torch.nn.functional
    heads, d = cfg["encoder_attention_heads"], cfg["d_model"]
    hd = d // heads
    B = mels.shape[0]
    assert not (plain and rnd is not None)
    r = rnd if rnd is not None else (lambda t: t)
    if plain:
        h = F.gelu(F.conv1d(mels, sd["conv1.weight"], sd["conv1.bias"], padding=1))
        h = F.gelu(F.conv1d(h, sd["conv2.weight"], sd["conv2.bias"], stride=2, padding=1)).permute(0, 2, 1)
    else:
        tm = lambda w: w.permute(0, 2, 1).reshape(w.shape[0], -1)
        h = _gelu(r(_taps(mels.transpose(1, 2), 1)) @ r(tm(sd["conv1.weight"])).t() + sd["conv1.bias"])
        h = _gelu(r(_taps(h, 2)) @ r(tm(sd["conv2.weight"])).t() + sd["conv2.bias"])
    h = h + sd["embed_positions.weight"]
    stem = h
    P = h.shape[1]
    for l in range(cfg["encoder_layers"]):
        p = f"layers.{l}."
        g = lambda n: sd[p + n]
        if plain:
            x = F.layer_norm(h, (d,), g("self_attn_layer_norm.weight"), g("self_attn_layer_norm.bias"))
        else:
            x = _ln(h, g("self_attn_layer_norm.weight"), g("self_attn_layer_norm.bias"))
        x = r(x)
        q = (x @ r(g("self_attn.q_proj.weight")).t() + g("self_attn.q_proj.bias")).view(B, P, heads, hd).transpose(1, 2)
        k = r((x @ r(g("self_attn.k_proj.weight")).t()).view(B, P, heads, hd).transpose(1, 2))
        v = r((x @ r(g("self_attn.v_proj.weight")).t() + g("self_attn.v_proj.bias")).view(B, P, heads, hd).transpose(1, 2))
        if plain:
            o = F.scaled_dot_product_attention(q, k, v)
        else:
            o = r(torch.softmax((r(q) @ k.transpose(-1, -2)) * (1.0 / math.sqrt(hd)), dim=-1)) @ v
        o = o.transpose(1, 2).reshape(B, P, d)
        h = h + (r(o) @ r(g("self_attn.out_proj.weight")).t() + g("self_attn.out_proj.bias"))
        if plain:
            x = F.gelu(F.linear(F.layer_norm(h, (d,), g("final_layer_norm.weight"), g("final_layer_norm.bias")), g("fc1.weight"), g("fc1.bias")))
        else:
            x = _gelu(r(_ln(h, g("final_layer_norm.weight"), g("final_layer_norm.bias"))) @ r(g("fc1.weight")).t() + g("fc1.bias"))
        h = h + (r(x) @ r(g("fc2.weight")).t() + g("fc2.bias"))
    if plain:
        return F.layer_norm(h, (d,), sd["layer_norm.weight"], sd["layer_norm.bias"]), stem
    return _ln(h, sd["layer_norm.weight"], sd["layer_norm.bias"]), stem
