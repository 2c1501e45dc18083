"""Float64 references, seeded inputs and deliberately wrong models of the chain every audio-understanding request enters through:
`reason_tokenizer.resample` (24 kHz -> 16 kHz on every segment, a file's rate -> 24 kHz in `tokenize`), the Whisper log-mel
(ua2_logmel) and the WhisperEncoder mirror.  Shared by tests/test_frontend_refs_host.py (which pins the references on the CPU and
shows that every wrong model exceeds the bar of its case) and tests/test_gpu_frontend_parity.py (which holds the device to them
under kernel_refs.bar).  Our own code: nothing of the reference project, of torchaudio or of transformers is imported.

Resampler: two independent statements of torchaudio's published sinc_interp_hann algorithm.
  resample_ref     the polyphase form the product runs (filter bank [new/g, 2 width + orig/g], frames every orig/g samples of the
                   (width, width + orig/g) zero-padded signal), in `dt`.  The bank is built in float64 and rounded to fp32 ONCE:
                   that fp32 bank is the operand the product hands to ua2_linear, hence the contract.
  resample_direct  the interpolation itself, y[j] = sum_i x[i] h(j / new - i / orig), h(tau) = (c / orig) sinc(c tau) hann(c tau),
                   c = 0.99 min(orig, new), hann(t) = cos^2(pi t / 12) for |t| < 6 and 0 beyond — no frames, no padding, no phases, no
                   gcd, no fp32.  The two differ by the bank's fp32 rounding alone: |ref - direct| <= sum|x| max|h| 2^-24.
Log-mel: whisper_ref.logmel_ref is the reference; `logmel_variant` restates it with one switch per wrong model (all switches at their
defaults: the same bits), `logmel_clip` generates the edge clips.
Encoder: whisper_ref.encoder_ref (with its operand-rounding hook for the bf16 plan); the geometries are ENCODER_GEOMS below."""
import math
from collections import OrderedDict

import torch

import kernel_refs as kr
import whisper_ref as wr

F64, F32 = torch.float64, torch.float32
LPW, ROLLOFF = 6, 0.99                 # torchaudio.functional.resample's defaults, which the reference calls it with


# ---- resampler --------------------------------------------------------------------------------------------------------------

def resample_geometry(orig, new):
    """(width, o, n, base): o = orig / g, n = new / g, base = 0.99 min(o, n), width = ceil(6 o / base) input samples."""
    g = math.gcd(int(orig), int(new))
    o, n = int(orig) // g, int(new) // g
    base = min(o, n) * ROLLOFF
    return math.ceil(LPW * o / base), o, n, base


def lowpass(t):
    """sinc(t) * cos^2(pi t / 12) on |t| < 6, zero beyond (t in zero crossings of the sinc), float64."""
    t = t.to(F64)
    inside = t.abs() < LPW
    tc = torch.where(inside, t, torch.zeros_like(t))
    x = tc * math.pi
    sinc = torch.where(x == 0, torch.ones_like(x), torch.sin(x) / torch.where(x == 0, torch.ones_like(x), x))
    return torch.where(inside, sinc * torch.cos(x / (2 * LPW)) ** 2, torch.zeros_like(t))


def resample_bank(orig, new):
    """fp32 filter bank [n, 2 width + o]: phase p, tap k = (base / o) lowpass(base ((k - width) / o - p / n)), evaluated in float64 on
    exact integer numerators, then rounded once."""
    width, o, n, base = resample_geometry(orig, new)
    k = torch.arange(-width, width + o, dtype=torch.int64)[None, :]
    p = torch.arange(n, dtype=torch.int64)[:, None]
    t = (k * n - p * o).to(F64) * (base / (o * n))
    return (lowpass(t) * (base / o)).to(F32)


def resample_ref(wav, orig, new, dt=F64, delay=0, reverse_phases=False, pad_swapped=False):
    """wav [C, L] -> [C, ceil(new L / orig)] in `dt` arithmetic.  The keyword switches build the wrong models of the host tests:
    delay = d delays the input by d samples, reverse_phases emits the phases of a frame in reversed order, pad_swapped pads
    (width + o, width) instead of (width, width + o)."""
    if int(orig) == int(new):
        return wav
    width, o, n, _ = resample_geometry(orig, new)
    bank = resample_bank(orig, new).to(dt)
    if reverse_phases:
        bank = bank.flip(0)
    C, L = wav.shape
    x = wav.to(dt)
    if delay:
        x = torch.nn.functional.pad(x, (delay, 0))[:, :L]
    x = torch.nn.functional.pad(x, (width + o, width) if pad_swapped else (width, width + o))
    frames = x.unfold(1, bank.shape[1], o)                               # [C, F, taps]
    y = frames @ bank.t()                                                # [C, F, n]
    return y.reshape(C, -1)[:, :resample_len(L, orig, new)]


def resample_len(L, orig, new):
    _, o, n, _ = resample_geometry(orig, new)
    return -(-n * L // o)


def resample_direct(wav, orig, new, rows=512):
    """y[j] = sum_i x[i] h(j / new - i / orig) as a plain double sum over every input sample, float64 throughout.
    j / new - i / orig = (j orig - i new) / (orig new) with an exact integer numerator."""
    orig, new = int(orig), int(new)
    C, L = wav.shape
    x = wav.to(F64)
    c = ROLLOFF * min(orig, new)
    nout = -(-new * L // orig)
    i = torch.arange(L, dtype=torch.int64)[None, :]
    out = torch.empty(C, nout, dtype=F64)
    for j0 in range(0, nout, rows):
        j = torch.arange(j0, min(j0 + rows, nout), dtype=torch.int64)[:, None]
        h = lowpass((j * orig - i * new).to(F64) * (c / (orig * new))) * (c / orig)      # [rows, L]
        out[:, j0:j0 + rows] = x @ h.t()
    return out


def resample_direct_bound(wav, orig, new):
    """The bank's fp32 rounding: sum|x| max|h| 2^-24 (max|h| = c / orig, at tau = 0), plus float64's own slack on the two sums."""
    c = ROLLOFF * min(int(orig), int(new))
    s = float(wav.to(F64).abs().sum(-1).max())
    return s * (c / int(orig)) * (2.0 ** -24 + 64 * 2.0 ** -52)


RESAMPLE_PAIRS = [(24000, 16000), (16000, 24000), (48000, 24000), (8000, 24000), (32000, 24000), (44100, 24000), (22050, 24000)]


def segment_len():
    """Samples of one segment of a 30-s request (reason_tokenizer.segment_plan(...)["segment"]): what 24 -> 16 kHz runs on."""
    from uniaudio2_amd.tools.tokenizer.ReasoningCodec_film.reason_tokenizer import segment_plan
    return segment_plan(30 * 24000)["segment"]


def resample_cases():
    """name -> (orig, new, L).  24 -> 16 kHz: L / 3 + 1 GEMM rows, so L = 45, 48, 381, 384 are 16, 17, 128 and 129 rows."""
    cases = OrderedDict()
    for L in (1, 2, 3, 45, 48, 381, 384, 26000):
        cases[f"24k-16k L{L}"] = (24000, 16000, L)
    cases["24k-16k segment"] = (24000, 16000, None)                       # resolved by segment_len() where the package is importable
    cases["16k-24k L48001"] = (16000, 24000, 48001)
    cases["48k-24k L96001"] = (48000, 24000, 96001)
    cases["8k-24k L8001"] = (8000, 24000, 8001)                           # 15 taps padded to 16: the zero tap
    cases["32k-24k L32003"] = (32000, 24000, 32003)
    cases["44.1k-24k L44101"] = (44100, 24000, 44101)
    cases["22.05k-24k L86848"] = (22050, 24000, 86848)
    return cases


def resample_inputs(L, seed):
    """name -> [1, L] fp32: seeded noise at 0.3, an un-normalised clip (int16-range samples, amplitude 3e4), single impulses at
    sample 0 and at sample L - 1 (one per padding)."""
    g = torch.Generator().manual_seed(seed)
    noise = 0.3 * torch.randn(1, L, generator=g)
    loud = (3e4 * torch.rand(1, L, generator=g) * torch.where(torch.rand(1, L, generator=g) < 0.5, -1.0, 1.0)).round()
    first, last = torch.zeros(1, L), torch.zeros(1, L)
    first[0, 0], last[0, L - 1] = 1.0, 1.0
    return OrderedDict(noise=noise, loud=loud, impulse_first=first, impulse_last=last)


def prefix_outputs(L1, orig, new):
    """Number of leading outputs whose taps lie inside the first L1 input samples: frame f reads samples f o - width ..
    f o + width + o - 1, so every phase of the frames f <= (L1 - width - o) / o."""
    width, o, n, _ = resample_geometry(orig, new)
    return max(0, (L1 - width - o) // o + 1) * n


# ---- log-mel ----------------------------------------------------------------------------------------------------------------

def logmel_variant(wav, dtype=F64, hann="periodic", pad="reflect", max_over="clip", floor=True, keep="first"):
    """whisper_ref.logmel_ref with one switch per wrong model: hann "symmetric" (window of period 399), pad "replicate" (the edge
    sample repeated instead of the reflection), max_over "batch" (one clamp for the whole batch), floor False (no 1e-10 floor),
    keep "last" (frames 1 .. 3000 instead of 0 .. 2999).  With the defaults it is logmel_ref bit for bit."""
    basis, fb = wr.logmel_tables()
    if hann == "symmetric":
        n = torch.arange(wr.N_FFT, dtype=F64)
        per = 0.5 - 0.5 * torch.cos(2 * math.pi * n / wr.N_FFT)
        sym = 0.5 - 0.5 * torch.cos(2 * math.pi * n / (wr.N_FFT - 1))
        basis = basis * (sym / per.clamp(min=1e-300))[:, None]            # row 0 is 0 for both windows
    basis, fb = basis.to(dtype), fb.to(dtype)
    x = wav.to(dtype)[:, :wr.N_SAMPLES]
    x = torch.nn.functional.pad(x, (0, wr.N_SAMPLES - x.shape[1]))
    half = wr.N_FFT // 2
    if pad == "reflect":
        x = torch.cat([x[:, 1:half + 1].flip(1), x, x[:, -half - 1:-1].flip(1)], 1)
    else:
        x = torch.cat([x[:, :1].expand(-1, half), x, x[:, -1:].expand(-1, half)], 1)
    frames = x.unfold(1, wr.N_FFT, wr.HOP)
    frames = frames[:, :wr.N_FRAMES] if keep == "first" else frames[:, 1:wr.N_FRAMES + 1]
    spec = frames @ basis
    power = spec[..., :wr.N_BINS] ** 2 + spec[..., wr.N_BINS:] ** 2
    mel = power @ fb
    if floor:
        mel = mel.clamp(min=1e-10)
    logm = torch.log10(mel).transpose(1, 2)
    top = logm.amax() if max_over == "batch" else logm.amax(dim=(1, 2), keepdim=True)
    logm = torch.maximum(logm, top - 8.0)
    return (logm + 4.0) / 4.0


LOGMEL_WRONG = OrderedDict(symmetric_hann=dict(hann="symmetric"), edge_replicate=dict(pad="replicate"), batch_max=dict(max_over="batch"),
                           no_floor=dict(floor=False), last_frames=dict(keep="last"))

# lengths: below / at / just past the 200-sample reflection; the second workgroup's 2800-sample span begins at sample 2360; 16 040
# puts the end of the signal inside a frame and inside a workgroup; the truncation point 480 000 and its neighbours
LOGMEL_LENGTHS = [1, 150, 200, 201, 2359, 2360, 2361, 16040, 479999, 480000, 480001, 480160]
LOGMEL_MAX_E_REF = 1e-4        # an input only counts if the fp32 replay stays within this of float64 (clip a: 4.4e-5)
LOGMEL_CASES = ["a", "b", "c"] + [f"n{n}" for n in LOGMEL_LENGTHS] + ["quiet_click", "dc", "loud", "floor"]


def _tone_noise(n, seed, amp=0.25, noise=0.05, f=523.0):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=F64) / 16000.0
    return amp * torch.sin(2 * math.pi * f * t + 0.3) + noise * torch.randn(n, generator=g, dtype=F64)


_CLIPS = {}


def logmel_clip(case):
    """fp32 numpy clip at 16 kHz of a LOGMEL_CASES name (seeded noise plus a tone unless the name says otherwise)."""
    if case in _CLIPS:
        return _CLIPS[case]
    if case in ("a", "b", "c"):
        for k, v in wr.clips().items():
            _CLIPS[k] = v
        return _CLIPS[case]
    seed = 7500 + LOGMEL_CASES.index(case)
    if case.startswith("n"):
        x = _tone_noise(int(case[1:]), seed)
    elif case == "quiet_click":              # the clamp max - 8 is active almost everywhere, and the maximum lives in one workgroup
        x = _tone_noise(100003, seed, amp=1e-5, noise=2e-6)
        x[61234] = 1.0
    elif case == "dc":                       # DC 0.5 plus noise 1e-2: with noise 1e-3 the fp32 replay itself is off by 2.5e-4 .. 4.2e-4 (the
        x = 0.5 + _tone_noise(16001, seed, amp=0.0, noise=1e-2)       # window's DC leakage against near-empty bins), beyond LOGMEL_MAX_E_REF
    elif case == "loud":
        x = _tone_noise(70001, seed, amp=2.5e4, noise=5e3)
    elif case == "floor":                    # every mel power below the 1e-10 floor
        x = _tone_noise(30001, seed, amp=1e-7, noise=2e-8)
    else:
        raise KeyError(case)
    _CLIPS[case] = x.float().numpy()
    return _CLIPS[case]


def logmel_batch():
    """[3, 480 160] fp32: different content per row, every row longer than the truncation point (the clip stride past it), maxima
    three decades apart (a clamp taken over the batch would flatten the quiet rows)."""
    n = wr.N_SAMPLES + 160
    rows = [_tone_noise(n, 7601, amp=0.3, noise=0.1, f=440.0), _tone_noise(n, 7602, amp=3e-3, noise=3e-6, f=1234.0),
            _tone_noise(n, 7603, amp=1e-5, noise=1e-9, f=3210.0)]
    return torch.stack(rows).float()


_REFS = {}


def logmel_refs(case):
    """(ref float64 [80, 3000], E_max, E_rms, scale) of a case, computed once: E = error of logmel_ref in fp32 on the same clip."""
    if case not in _REFS:
        x = torch.from_numpy(logmel_clip(case))[None]
        _REFS[case] = logmel_stats(x)
    r = _REFS[case]
    return r[0][0], r[1][0], r[2][0], r[3][0]


def logmel_stats(x):
    """x [B, N] fp32 -> (ref float64 [B, 80, 3000], per-row E_max, E_rms of the fp32 replay, per-row scale max(1, max|ref|))."""
    ref = wr.logmel_ref(x, dtype=F64)
    d = wr.logmel_ref(x, dtype=F32).to(F64) - ref
    return ref, d.abs().amax(dim=(1, 2)).tolist(), d.pow(2).mean(dim=(1, 2)).sqrt().tolist(), ref.abs().amax(dim=(1, 2)).clamp(min=1.0).tolist()


def max_rms(y, ref):
    """(max |y - ref|, rms of y - ref) of a device or host result against a float64 reference; inf if y is not finite."""
    y = y.detach().cpu().to(F64)
    if not bool(torch.isfinite(y).all()):
        return float("inf"), float("inf")
    d = y - ref
    return float(d.abs().max()), float(d.pow(2).mean().sqrt())


# ---- encoder ----------------------------------------------------------------------------------------------------------------

def _geom(d, heads, ffn, layers, P, T, B, seed):
    return dict(cfg=dict(d_model=d, encoder_layers=layers, encoder_attention_heads=heads, encoder_ffn_dim=ffn, num_mel_bins=80,
                         max_source_positions=P), T=T, B=B, seed=seed)


ENCODER_GEOMS = OrderedDict(
    oddT=_geom(192, 3, 320, 2, 75, 149, 3, 7700),          # odd T: the last stride-2 tap of conv2 reads the right zero pad
    p1500=_geom(128, 2, 256, 1, 1500, 3000, 1, 7701),       # the released number of positions
    p72=dict(cfg=wr.encoder_config(72), T=144, B=wr.ENCODER_BATCH, seed=None),
    p200=dict(cfg=wr.encoder_config(200), T=400, B=wr.ENCODER_BATCH, seed=None))


def encoder_inputs(name):
    """(cfg, state dict fp32, mels [B, 80, T] fp32) of a geometry; p72 / p200 are the golden cases' own seeds."""
    g = ENCODER_GEOMS[name]
    if g["seed"] is None:
        return g["cfg"], wr.encoder_state_dict(g["cfg"]), wr.encoder_mels(g["cfg"]["max_source_positions"])
    from weights import seeded_tensor
    return g["cfg"], wr.encoder_state_dict(g["cfg"], seed=g["seed"]), seeded_tensor((g["B"], 80, g["T"]), g["seed"] + 50, std=0.6)


_ENC = {}


def encoder_refs(name):
    """Computed once per geometry: dict(last, stem: float64 references [B, P, d]; e32_last, e32_stem: max error of encoder_ref in
    fp32; em_last, em_stem: max error of the float64 replay whose GEMM operands and cached k, v are rounded to bf16)."""
    if name not in _ENC:
        cfg, sd, mels = encoder_inputs(name)
        sd64 = {k: v.double() for k, v in sd.items()}
        last, stem = wr.encoder_ref(sd64, cfg, mels.double())
        l32, s32 = wr.encoder_ref(sd, cfg, mels)
        lm, sm = wr.encoder_ref(sd64, cfg, mels.double(), rnd=kr.bf16_once)
        err = lambda a, b: float((a.to(F64) - b).abs().max())
        _ENC[name] = dict(last=last, stem=stem, e32_last=err(l32, last), e32_stem=err(s32, stem), em_last=err(lm, last), em_stem=err(sm, stem))
    return _ENC[name]
