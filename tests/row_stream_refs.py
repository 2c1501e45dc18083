"""Shared pieces of the row-stream / admission GPU tests: toy prompts of different lengths and the REFERENCE of every comparison —
a sequence's own B = 1 run through the existing one-sequence path (begin_ragged of one prompt, set_sampling(topk, T, seed), the
shared sampler stream), computed once per (dtype, prompt, mode, sampling) and shared between the test files."""
import torch

from helpers import build_product_model, load_golden_lm, toy_state_dict

T, TOPK = 0.9, 5
LENGTHS = [(3, 4), (5, 9), (2, 2), (6, 5), (4, 12), (7, 3)]      # (text frames, audio frames) of prompt b
REF_FRAMES = 14                                                  # frames of every reference run; tests compare prefixes
_models, _refs, _sd = {}, {}, []


def seed_of(b):
    return 0x5EED0000FFFFFFF0 + 977 * b                          # low word near 2^32, high word set: both halves matter


def prompt(b, mode, vt=500, va=110):
    """Prompt b for feedback `mode`: text frames then audio frames (modes 0 / 2 continue the audio), plus a two-frame text tail
    for the text loop (mode 1)."""
    n_text, n_audio = LENGTHS[b]
    g = torch.Generator().manual_seed(100 + b)
    L = n_text + n_audio + (2 if mode == 1 else 0)
    t = torch.zeros(L, 9, dtype=torch.long)
    m = torch.zeros(L, 9, dtype=torch.bool)
    t[:n_text, -1] = torch.randint(0, vt, (n_text,), generator=g); m[:n_text, -1] = True
    t[n_text:n_text + n_audio, :8] = torch.randint(0, va, (n_audio, 8), generator=g); m[n_text:n_text + n_audio, :8] = True
    if mode == 1:
        t[-2:, -1] = torch.randint(0, vt, (2,), generator=g); m[-2:, -1] = True
    return t.cuda(), m.cuda()


def state_dict():
    if not _sd:
        _sd.append(toy_state_dict(load_golden_lm()[1]))
    return _sd[0]


def model(dtype, **kw):
    """The tests' 6-sequence plan of `dtype` (one per process); keyword arguments build a fresh one."""
    if kw:
        return build_product_model(state_dict(), dtype, batch=6, **kw)
    if dtype not in _models:
        _models[dtype] = build_product_model(state_dict(), dtype, batch=6)
    return _models[dtype]


def sampling(m, topk, seed=1):
    """set_sampling with the draw index rewound whatever the cached key is."""
    m.set_sampling(topk, T if topk > 1 else 1.0, seed=seed)
    m._st["counters"][1:2].zero_()


def single(dtype, b, mode, topk, ngram=0):
    """(REF_FRAMES, 9) ids of prompt b decoded alone on the shared stream under seed_of(b): the existing path, row streams off."""
    key = (dtype, b, mode, topk, ngram)
    if key not in _refs:
        m = model(dtype)
        m.set_row_seeds(None)
        sampling(m, topk, seed_of(b))
        m.begin_ragged([prompt(b, mode)])
        if ngram:
            m.set_ngram(ngram, 499, capacity=64)
        _refs[key] = m.generate_frames(REF_FRAMES, 1, mode, skip_audio_experts=(mode == 1)).clone()[:, 0].cpu()
        m.set_ngram(0)
    return _refs[key]
