"""Nucleus (top-p) sampling, host side: the numpy reference of the rule (tests/topp_ref.py) against masks recorded from the reference's
own sample_top_p (tests/golden/topp_mask.npz, written by tests/golden/make_golden_topp.py), the tie departure, the CLI flag, the
Generator's hand-over to the model, and the declared / exported symbols.  No GPU."""
import argparse
import ctypes as C
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import topp_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_topp_ref_reproduces_the_masks_of_the_reference():
    """The value rule (mass of strictly greater columns <= p) equals sample_top_p's sorted-prefix mask on tie-free rows — the float64
    part, the exact-integer part (through logits = log probs, T = 1) and the restated sort all give the recorded masks."""
    d = np.load(os.path.join(HERE, "golden", "topp_mask.npz"))
    probs, ps, mask = d["probs"], d["ps"], d["mask"]
    assert mask.shape == (probs.shape[0], ps.shape[0], probs.shape[1]) and mask.any(-1).all()
    sizes = set()
    for i, pr in enumerate(probs):
        assert np.unique(pr).shape[0] == pr.shape[0]                      # tie-free: the sort has nothing to split
        for j, p in enumerate(ps):
            want = mask[i, j]
            assert np.array_equal(topp_ref.kept_mask_probs(pr, p), want), (i, p)
            assert np.array_equal(topp_ref.sorted_prefix_mask(pr, p), want), (i, p)
            logits = np.log(pr.astype(np.float64))
            m64, margin = topp_ref.kept_mask_f64(logits, 1.0, 0, pr.shape[0], p)
            assert np.array_equal(m64, want) and margin > 5e-5, (i, p, margin)
            assert np.array_equal(topp_ref.kept_mask_int(logits, 1.0, 0, pr.shape[0], p), want), (i, p)
            sizes.add(int(want.sum()))
    assert min(sizes) == 1 and max(sizes) > 40                            # peaked rows and flat rows are both in the file


def test_ties_at_the_threshold_are_all_kept():
    """The stated departure from sample_top_p: [.4, .2, .2, .1, .1] under p = .5.  The second .2 has .4 of strictly greater mass,
    which is <= .5, so the value rule keeps both .2 columns (3 kept); the sorted prefix counts the first .2 against the second
    (.6 > .5) and keeps 2, and which of the two equal columns it drops is torch.sort's choice."""
    pr = [.4, .2, .2, .1, .1]
    assert topp_ref.kept_mask_probs(pr, .5).tolist() == [True, True, True, False, False]
    assert int(topp_ref.sorted_prefix_mask(pr, .5).sum()) == 2
    logits = np.log(np.asarray(pr))
    m64, _ = topp_ref.kept_mask_f64(logits, 1.0, 0, 5, .5)
    assert m64.tolist() == [True, True, True, False, False]
    assert topp_ref.kept_mask_int(logits, 1.0, 0, 5, .5).tolist() == [True, True, True, False, False]
    # the same rule inside a top-k set and behind a forbid prefix; p = 0 and p = 1 are off
    assert topp_ref.kept_mask_int(logits, 1.0, 1, 5, .5).tolist() == [False, True, True, False, False]
    assert topp_ref.kept_mask_int(logits, 1.0, 0, 2, .6).tolist() == [True, True, True, False, False]      # top-2 keeps the tie too (K's mass is .8)
    assert topp_ref.kept_mask_int(logits, 1.0, 0, 2, .4).tolist() == [True, False, False, False, False]
    for off in (0.0, 1.0):
        assert topp_ref.kept_mask_int(logits, 1.0, 0, 5, off).all() and topp_ref.kept_mask_f64(logits, 1.0, 0, 5, off)[0].all()
    flat = np.zeros(64)
    assert topp_ref.kept_mask_int(flat, 0.7, 0, 64, 0.5).all() and topp_ref.kept_mask_int(flat, 0.7, 0, 64, 1e-6).all()
    assert topp_ref.kept_mask_int(np.full(8, -np.inf), 1.0, 0, 8, 0.5).all()                                # Z == 0: no filter


def test_cli_flag_default_range_and_hand_over():
    from uniaudio2_amd import multi_task_inference as cli
    ns = cli.get_parser().parse_args(["--task", "TTS"])
    assert ns.top_p == 0.0 and cli._check_top_p(ns) == 0.0
    assert cli.get_parser().parse_args(["--task", "TTS", "--top_p", "0.9"]).top_p == 0.9

    class G:
        top_p = 0.0
    g = cli._apply_top_p(ns, G())
    assert "top_p" not in vars(g)                                         # the default touches nothing
    g = cli._apply_top_p(argparse.Namespace(top_p=0.9), G())
    assert g.top_p == 0.9
    assert cli._apply_top_p(argparse.Namespace(), G()).top_p == 0.0       # callers that build their own namespace
    for bad in ("-0.1", "1.5", "nan"):
        with pytest.raises(ValueError, match="--top_p"):                  # before any input check, config read or model
            cli.main(["--task", "TTS", "--top_p", bad])
        with pytest.raises(ValueError, match="--top_p"):
            cli.run_generation_stage1(argparse.Namespace(task="TTS", decode_type="greedy", top_p=float(bad)))
        with pytest.raises(ValueError, match="--top_p"):
            cli.run_understanding(argparse.Namespace(task="ASR", decode_type="greedy", top_p=float(bad)))


TA = types.SimpleNamespace(text_pad_token=128004, semantic_pad_token=9, semantic_eos=8193, semantic_bos=8192, reason_eos=4097,
                           reason_bos=4096, reason_pad_token=7, parallel_number=9, audio_reason_card=4100)


class _Model:
    """Stands in for Model_stage3 on CPU, as the existing generator tests' models do: set_sampling(topk, temperature, seed=None) and
    NO set_top_p."""

    def __init__(self, log):
        self.log, self.cursor, self.calls = log, 0, []
        self._p = torch.nn.Parameter(torch.zeros(1))

    def parameters(self): return iter([self._p])
    def setup_caches(self, b): self.batch = b
    def reset_caches(self): self.cursor = 0
    def forward_prefix(self, *a, **k): pass
    def begin_decode(self, *a, **k): pass
    def set_sampling(self, topk, temperature, seed=None): self.calls.append(("sampling", topk, temperature))

    def generate_frames(self, n, batch, mode, reason_eos=-1, reason_card=0, max_pos=None, skip_text_head=False, skip_audio_experts=False):
        out = self.log[self.cursor:self.cursor + n]
        self.cursor += n
        return out


class _ModelWithTopP(_Model):
    def set_top_p(self, top_p=0.0): self.calls.append(("top_p", top_p))


def _log():
    g = torch.Generator().manual_seed(5)
    frames = [torch.randint(0, 4096, (1, 8), generator=g, dtype=torch.int32) for _ in range(4)]
    frames.append(torch.full((1, 8), TA.reason_eos, dtype=torch.int32))
    frames += [torch.randint(4100, 12292, (1, 8), generator=g, dtype=torch.int32) for _ in range(5)]
    frames.append(torch.full((1, 8), TA.semantic_eos + TA.audio_reason_card, dtype=torch.int32))
    frames += [torch.zeros(1, 8, dtype=torch.int32)] * 24
    log = torch.zeros(len(frames), 1, 9, dtype=torch.int32)
    log[:, 0, 1:] = torch.cat(frames)
    return log


def test_generator_calls_set_top_p_only_while_it_is_on_and_once_to_reset():
    from uniaudio2_amd.evaluation.tts_task import Generator
    assert Generator.top_p == 0.0
    prompt, text = torch.tensor([128000, 1, 128001]), torch.tensor([128000, 2, 3, 128001])
    run = lambda gen: gen.generate_tts(prompt, "tts", text_token=text, topk=50, temperature=0.9)
    # a model without set_top_p runs unchanged at the default
    old = Generator(_Model(_log()), TA, text_tokenizer_path="ids")
    r0, s0 = run(old)
    assert old._model.calls == [("sampling", 50, 0.9)]
    gen = Generator(_ModelWithTopP(_log()), TA, text_tokenizer_path="ids")
    r1, s1 = run(gen)
    assert gen._model.calls == [("sampling", 50, 0.9)] and torch.equal(r0, r1) and torch.equal(s0, s1)
    gen.top_p = 0.9
    del gen._model.calls[:]
    run(gen)
    assert gen._model.calls == [("sampling", 50, 0.9), ("top_p", 0.9)]
    gen.top_p = 0.0
    del gen._model.calls[:]
    run(gen); run(gen)
    assert gen._model.calls == [("sampling", 50, 0.9), ("top_p", 0.0), ("sampling", 50, 0.9)]      # reset once, then silence
    old.top_p = 0.9
    with pytest.raises(AttributeError):                                   # asked for and missing: loud, never silently top-k
        run(old)


def test_model_set_top_p_validates_and_remembers_without_a_plan():
    from uniaudio2_amd.llm_models.model_new import Model_stage3
    m = Model_stage3.__new__(Model_stage3)
    m._h = None
    for bad in (-0.1, 1.5, math.nan):
        with pytest.raises(ValueError, match="top_p"):
            Model_stage3.set_top_p(m, bad)
    Model_stage3.set_top_p(m, 0.9)
    assert m.top_p == 0.9                                                 # setup_caches re-applies it to the plan it builds
    import inspect
    assert list(inspect.signature(Model_stage3.set_sampling).parameters) == ["self", "topk", "temperature", "seed"]


def test_new_symbols_are_declared_exported_and_bound():
    from uniaudio2_amd import _lib
    header = open(os.path.join(ROOT, "include", "ua2hip.h")).read()
    new = ("ua2_sample_topp", "ua2_sample_topp_rows", "ua2_stage3_set_top_p")
    for name in new:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.exported_symbols() and getattr(_lib.lib, name).restype is C.c_int
    # the two samplers take their top-k twins' arguments plus (float top_p, int32_t* keep_count) in front of the stream
    for name, twin in (("ua2_sample_topp", "ua2_sample_topk"), ("ua2_sample_topp_rows", "ua2_sample_topk_rows")):
        a, t = _lib._EXPORTS[name][1], _lib._EXPORTS[twin][1]
        assert a[:len(t) - 1] == t[:-1] and a[len(t) - 1:] == [C.c_float, C.c_void_p, C.c_void_p]
    assert _lib._EXPORTS["ua2_stage3_set_top_p"][1] == [C.c_void_p, C.c_float]
    assert _lib.lib.ua2_version() == 10
    assert topp_ref.MASS_BITS == 40 and "2^40" in header and topp_ref.P_BITS == 32 and "2^32" in header   # one scheme, two places
