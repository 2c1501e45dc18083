"""The repetition penalty on the CPU: the numpy reference of tests/rep_penalty_ref.py against a torch restatement of the Hugging Face
RepetitionPenaltyLogitsProcessor rule, the float64 anchor case qualified by the reference alone, and the CLI's refusals — all before
any model is built."""
import argparse
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import rep_penalty_ref as rp
import sampler_refs as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hf_rule(scores, ids, theta):
    """transformers' RepetitionPenaltyLogitsProcessor.__call__ restated: scores [1, V] fp32, ids [1, n] long."""
    th = torch.tensor(theta, dtype=torch.float32)
    score = torch.gather(scores, 1, ids)
    score = torch.where(score < 0, score * th, score / th)
    return scores.scatter(1, ids, score)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _ring(ids, cap):
    h, n = np.full(cap, -9, dtype=np.int32), 0
    for t in ids:
        h, n = rp.append(h, n, t)
    return h, n


V0 = 40
SPECIAL = {0: 0.0, 1: -0.0, 2: float("-inf"), 3: 2.5, 4: -2.5, V0 - 1: -0.75, V0 - 2: 1e-38, V0 - 3: -3e38}
# (name, produced ids oldest first, ring capacity, window)
RING_CASES = [
    ("empty", [], 4, 4),
    ("one", [3], 4, 4),
    ("duplicates", [3, 3, 4, 3, 4], 8, 8),
    ("window-shorter-than-history", [5, 6, 0, 1, 2, V0 - 1], 8, 3),
    ("window-longer-than-history", [4, V0 - 1], 16, 16),
    ("ring-wrap", list(range(14)) + [V0 - 1, 3, 3], 4, 4),
    ("ring-wrap-window-1", [1, 2, 3, 4, 5, 0], 1, 1),
    ("cap-above-window-wrapped", [7, 8, 9, 0, 1, 2, 3, 4, V0 - 2, V0 - 3, 2], 6, 4),
    ("edges", [0, V0 - 1, 0, V0 - 1], 4, 4),
]


def _row():
    row = (np.random.default_rng(4).standard_normal(V0) * 2).astype(np.float32)
    for c, v in SPECIAL.items():
        row[c] = np.float32(v)
    return row


@pytest.mark.parametrize("theta", [1.3, 0.8, 1.0])
@pytest.mark.parametrize("name,ids,cap,W", RING_CASES, ids=[c[0] for c in RING_CASES])
def test_penalize_is_the_hugging_face_rule_over_the_window(name, ids, cap, W, theta):
    row = _row()
    keep = row.copy()
    hist, n = _ring(ids, cap)
    assert n == len(ids)
    win = rp.window_ids(hist, n, W)
    assert win.tolist() == ids[len(ids) - min(len(ids), W):]             # the ring holds the last cap ids, the window the last W of them
    got = rp.penalize(row, hist, n, W, theta)
    assert np.array_equal(_bits(row), _bits(keep))                        # the input row is only read
    want = torch.from_numpy(row.copy())[None]
    if win.size:
        want = _hf_rule(want, torch.from_numpy(win)[None], theta)
    assert np.array_equal(_bits(got), _bits(want[0].numpy())), name
    try:
        from transformers import RepetitionPenaltyLogitsProcessor
    except ImportError:
        RepetitionPenaltyLogitsProcessor = None
    if RepetitionPenaltyLogitsProcessor is not None and win.size:
        hf = RepetitionPenaltyLogitsProcessor(penalty=float(np.float32(theta)))(torch.from_numpy(win)[None], torch.from_numpy(row.copy())[None])
        assert np.array_equal(_bits(got), _bits(hf[0].numpy())), name
    S = set(win.tolist())
    for c in range(V0):
        if c not in S or theta == 1.0:
            assert _bits(got[c:c + 1])[0] == _bits(row[c:c + 1])[0], (name, c)
    if theta != 1.0 and {0, 1, 2} <= S:                                  # +0 and -0 take the divide and keep their sign; -inf stays
        assert _bits(got[0:1])[0] == 0 and _bits(got[1:2])[0] == np.int32(-2 ** 31) and got[2] == -np.inf


def test_penalty_is_applied_once_per_distinct_id_and_nan_stays():
    row = np.array([2.0, -2.0, np.nan, 1.0], dtype=np.float32)
    hist, n = _ring([0, 0, 0, 1, 1, 2], 8)
    got = rp.penalize(row, hist, n, 8, 2.0)
    assert got[0] == 1.0 and got[1] == -4.0 and np.isnan(got[2]) and got[3] == 1.0
    h2, n2 = rp.append(hist, n, 3)
    assert n2 == n + 1 and h2[n % 8] == 3 and hist[n % 8] == -9           # append copies
    out = rp.replay_loop([row, row, row], lambda f, l: int(np.nanargmax(l)), 2, 2.0)
    # frame 0: nothing penalised, 0 wins (2.0); frame 1: 0 -> 1.0 ties 3 (1.0), the lower column; frame 2: window (0, 0): 0 still halved
    assert [t for t, _, _ in out] == [0, 0, 0] and out[-1][2] == 3 and out[-1][1].tolist() == [0, 0]


def test_anchor_case_is_decided_by_the_reference_alone():
    """The conditions sampler_refs.CASES are held to (tests/test_sampler_refs_host.py): 0 rows outside the exact assertion and
    E_ref <= 1e-4 — on the penalised rows, so the GPU test asserts every id exactly."""
    raw, hist, length, L = rp.anchor_case()
    a = rp.ANCHOR
    assert L.logits.shape == (a["M"], a["V"]) == (64, 12296) and L.topk == 50 and L.T == 0.9 and a["theta"] == 1.3 and a["W"] == 16
    assert {0, 1, 15, 16, 50} <= set(length.tolist())                     # empty, shorter than, equal to and past the window (wrapped)
    moved = 0
    for m in range(a["M"]):
        win = rp.window_ids(hist[m], length[m], a["W"])
        top = set(np.argsort(raw[m])[-50:].tolist())
        assert set(win.tolist()) <= top                                   # histories from the row's own top 50 columns
        moved += int((_bits(raw[m]) != _bits(L.logits[m])).sum())
        assert int((_bits(raw[m]) != _bits(L.logits[m])).sum()) == len(set(win.tolist()))
    assert moved > 300
    R = sr.replay(L)
    print(R.line("rep-penalty-anchor"))
    assert int((~R.exact).sum()) == 0 and R.e_ref <= 1e-4, (int((~R.exact).sum()), R.e_ref)
    plain = sr.ids_of(sr.Launch(raw, L.topk, L.T, None, seed=L.seed, counter=L.counter, stream_id=L.stream_id))
    assert int((plain != R.ids).sum()) >= 5                               # the penalty changes ids: the case can tell it from no penalty


def test_cli_flags_defaults_and_refusals_before_any_model():
    from uniaudio2_amd import multi_task_inference as cli
    ns = cli.get_parser().parse_args(["--task", "TTS"])
    assert ns.repetition_penalty == 1.0 and ns.repetition_window == 64
    assert cli._check_repetition(ns, True) == (1.0, 64)
    assert cli._check_repetition(argparse.Namespace(), True) == (1.0, 64)          # callers that build their own namespace

    class G:
        repetition_penalty, repetition_window = 1.0, 64
    g = cli._apply_repetition(ns, G(), True)
    assert not vars(g)                                                    # the defaults set no generator attribute
    ns2 = cli.get_parser().parse_args(["--task", "TTS", "--repetition_penalty", "1.2", "--repetition_window", "32"])
    g = cli._apply_repetition(ns2, G(), True)
    assert (g.repetition_penalty, g.repetition_window) == (1.2, 32)
    bad = [(["--repetition_penalty", "0"], "--repetition_penalty"), (["--repetition_penalty", "-1"], "--repetition_penalty"),
           (["--repetition_penalty", "nan"], "--repetition_penalty"), (["--repetition_penalty", "inf"], "--repetition_penalty"),
           (["--repetition_window", "0"], "--repetition_window"), (["--repetition_window", "513"], "--repetition_window"),
           (["--repetition_penalty", "1.2", "--topk", "1"], "--topk 1")]
    for extra, word in bad:
        with pytest.raises(ValueError, match=word):                       # before any input check, config read or model
            cli.main(["--task", "TTS"] + extra)
        kw = vars(cli.get_parser().parse_args(["--task", "TTS"] + extra))
        with pytest.raises(ValueError, match=word):
            cli.run_generation_stage1(argparse.Namespace(**dict(kw, decode_type="greedy")))
    for extra, word in bad[:6]:                                           # the understanding tasks validate the values too
        with pytest.raises(ValueError, match=word):
            cli.main(["--task", "speech_s2t"] + extra)
        kw = vars(cli.get_parser().parse_args(["--task", "ASR"] + extra))
        with pytest.raises(ValueError, match=word):
            cli.run_understanding(argparse.Namespace(**kw))
    with pytest.raises(ValueError, match="--beam_width"):
        cli.main(["--task", "ASR", "--repetition_penalty", "1.2", "--beam_width", "4"])
    with pytest.raises(ValueError, match="--beam_width"):
        cli.run_understanding(argparse.Namespace(**vars(cli.get_parser().parse_args(["--task", "ASR", "--repetition_penalty", "1.2", "--beam_width", "4"]))))
    # --topk 1 with a penalty on a greedy understanding task is not an error: the task ignores both flags
    assert cli._check_repetition(argparse.Namespace(repetition_penalty=1.2, topk=1), False) == (1.2, 64)
    help_text = cli.get_parser().format_help()
    assert "not measured" in " ".join(help_text.split()) and "ignore it" in " ".join(help_text.split())


class _Model:
    def __init__(self): self.calls = []
    def set_sampling(self, topk, temperature, seed=None): self.calls.append(("sampling", topk, temperature))
    def set_repetition_penalty(self, penalty=1.0, window=64): self.calls.append(("rep", penalty, window))


def test_generator_tells_the_model_only_while_on_and_once_to_reset():
    from uniaudio2_amd.evaluation._generator import GeneratorBase
    assert GeneratorBase.repetition_penalty == 1.0 and GeneratorBase.repetition_window == 64
    gen = GeneratorBase.__new__(GeneratorBase)
    gen._model = _Model()
    gen._set_sampling(50, 0.9)
    assert gen._model.calls == [("sampling", 50, 0.9)]                    # defaults: nothing new is called
    gen.repetition_penalty, gen.repetition_window = 1.2, 32
    gen._set_sampling(50, 0.9)
    assert gen._model.calls[-1] == ("rep", 1.2, 32)
    gen.repetition_penalty = 1.0
    del gen._model.calls[:]
    gen._set_sampling(50, 0.9); gen._set_sampling(50, 0.9)
    assert gen._model.calls == [("sampling", 50, 0.9), ("rep", 1.0, 32), ("sampling", 50, 0.9)]   # reset once, then silence


def test_model_validates_and_remembers_without_a_plan():
    from uniaudio2_amd.llm_models.model_new import Model_stage3
    m = Model_stage3.__new__(Model_stage3)
    m._h = None
    for bad in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError, match="penalty"):
            Model_stage3.set_repetition_penalty(m, bad)
    for bad in (0, 513):
        with pytest.raises(ValueError, match="window"):
            Model_stage3.set_repetition_penalty(m, 1.2, bad)
    Model_stage3.set_repetition_penalty(m, 1.2, 32)
    assert m.repetition_penalty == (1.2, 32)                              # setup_caches re-applies it to the plan it builds
    assert {"rep_hist", "rep_len"} <= set(Model_stage3._ROW_STATE)


def test_new_symbols_are_declared_exported_and_bound():
    from uniaudio2_amd import _lib
    header = open(os.path.join(ROOT, "include", "ua2hip.h")).read()
    for name in ("ua2_sample_penalized", "ua2_stage3_set_rep_penalty"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.exported_symbols() and getattr(_lib.lib, name).restype is C.c_int
    assert _lib._EXPORTS["ua2_stage3_set_rep_penalty"][1] == [C.c_void_p, C.c_float, C.c_int32, C.c_void_p, C.c_void_p]
    # the struct of the binding is the struct of the header, field for field
    end = header.index("} ua2_sample_args;")
    body = header[header.rindex("typedef struct {", 0, end) + len("typedef struct {"):end]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"[\s\*]", "", part).split(" ")[-1] for part in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl).split(",")]
    assert names == [f[0] for f in _lib.SampleArgs._fields_], names
    assert _lib.lib.ua2_version() == 10
    assert "not measured" in " ".join(header.lower().split())
