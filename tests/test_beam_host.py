"""Beam search without a GPU: the rule of tests/beam_ref.py against an example worked by hand, the Generator's signature against the
reference's (evaluation/asr_task.py:438-450), the CLI's routing of --beam_width through the real Generator classes on a scripted
model, every refused combination, and the backtracking of a step log."""
import inspect
import math
import types

import numpy as np
import pytest
import torch

import beam_ref
from beam_ref import DEAD, FINISHED, LIVE, Slot

TA = types.SimpleNamespace(text_pad_token=128004, semantic_pad_token=9, semantic_eos=8193, semantic_bos=8192,
                           reason_eos=4097, reason_bos=4096, reason_pad_token=7, parallel_number=9,
                           audio_reason_card=4100)
ln = math.log


def _rows(*probs):
    with np.errstate(divide="ignore"):
        return np.log(np.array(probs, dtype=np.float64))


def test_rule_on_an_example_worked_by_hand():
    """W = 2, five ids, EOS = 4, alpha = 0.6; logits = log p, so log-softmax is log p."""
    lp2, lp3 = (7 / 6) ** 0.6, (8 / 6) ** 0.6
    beam = beam_ref.start(2)
    assert [(b.score, b.fin) for b in beam] == [(0.0, LIVE), (-math.inf, DEAD)]
    # step 0: only slot 0 is live (the dead slot's row is never read); ids 0 and 1 tie exactly: the lower id is the first candidate,
    # and their equal scores stay in candidate order.  lp(1) = 1.
    beam, parents, fed, _ = beam_ref.select(_rows([.4, .4, .1, .05, .05], [0, 0, 0, 0, 1]), beam, 4)
    assert [b.ids for b in beam] == [[0], [1]] and parents == [0, 0] and fed == [0, 1]
    assert beam[0].score == beam[1].score == pytest.approx(ln(.4))
    # step 1: slot 0 offers EOS (finished, length stays 1: log .6 / lp(1)) and id 0; slot 1 offers id 2 and, among four equal
    # logits, the lowest id 0.  Best two: [1, 2] (live) and [0] + EOS (finished).
    beam, parents, fed, _ = beam_ref.select(_rows([.1, .1, .1, .1, .6], [.05, .05, .8, .05, .05]), beam, 4)
    c_score, a_score = ln(.4) + ln(.8) / lp2, ln(.4) + ln(.6)
    assert [b.ids for b in beam] == [[1, 2], [0]] and [b.fin for b in beam] == [LIVE, FINISHED]
    assert parents == [1, 0] and fed == [2, 0]
    assert beam[0].score == pytest.approx(c_score) and beam[1].score == pytest.approx(a_score)
    cut = beam_ref.finish(beam)                   # the max-length cut here: the live slot counts as finished, score unchanged, and wins
    assert cut[0] == 0 and cut[1] == pytest.approx(c_score - a_score)
    # step 2: the finished slot is carried as one candidate, unchanged; the live one finishes with EOS at length 2
    beam, parents, fed, (score_gap, logit_gap) = beam_ref.select(_rows([.05, .05, .05, .05, .8], [1, 0, 0, 0, 0]), beam, 4)
    assert [b.ids for b in beam] == [[1, 2], [0]] and [b.fin for b in beam] == [FINISHED, FINISHED] and parents == [0, 1] and fed == [0, 0]
    assert beam[0].score == pytest.approx(c_score + ln(.8) / lp2) and beam[1].score == pytest.approx(a_score)
    assert score_gap == pytest.approx(a_score - (c_score + ln(.05) / lp3)) and logit_gap == pytest.approx(0.0)
    # all finished: a further step reproduces the beam in the same order, whatever the logits
    again, parents, fed, _ = beam_ref.select(_rows([.2] * 5, [.2] * 5), beam, 4)
    assert [(b.ids, b.score, b.fin) for b in again] == [(b.ids, b.score, b.fin) for b in beam] and parents == [0, 1]
    assert beam_ref.finish(beam)[0] == 0
    # an EOS id outside the vocabulary never matches; NaN is ordered as -inf; ties in the final choice go to the first slot
    x = np.array([[np.nan, 1.0, 2.0, -np.inf, 0.5]])
    b1, _, fed, _ = beam_ref.select(x, beam_ref.start(1), 128001)
    assert fed == [2] and b1[0].ids == [2] and b1[0].score == pytest.approx(2.0 - ln(math.e + math.e ** 2 + math.e ** .5))
    assert beam_ref.finish([Slot(-1.0, FINISHED, [1]), Slot(-1.0, LIVE, [2])])[0] == 0


def test_backtracking_of_a_hand_made_step_log():
    from uniaudio2_amd.llm_models.model_new import backtrack_beam_log
    f = lambda s: int(np.float32(s).view(np.int32))
    log = np.array([   # (parent, id or -1, score bits, fin) per step and slot, W = 3
        [[0, 10, f(-1.0), 0], [0, 11, f(-1.5), 0], [0, 12, f(-2.0), 0]],
        [[1, 20, f(-2.0), 0], [0, -1, f(-2.1), 1], [1, 21, f(-2.2), 0]],     # slot 1: [10] + EOS
        [[2, 30, f(-3.0), 0], [1, -1, f(-2.1), 1], [0, -1, f(-3.1), 1]],     # slot 1 carried; slot 2: [11, 20] + EOS
        [[0, 40, f(-4.0), 0], [1, -1, f(-2.1), 1], [2, -1, f(-3.1), 1]]])
    want = [[11, 21, 30, 40], [10], [11, 20]]
    for j in range(3):
        assert backtrack_beam_log(log, j) == want[j] == beam_ref.backtrack(log, j)
    assert backtrack_beam_log(log[:0], 1) == []


def test_generator_signature_equals_the_reference():
    from uniaudio2_amd.evaluation.asr_task import Generator
    from uniaudio2_amd.llm_models.model_new import Model_stage3
    sig = inspect.signature(Generator.generate_asr_beam_search)
    assert [(p.name, p.default) for p in sig.parameters.values()][1:] == [
        ("task_prompt", inspect.Parameter.empty), ("task_name", inspect.Parameter.empty), ("text_token", None),
        ("semantic_token", None), ("reason_token", None), ("beam_width", 5), ("length_penalty", 0.6),
        ("no_repeat_ngram_size", 3), ("early_stopping", True), ("max_length", 500)]
    sig = inspect.signature(Model_stage3.beam_search)
    assert [(p.name, p.default) for p in sig.parameters.values()][1:9] == [
        ("tokens", inspect.Parameter.empty), ("tokens_mask", inspect.Parameter.empty), ("beam_width", 5), ("length_penalty", 0.6),
        ("max_length", 500), ("eos_id", 128001), ("early_stopping", True), ("chunk_frames", 16)]


class _BeamModel:
    """Model_stage3 stand-in on CPU: records the calls the generators make and answers beam_search with scripted ids."""

    def __init__(self, ids=(21, 22, 23)):
        self.ids, self.calls, self._st = list(ids), [], None
        self._p = torch.nn.Parameter(torch.zeros(1))

    def parameters(self):
        return iter([self._p])

    def setup_caches(self, b):
        self.calls.append(("setup", b))
        self._st = {"B": b}

    def reset_caches(self): pass
    def forward_prefix(self, *a, **k): pass
    def begin_decode(self, *a, **k): pass
    def set_sampling(self, topk, temperature, seed=None): self.calls.append(("sampling", topk, temperature))
    def set_ngram(self, n=0, fallback=128000, capacity=512): self.calls.append(("ngram", n))

    def generate_frames(self, n, batch, mode, **k):
        self.calls.append(("frames", n, batch, mode))
        log = torch.zeros(n, batch, 9, dtype=torch.int32)
        log[:, :, 0] = 128001
        return log

    def beam_search(self, tokens, tokens_mask, **kw):
        assert tokens.shape == tokens_mask.shape and tokens.shape[1] == 9 and tokens_mask.dtype == torch.bool
        self.calls.append(("beam", kw))
        return list(self.ids), -1.25, [dict(ids=list(self.ids), score=-1.25, finished=True)]


def _token_dir(tmp_path):
    g = torch.Generator().manual_seed(5)
    torch.save(torch.randint(0, 4096, (8, 4), generator=g, dtype=torch.int32), tmp_path / "u_reason.pt")
    torch.save(torch.randint(0, 8192, (8, 6), generator=g, dtype=torch.int32), tmp_path / "u_semantic.pt")
    return tmp_path


def _run_cli(tmp_path, monkeypatch, task, extra):
    from uniaudio2_amd import multi_task_inference as cli
    model = _BeamModel()
    monkeypatch.setattr(cli, "_load_config_and_llm", lambda args: (TA, model, torch.device("cpu")))
    out = tmp_path / "res.txt"
    cli.main(["--task", task, "--token_dir", str(_token_dir(tmp_path)), "--llm_train_config", "unused", "--text_tokenizer_path", "ids",
              "--prompt_text", "1 2", "--results", str(out)] + extra)
    return model, out.read_text()


@pytest.mark.parametrize("task", ["ASR", "Yue_ASR"])
def test_cli_beam_width_reaches_the_beam_search(tmp_path, monkeypatch, task):
    model, text = _run_cli(tmp_path, monkeypatch, task, ["--beam_width", "4", "--length_penalty", "0.8", "--topk", "7"])
    assert text == "u\t21 22 23\n"
    beam = [c for c in model.calls if c[0] == "beam"]
    assert len(beam) == 1 and not [c for c in model.calls if c[0] in ("frames", "ngram")]
    kw = beam[0][1]
    assert (kw["beam_width"], kw["length_penalty"], kw["max_length"], kw["eos_id"], kw["early_stopping"]) == (4, 0.8, 500, 128001, True)
    assert ("setup", 8) in model.calls and model._st["B"] == 8            # the plan holds 2 N sequences
    assert ("sampling", 1, 1.0) in model.calls                            # greedy ranking whatever --topk says


def test_cli_defaults_leave_the_greedy_loop_alone(tmp_path, monkeypatch):
    from uniaudio2_amd.multi_task_inference import get_parser
    ns = get_parser().parse_args(["--task", "ASR"])
    assert ns.beam_width == 0 and ns.length_penalty == 0.6 and ns.decode_type == "greedy"
    model, _ = _run_cli(tmp_path, monkeypatch, "ASR", [])
    assert not [c for c in model.calls if c[0] == "beam"] and [c for c in model.calls if c[0] == "frames"]
    assert model.calls[0] == ("setup", 1) and ("setup", 2) not in model.calls


@pytest.mark.parametrize("task,extra,match", [
    ("ASR", ["--beam_width", "3", "--decode_type", "ngram"], "ngram"),
    ("lyric_recognition", ["--beam_width", "3"], "lyric_recognition"),
    ("audio_caption", ["--beam_width", "3"], "audio_caption"),
    ("music_caption", ["--beam_width", "2"], "music_caption"),
    ("audio_understanding", ["--beam_width", "2"], "audio_understanding"),
    ("speech_s2t", ["--beam_width", "2"], "speech_s2t"),
    ("ASR", ["--beam_width", "9"], "0..8"),
    ("ASR", ["--beam_width", "-1"], "0..8"),
])
def test_cli_refuses_every_other_combination(tmp_path, monkeypatch, task, extra, match):
    with pytest.raises(ValueError, match=match):
        _run_cli(tmp_path, monkeypatch, task, extra)


def test_cli_beamsearch_message_points_to_beam_width(tmp_path, monkeypatch):
    with pytest.raises(NotImplementedError, match="--beam_width"):
        _run_cli(tmp_path, monkeypatch, "ASR", ["--decode_type", "beamsearch"])
    with pytest.raises(NotImplementedError, match="cannot run"):
        _run_cli(tmp_path, monkeypatch, "Yue_ASR", ["--decode_type", "beamsearch", "--beam_width", "3"])


def test_generators_refuse_or_resize():
    from uniaudio2_amd.evaluation.asr_task import Generator
    from uniaudio2_amd.evaluation.lyric_asr_task import Generator as Lyric
    tp, rt, st = torch.tensor([128000, 1, 128001]), torch.zeros(2, 8), torch.zeros(3, 8)
    with pytest.raises(ValueError, match="lyric"):
        Lyric(_BeamModel(), TA, text_tokenizer_path="ids").generate_asr_beam_search(tp, "lyric_recognition")
    model = _BeamModel([5, 6])
    gen = Generator(model, TA, text_tokenizer_path="ids")
    for bad in (0, 9):
        with pytest.raises(ValueError, match="beam_width"):
            gen.generate_asr_beam_search(tp, "asr", semantic_token=st, reason_token=rt, beam_width=bad)
    # no_repeat_ngram_size is accepted and changes nothing, as in the reference; a plan that is too small is re-made for 2 W sequences
    for n in (0, 3, 7):
        assert gen.generate_asr_beam_search(tp, "asr", semantic_token=st, reason_token=rt, no_repeat_ngram_size=n) == "5 6"
    assert model.calls.count(("setup", 10)) == 1 and not [c for c in model.calls if c[0] == "ngram"]
    kws = [c[1] for c in model.calls if c[0] == "beam"]
    assert len(kws) == 3 and all(k == kws[0] for k in kws) and kws[0]["beam_width"] == 5 and kws[0]["length_penalty"] == 0.6
