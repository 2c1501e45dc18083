"""Host side of the admitting decode session (no GPU): model_new.admitting_session, the one loop under generate_ragged and the batched
generators, held to the plan test_admission.py checks (model_new.admission_schedule) on a recording stand-in for Model_stage3."""
import random

import pytest
import torch

from test_admission import CASES
from test_batch_scheduler import PROMPT, _AdmittingModel, _generator, _stream
from test_generators import TA, reference_loop
from uniaudio2_amd.llm_models.model_new import Model_stage3, admission_schedule

LOG_FRAMES = 4                                     # steps split into chunks, sessions outlive the log
ALL_CASES = CASES + [[random.Random(s).randint(0, 9) for _ in range(11)] for s in range(4)]      # (test_admission's: one value, 11 times)
ALL_CASES += [[rng.randint(0, 9) for _ in range(11)] for rng in map(random.Random, range(4))]    # ... and 11 different ones


class _FixedLengthModel:
    """The calls admitting_session and generate_ragged make, recorded in order: sequence b is recognised by its prompt length
    (1 + b), knows its frame count and logs (b, its own frame index) in every frame; rows follow retire_rows / admit_rows."""

    def __init__(self, n_frames, fail_at_call=None):
        self.n_frames, self.fail_at_call = list(n_frames), fail_at_call
        self._st = {"log_frames": LOG_FRAMES, "ncb": 8, "device": torch.device("cpu")}
        self.rows, self.cursor, self.slot, self.events, self.seed_calls, self.seeds, self.calls = [], {}, 0, [], [], {}, 0

    def _start(self, prompts):
        new = [int(t.shape[0]) - 1 for t, _ in prompts]
        self.cursor.update({b: 0 for b in new})
        return new

    def begin_ragged(self, prompts):
        self.rows, self.slot = self._start(prompts), 0
        self.events.append(("begin", list(self.rows)))

    def set_row_seeds(self, seeds, rows=None):
        self.seed_calls.append(None if seeds is None else list(seeds))
        for r, s in zip(range(len(seeds or [])) if rows is None else rows, seeds or []):
            self.seeds.setdefault(self.rows[r], []).append(s)

    def rewind_frame_log(self):
        self.slot = 0
        self.events.append(("rewind",))

    def generate_frames(self, n, batch, mode, reason_eos=-1, reason_card=0, skip_text_head=False):
        assert n >= 1 and batch == len(self.rows) and (mode, reason_eos, reason_card, skip_text_head) == (0, 77, 5, True)
        assert self.slot + n <= self._st["log_frames"], "frame log too small"
        assert all(self.cursor[b] + n <= self.n_frames[b] for b in self.rows), "a sequence runs past its count"
        if self.calls == self.fail_at_call:
            raise RuntimeError("scripted frame failure")
        self.calls += 1
        self.slot += n
        self.events.append(("frames", n, list(self.rows)))
        out = torch.zeros(n, batch, 9, dtype=torch.int32)
        for r, b in enumerate(self.rows):
            out[:, r, 0] = b
            out[:, r, 1] = torch.arange(self.cursor[b], self.cursor[b] + n)
            self.cursor[b] += n
        return out

    def retire_rows(self, keep, batch):
        assert batch == len(self.rows) and len(keep) < batch, "retirement is for when somebody leaves"
        self.events.append(("retire", list(self.rows), list(keep)))
        self.rows = [self.rows[r] for r in keep]
        return len(keep)

    def admit_rows(self, prompts, batch, seeds=None):
        assert batch == len(self.rows)
        assert (seeds is not None) == (bool(self.seed_calls) and self.seed_calls[-1] is not None)
        new = self._start(prompts)
        self.rows += new
        if seeds is not None:
            assert len(seeds) == len(prompts)
            self.set_row_seeds(seeds, rows=range(batch, batch + len(prompts)))
            self.seed_calls.pop()                          # (the stand-in's own call, not the loop's)
        self.events.append(("admit", new))
        return batch + len(prompts)


def _steps(events):
    """The recorded trace as the plan's tuples (step, active, keep, admit): the chunks between two retirements are one step."""
    out, step = [], 0
    for e in events:
        if e[0] == "frames":
            step += e[1]
        elif e[0] == "retire":
            out.append([step, e[1], e[2], []])
            step = 0
        elif e[0] == "admit":
            out[-1][3] = e[1]
    assert step == 0, "frames ran after the last retirement"
    return [tuple(s) for s in out]


def _ragged(model, n_frames, batch_size, seeds=None):
    prompts = [(torch.zeros(1 + b, 9, dtype=torch.long), torch.ones(1 + b, 9, dtype=torch.bool)) for b in range(len(n_frames))]
    return Model_stage3.generate_ragged(model, prompts, n_frames, mode=0, reason_eos=77, reason_card=5, skip_text_head=True,
                                        batch_size=batch_size, seeds=seeds)


@pytest.mark.parametrize("batch_size", [1, 2, 3, None])
@pytest.mark.parametrize("case", ALL_CASES)
def test_the_running_loop_follows_the_plan(case, batch_size):
    model = _FixedLengthModel(case)
    seeds = [500 + b for b in range(len(case))]
    out = _ragged(model, case, batch_size, seeds)
    assert _steps(model.events) == list(admission_schedule(case, batch_size))
    assert model.events[0][0] == "begin" and all(n <= LOG_FRAMES for e in model.events if e[0] == "frames" for n in e[1:2])
    for b, (o, k) in enumerate(zip(out, case)):                    # exactly its frames, its own, in order
        assert o.shape == (k, 9) and o.dtype == torch.int32
        assert o[:, 0].tolist() == [b] * k and o[:, 1].tolist() == list(range(k))
    assert model.cursor == {b: k for b, k in enumerate(case)}
    if max(case) > LOG_FRAMES:                                     # one sequence alone outlives the log
        assert ("rewind",) in model.events
    assert model.seeds == {b: [seeds[b]] for b in range(len(case))}
    first = model.events[0][1]
    assert model.seed_calls == [[seeds[b] for b in first], None]  # on for the first rows, off at the end; admissions carry their own
    # without seeds the streams are never touched
    plain = _FixedLengthModel(case)
    _ragged(plain, case, batch_size)
    assert plain.seed_calls == [] and plain.events == model.events


def test_some_kept_case_needs_a_rewind_and_some_needs_a_zero_step():
    assert any(max(c) > LOG_FRAMES for c in ALL_CASES) and any(0 in c for c in ALL_CASES)


@pytest.mark.parametrize("fail", [0, 2, 5])
@pytest.mark.parametrize("seeded", [True, False])
def test_row_seeds_are_cleared_when_a_frame_raises(fail, seeded):
    case = [7, 1, 1, 1, 9, 2]
    model = _FixedLengthModel(case, fail_at_call=fail)
    with pytest.raises(RuntimeError, match="scripted frame failure"):
        _ragged(model, case, 2, [500 + b for b in range(len(case))] if seeded else None)
    assert model.calls == fail
    assert (model.seed_calls[-1] is None and len(model.seed_calls) == 2) if seeded else model.seed_calls == []


def test_edges():
    assert _ragged(_FixedLengthModel([]), [], 4) == [] and _ragged(_FixedLengthModel([]), [], 0) == []
    model = _FixedLengthModel([1, 2])
    with pytest.raises(ValueError, match="batch_size must be >= 1"):
        _ragged(model, [1, 2], 0)
    assert model.events == []                                      # refused before the model is touched
    model = _FixedLengthModel([0, 0])                              # nobody runs a frame: no call, everybody leaves, empty results
    out = _ragged(model, [0, 0], None)
    assert [e[0] for e in model.events] == ["begin", "retire"] and [o.shape for o in out] == [(0, 9), (0, 9)]


class _RecordingPairModel(_AdmittingModel):
    """_AdmittingModel (row pairs, its pair assertions) that also records frames and retirements in `events`, by utterance."""

    def generate_frames(self, n, batch, *a, **k):
        self.events.append(("frames", n, list(self.rows)))
        return super().generate_frames(n, batch, *a, **k)

    def retire_rows(self, keep, batch):
        assert len(keep) < batch, "retirement is for when somebody leaves"
        self.events.append(("retire", list(self.rows), [r // self.per for r in keep[::self.per]]))
        return super().retire_rows(keep, batch)


def test_row_pairs_follow_the_plan_through_the_audio_generator():
    from uniaudio2_amd.evaluation.tts_task import Generator
    g = torch.Generator().manual_seed(5)
    shapes = [(2, 2), (3, 5), (2, 3), (4, 2), (2, 6)]              # (reason, semantic) frames: utterance b stops in frame r + s + 2
    streams = [_stream(g, r, s) for r, s in shapes]
    frames = [r + s + 2 for r, s in shapes]
    model = _RecordingPairModel(streams, {3 + 2 + 3 + i: i for i in range(len(shapes))}, per=2, log_frames=8)
    gen = _generator(Generator, model, is_cfg=True)
    gen.chunk_frames = 1                                           # every frame is a chunk boundary: the plan of the stop frames, exactly
    seeds = [9000 + i for i in range(len(shapes))]
    out = gen.generate_tts_batch(PROMPT, "tts", [torch.arange(3 + i) for i in range(len(shapes))], topk=5, seeds=seeds, batch_size=2)
    assert _steps(model.events) == list(admission_schedule(frames, 2))
    assert all(batch == 2 * len(e[2]) for e, (_, batch) in zip([e for e in model.events if e[0] == "frames"], model.calls))
    assert ("rewind",) in model.events and model.cursor == {b: k for b, k in enumerate(frames)}
    assert model.seeds == {b: [seeds[b]] * 2 for b in range(len(shapes))} and not model.streams_on
    for b, fr in enumerate(streams):
        rr, rs = reference_loop(fr, TA.reason_eos, TA.semantic_eos, TA.audio_reason_card)
        assert torch.equal(out[b][0], rr) and torch.equal(out[b][1], rs), b
