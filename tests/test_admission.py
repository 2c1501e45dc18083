"""Host side of admission (no GPU): the plan generate_ragged follows (model_new.admission_schedule)."""
import random

import pytest

from uniaudio2_amd.llm_models.model_new import _seed_words, admission_schedule, ragged_schedule

CASES = [[5], [3, 3, 3], [4, 9, 12], [0, 2, 0, 1], [7, 1, 1, 1, 9, 2], [2, 0, 0, 0, 3]]


def _replay(n_frames, batch_size):
    """Runs the plan on the host: frames per sequence, the live set after every step, (time, sequence) of every admission."""
    plan = list(admission_schedule(n_frames, batch_size))
    got = [0] * len(n_frames)
    admitted_at, live, t = {}, None, 0
    for step, active, keep, admit in plan:
        if live is None:
            live = list(active)
            admitted_at.update({b: 0 for b in active})
        assert active == live and step >= 0
        assert len(active) <= batch_size
        for b in active:
            got[b] += step
        t += step
        assert all(0 <= r < len(active) for r in keep) and keep == sorted(keep)
        assert all(got[active[r]] < n_frames[active[r]] for r in keep)                      # nobody runs past its count
        assert all(got[b] == n_frames[b] for r, b in enumerate(active) if r not in keep)     # ... and leaves the frame it finishes
        live = [active[r] for r in keep] + admit
        admitted_at.update({b: t for b in admit})
    assert not live
    return got, admitted_at, plan


@pytest.mark.parametrize("batch_size", [1, 2, 3])
@pytest.mark.parametrize("case", CASES + [[random.Random(s).randint(0, 9) for _ in range(11)] for s in range(4)])
def test_every_sequence_runs_its_frames_and_never_more_than_batch_size_live(case, batch_size):
    got, admitted_at, plan = _replay(case, batch_size)
    assert got == list(case) and sorted(admitted_at) == list(range(len(case)))
    # input order, and at the FIRST boundary with a free row: after every step the rows are full or nobody waits
    order = sorted(admitted_at, key=lambda b: (admitted_at[b], b))
    assert order == list(range(len(case)))
    waiting = len(case) - min(batch_size, len(case))
    for step, active, keep, admit in plan:
        assert len(admit) == min(waiting, batch_size - len(keep))
        waiting -= len(admit)
    assert waiting == 0


@pytest.mark.parametrize("case", CASES)
def test_enough_rows_for_everybody_is_ragged_schedule(case):
    want = [(s, a, k, []) for s, a, k in ragged_schedule(case)]
    assert list(admission_schedule(case, len(case))) == want
    assert list(admission_schedule(case, len(case) + 3)) == want
    assert list(admission_schedule(case)) == want


def test_edges():
    assert list(admission_schedule([], 4)) == []
    with pytest.raises(ValueError):
        list(admission_schedule([1, 2], 0))
    assert _seed_words(0x5EED0000FFFFFFF0) == [-16, 0x5EED0000] and _seed_words(-1) == [-1, -1] and _seed_words(7) == [7, 0]
