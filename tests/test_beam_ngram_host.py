"""The no-repeat-n-gram ban of the beam search without a GPU: tests/beam_ngram_ref.py's `banned` against a brute-force set of all
n-grams, the launches of tests/beam_ngram_cases.py (decided; where the ban matters the float64 rule with and without it end in
different beams; the shapes, lengths and banned columns the GPU test relies on are there), the six-step sequence (a swap, a fan-out),
the CLI's --beam_no_repeat_ngram (validated before a model is built, routed through the real Generator on scripted models), and the
defaults: without the opt-in generate_asr_beam_search[_batch] call the model exactly as before."""
import itertools

import numpy as np
import pytest
import torch

import beam_ngram_cases as nc
import beam_ngram_ref
import beam_ref
from beam_ref import FINISHED, LIVE
from test_beam_groups_host import _BatchModel
from test_beam_groups_host import _run_cli as _run_cli_batch
from test_beam_host import TA, _BeamModel, _run_cli


def test_banned_against_all_ngrams():
    rng = np.random.default_rng(11)
    fired = 0
    for n, L, alphabet in itertools.product([2, 3, 4, 16], [0, 1, 2, 3, 4, 5, 17, 40], [1, 2, 3]):
        for _ in range(6):
            ids = rng.integers(0, alphabet, size=L).tolist()
            grams = {tuple(ids[i:i + n]) for i in range(L - n + 1)}                     # every n-gram of the text
            want = {k for k in range(alphabet) if L >= n - 1 and tuple(ids[L - n + 1:] + [k]) in grams}
            assert beam_ngram_ref.banned(ids, n) == want, (n, ids)
            fired += bool(want)
    assert fired > 100
    assert beam_ngram_ref.banned([7, 7], 2) == {7} and beam_ngram_ref.banned([7], 2) == set() and beam_ngram_ref.banned([1, 2, 1, 2], 0) == set()
    assert beam_ngram_ref.banned([1, 2, 3, 1, 2], 3) == {3} and beam_ngram_ref.banned([1, 2, 3, 1, 2], 2) == {3}
    assert beam_ngram_ref.banned([5, 1, 5, 2, 5, 1, 5], 2) == {1, 2}


def test_every_launch_is_decided_and_the_ban_matters_where_it_says_so():
    cases = list(nc.all_cases())
    assert len({c.name for c in cases}) == len(cases) >= 100
    matters = 0
    for c in cases:
        assert nc.bc.decided(*beam_ngram_ref.rank(c.x[:, :c.V], c.beam, c.eos, c.n, lp_n=c.lp_n, cap=c.cap), c.W), c.name
        assert (c.x[:, c.V:] == nc.PAD).all() and c.x.shape == (c.W, c.ld), c.name
        assert all(c.eos not in b.ids for b in c.beam), c.name                          # the EOS id is never part of a text
        new, parents, _ = nc.after(c)
        plain = beam_ref.select(c.x[:, :c.V], c.beam, c.eos, lp_n=c.lp_n)[0]
        for s, p in zip(new, parents):                                                  # the rule itself: no new id is a banned one
            if s.fin == LIVE and c.beam[p].len <= c.cap:
                assert s.ids[-1] not in beam_ngram_ref.banned(c.beam[p].ids, c.n), c.name
        if c.matters:
            matters += 1
            assert [(s.ids, s.fin) for s in new] != [(s.ids, s.fin) for s in plain], c.name
        m = nc.masked(c)
        assert np.array_equal(np.isneginf(m[:, :c.V]), np.isneginf(beam_ngram_ref.mask(c.x[:, :c.V], c.beam, c.n, c.cap))), c.name
    assert matters >= 60


def test_the_launches_cover_the_shapes_lengths_and_columns():
    cases = list(nc.all_cases())
    assert {c.V for c in cases} == {9217, 16385, 128256} and {c.W for c in cases} == {1, 5, 8} and {c.n for c in cases} == {2, 3, 4, 16}
    assert sum(c.V == 128256 for c in cases) == 1
    seen = set()
    for c in cases:
        for b in c.beam:
            if b.fin == LIVE:
                seen.add((c.n, b.len - c.n if b.len <= c.n else b.len))
    for n in (2, 3, 4, 16):
        assert {(n, -2), (n, -1), (n, 0), (n, 40)} <= seen, n                          # L = n - 2, n - 1, n, 40 under every n
    bans = [(c, b, beam_ngram_ref.banned(b.ids, c.n)) for c in cases for b in c.beam if b.fin == LIVE and b.len <= c.cap]
    assert any(0 in s for _, _, s in bans) and any(c.V - 1 in s for c, _, s in bans)
    assert any(len({k % 1024 for k in s}) < len(s) for _, _, s in bans)                 # two in one thread's residue
    assert any(int(np.argmax(c.x[j, :c.V])) in beam_ngram_ref.banned(b.ids, c.n) for c in cases for j, b in enumerate(c.beam) if b.fin == LIVE)
    twice = [b for c, b, s in bans if c.kind == "twice" and b.len == 40 and c.n <= 4]
    assert twice and all(sum(b.ids[i:i + 1] == [77] for i in range(b.len)) == 2 for b in twice)       # one id banned by two windows
    outside = [(c, j) for c in cases if c.kind == "outside" for j, b in enumerate(c.beam) if b.fin == LIVE and b.len == 40 and c.n <= 4]
    assert outside and all(600 not in beam_ref.topw_ref(c.x[j, :c.V], c.W + 3)[0] for c, j in outside)
    # a finished slot whose text would ban; a dead one; the start; histories in the second trip of a 1024-thread scan; L = cap + 1
    assert any(b.fin == FINISHED and beam_ngram_ref.banned(b.ids, c.n) for c in cases for b in c.beam)
    assert any(b.fin == beam_ref.DEAD for c in cases for b in c.beam) and any(c.beam[0].len == 0 and c.W > 1 and c.beam[1].fin == beam_ref.DEAD for c in cases)
    long = [c for c in cases if c.cap == 1100]
    assert len(long) == 1 and all(b.len == 1030 and b.ids[1025:1028] == [nc.P0, nc.P0 + 1, 5 + 2048] for b in long[0].beam)
    over = [c for c in cases if any(b.len == c.cap + 1 for b in c.beam)]
    assert len(over) == 1 and not over[0].matters and beam_ngram_ref.banned(over[0].beam[0].ids, over[0].n)
    assert int(np.argmax(over[0].x[0, :over[0].V])) in beam_ngram_ref.banned(over[0].beam[0].ids, over[0].n)      # filtering it would show
    assert {len(nc.group_cases(V, W)) for V in nc.SMALL for W in nc.WIDTHS} == {3}


def test_the_sequence_has_a_swap_a_fan_out_and_a_ban_that_changes_the_result():
    seq, plain = nc.sequence()
    assert len(seq) == nc.SEQ_STEPS == 6 and all(s["decided"] for s in seq)
    assert any(nc.has_swap(s["parents"]) for s in seq) and any(nc.has_fan_out(s["parents"]) for s in seq[1:])
    assert sum(any(s["bans"]) for s in seq) >= 2 and [b.ids for b in seq[-1]["beam"]] != plain
    for s in seq:                                                                       # the texts grow from their parents'
        for b, p in zip(s["beam"], s["parents"]):
            assert b.ids[:-1] == s["before"][p].ids and b.len <= nc.SEQ_CAP
    assert not nc.has_swap([0, 0, 1]) and nc.has_swap([1, 0, 2]) and nc.has_fan_out([2, 2, 0, 2]) and not nc.has_fan_out([0, 0, 1, 1])


# ---- the command line ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra,match", [
    (["--beam_no_repeat_ngram", "3"], "--beam_no_repeat_ngram"),                        # without --beam_width
    (["--beam_width", "0", "--beam_no_repeat_ngram", "2"], "--beam_no_repeat_ngram"),
    (["--beam_width", "3", "--beam_no_repeat_ngram", "1"], "--beam_no_repeat_ngram"),
    (["--beam_width", "3", "--beam_no_repeat_ngram", "17"], "--beam_no_repeat_ngram"),
    (["--beam_width", "3", "--beam_no_repeat_ngram", "-2"], "--beam_no_repeat_ngram"),
    (["--beam_width", "3", "--beam_no_repeat_ngram", "3", "--decode_type", "ngram"], "ngram"),
])
def test_cli_refuses_bad_values_before_a_model_is_built(tmp_path, monkeypatch, extra, match):
    from uniaudio2_amd import multi_task_inference as cli
    ns = cli.get_parser().parse_args(["--task", "ASR"] + extra)
    with pytest.raises(ValueError, match=match):
        cli._check_understanding_decode(ns, "asr")
    built = []
    monkeypatch.setattr(cli, "_load_config_and_llm", lambda args: built.append(1))
    with pytest.raises(ValueError, match=match):
        cli.main(["--task", "ASR", "--token_dir", str(tmp_path), "--llm_train_config", "unused", "--text_tokenizer_path", "ids",
                  "--prompt_text", "1 2", "--results", str(tmp_path / "r.txt")] + extra)
    assert not built


def test_cli_flag_reaches_the_search_and_the_default_does_not(tmp_path, monkeypatch):
    from uniaudio2_amd import multi_task_inference as cli
    assert cli.get_parser().parse_args(["--task", "ASR"]).beam_no_repeat_ngram == 0
    assert "--beam_no_repeat_ngram" in cli.__doc__ and "not measured" in cli.__doc__
    for n in (2, 16):
        cli._check_understanding_decode(cli.get_parser().parse_args(["--task", "ASR", "--beam_width", "1", "--beam_no_repeat_ngram", str(n)]), "asr")
    (tmp_path / "on").mkdir()
    (tmp_path / "off").mkdir()
    model, text = _run_cli(tmp_path / "on", monkeypatch, "ASR", ["--beam_width", "4", "--beam_no_repeat_ngram", "3"])
    assert text == "u\t21 22 23\n"
    kw = [c[1] for c in model.calls if c[0] == "beam"]
    assert len(kw) == 1 and kw[0]["no_repeat_ngram_size"] == 3 and kw[0]["beam_width"] == 4
    assert not [c for c in model.calls if c[0] == "ngram"]                              # the greedy filter stays off
    model, _ = _run_cli(tmp_path / "off", monkeypatch, "ASR", ["--beam_width", "4"])
    kw = [c[1] for c in model.calls if c[0] == "beam"]
    assert len(kw) == 1 and "no_repeat_ngram_size" not in kw[0]


def test_cli_flag_works_with_batch_size(tmp_path, monkeypatch):
    names = ["k", "l", "m"]
    model, text = _run_cli_batch(tmp_path, monkeypatch, "Yue_ASR", ["--beam_width", "2", "--batch_size", "2", "--beam_no_repeat_ngram", "2"], names)
    batch = [c for c in model.calls if c[0] == "beam_batch"]
    assert [c[1] for c in batch] == [2, 1] and all(c[2]["no_repeat_ngram_size"] == 2 for c in batch)
    assert [line.split("\t")[0] for line in text.splitlines()] == names


# ---- the generators --------------------------------------------------------------------------------------------------------------
def test_generator_defaults_leave_the_search_as_it_was():
    from uniaudio2_amd.evaluation.asr_task import Generator
    tp, rt, st = torch.tensor([128000, 1, 128001]), torch.zeros(2, 8), torch.zeros(3, 8)
    model = _BeamModel([5, 6])
    gen = Generator(model, TA, text_tokenizer_path="ids")
    assert Generator.enforce_ngram is False
    for n in (0, 3, 7, 99):                                                             # accepted, no effect: whatever the value
        assert gen.generate_asr_beam_search(tp, "asr", semantic_token=st, reason_token=rt, no_repeat_ngram_size=n) == "5 6"
    kws = [c[1] for c in model.calls if c[0] == "beam"]
    assert len(kws) == 4 and all(k == kws[0] for k in kws) and "no_repeat_ngram_size" not in kws[0]
    gen.enforce_ngram = True                                                            # the opt-in
    assert gen.generate_asr_beam_search(tp, "asr", semantic_token=st, reason_token=rt) == "5 6"
    assert gen.generate_asr_beam_search(tp, "asr", semantic_token=st, reason_token=rt, no_repeat_ngram_size=2) == "5 6"
    assert gen.generate_asr_beam_search(tp, "asr", semantic_token=st, reason_token=rt, no_repeat_ngram_size=0) == "5 6"
    kws = [c[1] for c in model.calls if c[0] == "beam"][4:]
    assert [k.get("no_repeat_ngram_size") for k in kws] == [3, 2, None]
    assert {k: v for k, v in kws[0].items() if k != "no_repeat_ngram_size"} == kws[2]
    for bad in (1, 17, -1):
        with pytest.raises(ValueError, match="no_repeat_ngram_size"):
            gen.generate_asr_beam_search(tp, "asr", semantic_token=st, reason_token=rt, no_repeat_ngram_size=bad)


def test_batched_generator_defaults_and_opt_in():
    from uniaudio2_amd.evaluation.asr_task import Generator
    model = _BatchModel()
    gen = Generator(model, TA, text_tokenizer_path="ids")
    tp = torch.tensor([128000, 1, 128001])
    rs, ss = [torch.zeros(2 + i, 8, dtype=torch.long) for i in range(2)], [torch.zeros(3 + i, 8, dtype=torch.long) for i in range(2)]
    base = gen.generate_asr_beam_search_batch(tp, "asr", rs, ss, beam_width=2)
    assert gen.generate_asr_beam_search_batch(tp, "asr", rs, ss, beam_width=2, no_repeat_ngram_size=4) == base
    gen.enforce_ngram = True
    assert gen.generate_asr_beam_search_batch(tp, "asr", rs, ss, beam_width=2, no_repeat_ngram_size=4) == base
    kws = [c[2] for c in model.calls if c[0] == "beam_batch"]
    assert [k.get("no_repeat_ngram_size") for k in kws] == [None, None, 4] and kws[0] == kws[1]
    with pytest.raises(ValueError, match="no_repeat_ngram_size"):
        gen.generate_asr_beam_search_batch(tp, "asr", rs, ss, beam_width=2, no_repeat_ngram_size=40)


def test_binding_declares_the_struct_and_the_entry_points():
    import ctypes as C
    from uniaudio2_amd import _lib
    assert _lib.ABI_STRUCTS[7] is _lib.BeamNgram and _lib.lib.ua2_struct_size(7) == C.sizeof(_lib.BeamNgram) == 16
    assert [f[0] for f in _lib.BeamNgram._fields_] == ["n", "cap", "hist"]
    assert {"ua2_beam_step_groups_ngram", "ua2_stage3_set_beam_ngram"} <= set(_lib.exported_symbols())
    assert _lib.lib.ua2_version() == 10
    # checked before any launch (nothing here touches a device): a bad n, a bad capacity, a missing history, a missing handle
    st = _lib.BeamState()
    for ng, what in [(_lib.BeamNgram(1, 8, 1), "2..16"), (_lib.BeamNgram(17, 8, 1), "2..16"), (_lib.BeamNgram(3, 0, 1), "capacity"),
                     (_lib.BeamNgram(3, 8, None), "NULL history")]:
        assert _lib.lib.ua2_beam_step_groups_ngram(None, 16, 16, 1, 1, 3, C.byref(st), C.byref(ng), None, 1, None) != 0
        assert what in _lib.lib.ua2_last_error().decode(), what
    assert _lib.lib.ua2_stage3_set_beam_ngram(None, None) != 0 and b"NULL handle" in _lib.lib.ua2_last_error()
