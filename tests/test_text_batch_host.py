"""Host side of the batched text loop (no GPU): GeneratorBase._generate_text_batch — EOS scan, retirement, admission, row seeds and
the n-gram filter around the call — the five modules' batched twins, and the command line's route for --batch_size N without a beam,
on a scripted stand-in for Model_stage3 in the style of test_batch_scheduler._AdmittingModel."""
import pytest
import torch

from test_ngram import EOS, TA, ngram_banned, ngram_loop

PROMPT = torch.tensor([128000, 1, 2, 128001])


class _TextModel:
    """Model_stage3's text-loop interface, single and batched: a sequence is recognised by its prompt length (`by_len`: prompt
    length -> utterance) and replays its own scripted text ids (the last one repeats for ever); rows follow retire_rows / admit_rows
    as the device state does; with set_ngram on, every row's ids pass the rule against the row's own history."""

    def __init__(self, streams, by_len, log_frames=512, fail_at_call=None):
        self.streams, self.by_len, self.log_frames, self.fail_at_call = streams, by_len, log_frames, fail_at_call
        self._p = torch.nn.Parameter(torch.zeros(1))
        self._st = None
        self.rows, self.cursor, self.hist, self.calls, self.seeds, self.slot, self.events = [], {}, {}, [], {}, 0, []
        self.streams_on, self.ngram, self.ngram_calls, self.sampling = False, None, [], None

    def parameters(self):
        return iter([self._p])

    def setup_caches(self, b, max_rows=64, log_frames=512):
        self._st = {"B": b, "max_rows": max_rows, "log_frames": self.log_frames}

    def _start(self, utts):
        for u in utts:
            self.cursor[u], self.hist[u] = 0, []

    # the single path (_prefill)
    def reset_caches(self): self.slot = 0
    def forward_prefix(self, *a, **k): pass

    def begin_decode(self, tokens, mask, input_pos):
        self.rows = [self.by_len[int(input_pos) + 1]]
        self._start(self.rows)
        self.events.append(("single", list(self.rows)))

    # the batched path
    def begin_ragged(self, prompts):
        assert len(prompts) <= self._st["B"] and all(m.dtype == torch.bool and t.shape == m.shape for t, m in prompts)
        self.rows = [self.by_len[int(t.shape[0])] for t, _ in prompts]
        self._start(self.rows)
        self.slot = 0
        self.events.append(("begin", list(self.rows)))

    def set_sampling(self, topk, temperature, seed=None):
        self.sampling = (topk, temperature)

    def set_row_seeds(self, seeds, rows=None):
        self.streams_on = seeds is not None
        if seeds is None:
            return
        rows = list(range(len(seeds))) if rows is None else list(rows)
        for r, s in zip(rows, seeds):
            self.seeds.setdefault(self.rows[r], []).append(s)

    def set_ngram(self, n=0, fallback=128000, capacity=512):
        self.ngram_calls.append((n, fallback, capacity))
        self.ngram = (n, fallback, capacity) if n > 1 else None

    def rewind_frame_log(self):
        self.slot = 0
        self.events.append(("rewind",))

    def generate_frames(self, n, batch, mode, reason_eos=-1, reason_card=0, max_pos=None, skip_text_head=False, skip_audio_experts=False):
        assert batch == len(self.rows) <= self._st["B"] and mode == 1
        assert self.slot + n <= self._st["log_frames"], "frame log too small"
        if self.fail_at_call is not None and len(self.calls) == self.fail_at_call:
            raise RuntimeError("scripted frame failure")
        self.slot += n
        self.calls.append((n, batch, skip_audio_experts))
        out = torch.zeros(n, batch, 9, dtype=torch.int32)
        for r, u in enumerate(self.rows):
            for f in range(n):
                c = self.streams[u][min(self.cursor[u], len(self.streams[u]) - 1)]
                self.cursor[u] += 1
                if self.ngram:
                    assert len(self.hist[u]) < self.ngram[2], "n-gram history past its capacity"
                    if ngram_banned(self.hist[u], c, self.ngram[0]):
                        c = self.ngram[1]
                self.hist[u].append(c)
                out[f, r, 0] = c
        return out

    def retire_rows(self, keep, batch):
        assert batch == len(self.rows) and len(set(keep)) == len(keep)
        self.events.append(("retire", [u for r, u in enumerate(self.rows) if r not in keep]))
        self.rows = [self.rows[r] for r in keep]
        return len(keep)

    def admit_rows(self, prompts, batch, seeds=None):
        assert batch == len(self.rows) and batch + len(prompts) <= self._st["B"]
        assert (seeds is not None) == self.streams_on
        new = [self.by_len[int(t.shape[0])] for t, _ in prompts]
        self.rows += new
        self._start(new)
        if seeds is not None:
            assert len(seeds) == len(prompts)
            self.set_row_seeds(seeds, rows=range(batch, batch + len(prompts)))
        self.events.append(("admit", new))
        return batch + len(prompts)


def _prompts(n):
    """n prompts of distinct lengths 5, 6, ...; the loop never looks inside them."""
    return [(torch.zeros(5 + b, 9, dtype=torch.long), torch.ones(5 + b, 9)) for b in range(n)]


def _generator(model, chunk=4):
    from uniaudio2_amd.evaluation.asr_task import Generator
    gen = Generator(model, TA, text_tokenizer_path="ids")
    gen.chunk_frames = chunk
    return gen


def _want(stream, max_frames):
    ids = []
    for f in range(max_frames):
        t = stream[min(f, len(stream) - 1)]
        if t == EOS:
            break
        ids.append(t)
    return " ".join(str(t) for t in ids)


# chunk_frames = 4.  EOS in the first frame of a chunk (frames 0 and 4), in the last (frames 3 and 7), in between, and never
STREAMS = [[EOS, 5], [11, 12, 13, EOS, 9], [21, 22, 23, 24, EOS, 9], [31, 32, 33, 34, 35, 36, 37, EOS, 9], [41, 42], [51, 52, EOS],
           [61 + i for i in range(40)]]
MAX_FRAMES = [6, 6, 9, 12, 7, 2, 10]               # utterance 4 and 6 never meet EOS: 7 and 10 frames; 5 stops at its limit before EOS


@pytest.mark.parametrize("batch_size", [1, 2, 3, None])
def test_each_text_is_its_stream_up_to_eos_or_max_frames(batch_size):
    model = _TextModel(STREAMS, {5 + b: b for b in range(len(STREAMS))}, log_frames=8)
    gen = _generator(model)
    texts = gen._generate_text_batch(_prompts(len(STREAMS)), max_frames=MAX_FRAMES, batch_size=batch_size)
    assert texts == [_want(s, k) for s, k in zip(STREAMS, MAX_FRAMES)]
    assert texts[0] == "" and texts[4] == "41 42 42 42 42 42 42" and texts[5] == "51 52"
    cap = len(STREAMS) if batch_size is None else batch_size
    assert model._st["B"] == cap and max(b for _, b, _ in model.calls) == cap            # never more than batch_size live
    assert all(n <= 4 for n, _, _ in model.calls) and all(skip for _, _, skip in model.calls)
    assert model.events[0] == ("begin", list(range(cap)))
    assert [u for e in model.events if e[0] == "admit" for u in e[1]] == list(range(cap, len(STREAMS)))    # the queue, in input order
    assert sorted(u for e in model.events if e[0] == "retire" for u in e[1]) == list(range(len(STREAMS)))
    assert all(model.cursor[b] <= MAX_FRAMES[b] + 3 for b in model.cursor)               # max_frames counts per utterance
    assert ("rewind",) in model.events                                                   # every session here outlives the log's 8 slots
    assert not model.streams_on and model.seeds == {} and model.ngram_calls == []
    # an int serves every utterance
    model2 = _TextModel(STREAMS, model.by_len)
    assert _generator(model2)._generate_text_batch(_prompts(len(STREAMS)), max_frames=5, batch_size=2) == [_want(s, 5) for s in STREAMS]


def test_admission_happens_at_the_first_boundary_with_a_free_row():
    model = _TextModel(STREAMS, {5 + b: b for b in range(len(STREAMS))})
    gen = _generator(model)
    gen._generate_text_batch(_prompts(len(STREAMS)), max_frames=MAX_FRAMES, batch_size=3)
    ev = [e for e in model.events if e[0] != "rewind"]
    # chunk 1 (4 frames): 0 meets EOS at frame 0, 1 at frame 3; 2 lives on.  Both free rows are taken at once, in input order
    assert ev[:3] == [("begin", [0, 1, 2]), ("retire", [0, 1]), ("admit", [3, 4])]
    # chunk 2: 2 meets EOS in its frame 4; 4 has run 4 of 7.  chunk 3 is cut to the 3 frames utterance 4 has left
    assert ev[3:5] == [("retire", [2]), ("admit", [5])]
    assert [c[:2] for c in model.calls[:4]] == [(4, 3), (4, 3), (2, 3), (1, 3)]
    assert gen._generate_text_batch([], batch_size=3) == []
    with pytest.raises(ValueError, match="one seed per utterance"):
        gen._generate_text_batch(_prompts(3), seeds=[1], batch_size=2)
    with pytest.raises(ValueError, match="max_frames"):
        gen._generate_text_batch(_prompts(3), max_frames=[1, 2])
    with pytest.raises(ValueError, match="max_frames"):
        gen._generate_text_batch(_prompts(3), max_frames=[1, 0, 2])


@pytest.mark.parametrize("fail", [None, 0, 2])
def test_row_seeds_and_ngram_are_on_for_the_call_only(fail):
    model = _TextModel(STREAMS, {5 + b: b for b in range(len(STREAMS))}, fail_at_call=fail)
    gen = _generator(model)
    seeds = [7000 + b for b in range(len(STREAMS))]
    kw = dict(max_frames=MAX_FRAMES, topk=5, temperature=0.8, no_repeat_ngram_size=3, ngram_fallback=499, seeds=seeds, batch_size=2)
    if fail is None:
        gen._generate_text_batch(_prompts(len(STREAMS)), **kw)
        assert model.seeds == {b: [seeds[b]] for b in range(len(STREAMS))}               # one key per utterance, on its row
    else:
        with pytest.raises(RuntimeError, match="scripted frame failure"):
            gen._generate_text_batch(_prompts(len(STREAMS)), **kw)
    assert model.sampling == (5, 0.8)
    assert not model.streams_on and model.ngram is None                                  # cleared, also when a frame raised
    assert model.ngram_calls == [(3, 499, max(MAX_FRAMES)), (0, 128000, 512)]


def test_ngram_filter_runs_per_row_against_the_rows_own_history():
    streams = [[4, 4, 4, 9, 4, 4, EOS], [3, 3, 3, 3, 3], [8, 9, 8, 9, 8, 9, 8, EOS], [5, 5, EOS]]
    limits = [8, 5, 8, 8]
    model = _TextModel(streams, {5 + b: b for b in range(4)})
    texts = _generator(model)._generate_text_batch(_prompts(4), max_frames=limits, no_repeat_ngram_size=2, ngram_fallback=499, batch_size=2)
    want = [" ".join(str(t) for t in ngram_loop((s + [s[-1]] * 8)[:k], 2, 499)) for s, k in zip(streams, limits)]
    assert texts == want and "499" in texts[0] and "499" in texts[1]
    assert sum(limits) > max(limits)                                                    # more frames in all than the capacity, no row past it


# ---- the twins -----------------------------------------------------------------------------------------------------------------
def test_every_understanding_module_has_its_batched_twin():
    from uniaudio2_amd.evaluation import (asr_task, audio_music_caption_task, audio_understanding, lyric_asr_task, speech_edit_ss, speech_s2s,
                                          speech_s2t)
    for mod, names in ((asr_task, ("generate_asr_batch", "generate_asr_with_ngram_sampling_batch")),
                       (lyric_asr_task, ("generate_lyric_asr_batch", "generate_asr_batch")),
                       (audio_music_caption_task, ("generate_audio_caption_batch",)),
                       (audio_understanding, ("generate_answer_batch",)), (speech_s2t, ("generate_answer_batch",))):
        for name in names:
            assert callable(getattr(mod.Generator, name, None)), (mod.__name__, name)
    assert not hasattr(speech_s2s.Generator, "generate_audio_batch") and not hasattr(speech_edit_ss.Generator, "generate_audio_batch")
    gen = lyric_asr_task.Generator(_TextModel([], {}), TA, text_tokenizer_path="ids")
    with pytest.raises(ValueError, match="lyric"):
        gen.generate_asr_with_ngram_sampling_batch(PROMPT, "lyric_recognition", [], [])


def _pairs(n, g):
    return ([torch.randint(0, 4096, (3 + i, 8), generator=g) for i in range(n)], [torch.randint(0, 8192, (5 + 2 * i, 8), generator=g) for i in range(n)])


ASR_LEN = lambda i: 4 + (3 + i + 2) + (5 + 2 * i + 2)        # task prompt | reason bos..eos | semantic bos..eos


@pytest.mark.parametrize("module,twin,single", [("asr_task", "generate_asr_batch", "generate_asr"),
                                                ("asr_task", "generate_asr_with_ngram_sampling_batch", "generate_asr_with_ngram_sampling"),
                                                ("lyric_asr_task", "generate_lyric_asr_batch", "generate_lyric_asr"),
                                                ("lyric_asr_task", "generate_asr_batch", "generate_asr"),
                                                ("audio_music_caption_task", "generate_audio_caption_batch", "generate_audio_caption")])
def test_asr_shaped_twins_equal_their_single_forms(module, twin, single):
    import importlib
    cls = importlib.import_module(f"uniaudio2_amd.evaluation.{module}").Generator
    streams = [[4, 4, 4, 4, 7, EOS], [11, 12, 11, 12, 11, 12, 13, EOS], [EOS], [9, 9, 9, EOS], [1, 2, 3, 4, 5, 6, 7, 8, 9, EOS]]
    rs, ss = _pairs(5, torch.Generator().manual_seed(3))
    model = _TextModel(streams, {ASR_LEN(i): i for i in range(5)})
    gen = cls(model, TA, text_tokenizer_path="ids")
    gen.chunk_frames = 4
    texts = getattr(gen, twin)(PROMPT, "asr", rs, ss, topk=1, batch_size=2)
    assert max(b for _, b, _ in model.calls) == 2 and model.sampling == (1, 0.9)
    one = [getattr(gen, single)(PROMPT, "asr", reason_token=r, semantic_token=s, topk=1) for r, s in zip(rs, ss)]
    assert texts == one and len(set(texts)) == 5
    n = 3 if "ngram" in twin else 0
    assert texts == [" ".join(str(t) for t in ngram_loop(s, n, 128000)) for s in streams]
    with pytest.raises(ValueError):
        getattr(gen, twin)(PROMPT, "asr", rs, ss[:2])


def test_answer_twins_and_the_s2t_length_refusal():
    from uniaudio2_amd.evaluation import audio_understanding, speech_s2t
    g = torch.Generator().manual_seed(8)
    rs, ss = _pairs(4, g)
    streams = [[5, 6, EOS], [7, EOS], [8, 9, 10, 11, 12, EOS], [13, 14, 15, EOS]]
    q = torch.tensor([128000, 40, 41, 128001])
    model = _TextModel(streams, {ASR_LEN(i) + 4: i for i in range(4)})
    gen = audio_understanding.Generator(model, TA, text_tokenizer_path="ids")
    ds = [{"text_seq_question": q, "reason_seq": r.T, "semantic_seq": s.T} for r, s in zip(rs, ss)]
    texts = gen.generate_answer_batch(PROMPT, "audio_understanding", ds, list(ds[0]), ["text", "audio", "audio"], topk=1, batch_size=3)
    assert texts == [gen.generate_answer(PROMPT, "audio_understanding", d=d, keys=list(d), types=["text", "audio", "audio"], topk=1) for d in ds]
    assert texts == ["5 6", "7", "8 9 10 11 12", "13 14 15"]
    # speech_s2t: utterance 1's prompt has 1500 frames or more: its slot is (-1, -1), it takes no row and no seed
    rs[1] = torch.randint(0, 4096, (speech_s2t.MAX_PROMPT_FRAMES, 8), generator=g)
    model = _TextModel(streams, {ASR_LEN(i): i for i in (0, 2, 3)})
    gen = speech_s2t.Generator(model, TA, text_tokenizer_path="ids")
    ds = [{"reason_seq": r, "semantic_seq": s} for r, s in zip(rs, ss)]
    out = gen.generate_answer_batch(PROMPT, "speech_s2t", ds, ["reason_seq", "semantic_seq"], ["audio", "audio"], topk=5, temperature=0.7,
                                    seeds=[90, 91, 92, 93], batch_size=2)
    assert out == [("5 6", 1), (-1, -1), ("8 9 10 11 12", 1), ("13 14 15", 1)]
    assert model.seeds == {0: [90], 2: [92], 3: [93]} and model.sampling == (5, 0.7) and max(b for _, b, _ in model.calls) == 2
    with pytest.raises(ValueError, match="one seed per utterance"):
        gen.generate_answer_batch(PROMPT, "speech_s2t", ds, ["reason_seq", "semantic_seq"], ["audio", "audio"], seeds=[1, 2])


# ---- the command line -------------------------------------------------------------------------------------------------------------
NAMES = ["k", "l", "m", "n", "o"]
CLI_STREAMS = [[11, 12, 11, 12, 11, 12, 13, EOS], [EOS], [1], [21, 22, 23, 24, EOS], [31, 31, 31, 31, 31, 32, EOS]]


def _token_dir(tmp_path, missing=(), long=()):
    g = torch.Generator().manual_seed(5)
    d = tmp_path / "tok"
    d.mkdir(exist_ok=True)
    for i, name in enumerate(NAMES):
        t_r = 1500 if name in long else 3 + i
        torch.save(torch.randint(0, 4096, (8, t_r), generator=g, dtype=torch.int32), d / f"{name}_reason.pt")
        if name not in missing:
            torch.save(torch.randint(0, 8192, (8, 5 + 2 * i), generator=g, dtype=torch.int32), d / f"{name}_semantic.pt")
    return d


def _run_cli(tmp_path, monkeypatch, task, extra, module, twins, plus=0, **dir_kw):
    import importlib
    from uniaudio2_amd import multi_task_inference as cli
    model = _TextModel(CLI_STREAMS, {ASR_LEN(i) + plus: i for i in range(len(NAMES))})
    monkeypatch.setattr(cli, "_load_config_and_llm", lambda args: (TA, model, torch.device("cpu")))
    cls = importlib.import_module(f"uniaudio2_amd.evaluation.{module}").Generator
    calls = []
    for twin in twins:
        real = getattr(getattr(cls, twin), "_real", getattr(cls, twin))        # (an earlier run of this helper wrapped it already)
        spy = lambda self, *a, _real=real, _name=twin, **kw: (calls.append((_name, kw)), _real(self, *a, **kw))[1]
        spy._real = real
        monkeypatch.setattr(cls, twin, spy)
    tmp_path.mkdir(exist_ok=True)
    out = tmp_path / "res.txt"
    cli.main(["--task", task, "--token_dir", str(_token_dir(tmp_path, **dir_kw)), "--llm_train_config", "unused", "--text_tokenizer_path",
              "ids", "--prompt_text", "1 2", "--results", str(out), "--seed", "31"] + extra)
    return model, calls, out.read_text()


@pytest.mark.parametrize("task,decode", [("ASR", "greedy"), ("Yue_ASR", "ngram")])
def test_cli_asr_batched_results_equal_one_by_one(tmp_path, monkeypatch, capsys, task, decode):
    twins = ["generate_asr_batch", "generate_asr_with_ngram_sampling_batch"]
    m1, c1, one = _run_cli(tmp_path / "one", monkeypatch, task, ["--batch_size", "1", "--decode_type", decode], "asr_task", twins, missing=("m",))
    skip1 = [l for l in capsys.readouterr().out.splitlines() if l.startswith("[Skip]")]
    m3, c3, many = _run_cli(tmp_path / "many", monkeypatch, task, ["--batch_size", "3", "--decode_type", decode], "asr_task", twins, missing=("m",))
    skip3 = [l for l in capsys.readouterr().out.splitlines() if l.startswith("[Skip]")]
    assert one == many and skip1 == skip3 == ["[Skip] m: missing reason/semantic .pt"]
    n = 3 if decode == "ngram" else 0
    want = {name: " ".join(str(t) for t in ngram_loop(s, n, 128000)) for name, s in zip(NAMES, CLI_STREAMS)}
    assert many == "".join(f"{name}\t{want[name]}\n" for name in NAMES if name != "m")
    assert c1 == [] and [e[0] for e in m1.events] == ["single"] * 4                      # --batch_size 1: the one-by-one path
    assert [c[0] for c in c3] == ["generate_asr_with_ngram_sampling_batch" if decode == "ngram" else "generate_asr_batch"]
    assert c3[0][1]["batch_size"] == 3 and c3[0][1]["topk"] == 1 and len(c3[0][1]["reason_tokens"]) == 4
    assert m3.events[0] == ("begin", [0, 1, 3]) and not [e for e in m3.events if e[0] == "single"]
    assert max(b for _, b, _ in m3.calls) == 3 and (decode == "ngram") == ("128000" in many)


@pytest.mark.parametrize("task,module,twin", [("lyric_recognition", "lyric_asr_task", "generate_asr_batch"),
                                              ("audio_caption", "audio_music_caption_task", "generate_audio_caption_batch"),
                                              ("music_caption", "audio_music_caption_task", "generate_audio_caption_batch")])
def test_cli_lyric_and_caption_tasks_take_one_batched_call(tmp_path, monkeypatch, task, module, twin):
    _, c1, one = _run_cli(tmp_path / "one", monkeypatch, task, [], module, [twin])
    m, c, many = _run_cli(tmp_path / "many", monkeypatch, task, ["--batch_size", "100"], module, [twin])      # clamped to the 5 utterances
    assert c1 == [] and [x[0] for x in c] == [twin] and one == many
    want = [" ".join(str(t) for t in ngram_loop((s + [s[-1]] * 500)[:500], 0, 0)) for s in CLI_STREAMS]       # "m" never meets EOS: 500 frames
    assert many == "".join(f"{name}\t{text}\n" for name, text in zip(NAMES, want))
    assert m._st["B"] == 5 and m.events[0] == ("begin", [0, 1, 2, 3, 4])


def test_cli_audio_understanding_batched_equals_one_by_one(tmp_path, monkeypatch):
    q = ["--question", "40 41"]                                  # the id tokenizer: bos 40 41 eos = 4 more prompt frames
    _, c1, one = _run_cli(tmp_path / "one", monkeypatch, "audio_understanding", q, "audio_understanding", ["generate_answer_batch"], plus=4)
    m, c, many = _run_cli(tmp_path / "many", monkeypatch, "audio_understanding", q + ["--batch_size", "2"], "audio_understanding",
                          ["generate_answer_batch"], plus=4)
    assert c1 == [] and len(c) == 1 and c[0][1]["topk"] == 1 and c[0][1]["batch_size"] == 2 and one == many
    assert [line.split("\t")[0] for line in many.splitlines()] == NAMES and max(b for _, b, _ in m.calls) == 2


@pytest.mark.parametrize("n", [2, 4])
def test_cli_speech_s2t_seeds_every_utterance_by_its_index_in_names(tmp_path, monkeypatch, capsys, n):
    from uniaudio2_amd import parallel
    m, c, text = _run_cli(tmp_path, monkeypatch, "speech_s2t", ["--batch_size", str(n), "--topk", "7", "--temperature", "0.8"], "speech_s2t",
                          ["generate_answer_batch"], missing=("l",), long=("n",))
    out = capsys.readouterr().out
    assert "[Skip] l: missing reason/semantic .pt" in out and "[Skip] n: sequence too long for speech_s2t" in out
    assert len(c) == 1 and c[0][1]["topk"] == 7 and c[0][1]["batch_size"] == n
    assert c[0][1]["seeds"] == [parallel.utterance_seed(31, i) for i in (0, 2, 3, 4)]     # the loaded ones, keyed by their index in names
    assert m.seeds == {i: [parallel.utterance_seed(31, i)] for i in (0, 2, 4)}            # what reached the model: nothing shifted
    assert m.sampling == (7, 0.8) and not m.streams_on
    want = {name: " ".join(str(t) for t in ngram_loop((s + [s[-1]] * 500)[:500], 0, 0)) for name, s in zip(NAMES, CLI_STREAMS)}
    assert text == "".join(f"{name}\t{want[name]}\n" for name in ("k", "m", "o"))


def test_check_and_help_keep_what_they_pinned():
    from uniaudio2_amd import multi_task_inference as cli
    ns = cli.get_parser().parse_args(["--task", "ASR", "--batch_size", "100"])
    cli._check_understanding_decode(ns, "asr")                                            # no beam: accepted, clamped later
    for argv, task in ((["--task", "audio_caption", "--batch_size", "4", "--beam_width", "4"], "audio_caption"),
                       (["--task", "ASR", "--batch_size", "4", "--beam_width", "4", "--decode_type", "ngram"], "asr"),
                       (["--task", "lyric_recognition", "--batch_size", "4", "--decode_type", "ngram"], "lyric_recognition")):
        with pytest.raises(ValueError):
            cli._check_understanding_decode(cli.get_parser().parse_args(argv), task)
    text = " ".join(cli.get_parser().format_help().split())
    assert "N * W <= 64" in text and "35 GB" in text and "speech_s2t" in text
    assert "utterance_seed" in cli.__doc__ and "byte-identical" in cli.__doc__
