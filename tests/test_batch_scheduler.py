"""Host side of batched generation with admission (no GPU): the generators' scheduler (_generate_audio_tokens_batch with
batch_size / seeds) and the command line's routing, on a scripted stand-in for Model_stage3 in the style of test_generators.py."""
import pytest
import torch

from test_generators import TA, reference_loop

PROMPT = torch.tensor([128000, 1, 128001])


def _stream(g, n_reason, n_sem, eos=True):
    """eos=False: the reason phase never ends — no semantic frame is ever produced, PhaseSplitter.result fails."""
    frames = [torch.randint(0, 4096, (1, 8), generator=g, dtype=torch.int32) for _ in range(n_reason)]
    if eos:
        frames.append(torch.full((1, 8), TA.reason_eos, dtype=torch.int32))
        frames += [torch.randint(4100, 12292, (1, 8), generator=g, dtype=torch.int32) for _ in range(n_sem)]
        frames.append(torch.full((1, 8), TA.semantic_eos + TA.audio_reason_card, dtype=torch.int32))
    frames += [torch.randint(0, 100, (1, 8), generator=g, dtype=torch.int32) for _ in range(600)]
    return frames


class _AdmittingModel:
    """Model_stage3's batched interface with admission: a sequence is recognised by its prompt length (`by_len`: prompt length ->
    utterance) and replays its own scripted stream; rows follow retire_rows / admit_rows as the device state would; with
    per = 2 an utterance owns a row pair."""

    def __init__(self, streams, by_len, per=1, log_frames=512):
        self.streams, self.by_len, self.per, self.log_frames = streams, by_len, per, log_frames
        self._p = torch.nn.Parameter(torch.zeros(1))
        self._st = None
        self.rows, self.cursor, self.calls, self.seeds, self.slot, self.events = [], {}, [], {}, 0, []
        self.streams_on = False

    def parameters(self):
        return iter([self._p])

    def setup_caches(self, b, max_rows=64, log_frames=512):
        self._st = {"B": b, "max_rows": max_rows, "log_frames": self.log_frames}

    def _utts(self, prompts):
        assert len(prompts) % self.per == 0
        return [self.by_len[int(prompts[i][0].shape[0])] for i in range(0, len(prompts), self.per)]

    def begin_ragged(self, prompts):
        assert len(prompts) <= self._st["B"]
        self.rows = self._utts(prompts)
        self.cursor.update({u: 0 for u in self.rows})
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
            self.seeds.setdefault(self.rows[r // self.per], []).append(s)

    def rewind_frame_log(self):
        self.slot = 0
        self.events.append(("rewind",))

    def generate_frames(self, n, batch, mode, reason_eos=-1, reason_card=0, max_pos=None, skip_text_head=False, skip_audio_experts=False):
        assert batch == self.per * len(self.rows) <= self._st["B"] and mode == (2 if self.per == 2 else 0)
        assert self.slot + n <= self._st["log_frames"], "frame log too small"
        self.slot += n
        self.calls.append((n, batch))
        out = torch.zeros(n, batch, 9, dtype=torch.int32)
        for r, u in enumerate(self.rows):
            s = torch.cat(self.streams[u][self.cursor[u]:self.cursor[u] + n])
            for j in range(self.per):
                out[:, self.per * r + j, 1:] = s
            self.cursor[u] += n
        return out

    def retire_rows(self, keep, batch):
        assert batch == self.per * len(self.rows)
        assert self.per == 1 or all(keep[i] + 1 == keep[i + 1] and keep[i] % 2 == 0 for i in range(0, len(keep), 2)), "pairs stay together"
        self.rows = [self.rows[r // self.per] for r in keep[::self.per]]
        return len(keep)

    def admit_rows(self, prompts, batch, seeds=None):
        assert batch == self.per * len(self.rows) and batch + len(prompts) <= self._st["B"] and batch % self.per == 0
        assert (seeds is not None) == self.streams_on
        new = self._utts(prompts)
        self.rows += new
        self.cursor.update({u: 0 for u in new})
        if seeds is not None:
            assert len(seeds) == len(prompts)
            self.set_row_seeds(seeds, rows=range(batch, batch + len(prompts)))
        self.events.append(("admit", new))
        return batch + len(prompts)


def _generator(cls, model, is_cfg=False):
    gen = cls.__new__(cls)
    for k, v in vars(TA).items():
        setattr(gen, k, v)
    gen.empty_token, gen.is_cfg, gen._model, gen.device = 0, is_cfg, model, torch.device("cpu")
    gen.special_token_dict = gen.get_special_token()
    return gen


@pytest.mark.parametrize("is_cfg", [False, True])
def test_scheduler_admits_into_freed_rows_and_returns_input_order(is_cfg):
    from uniaudio2_amd.evaluation.tts_task import Generator
    from uniaudio2_amd.parallel import GenerationFailed
    g = torch.Generator().manual_seed(21)
    shapes = [(5, 9), (16, 30), (3, 4), (30, 2), (2, 2), (8, 40), (4, 4)]            # all within max_audio_frames = 64
    streams = [_stream(g, r, s, eos=(b != 3)) for b, (r, s) in enumerate(shapes)]        # utterance 3 never ends: it fails alone
    texts = [torch.arange(3 + i) for i in range(len(shapes))]
    per = 2 if is_cfg else 1
    model = _AdmittingModel(streams, {3 + 2 + 3 + i: i for i in range(len(shapes))}, per=per, log_frames=64)
    gen = _generator(Generator, model, is_cfg)
    seeds = [9000 + i for i in range(len(shapes))]
    real = Generator._generate_audio_tokens_batch
    gen._generate_audio_tokens_batch = lambda prompts, **kw: real(gen, prompts, max_audio_frames=64, **kw)
    out = gen.generate_tts_batch(PROMPT, "tts", texts, topk=5, seeds=seeds, batch_size=3)
    assert model._st["B"] == 3 * per and max(b for _, b in model.calls) == 3 * per       # never more than batch_size live
    for b, frames in enumerate(streams):
        if b == 3:
            assert isinstance(out[b], GenerationFailed)                                  # its own slot, and only its own
            continue
        rr, rs = reference_loop(frames, TA.reason_eos, TA.semantic_eos, TA.audio_reason_card)
        assert torch.equal(out[b][0], rr) and torch.equal(out[b][1], rs), b
    assert model.events[0] == ("begin", [0, 1, 2])
    assert [u for e in model.events if e[0] == "admit" for u in e[1]] == [3, 4, 5, 6]     # the queue, in input order
    assert ("rewind",) in model.events                                                   # more frames than the log holds
    assert model.seeds == {b: [seeds[b]] * per for b in range(len(shapes))}              # one key per utterance, on each of its rows
    assert not model.streams_on
    assert model.cursor[3] == 64 and all(model.cursor[b] <= 64 for b in model.cursor)    # max_audio_frames counts per utterance
    # without seeds or batch_size the call is the one-session form: no admission, no streams
    model2 = _AdmittingModel(streams, model.by_len, per=per)
    gen2 = _generator(Generator, model2, is_cfg)
    out2 = gen2.generate_tts_batch(PROMPT, "tts", texts[:3], topk=1)
    assert [e[0] for e in model2.events] == ["begin"] and model2.seeds == {}
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(out2, out[:3]))
    with pytest.raises(ValueError, match="one seed per utterance"):
        gen2.generate_tts_batch(PROMPT, "tts", texts[:3], topk=1, seeds=[1])


def test_every_failure_raises_as_the_single_loop_does():
    from uniaudio2_amd.evaluation.tts_task import Generator
    from uniaudio2_amd.parallel import GenerationFailed
    g = torch.Generator().manual_seed(2)
    streams = [_stream(g, 3, 3, eos=False) for _ in range(2)]
    model = _AdmittingModel(streams, {3 + 2 + 3 + i: i for i in range(2)})
    gen = _generator(Generator, model)
    real = Generator._generate_audio_tokens_batch
    gen._generate_audio_tokens_batch = lambda prompts, **kw: real(gen, prompts, max_audio_frames=1, **kw)
    with pytest.raises(GenerationFailed, match="non-empty TensorList"):
        gen.generate_tts_batch(PROMPT, "tts", [torch.arange(3), torch.arange(4)], topk=1, batch_size=1)


def test_run_sharded_stream_maps_slot_failures():
    from uniaudio2_amd import parallel
    ok = (torch.zeros(8, 2, dtype=torch.int32), torch.ones(8, 3, dtype=torch.int32))
    seen = []

    def stream(idx):
        seen.append(list(idx))
        return [parallel.GenerationFailed("no frames") if i == 1 else ok for i in idx]

    res = parallel.run_sharded_stream([0, 1, 2], [5, 9, 7], stream)
    assert seen == [[1, 2, 0]]                                                            # the whole shard, longest first, in one call
    assert isinstance(res[1], parallel.Failed) and "no frames" in res[1].message
    assert torch.equal(res[0][1], ok[1]) and torch.equal(res[2][0], ok[0])


CLI_TASKS = [("TTS", "tts_task", "generate_tts_batch"), ("TTA", "audiogen_task", "generate_audio_batch"), ("TTM", "musicgen_task", "generate_audio_batch"),
             ("LTS", "songen_task", "generate_LTS_batch"), ("InstructTTS", "insturct_tts_task", "generate_instruct_tts_batch")]


@pytest.mark.parametrize("task,module,twin", CLI_TASKS)
def test_cli_routes_batched_tasks_to_their_twins_with_per_utterance_seeds(tmp_path, monkeypatch, task, module, twin):
    import importlib
    from uniaudio2_amd import multi_task_inference as cli
    from uniaudio2_amd import parallel
    lines = ["5 6 7", "8 9", "10 11 12 13 14", "15 16 17 18"]                             # distinct lengths: 3, 2, 5, 4 ids
    (tmp_path / "texts.txt").write_text("\n".join(lines) + "\n")
    g = torch.Generator().manual_seed(4)
    streams = [_stream(g, 3 + i, 4 + i) for i in range(4)]
    n_ids = [len(l.split()) + 2 for l in lines]                                          # the id tokenizer adds bos / eos
    # prompt length = task prompt (bos 1 2 eos) + text + 2 special tokens (InstructTTS: + the caption, which is the text, + 2)
    plen = lambda n: 4 + n + 2 + ((n + 2) if task == "InstructTTS" else 0)
    model = _AdmittingModel(streams, {plen(n): i for i, n in enumerate(n_ids)})
    monkeypatch.setattr(cli, "_load_config_and_llm", lambda args: (TA, model, torch.device("cpu")))
    mod = importlib.import_module(f"uniaudio2_amd.evaluation.{module}")
    calls = []
    real = getattr(mod.Generator, twin)
    monkeypatch.setattr(mod.Generator, twin, lambda self, **kw: (calls.append(kw), real(self, **kw))[1])
    cli.main(["--task", task, "--stage", "1", "--text_file", str(tmp_path / "texts.txt"), "--llm_train_config", "unused", "--text_tokenizer_path",
              "ids", "--prompt_text", "1 2", "--batch_size", "2", "--topk", "7", "--seed", "31", "--output_dir", str(tmp_path)])
    order = parallel.shard_indices(n_ids, 1, 0)                                           # longest first: [2, 3, 0, 1]
    groups = [order]                                                                      # the whole shard in one call
    assert len(calls) == len(groups)
    for kw, idx in zip(calls, groups):
        assert kw["batch_size"] == 2 and kw["topk"] == 7
        assert kw["seeds"] == [parallel.utterance_seed(31, i) for i in idx]
        assert [t.tolist() for t in kw["text_tokens"]] == [[128000] + [int(x) for x in lines[i].split()] + [128001] for i in idx]
        assert task != "InstructTTS" or [t.tolist() for t in kw["captions"]] == [t.tolist() for t in kw["text_tokens"]]
    assert model.seeds == {i: [parallel.utterance_seed(31, i)] for i in range(4)}         # what reached the model, per utterance
    assert [u for e in model.events if e[0] == "admit" for u in e[1]] == order[2:]       # two rows, the rest admitted in shard order
    for i, frames in enumerate(streams):
        rr, rs = reference_loop(frames, TA.reason_eos, TA.semantic_eos, TA.audio_reason_card)
        assert torch.equal(torch.load(tmp_path / f"utt_{i}_reason.pt"), rr) and torch.equal(torch.load(tmp_path / f"utt_{i}_semantic.pt"), rs)


def test_cli_single_tasks_and_batch_size_one_keep_the_one_by_one_path():
    from uniaudio2_amd import multi_task_inference as cli
    from uniaudio2_amd.evaluation import speech_s2s, speech_edit_ss
    assert not hasattr(speech_s2s.Generator, "generate_audio_batch") and not hasattr(speech_edit_ss.Generator, "generate_audio_batch")
    a = cli.get_parser().parse_args(["--task", "TTS"])
    assert a.batch_size == 1
