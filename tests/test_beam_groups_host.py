"""Batched beam search without a GPU: the CLI's checks of --batch_size with --beam_width, the chunking of the names of a token
directory (order, missing files, the results file), the Generator's batched method on a scripted model, and the three grouped entry
points in the ctypes bindings."""
import ctypes as C
import io
import os
import re
import types

import pytest
import torch

TA = types.SimpleNamespace(text_pad_token=128004, semantic_pad_token=9, semantic_eos=8193, semantic_bos=8192,
                           reason_eos=4097, reason_bos=4096, reason_pad_token=7, parallel_number=9,
                           audio_reason_card=4100)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _BatchModel:
    """Model_stage3 stand-in on CPU: answers beam_search / beam_search_batch with ids that name the prompt (its length)."""

    def __init__(self):
        self.calls, self._st = [], None
        self._p = torch.nn.Parameter(torch.zeros(1))

    def parameters(self):
        return iter([self._p])

    def setup_caches(self, b):
        self.calls.append(("setup", b))
        self._st = {"B": b}

    def reset_caches(self): pass
    def set_sampling(self, topk, temperature, seed=None): self.calls.append(("sampling", topk, temperature))

    @staticmethod
    def _answer(tokens):
        ids = [int(tokens.shape[0]), 7]
        return ids, -0.5, [dict(ids=ids, score=-0.5, finished=True)]

    def beam_search(self, tokens, tokens_mask, **kw):
        self.calls.append(("beam", kw))
        return self._answer(tokens)

    def beam_search_batch(self, prompts, **kw):
        for t, m in prompts:
            assert t.shape == m.shape and t.shape[1] == 9 and m.dtype == torch.bool
        self.calls.append(("beam_batch", len(prompts), kw))
        return [self._answer(t) for t, _ in prompts]


def _token_dir(tmp_path, names, missing=()):
    g = torch.Generator().manual_seed(5)
    d = tmp_path / "tok"
    d.mkdir(exist_ok=True)
    for i, name in enumerate(names):
        torch.save(torch.randint(0, 4096, (8, 3 + i), generator=g, dtype=torch.int32), d / f"{name}_reason.pt")
        if name not in missing:
            torch.save(torch.randint(0, 8192, (8, 5 + 2 * i), generator=g, dtype=torch.int32), d / f"{name}_semantic.pt")
    return d


def _run_cli(tmp_path, monkeypatch, task, extra, names=("u",), missing=()):
    from uniaudio2_amd import multi_task_inference as cli
    model = _BatchModel()
    monkeypatch.setattr(cli, "_load_config_and_llm", lambda args: (TA, model, torch.device("cpu")))
    out = tmp_path / "res.txt"
    cli.main(["--task", task, "--token_dir", str(_token_dir(tmp_path, names, missing)), "--llm_train_config", "unused",
              "--text_tokenizer_path", "ids", "--prompt_text", "1 2", "--results", str(out)] + extra)
    return model, out.read_text()


# ---- the checks ------------------------------------------------------------------------------------------------------------------
def test_too_many_rows_names_both_flags(tmp_path, monkeypatch):
    from uniaudio2_amd.multi_task_inference import _check_understanding_decode, get_parser
    ns = get_parser().parse_args(["--task", "ASR", "--batch_size", "9", "--beam_width", "8"])
    with pytest.raises(ValueError, match=r"--batch_size.*--beam_width|--beam_width.*--batch_size"):
        _check_understanding_decode(ns, "asr")
    with pytest.raises(ValueError, match="--batch_size") as e:
        _run_cli(tmp_path, monkeypatch, "Yue_ASR", ["--batch_size", "9", "--beam_width", "8"])
    assert "--beam_width" in str(e.value)
    ns = get_parser().parse_args(["--task", "ASR", "--batch_size", "8", "--beam_width", "8"])      # 64 rows: the limit itself
    _check_understanding_decode(ns, "asr")
    ns = get_parser().parse_args(["--task", "ASR", "--batch_size", "100"])                         # without a beam the flag is ignored
    _check_understanding_decode(ns, "asr")


def test_other_tasks_keep_their_refusal(tmp_path, monkeypatch):
    with pytest.raises(ValueError, match="audio_caption"):
        _run_cli(tmp_path, monkeypatch, "audio_caption", ["--batch_size", "4", "--beam_width", "4"])
    with pytest.raises(ValueError, match="ngram"):
        _run_cli(tmp_path, monkeypatch, "ASR", ["--batch_size", "4", "--beam_width", "4", "--decode_type", "ngram"])


def test_help_states_the_limit_and_the_memory():
    from uniaudio2_amd import multi_task_inference as cli
    text = " ".join(cli.get_parser().format_help().split())
    assert "N * W <= 64" in text and "35 GB" in text
    assert "--batch_size" in cli.__doc__ and "generate_asr_beam_search_batch" in cli.__doc__


# ---- chunking --------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """Generator stand-in: records what each call was handed and answers with the shapes it saw."""

    def __init__(self):
        self.calls = []

    def generate_asr_beam_search_batch(self, task_prompt, task_name, reason_tokens, semantic_tokens, beam_width=5, length_penalty=0.6,
                                       max_length=500):
        self.calls.append((task_name, [tuple(r.shape) for r in reason_tokens], [tuple(s.shape) for s in semantic_tokens],
                           beam_width, length_penalty))
        return [f"r{r.shape[0]} s{s.shape[0]}" for r, s in zip(reason_tokens, semantic_tokens)]


def test_names_go_over_in_chunks_and_keep_their_order(tmp_path, capsys):
    from uniaudio2_amd.multi_task_inference import _beam_search_in_chunks
    names = ["a", "b", "c", "d", "e", "f", "g", "h"]
    d = _token_dir(tmp_path, names, missing=("c",))                        # "c" has no semantic file: skipped, nothing shifts
    args = types.SimpleNamespace(batch_size=3, beam_width=4, length_penalty=0.7)
    gen, out = _Recorder(), io.StringIO()
    _beam_search_in_chunks(args, gen, "asr", torch.tensor([1, 2]), str(d), names, out)
    shape = {n: (3 + i, 5 + 2 * i) for i, n in enumerate(names)}             # (T_reason, T_semantic) per name, (T, 8) after the transpose
    live = [n for n in names if n != "c"]
    want_chunks = [live[0:3], live[3:6], live[6:7]]
    assert [len(c[1]) for c in gen.calls] == [3, 3, 1]
    for call, chunk in zip(gen.calls, want_chunks):
        assert call[0] == "asr" and call[3] == 4 and call[4] == 0.7
        assert call[1] == [(shape[n][0], 8) for n in chunk] and call[2] == [(shape[n][1], 8) for n in chunk]
    assert out.getvalue() == "".join(f"{n}\tr{shape[n][0]} s{shape[n][1]}\n" for n in live)
    assert "[Skip] c" in capsys.readouterr().out


def test_cli_batched_equals_one_by_one(tmp_path, monkeypatch):
    names = ["k", "l", "m", "n", "o"]
    (tmp_path / "one").mkdir()
    (tmp_path / "many").mkdir()
    m1, one = _run_cli(tmp_path / "one", monkeypatch, "ASR", ["--beam_width", "4", "--batch_size", "1"], names, missing=("m",))
    m2, many = _run_cli(tmp_path / "many", monkeypatch, "ASR", ["--beam_width", "4", "--batch_size", "2", "--length_penalty", "0.8"],
                        names, missing=("m",))
    assert one == many and [line.split("\t")[0] for line in many.splitlines()] == ["k", "l", "n", "o"]
    assert len({line.split("\t")[1] for line in many.splitlines()}) == 4     # every utterance has its own text: nothing was swapped
    assert [c[0] for c in m1.calls if c[0].startswith("beam")] == ["beam"] * 4          # --batch_size 1 is the single path
    batch = [c for c in m2.calls if c[0] == "beam_batch"]
    assert [c[1] for c in batch] == [2, 2] and not [c for c in m2.calls if c[0] == "beam"]
    kw = batch[0][2]
    assert (kw["beam_width"], kw["length_penalty"], kw["max_length"], kw["eos_id"]) == (4, 0.8, 500, 128001)
    assert ("setup", 16) in m2.calls and m2._st["B"] == 16                 # 2 * N * W sequences
    assert ("setup", 8) in m1.calls and m1._st["B"] == 8


def test_generator_batch_resizes_and_refuses():
    from uniaudio2_amd.evaluation.asr_task import Generator
    model = _BatchModel()
    gen = Generator(model, TA, text_tokenizer_path="ids")
    tp = torch.tensor([128000, 1, 128001])
    rs, ss = [torch.zeros(2 + i, 8, dtype=torch.long) for i in range(3)], [torch.zeros(3 + i, 8, dtype=torch.long) for i in range(3)]
    model.setup_caches(4)
    texts = gen.generate_asr_beam_search_batch(tp, "asr", rs, ss, beam_width=2)
    assert len(texts) == 3 and len(set(texts)) == 3 and all(t.endswith(" 7") for t in texts)
    assert texts == [gen.generate_asr_beam_search(tp, "asr", reason_token=r, semantic_token=s, beam_width=2) for r, s in zip(rs, ss)]
    assert model.calls.count(("setup", 12)) == 1                           # re-made once for 2 * 3 * 2, kept for the single calls
    for bad in (0, 9):
        with pytest.raises(ValueError, match="beam_width"):
            gen.generate_asr_beam_search_batch(tp, "asr", rs, ss, beam_width=bad)
    with pytest.raises(ValueError, match="64"):
        gen.generate_asr_beam_search_batch(tp, "asr", rs * 3, ss * 3, beam_width=8)
    with pytest.raises(ValueError):
        gen.generate_asr_beam_search_batch(tp, "asr", [], [], beam_width=2)
    with pytest.raises(ValueError):
        gen.generate_asr_beam_search_batch(tp, "asr", rs, ss[:2], beam_width=2)


# ---- the bindings ----------------------------------------------------------------------------------------------------------------
def test_grouped_entry_points_are_bound_and_declared():
    from uniaudio2_amd import _lib
    i32, vp = C.c_int32, C.c_void_p
    want = {"ua2_beam_step_groups": [vp, i32, i32, i32, i32, i32, C.POINTER(_lib.BeamState), vp, i32, vp],
            "ua2_beam_reorder_groups": [i32, i32, vp, vp, i32, vp, i32, C.POINTER(vp), i32, i32, i32, vp],
            "ua2_stage3_set_beam_groups": [vp, i32, i32, i32, C.POINTER(_lib.BeamState), vp, i32]}
    header = open(os.path.join(ROOT, "include", "ua2hip.h")).read()
    declared = set(re.findall(r"\b(ua2_[a-z0-9_]+)\s*\(", header)) - {"ua2_linear_args", "ua2_attn_args"}
    for name, argtypes in want.items():
        fn = getattr(_lib.lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name
        assert name in declared and name in _lib.exported_symbols()
        # the grouped call takes the single call's arguments with G behind W
        single = getattr(_lib.lib, name[:-len("_groups")])
        at = 2 if name == "ua2_stage3_set_beam_groups" else (4 if name == "ua2_beam_step_groups" else 1)
        assert argtypes[:at] + argtypes[at + 1:] == list(single.argtypes), name
    assert set(_lib.exported_symbols()) == declared
    assert _lib.lib.ua2_version() == 10
    # refused on the host, before any launch: no device is touched
    assert _lib.lib.ua2_beam_reorder_groups(9, 1, None, None, 0, None, 0, None, 1, 18, 4, None) != 0
    assert b"beam width" in _lib.lib.ua2_last_error()
    assert _lib.lib.ua2_beam_reorder_groups(5, 13, None, None, 0, None, 0, None, 1, 130, 4, None) != 0
    assert b"64" in _lib.lib.ua2_last_error()
    assert _lib.lib.ua2_stage3_set_beam_groups(None, 2, 2, 0, None, None, 0) != 0
