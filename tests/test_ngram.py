"""The n-gram-constrained ASR loop without a GPU: the ban rule restated in plain Python against the golden the reference's own
rule produced (tests/golden/make_golden_ngram.py), and the CLI's routing of --decode_type (multi_task_inference.py:310-322 of
the reference) through the real Generator classes on a scripted model."""
import json
import os
import types

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TA = types.SimpleNamespace(text_pad_token=128004, semantic_pad_token=9, semantic_eos=8193, semantic_bos=8192,
                           reason_eos=4097, reason_bos=4096, reason_pad_token=7, parallel_number=9,
                           audio_reason_card=4100)
EOS = 128001


def ngram_banned(hist, c, n):
    """evaluation/asr_task.py:407-432: with n >= 2 and len(H) >= n - 1, c is banned when (H[-(n-1):], c) is an n-gram of H.
    n <= 1 bans nothing (the reference's n == 1 looks the whole history up as a prefix and never finds it)."""
    if n <= 1 or len(hist) < n - 1:
        return False
    gram = list(hist[len(hist) - n + 1:]) + [c]
    return any(list(hist[i:i + n]) == gram for i in range(len(hist) - n + 1))


def ngram_loop(candidates, n, fallback, eos=EOS):
    """asr_task.py:359-400 on a given stream of candidates: replace banned ids, stop at EOS (which never enters the history)."""
    hist = []
    for c in candidates:
        t = fallback if ngram_banned(hist, int(c), n) else int(c)
        if t == eos:
            break
        hist.append(t)
    return hist


def load_golden():
    return np.load(os.path.join(GOLDEN, "lm_ngram.npz")), json.load(open(os.path.join(GOLDEN, "lm_ngram.json")))


def test_rule_reproduces_the_reference_golden():
    d, meta = load_golden()
    assert len(meta["cases"]) == 3 and {c["n"] for c in meta["cases"]} == {2, 3}
    for case in meta["cases"]:
        name, n = case["name"], case["n"]
        cand, final = d[f"{name}_cand"], d[f"{name}_final"]
        assert ngram_loop(cand, n, meta["fallback"]) == final.tolist(), name
        assert (cand != final).sum() == case["bans"] >= 1, name
        assert not np.array_equal(final, d[f"{name}_plain"]), name
        assert d[f"{name}_tokens"].shape[-1] == 9 and d[f"{name}_margin"].shape == final.shape


def test_rule_edges():
    assert not ngram_banned([], 5, 2)
    assert ngram_banned([5, 5], 5, 2) and not ngram_banned([5], 5, 2)      # L == n - 1: no n-gram in H yet
    assert ngram_banned([1, 2, 3, 1, 2], 3, 3) and not ngram_banned([1, 2, 3, 1, 2], 4, 3)
    assert not any(ngram_banned([7] * k, 7, 1) for k in range(5))          # n == 1: off
    # the fallback id enters the history and is never itself filtered
    assert ngram_loop([4, 4, 4, 9, 4, 4], 2, 9) == [4, 4, 9, 9, 4, 9]
    # EOS stops the loop and is never banned
    assert ngram_loop([3, EOS, 3], 2, 9) == [3]


class _ScriptedModel:
    """Model_stage3 stand-in on CPU: replays a scripted text log through generate_frames, applying the n-gram rule to it the
    way the device filter does when set_ngram is on, and records every call."""

    def __init__(self, ids):
        self.ids, self.cursor, self.calls, self.ngram = list(ids), 0, [], None
        self._p = torch.nn.Parameter(torch.zeros(1))

    def parameters(self):
        return iter([self._p])

    def setup_caches(self, b): self.batch = b
    def reset_caches(self): self.cursor, self.hist = 0, []
    def forward_prefix(self, *a, **k): pass
    def begin_decode(self, *a, **k): self.hist = []
    def set_sampling(self, topk, temperature, seed=None): self.calls.append(("sampling", topk, temperature))

    def set_ngram(self, n=0, fallback=128000, capacity=512):
        self.calls.append(("ngram", n, fallback, capacity))
        self.ngram = (n, fallback) if n > 1 else None

    def generate_frames(self, n, batch, mode, reason_eos=-1, reason_card=0, max_pos=None, skip_text_head=False,
                        skip_audio_experts=False):
        self.calls.append(("frames", n, batch, mode))
        log = torch.zeros(n, 1, 9, dtype=torch.int32)
        for f in range(n):
            c = self.ids[min(self.cursor, len(self.ids) - 1)]
            self.cursor += 1
            if self.ngram and ngram_banned(self.hist, c, self.ngram[0]):
                c = self.ngram[1]
            self.hist.append(c)
            log[f, 0, 0] = c
        return log


SCRIPT = [11, 12, 11, 12, 11, 12, 13, EOS]


def _token_dir(tmp_path):
    g = torch.Generator().manual_seed(5)
    torch.save(torch.randint(0, 4096, (8, 4), generator=g, dtype=torch.int32), tmp_path / "u_reason.pt")
    torch.save(torch.randint(0, 8192, (8, 6), generator=g, dtype=torch.int32), tmp_path / "u_semantic.pt")
    return tmp_path


def _run_cli(tmp_path, monkeypatch, task, decode_type):
    from uniaudio2_amd import multi_task_inference as cli
    model = _ScriptedModel(SCRIPT)
    monkeypatch.setattr(cli, "_load_config_and_llm", lambda args: (TA, model, torch.device("cpu")))
    out = tmp_path / "res.txt"
    cli.main(["--task", task, "--token_dir", str(_token_dir(tmp_path)), "--llm_train_config", "unused", "--text_tokenizer_path",
              "ids", "--prompt_text", "1 2", "--decode_type", decode_type, "--topk", "7", "--results", str(out)])
    return model, out.read_text()


@pytest.mark.parametrize("task", ["ASR", "Yue_ASR"])
def test_cli_ngram_reaches_the_ngram_loop_greedy(tmp_path, monkeypatch, task):
    model, text = _run_cli(tmp_path, monkeypatch, task, "ngram")
    assert ("sampling", 1, 0.9) in model.calls                             # topk=1 whatever --topk says (:316-321)
    ng = [c for c in model.calls if c[0] == "ngram"]
    assert ng[0][1:3] == (3, 128000) and ng[-1][1] == 0                    # the reference's n = 3 and fallback, off afterwards
    assert all(c[3] == 1 for c in model.calls if c[0] == "frames")       # the text-feedback mode
    want = " ".join(str(t) for t in ngram_loop(SCRIPT, 3, 128000))
    assert text == f"u\t{want}\n" and "128000" in want


@pytest.mark.parametrize("task", ["ASR", "audio_caption", "music_caption"])
def test_cli_greedy_and_caption_tasks_run_the_plain_loop(tmp_path, monkeypatch, task):
    decode = "greedy" if task == "ASR" else "ngram"                       # the caption tasks ignore --decode_type
    model, text = _run_cli(tmp_path, monkeypatch, task, decode)
    assert not [c for c in model.calls if c[0] == "ngram"]
    assert text == "u\t" + " ".join(str(t) for t in SCRIPT[:-1]) + "\n"


def test_cli_lyric_recognition_refuses_ngram(tmp_path, monkeypatch):
    with pytest.raises(ValueError, match="lyric_recognition"):
        _run_cli(tmp_path, monkeypatch, "lyric_recognition", "ngram")
    from uniaudio2_amd.evaluation.lyric_asr_task import Generator
    gen = Generator(_ScriptedModel(SCRIPT), TA, text_tokenizer_path="ids")
    with pytest.raises(ValueError, match="lyric"):
        gen.generate_asr_with_ngram_sampling(torch.tensor([1]), "lyric_recognition")


@pytest.mark.parametrize("task", ["ASR", "audio_caption"])
def test_cli_beamsearch_still_raises(tmp_path, monkeypatch, task):
    with pytest.raises(NotImplementedError):
        _run_cli(tmp_path, monkeypatch, task, "beamsearch")


def test_generator_signature_and_small_n():
    import inspect
    from uniaudio2_amd.evaluation.asr_task import Generator
    sig = inspect.signature(Generator.generate_asr_with_ngram_sampling)
    assert [(p.name, p.default) for p in sig.parameters.values() if p.default is not inspect.Parameter.empty] == [
        ("text_token", None), ("semantic_token", None), ("reason_token", None), ("temperature", 0.9), ("topk", 200),
        ("cfg_scale", 1.0), ("no_repeat_ngram_size", 3), ("repetition_penalty", 1.2), ("fallback_token", 128000)]
    assert sig.parameters["fallback_token"].kind is inspect.Parameter.KEYWORD_ONLY
    for n in (0, 1):                                                       # n <= 1: the plain loop, the filter never switched on
        model = _ScriptedModel([4, 4, 4, EOS])
        gen = Generator(model, TA, text_tokenizer_path="ids")
        out = gen.generate_asr_with_ngram_sampling(torch.tensor([128000, 1, 128001]), "asr", semantic_token=torch.zeros(3, 8),
                                                   reason_token=torch.zeros(2, 8), topk=1, no_repeat_ngram_size=n)
        assert out == "4 4 4" and not [c for c in model.calls if c[0] == "ngram"]
