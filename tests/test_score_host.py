"""Teacher-forced scoring, host side (no GPU): the oracle restatement against the reference's own forward (tests/golden/lm_score.npz,
written by make_golden_score.py), the package's two cross-entropy functions against the reference's metric dicts, the label / mask
convention of score_sequence, the label range check, the scoring CLI with a stand-in model, and the host figure the kernel parity
bar of tests/test_gpu_score.py is derived from."""
import json
import os
import types

import numpy as np
import pytest
import torch

import score_ref
from helpers import GOLDEN, build_oracle, build_toy_module, toy_state_dict

CASES = ("mix1", "pair2")


def load_golden_score():
    d = np.load(os.path.join(GOLDEN, "lm_score.npz"))
    meta = json.load(open(os.path.join(GOLDEN, "lm_score.json")))
    return d, meta


def case_inputs(d, case):
    tokens = torch.from_numpy(d[f"{case}_tokens"]).long()
    mask = torch.from_numpy(d[f"{case}_mask"]).bool()
    loss_mask = torch.from_numpy(d[f"{case}_loss_mask"]).bool()
    return tokens, mask, loss_mask


@pytest.fixture(scope="module")
def golden():
    return load_golden_score()


@pytest.mark.parametrize("case", CASES)
def test_score_ref_reproduces_the_reference_forward(golden, case):
    d, meta = golden
    sd = toy_state_dict(dict(meta, keys=json.load(open(os.path.join(GOLDEN, "lm_toy_fp32.json")))["keys"]))
    tokens, mask, loss_mask = case_inputs(d, case)
    tl, al = score_ref.teacher_forced(build_oracle(sd, "fp32", batch=tokens.shape[0]), tokens[:, :-1], tokens[:, 1:, :-1], mask)
    text_logits, ci_logits, label, cmask = score_ref.forward_outputs(tl, al, tokens[:, 1:, :-1], mask, loss_mask)
    assert float(np.abs(text_logits.numpy() - d[f"{case}_text_logits"]).max()) < 5e-5
    assert ci_logits.shape == d[f"{case}_ci_logits"].shape
    assert float(np.abs(ci_logits.numpy() - d[f"{case}_ci_logits"]).max()) < 5e-5
    assert np.array_equal(label.numpy(), d[f"{case}_choosed_label"])
    assert np.array_equal(cmask.numpy(), d[f"{case}_choosed_mask"])


@pytest.mark.parametrize("case", CASES)
def test_cross_entropy_functions_reproduce_the_reference_metrics(golden, case):
    from uniaudio2_amd.llm_models.model_new import CrossEntropyAndAccuracy_residual, CrossEntropyAndAccuracy_text
    d, meta = golden
    want = meta["metrics"][case]
    t = lambda k: torch.from_numpy(d[f"{case}_{k}"])
    loss, m = CrossEntropyAndAccuracy_text(t("text_logits"), t("text_labels"), t("text_mask"))
    assert set(m) == set(want["text"]) and float(loss) == float(m["loss_text"])
    for k, v in want["text"].items():
        assert float(m[k]) == pytest.approx(v, rel=1e-6, abs=1e-12), k
    for key, kw in (("residual8", dict(loss_weights=[1] * 8)), ("residual3", {})):
        loss, m = CrossEntropyAndAccuracy_residual(t("ci_logits"), t("choosed_label"), t("choosed_mask"), **kw)
        assert list(m) == list(want[key])                       # the reference's key order: every acc_i, then every loss_i
        for k, v in want[key].items():
            assert float(m[k]) == pytest.approx(v, rel=1e-6, abs=1e-12), (key, k)
        n = len(kw.get("loss_weights", [1, 1, 1]))
        assert float(loss) == pytest.approx(sum(want[key][f"loss_{i + 1}"] for i in range(n)) / n, rel=1e-6)
    # float64 restatement of the same formulas (what the GPU tests compare the device metrics with)
    ref = score_ref.reference_metrics(d[f"{case}_text_logits"], d[f"{case}_text_labels"], d[f"{case}_text_mask"], d[f"{case}_ci_logits"],
                                      d[f"{case}_choosed_label"], d[f"{case}_choosed_mask"], 8)
    for k, v in {**want["text"], **want["residual8"]}.items():
        assert ref[k] == pytest.approx(v, rel=2e-6, abs=1e-12), k


def test_score_stats_follow_the_reference_formulas(golden):
    """nll / pred taken on the host from the golden logits, laid out as Model_stage3.score returns them -> the metric dicts."""
    from uniaudio2_amd.llm_models.model_new import metrics_from_stats, score_stats
    d, meta = golden
    for case in CASES:
        tokens, mask, loss_mask = case_inputs(d, case)
        B, L, W = tokens.shape
        sel = mask[:, 1:, 0]
        nll, pred = torch.zeros(B, L - 1, W), torch.full((B, L - 1, W), -1, dtype=torch.int32)
        lab = torch.full((B, L - 1, W), -1, dtype=torch.long)
        nll[..., -1] = torch.from_numpy(score_ref.xent64(d[f"{case}_text_logits"], d[f"{case}_text_labels"])).float()
        pred[..., -1] = torch.from_numpy(d[f"{case}_text_logits"].argmax(-1)).int()
        lab[..., -1] = torch.from_numpy(d[f"{case}_text_labels"])
        ci, y = d[f"{case}_ci_logits"], d[f"{case}_choosed_label"]
        nll[..., :-1][sel] = torch.from_numpy(score_ref.xent64(ci, y)).float()
        pred[..., :-1][sel] = torch.from_numpy(ci.argmax(-1)).int()
        lab[..., :-1][sel] = torch.from_numpy(y)
        stats = score_stats(nll, pred, lab, mask[:, 1:], loss_mask[:, 1:])
        for n_w, key in ((None, "residual8"), (3, "residual3")):
            got = metrics_from_stats(stats, n_w)
            want = {**meta["metrics"][case]["text"], **meta["metrics"][case][key]}
            assert list(got) == ["acc_text", "loss_text"] + list(meta["metrics"][case][key])
            for k, v in want.items():
                assert float(got[k]) == pytest.approx(v, rel=1e-6, abs=1e-12), (case, key, k)


def test_score_sequence_derives_labels_and_masks():
    from uniaudio2_amd.llm_models.model_new import Model_stage3
    seen = {}

    def score(self, tokens, labels, tokens_mask, loss_mask=None, text_labels=None, input_pos=None, loss_weights=None):
        seen.update(tokens=tokens, labels=labels, tokens_mask=tokens_mask, loss_mask=loss_mask, text_labels=text_labels)
        return "result"

    g = torch.Generator().manual_seed(3)
    tokens = torch.randint(0, 100, (2, 7, 9), generator=g)
    mask = torch.zeros(2, 7, 9, dtype=torch.bool)
    mask[:, :3, -1] = True
    mask[:, 3:6, :-1] = True                                     # frame 6: padding (no stream masked in)
    loss_mask = torch.rand(2, 7, 9, generator=g) > 0.5
    fake = types.SimpleNamespace(score=types.MethodType(score, object()))
    assert Model_stage3.score_sequence(fake, tokens, mask, loss_mask) == "result"
    assert torch.equal(seen["tokens"], tokens[:, :-1]) and torch.equal(seen["labels"], tokens[:, 1:, :-1])
    assert seen["tokens_mask"] is mask and seen["loss_mask"] is loss_mask
    want = tokens[:, 1:, -1].clone()
    want[:, 2:] = -1                                             # steps 3.. are audio steps / padding: no text label
    assert torch.equal(seen["text_labels"], want)


def test_score_continuation_masks_the_loss_to_the_continuation():
    from uniaudio2_amd.evaluation._generator import GeneratorBase
    seen = {}

    class Model:
        def score_sequence(self, tokens, mask, loss_mask=None):
            seen.update(tokens=tokens, mask=mask, loss_mask=loss_mask)
            return "result"

    gen = GeneratorBase.__new__(GeneratorBase)
    gen._model, gen.device, gen.parallel_number, gen.empty_token = Model(), torch.device("cpu"), 9, 0
    prompt, pmask = gen._text_block(torch.tensor([5, 6, 7]))
    cont, cmask = gen._audio_block(torch.arange(16).view(2, 8))
    assert gen.score_continuation(prompt, pmask, cont, cmask) == "result"
    assert seen["tokens"].shape == (1, 5, 9) and seen["tokens"].dtype == torch.int64
    assert torch.equal(seen["tokens"][0, :3], prompt) and torch.equal(seen["tokens"][0, 3:], cont)
    assert seen["mask"].dtype == torch.bool and torch.equal(seen["mask"][0], torch.cat([pmask, cmask]).bool())
    assert not seen["loss_mask"][0, :3].any() and seen["loss_mask"][0, 3:].all()


@pytest.mark.parametrize("bad", ["audio_high", "audio_low", "text_high", "text_low"])
def test_label_range_errors_raise_before_any_launch(bad):
    m = build_toy_module()
    m._h, m._beam = object(), None                                # a plan that must never be reached
    m._st = dict(device=torch.device("cpu"), ncb=8, va=110, B=2, dtype=torch.float32)
    tokens = torch.zeros(1, 4, 9, dtype=torch.long)
    labels = torch.zeros(1, 4, 8, dtype=torch.long)
    text_labels = torch.full((1, 4), -1, dtype=torch.long)
    mask = torch.ones(1, 5, 9, dtype=torch.bool)
    if bad == "audio_high":
        labels[0, 1, 3] = 110
    elif bad == "audio_low":
        labels[0, 2, 0] = -2
    elif bad == "text_high":
        text_labels[0, 0] = m.backbone.config.padded_vocab_size
    else:
        text_labels[0, 3] = -2
    try:
        with pytest.raises(ValueError, match=r"must lie in \[-1, "):
            m.score(tokens, labels, mask, text_labels=text_labels)
    finally:
        m._h = None                                               # nothing to destroy


def test_score_needs_setup_caches():
    m = build_toy_module()
    with pytest.raises(TypeError, match="setup_caches"):
        m.score(torch.zeros(1, 2, 9, dtype=torch.long), torch.zeros(1, 2, 8, dtype=torch.long), torch.ones(1, 3, 9, dtype=torch.bool))


class StandInModel:
    """Scores like Model_stage3.score_sequence would if every logit row were uniform except for a preference for id (step + stream):
    enough structure for the CLI's bookkeeping to be checked exactly."""

    def __init__(self):
        self.batches = []

    def setup_caches(self, batch):
        self.max_batch = batch

    def score_sequence(self, tokens, mask, loss_mask=None):
        B, L, W = tokens.shape
        assert B <= self.max_batch
        self.batches.append((B, L))
        nll = torch.zeros(B, L - 1, W)
        pred = torch.full((B, L - 1, W), -1, dtype=torch.int32)
        step = torch.arange(1, L).view(1, L - 1, 1) + torch.arange(W).view(1, 1, W)
        audio = mask[:, 1:, :1].expand(-1, -1, W - 1)
        nll[..., :-1] = torch.where(audio, 0.5 + 0.25 * torch.arange(W - 1).float(), torch.zeros(()))
        pred[..., :-1] = torch.where(audio, step[..., :-1].expand(B, -1, -1).int(), pred[..., :-1])
        nll[..., -1] = torch.where(mask[:, 1:, -1], torch.tensor(2.0), torch.tensor(0.0))
        pred[..., -1] = step[..., -1].int()
        return {"nll": nll, "pred": pred, "metrics": {}}


def test_cli_writes_one_json_line_per_sequence_and_a_total(tmp_path, monkeypatch):
    from uniaudio2_amd import score as cli

    def seq(name, n_text, n_audio, with_loss_mask):
        L = n_text + n_audio
        t = torch.zeros(L, 9, dtype=torch.long)
        m = torch.zeros(L, 9, dtype=torch.bool)
        m[:n_text, -1] = True
        m[n_text:, :-1] = True
        t[:, -1] = torch.arange(L) + 8                           # text id of step s = s + 8: the stand-in predicts it
        t[n_text:, :-1] = 1000                                   # audio ids it never predicts ...
        t[n_text:, 2] = torch.arange(n_text, L) + 2              # ... except codebook 2
        d = dict(name=name, tokens=t, mask=m)
        if with_loss_mask:
            lm = torch.ones(L, 9, dtype=torch.bool)
            lm[:2] = False
            d["loss_mask"] = lm
        return d

    seqs = [seq("a", 4, 3, False), seq("b", 3, 6, True), seq("c", 5, 0, False)]
    torch.save(seqs, tmp_path / "seqs.pt")
    model = StandInModel()
    monkeypatch.setattr(cli, "_load_config_and_llm", lambda args: (None, model, torch.device("cpu")))
    cli.main(["--llm_train_config", "unused.yaml", "--sequences", str(tmp_path / "seqs.pt"), "--results", str(tmp_path / "out.jsonl"),
              "--batch_size", "2"])
    assert model.batches == [(2, 9), (1, 5)]                      # two at a time, padded to the longer one
    lines = [json.loads(l) for l in open(tmp_path / "out.jsonl")]
    assert [l["name"] for l in lines] == ["a", "b", "c", "__total__"]
    a, b, c, tot = lines
    assert a["frames"] == 7 and a["n_tokens"] == [3] * 8 + [3] and a["sum_nll"][:2] == [1.5, 2.25] and a["sum_nll"][-1] == 6.0
    assert a["metrics"]["acc_text"] == 1.0 and a["metrics"]["loss_text"] == 2.0
    assert a["metrics"]["acc_3"] == 1.0 and a["metrics"]["acc_1"] == 0.0 and a["metrics"]["loss_2"] == 0.75
    assert b["n_tokens"] == [6] * 8 + [1]                         # the loss mask drops step 1 of the text stream (step 0 is never scored)
    assert c["n_tokens"] == [0] * 8 + [4] and c["metrics"]["acc_1"] is None      # no audio step: no figure
    assert tot["frames"] == 21 and tot["n_tokens"] == [9] * 8 + [8]
    assert tot["sum_nll"][0] == 4.5 and tot["sum_nll"][-1] == 16.0 and tot["metrics"]["loss_1"] == 0.5


def test_cli_rejects_missing_arguments():
    from uniaudio2_amd import score as cli
    with pytest.raises(ValueError, match="--sequences"):
        cli.main(["--llm_train_config", "x.yaml"])


# ---- the host figure behind the kernel parity bar ------------------------------------------------------------------------------
def test_host_fp32_restatement_error_is_the_constant_the_gpu_bar_uses():
    """tests/test_gpu_score.py bounds the kernel's finite nll by 8 x HOST_FP32_ERR: the constant must be what the fp32 restatement
    of the kernel's formula (score_ref.xent32) really misses float64 by on the very inputs of that test."""
    from test_gpu_score import HOST_FP32_ERR, NLL_BAR
    worst = 0.0
    for V, ld in score_ref.XENT_SHAPES:
        for M in score_ref.XENT_ROWS:
            x, y = score_ref.xent_rows(V, ld, M)
            a, b = score_ref.xent32(x[:, :V], y), score_ref.xent64_stable(x[:, :V], y)
            fin = np.isfinite(b)
            assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b))
            if fin.any():
                worst = max(worst, float(np.abs(a[fin].astype(np.float64) - b[fin]).max()))
    assert worst <= HOST_FP32_ERR and worst >= 0.5 * HOST_FP32_ERR, worst     # (numpy's exp / log may move the last digit between versions)
    assert NLL_BAR == 8 * HOST_FP32_ERR
