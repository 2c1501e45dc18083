"""fp8 weights in batched decode frames, through the frame executor.  The toy model never reaches the weights-stationary kernel (its K
geometries are outside the kernel's table), so the plan-level check runs Model_stage3 at the RELEASED widths with the registry's layer
counts shrunk (backbone 2, experts 1, depth decoder 1), random init as bench.build_model does it.

Plan A: weight_dtype = fp8.  Plan B: the bf16 plan of the same module after every quantised tensor was replaced by W' = q 2^e
(ops.dequant_w8, the in-place recipe of tests/test_gpu_w8_fullsize.py).  The property is an identity: A == B bit for bit, and inside A the
graph replay, the row-limit switch and the B = 1 run (the decode kernel on the image) give the same bits as the batched un-graphed frames."""
import copy
import os

import pytest
import torch

from w8_ref import is_quantised

pytestmark = pytest.mark.gpu
FP8 = torch.float8_e4m3fn
DEV = "cuda"
FRAMES, L = 3, 6
LAYERS = {"Llama-3.2-3B": 2, "Llama-3.2-Understanding": 1, "Llama-3.2-Generation": 1, "Llama-3.2-300M": 1}
COUNTERS = ("skinny2", "skinny2_w8", "gemv", "gemv_w8")


class shallow_registry:
    """The released widths with fewer layers, for the duration of the block; name_to_config is restored on exit (as helpers.toy_registry)."""

    def __enter__(self):
        from uniaudio2_amd.llm_models import config as cfg
        self.cfg, self.saved = cfg, copy.deepcopy(cfg.name_to_config)
        for name, n in LAYERS.items():
            for key in (name, name + "-Instruct"):
                cfg.name_to_config[key]["n_layer"] = n
        return self

    def __exit__(self, *exc):
        self.cfg.name_to_config.clear()
        self.cfg.name_to_config.update(self.saved)
        return False


def _launches():
    from uniaudio2_amd._lib import lib
    return {k: lib.ua2_debug_kernel_launches(k.encode()) for k in COUNTERS}


def _prompts(B):
    g = torch.Generator().manual_seed(4242)
    t = torch.zeros(B, L, 9, dtype=torch.long)
    t[:, :, -1] = torch.randint(0, 128000, (B, L), generator=g)            # row b's prompt does not depend on B: row 0 is the B = 1 prompt
    m = torch.zeros(B, L, 9, dtype=torch.bool)
    m[:, :, -1] = True
    return t.to(DEV), m.to(DEV)


def _session(m, B, mode, use_graph=False):
    """prefill + FRAMES frames of `mode` (0 = audio feedback, 1 = text feedback) -> outputs and the counters' movement over the DECODE frames"""
    import bench
    tk, mk = _prompts(B)
    m.reset_caches()
    pos = torch.arange(L, device=DEV).unsqueeze(0).repeat(B, 1)
    m.forward_prefix(tk[:, :-1], tokens_mask=mk, input_pos=pos[:, :-1])
    m.begin_decode(tk[:, -1:], mk[:, -1:], torch.tensor([L - 1], device=DEV))
    torch.cuda.synchronize()
    n0 = _launches()
    log = m.generate_frames(FRAMES, B, mode, reason_eos=-1, reason_card=bench.REASON_CARD, use_graph=use_graph).cpu().clone()
    torch.cuda.synchronize()
    moved = {k: v - n0[k] for k, v in _launches().items()}
    pools = [t.cpu().clone() for g in (m.audio_understanding_expert, m.backbone, m.audio_generation_expert, m.decoder)
             for t in g.kv_cache.k + g.kv_cache.v]
    return dict(log=log, text=m.buffer("text_logits", B).cpu().clone(), audio=m.buffer("audio_logits", B).cpu().clone(), pools=pools, moved=moved)


def _equal(a, b, what, audio=True):
    assert torch.equal(a["log"], b["log"]), (what, "log")
    assert torch.equal(a["text"], b["text"]), (what, "text_logits")
    if audio:
        assert torch.equal(a["audio"], b["audio"]), (what, "audio_logits")
    for x, y in zip(a["pools"], b["pools"]):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16)), (what, "K/V pools")


@pytest.fixture(scope="module")
def runs():
    import bench
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import lib
    with shallow_registry():
        m = bench.build_model(torch.device(DEV), seed=0)
    kw = dict(dtype=torch.bfloat16, max_seq_length=64, max_rows=64, log_frames=16)
    r = {}
    m.setup_caches(33, weight_dtype=FP8, **kw)
    # the K/V pools are compared whole, so the order matters: the sessions that repeat (8, audio) come right behind it (they rewrite what
    # it wrote), and the rest follows in plan B's order
    r["A", 8, 0] = _session(m, 8, 0)
    r["A", 8, 0, "graph"] = _session(m, 8, 0, use_graph=True)
    os.environ["UA2_SKINNY_W8_MAX_ROWS"] = "0"
    lib.ua2_debug_refresh_env()
    try:
        r["A", 8, 0, "off"] = _session(m, 8, 0)
    finally:
        del os.environ["UA2_SKINNY_W8_MAX_ROWS"]
        lib.ua2_debug_refresh_env()
    r["A", 8, 1] = _session(m, 8, 1)
    r["A", 33, 0] = _session(m, 33, 0)
    r["A", 33, 1] = _session(m, 33, 1)
    r["A", 1, 0] = _session(m, 1, 0)
    with torch.no_grad():                                                  # plan B: the same module with W' in place of every quantised tensor
        for k, p in m.state_dict().items():
            if not is_quantised(k, p):
                continue
            if k == "audio_head":
                for i in range(p.shape[0]):
                    p[i].copy_(ops.dequant_w8(p[i].float().t().contiguous()).t())
            else:
                p.copy_(ops.dequant_w8(p.float()))
    m.setup_caches(33, **kw)
    for B in (8, 33):
        for mode in (0, 1):
            r["B", B, mode] = _session(m, B, mode)
    return r


@pytest.mark.parametrize("B", [8, 33])
def test_plan_identity_with_the_bf16_plan_on_w_prime(runs, B):
    _equal(runs["A", B, 0], runs["B", B, 0], (B, "audio feedback"))
    _equal(runs["A", B, 1], runs["B", B, 1], (B, "text feedback"), audio=False)     # the text loop never runs the depth decoder
    assert (runs["A", B, 0]["log"] >= 0).all() and float(runs["A", B, 0]["audio"].abs().max()) > 0
    tk, _ = _prompts(B)
    assert len({tuple(row.tolist()) for row in tk[:, :, -1].cpu()}) == B, "the rows differ in their prompt ids"


@pytest.mark.parametrize("B", [8, 33])
def test_counters_over_the_decode_frames(runs, B):
    for mode in (0, 1):
        a, b = runs["A", B, mode]["moved"], runs["B", B, mode]["moved"]
        # plan A: every Linear the weights-stationary kernel takes streams the fp8 image — "skinny2" (that kernel on the bf16 twin) does not
        # move at all; lm_head (128 k columns) is not that kernel's launch in either plan: the tiled kernel reads its twin
        assert a["skinny2_w8"] > 0 and a["gemv_w8"] == 0 and a["gemv"] == 0 and a["skinny2"] == 0, (B, mode, a)
        assert b["skinny2_w8"] == 0 and b["gemv_w8"] == 0 and b["skinny2"] == a["skinny2_w8"], (B, mode, a, b)


def test_graph_replay_equals_the_ungraphed_frames(runs):
    _equal(runs["A", 8, 0], runs["A", 8, 0, "graph"], "graph replay")


def test_row_limit_switch_gives_the_same_bits_on_the_twin(runs):
    off = runs["A", 8, 0, "off"]
    _equal(runs["A", 8, 0], off, "UA2_SKINNY_W8_MAX_ROWS=0")
    assert off["moved"]["skinny2_w8"] == 0 and off["moved"]["skinny2"] == runs["A", 8, 0]["moved"]["skinny2_w8"], off["moved"]


def test_row_0_of_the_batch_equals_its_single_run_on_the_decode_kernel(runs):
    one, many = runs["A", 1, 0], runs["A", 8, 0]
    assert one["moved"]["gemv_w8"] > 0 and one["moved"]["skinny2_w8"] == 0, one["moved"]
    assert torch.equal(one["log"][:, 0], many["log"][:, 0])
    assert torch.equal(one["text"][0], many["text"][0]) and torch.equal(one["audio"][0], many["audio"][0])
