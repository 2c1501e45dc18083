"""fp8 weight-only plan at the released sizes (bench.build_model: Llama-3.2-3B backbone + experts + 4-layer depth decoder, random init):
plan identity over 4 frames at B = 1 — the fp8 plan against the bf16 plan of the SAME model after every quantised tensor was replaced
by W' = q 2^e (ops.dequant_w8) — and graph replay against the un-graphed frame."""
import pytest
import torch

from w8_ref import is_quantised

pytestmark = pytest.mark.gpu
FRAMES = 4
FP8 = torch.float8_e4m3fn


def _launches(name):
    from uniaudio2_amd._lib import lib
    return lib.ua2_debug_kernel_launches(name.encode())


def test_fullsize_plan_identity_and_graph_replay():
    import bench
    from uniaudio2_amd import ops
    dev = torch.device("cuda")
    m = bench.build_model(dev, seed=0)
    tokens, mask = bench.make_prompt(dev, seed=4242)
    L = tokens.size(1)

    def run(use_graph):
        m.reset_caches()
        m.forward_prefix(tokens[:, :-1], tokens_mask=mask, input_pos=torch.arange(L - 1, device=dev).unsqueeze(0))
        m.begin_decode(tokens[:, -1:], mask[:, -1:], torch.tensor([L - 1], device=dev))
        n_g, n_w = _launches("gemv"), _launches("gemv_w8")
        log = m.generate_frames(FRAMES, 1, 0, reason_eos=-1, reason_card=bench.REASON_CARD, use_graph=use_graph).cpu().clone()
        torch.cuda.synchronize()
        return (log, m.buffer("text_logits", 1).cpu().clone(), m.buffer("audio_logits", 1).cpu().clone(),
                _launches("gemv") - n_g, _launches("gemv_w8") - n_w)

    m.setup_caches(1, dtype=torch.bfloat16, max_seq_length=256, max_rows=64, log_frames=16, weight_dtype=FP8)
    log_a, tl_a, al_a, g_a, w_a = run(False)           # model A, un-graphed: every launch is counted
    log_r, tl_r, al_r, _, _ = run(True)                # model A, graph replay
    assert w_a > 0 and g_a == 0, (g_a, w_a)            # every Linear of the B = 1 frame has a twin and runs on the fp8 kernel
    assert torch.equal(log_a, log_r) and torch.equal(tl_a, tl_r) and torch.equal(al_a, al_r), "graph replay == un-graphed frame"
    pools_a = [t.cpu().clone() for t in m.backbone.kv_cache.k[:2] + m.decoder.kv_cache.v]

    with torch.no_grad():                              # model B: the same module with W' in place of every quantised tensor
        for k, p in m.state_dict().items():
            if not is_quantised(k, p):
                continue
            if k == "audio_head":
                for i in range(p.shape[0]):
                    p[i].copy_(ops.dequant_w8(p[i].float().t().contiguous()).t())
            else:
                p.copy_(ops.dequant_w8(p.float()))
    m.setup_caches(1, dtype=torch.bfloat16, max_seq_length=256, max_rows=64, log_frames=16)
    log_b, tl_b, al_b, g_b, w_b = run(False)
    assert w_b == 0 and g_b > 0, (g_b, w_b)
    assert torch.equal(log_a, log_b), (log_a.tolist(), log_b.tolist())
    assert torch.equal(tl_a, tl_b) and torch.equal(al_a, al_b), (float((tl_a - tl_b).abs().max()), float((al_a - al_b).abs().max()))
    pools_b = [t.cpu().clone() for t in m.backbone.kv_cache.k[:2] + m.decoder.kv_cache.v]
    for x, y in zip(pools_a, pools_b):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16)), "K/V pools"
    assert (log_a[:, :, 0] >= 0).all()
