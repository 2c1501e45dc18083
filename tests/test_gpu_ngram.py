"""The on-device n-gram filter of the text loop (include/ua2hip.h ua2_ngram_filter, ua2_stage3_set_ngram; Model_stage3.set_ngram;
Generator.generate_asr_with_ngram_sampling): the kernel against the plain-Python rule, the generator against the golden the
reference's own rule produced, and the device loop against a host replay (generate_frame per frame + the rule)."""
import numpy as np
import pytest
import torch

from helpers import build_product_model, load_golden_lm, toy_state_dict
from test_ngram import TA, load_golden, ngram_banned

pytestmark = pytest.mark.gpu
FALLBACK = 499             # the golden's toy fallback id (the toy vocabulary has 500 ids)


@pytest.fixture(scope="module")
def sd():
    return toy_state_dict(load_golden_lm()[1])


@pytest.fixture(scope="module")
def golden():
    return load_golden()


def _prompt(golden, name):
    d = golden[0]
    return torch.from_numpy(d[f"{name}_tokens"]).long(), torch.from_numpy(d[f"{name}_mask"]).bool()


def _asr_prompt(seed, n_text, n_audio, vt=500, va=110):
    """Same shape as the golden's prompts: text frames, audio frames, a two-frame text tail."""
    g = torch.Generator().manual_seed(seed)
    L = n_text + n_audio + 2
    t = torch.zeros(L, 9, dtype=torch.long)
    m = torch.zeros(L, 9, dtype=torch.bool)
    t[:n_text, -1] = torch.randint(0, vt, (n_text,), generator=g); m[:n_text, -1] = True
    t[n_text:n_text + n_audio, :8] = torch.randint(0, va, (n_audio, 8), generator=g); m[n_text:n_text + n_audio, :8] = True
    t[-2:, -1] = torch.randint(0, vt, (2,), generator=g); m[-2:, -1] = True
    return t, m


def _decided_prefix(golden, name, atol=5e-5):
    """Frames before the first one whose reference top-2 margin is under 2 x the fp32 logit tolerance of the golden tests
    (tests/test_gpu_lm.py): a flip there is legitimate and changes every later frame."""
    low = np.nonzero(golden[0][f"{name}_margin"] < 2 * atol)[0]
    return int(low[0]) if low.size else len(golden[0][f"{name}_margin"])


def host_replay(m, tokens, mask, frames, n, fallback, init=None):
    """(B, L, 9) prompts of one length: forward_prefix, then generate_frame per frame with the rule applied on the host.
    init: per-row histories the loop starts from (default empty); only the new ids are returned."""
    dev = "cuda"
    tokens, mask = tokens.to(dev), mask.to(dev)
    B, L, _ = tokens.shape
    m.reset_caches()
    pos = torch.arange(0, L, device=dev).unsqueeze(0).repeat(B, 1)
    m.forward_prefix(tokens[:, :-1], labels=tokens[:, 1:, :-1], tokens_mask=mask, loss_mask=mask, input_pos=pos[:, :-1])
    cp, maxp1 = torch.tensor([L - 1], device=dev), L
    ct, cm = tokens[:, -1:], mask[:, -1:]
    hist = [list(h) for h in init] if init is not None else [[] for _ in range(B)]
    k0 = len(hist[0])
    for _ in range(frames):
        s = m.generate_frame(ct, cm, input_pos=cp, input_pos_maxp1=maxp1, temperature=1.0, topk=1).cpu()
        ids = []
        for b in range(B):
            c = int(s[b, 0])
            t = fallback if ngram_banned(hist[b], c, n) else c
            hist[b].append(t)
            ids.append(t)
        ct = torch.zeros(B, 1, 9, dtype=torch.long, device=dev)
        ct[:, 0, -1] = torch.tensor(ids, device=dev)
        cm = torch.zeros(B, 1, 9, dtype=torch.bool, device=dev); cm[:, 0, -1] = True
        cp, maxp1 = cp + 1, maxp1 + 1
    return torch.tensor([h[k0:] for h in hist], dtype=torch.int32).T      # (F, B)


def device_loop(m, prompts, frames, n, fallback=FALLBACK, capacity=64, chunk=16, retire=None, init=None):
    """The generators' on-device loop: ragged prefill, set_ngram, text frames in chunks with the experts skipped after frame 1.
    retire = (after_frames, keep): retire_rows at that chunk boundary.  init: per-row histories of one length written into the
    decode state before the first frame.  Returns per-prompt id lists."""
    dev = "cuda"
    m.begin_ragged([(t.to(dev), k.to(dev)) for t, k in prompts])
    m.set_ngram(n, fallback, capacity=capacity)
    if init is not None:
        k0 = len(init[0])
        m._st["ngram_hist"][:len(init), :k0] = torch.tensor(init, dtype=torch.int32, device=dev)
        m._st["ngram_len"][:len(init)] = k0
        m._ngram_hi = k0
    rows = list(range(len(prompts)))
    out = [[] for _ in prompts]
    done = 0
    while done < frames:
        if retire is not None and done == retire[0]:
            m.retire_rows(retire[1], len(rows))
            rows = [rows[k] for k in retire[1]]
        k = min(chunk, frames - done)
        log = m.generate_frames(k, len(rows), 1, skip_audio_experts=True).cpu()
        for r, b in enumerate(rows):
            out[b] += log[:, r, 0].tolist()
        done += k
    m.set_ngram(0)
    return out


def _repeats(ids, n, fallback):
    """Frames whose id is not the fallback but completes an n-gram that occurred before it (the filter forbids these)."""
    bad = []
    for t in range(n - 1, len(ids)):
        if ids[t] != fallback and ngram_banned(ids[:t], ids[t], n):
            bad.append(t)
    return bad


# ---- 1. the kernel -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 4, 8, 16])
def test_ngram_filter_kernel_against_the_rule(n):
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import check, lib
    R, cap, ld, guard, fb = 64, 48, 9, 64, 128000
    g = np.random.default_rng(100 + n)
    Ls = [0, max(n - 2, 0), n - 1, n, 37, cap - 1, cap, cap + 1]
    hist = g.integers(0, 128256, size=(R, cap)).astype(np.int32)
    hl = np.zeros(R, np.int32)
    out = g.integers(0, 128256, size=(R, ld)).astype(np.int32)
    for r in range(R):
        L, kind = Ls[r % len(Ls)], (r // len(Ls)) % 4
        hl[r] = L
        h = hist[r]
        if kind == 3:                                                      # the fallback id inside H, and as the candidate
            h[g.integers(0, cap, size=3)] = fb
        Ls_ = min(L, cap)
        if kind in (0, 3) and Ls_ >= n:                                    # a hit somewhere in H
            i = int(g.integers(0, Ls_ - n + 1))
        elif kind == 1 and Ls_ >= n:                                       # a hit only at the most recent n-gram
            i = Ls_ - n
        else:
            i = None
        if i is not None:
            for j in range(n - 1):
                h[Ls_ - n + 1 + j] = h[i + j]
            out[r, 0] = h[i + n - 1]
        if kind == 3 and r % 2:
            out[r, 0] = fb
    dev = "cuda"
    hbuf = torch.full((R * cap + guard,), -7, dtype=torch.int32, device=dev)
    hbuf[:R * cap] = torch.from_numpy(hist.reshape(-1)).to(dev)
    lbuf = torch.full((R + guard,), -7, dtype=torch.int32, device=dev)
    lbuf[:R] = torch.from_numpy(hl).to(dev)
    obuf = torch.from_numpy(out).to(dev)
    check(lib.ua2_ngram_filter(obuf.data_ptr(), ld, R, n, fb, hbuf.data_ptr(), lbuf.data_ptr(), cap, ops.stream()), "ua2_ngram_filter")
    torch.cuda.synchronize()
    want_out, want_hist, want_len = out.copy(), hist.copy(), hl + 1
    bans = 0
    for r in range(R):
        L = int(hl[r])
        if L <= cap and ngram_banned(hist[r, :L].tolist(), int(out[r, 0]), n):
            want_out[r, 0] = fb
            bans += 1
        if L < cap:
            want_hist[r, L] = want_out[r, 0]
    got_h = hbuf.cpu().numpy()
    np.testing.assert_array_equal(obuf.cpu().numpy(), want_out)
    np.testing.assert_array_equal(got_h[:R * cap].reshape(R, cap), want_hist)
    np.testing.assert_array_equal(lbuf.cpu().numpy()[:R], want_len)
    assert (got_h[R * cap:] == -7).all() and (lbuf.cpu().numpy()[R:] == -7).all()       # nothing past the end
    assert bans >= 8 and bans < R
    with pytest.raises(RuntimeError):
        check(lib.ua2_ngram_filter(obuf.data_ptr(), ld, R, 17, fb, hbuf.data_ptr(), lbuf.data_ptr(), cap, ops.stream()), "n=17")


# ---- 2. the generator against the reference's golden --------------------------------------------------------------------------
def test_generate_asr_with_ngram_sampling_fp32_equals_reference_golden(golden, sd):
    from helpers import build_toy_module
    from uniaudio2_amd.evaluation.asr_task import Generator
    d, meta = golden
    m = build_toy_module()
    m.load_state_dict(sd)
    m = m.to("cuda").float()
    gen = Generator(m, TA, text_tokenizer_path="ids")
    for case in meta["cases"]:
        name = case["name"]
        tokens, mask = _prompt(golden, name)
        tp, rt, st = torch.tensor([128000, 1, 128001]), torch.zeros(2, 8), torch.zeros(3, 8)
        # the golden's prompt stands in for prepare_asr_task's layout of (task prompt, reason, semantic)
        gen.prepare_asr_task = lambda a, b, c: (tokens, mask) if (a is tp and b is rt and c is st) else None
        text = gen.generate_asr_with_ngram_sampling(tp, "asr", semantic_token=st, reason_token=rt, topk=1,
                                                    no_repeat_ngram_size=case["n"], fallback_token=meta["fallback"])
        ids = [int(t) for t in text.split()]
        k = _decided_prefix(golden, name)
        assert len(ids) == 500                                             # no EOS in the toy vocabulary: the loop's 500 frames
        assert ids[:k] == d[f"{name}_final"][:k].tolist(), name
        assert (d[f"{name}_cand"][:k] != d[f"{name}_final"][:k]).any(), name   # a ban inside the compared frames
        assert m._ngram is None                                            # the filter is off after the loop
        assert not _repeats(ids, case["n"], meta["fallback"]), name


# ---- 3. device loop == host replay ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", [2, 3])
def test_device_loop_equals_host_replay(golden, sd, dtype, n):
    prompts = [_prompt(golden, "ng3"), _prompt(golden, "ng3b"), _asr_prompt(31, 4, 11), _asr_prompt(32, 7, 6)]
    frames = 40
    solo = []
    m = build_product_model(sd, dtype, batch=4)
    for t, k in prompts:
        want = host_replay(m, t[None], k[None], frames, n, FALLBACK)[:, 0].tolist()
        got = device_loop(m, [(t, k)], frames, n)[0]
        assert got == want
        solo.append(got)
    assert any(FALLBACK in s for s in solo)                                # bans fired
    assert device_loop(m, prompts, frames, n) == solo                      # B = 4, different prompts: each row = its solo run


# ---- 4. retire_rows in the middle of the loop ----------------------------------------------------------------------------------
def test_retire_rows_keeps_the_survivors_histories(golden, sd):
    prompts = [_prompt(golden, "ng3"), _asr_prompt(41, 5, 9), _prompt(golden, "ng3b"), _asr_prompt(42, 6, 8)]
    m = build_product_model(sd, torch.bfloat16, batch=4)
    solo = [device_loop(m, [p], 48, 3)[0] for p in prompts]
    got = device_loop(m, prompts, 48, 3, retire=(16, [3, 1]))
    assert got[3] == solo[3] and got[1] == solo[1]
    assert len(got[0]) == 16 and got[0] == solo[0][:16] and got[2] == solo[2][:16]


# ---- 5. sampling ---------------------------------------------------------------------------------------------------------------
def test_sampling_never_repeats_an_ngram_and_is_reproducible(golden, sd):
    prompts = [_prompt(golden, "ng2"), _asr_prompt(51, 4, 10)]
    m = build_product_model(sd, torch.float32, batch=2)
    runs = []
    for _ in range(2):
        m.set_sampling(1)
        m.set_sampling(4, 1.0, seed=1234)                                  # a new key rewinds the draw index
        runs.append(device_loop(m, prompts, 64, 2, capacity=64))
    m.set_sampling(1)
    assert runs[0] == runs[1]
    for ids in runs[0]:
        assert not _repeats(ids, 2, FALLBACK)
    assert runs[0][0] != runs[0][1]


# ---- 6. the graph cache follows the filter -----------------------------------------------------------------------------------
def test_greedy_ngram_greedy_on_one_model(golden, sd):
    p = [_prompt(golden, "ng2")]
    m = build_product_model(sd, torch.float32, batch=1)
    plain1 = device_loop(m, p, 48, 0)
    ng = device_loop(m, p, 48, 2)
    plain2 = device_loop(m, p, 48, 0)
    fresh = device_loop(build_product_model(sd, torch.float32, batch=1), p, 48, 2)
    assert plain1 == plain2 and ng == fresh and ng != plain1
    k = _decided_prefix(golden, "ng2")
    assert ng[0][:k] == golden[0]["ng2_final"][:k].tolist()
    # a call that would push the history past its capacity is refused before it runs; so is n > 16
    m.begin_ragged([(t.cuda(), k_.cuda()) for t, k_ in p])
    m.set_ngram(3, FALLBACK, capacity=20)
    m.generate_frames(16, 1, 1)
    with pytest.raises(ValueError, match="n-gram history"):
        m.generate_frames(8, 1, 1)
    m.generate_frames(4, 1, 1)
    with pytest.raises(ValueError):
        m.set_ngram(17)
    m.set_ngram(0)
    m.generate_frames(8, 1, 1)                                             # off: no history, no limit


def test_standalone_feedback_filters_text_mode_only(sd):
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import check, lib
    m = build_product_model(sd, torch.float32, batch=1)
    st = m._st
    m.set_ngram(3, FALLBACK, capacity=8)
    for mode, want in ((0, 7), (1, FALLBACK)):
        st["ngram_hist"][0, :5] = torch.tensor([5, 6, 7, 5, 6], dtype=torch.int32)
        st["ngram_len"][0] = 5
        st["out_tokens"][0] = torch.tensor([7] + [1] * 8, dtype=torch.int32)
        check(lib.ua2_stage3_feedback(m._h, 1, mode, -1, 0, ops.stream()), "ua2_stage3_feedback")
        torch.cuda.synchronize()
        assert int(st["tokens"][0, -1]) == want and int(st["out_tokens"][0, 0]) == want
        assert int(st["ngram_len"][0]) == (6 if mode == 1 else 5)
    assert int(st["ngram_hist"][0, 5]) == FALLBACK
    m.set_ngram(0)


# ---- 7. released size ---------------------------------------------------------------------------------------------------------
def test_fullsize_bf16_device_loop_equals_host_replay():
    import bench
    dev = torch.device("cuda")
    m = bench.build_model(dev, seed=0)
    B, frames, n = 32, 32, 2
    g = torch.Generator().manual_seed(77)
    L = 40
    t = torch.zeros(B, L, 9, dtype=torch.long)
    k = torch.zeros(B, L, 9, dtype=torch.bool)
    t[:, :10, -1] = torch.randint(0, 128000, (B, 10), generator=g); k[:, :10, -1] = True
    t[:, 10:, :8] = torch.randint(0, bench.REASON_CARD + bench.SEM_CARD, (B, L - 10, 8), generator=g); k[:, 10:, :8] = True
    m.setup_caches(B, dtype=torch.bfloat16, max_seq_length=256, max_rows=B * (L - 1), log_frames=frames + 8)
    # random weights at this size hardly repeat themselves within 32 frames: every row starts from the history [7, c0, 7], where c0
    # is the row's first greedy id, so that its first frame is banned and the loop continues from the fallback id
    c0 = host_replay(m, t, k, 1, 0, 128000)[0].tolist()
    init = [[7, c, 7] for c in c0]
    want = host_replay(m, t, k, frames, n, 128000, init=init)              # (F, B)
    assert (want[0] == 128000).all()
    got = device_loop(m, [(t[b], k[b]) for b in range(B)], frames, n, fallback=128000, init=init)
    assert got == want.T.tolist()
    one = device_loop(m, [(t[0], k[0])], frames, n, fallback=128000, init=init[:1])[0]
    assert one == want[:, 0].tolist()
    print(f"  full size: {int((want == 128000).sum())} fallback ids in {B} x {frames} frames")
