"""B = 1 greedy frames without arg-max launches inside the depth decoder (ua2_stage3.hip; opt-out UA2_NO_ARGMAX_FOLD=1, read when a
plan is created): the arg-max + table gather after a codebook step is done by layer 0's O-projection of the next step (ua2_argmax_fold
of ua2_linear_args, the UA2_PRO_LOCAL_ATTN prologue), the last step's arg-max by feedback_kernel's block.

Op level: the folded launch against the stand-alone greedy tail (ua2_argmax_embed: the same ua2_row_token rule) followed by the table
gathers (plain copies, done here in torch as argmax_gather_kernel does them) and today's launch on those buffers — every output bit
for bit.  Frame level: two plans in one process — fold on, fold off, the latter running argmax_gather_kernel itself — must agree bit
for bit on everything a frame leaves behind, the folded plan must issue exactly eight arg-max launches per frame fewer, and frames of
more rows must not change at all."""
import pytest
import torch

from helpers import build_product_model, load_golden_lm, toy_state_dict

pytestmark = pytest.mark.gpu

FRAMES = 12


def _partials(kind, n_part, seed):
    """(part_max, part_idx) [1, n_part] as audio_head's STORE epilogue writes them: partial p holds the best (value, column) of columns
    16 p .. 16 p + 15; a tile below forbid_prefix holds (-inf, its first column)."""
    g = torch.Generator().manual_seed(seed)
    pm = torch.randn(n_part, generator=g)
    pi = torch.arange(n_part, dtype=torch.int32) * 16 + torch.randint(0, 16, (n_part,), generator=g, dtype=torch.int32)
    a, b = n_part // 3, n_part - 1                             # two distinct partials (n_part >= 5)
    if kind == "unique":
        pm[b] = 9.0
    elif kind == "tie":                                        # exact tie across two partials: the lower index (partial a) must win
        pm[a] = pm[b] = 9.0
    elif kind == "forbid_tie":                                 # forbidden tiles in front, the maximum tied with the first allowed tile
        nf = max(1, n_part // 4)
        pm[:nf] = float("-inf")
        pi[:nf] = torch.arange(nf, dtype=torch.int32) * 16
        pm[nf] = pm[b] = 9.0
    elif kind == "all_neg_inf":                                # every column forbidden: lowest index
        pm[:] = float("-inf")
        pi[:] = torch.arange(n_part, dtype=torch.int32) * 16
    elif kind == "all_nan":                                    # nobody wins: the fallback branch (lowest candidate id)
        pm[:] = float("nan")
    return pm.view(1, -1).cuda(), pi.view(1, -1).cuda()


@pytest.mark.parametrize("kind", ["unique", "tie", "forbid_tie", "all_neg_inf", "all_nan"])
@pytest.mark.parametrize("n_part", [5, 64, 65, 769])
@pytest.mark.parametrize("Cd,hs", [(128, 32), (256, 64), (256, 32), (128, 64)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_folded_launch_equals_argmax_then_gather_then_launch(dtype, Cd, hs, n_part, kind):
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import EPI_RESIDUAL, PRO_LOCAL_ATTN
    dev = torch.device("cuda")
    nkv, nh = 2, Cd // hs
    qn, kvw, limit, row_off = nh * hs, nkv * hs, 16 * n_part, 7
    rows = limit + row_off
    g = torch.Generator().manual_seed(Cd + hs + n_part)
    tab_y = torch.randn(rows, Cd, generator=g).to(dev)
    tab_q = torch.randn(rows, qn, generator=g).to(dev)
    tab_k = torch.randn(rows, kvw, generator=g).to(device=dev, dtype=dtype)
    tab_v = torch.randn(rows, kvw, generator=g).to(device=dev, dtype=dtype)
    w = ops.pack_linear((torch.randn(Cd, qn, generator=g) * qn ** -0.5).to(dev), dtype)
    norm_w = torch.randn(Cd, generator=g).to(dev)
    kp0 = torch.randn(3, nkv, 64, hs, generator=g).to(device=dev, dtype=dtype)      # three pages, the sequence's is page 2
    vp0 = torch.randn(3, nkv, 64, hs, generator=g).to(device=dev, dtype=dtype)
    pt = torch.tensor([[2]], dtype=torch.int32, device=dev)
    pm, pi = _partials(kind, n_part, seed=n_part)
    ho = dtype == torch.bfloat16                                                    # the scaled-norm hand-over is a bf16 contract
    for pos in range(1, 8):
        posd = torch.tensor([pos], dtype=torch.int32, device=dev)

        def launch(kp, vp, x, resid, fold):
            y = torch.full((1, Cd), float("nan"), device=dev)
            yh = torch.zeros(1, Cd, dtype=torch.bfloat16, device=dev)
            ssq = torch.full((1, Cd // 16), float("nan"), device=dev)
            ops.linear(dtype=dtype, M=1, N=Cd, K=qn, w0=w, prologue=PRO_LOCAL_ATTN, epilogue=EPI_RESIDUAL, x=x, y=y, resid=resid, row_pos=posd,
                       kv=ops.kv_geom(kp, vp, pt, nh, nkv, hs), fold=fold,
                       **(dict(y_norm_w=norm_w, y_h=yh, y_ssq=ssq) if ho else {}))
            torch.cuda.synchronize()
            return y, yh, ssq

        # reference: the stand-alone tail, the gathers, today's launch
        tok_ref = torch.full((1, 1), -1, dtype=torch.int32, device=dev)
        ops.argmax_embed(dtype, pm, pi, tok_ref, 0)
        torch.cuda.synchronize()
        t = int(tok_ref[0, 0])
        assert 0 <= t < limit
        row = t + row_off
        kp_r, vp_r = kp0.clone(), vp0.clone()
        kp_r[2, :, pos] = tab_k[row].view(nkv, hs)
        vp_r[2, :, pos] = tab_v[row].view(nkv, hs)
        y_r, yh_r, ssq_r = launch(kp_r, vp_r, tab_q[row:row + 1].contiguous(), tab_y[row:row + 1].contiguous(), None)
        # folded: x and resid are not read (poisoned), the cache row of `pos` is not there yet
        kp_f, vp_f = kp0.clone(), vp0.clone()
        tok = torch.full((1,), -1, dtype=torch.int32, device=dev)
        poison = torch.full((1, max(Cd, qn)), float("nan"), device=dev)
        fold = dict(part_max=pm, part_idx=pi, n_part=n_part, limit=limit, out_token=tok, row_off=row_off, pos=pos,
                    tab_y=tab_y, tab_q=tab_q, tab_k=tab_k, tab_v=tab_v)
        y_f, yh_f, ssq_f = launch(kp_f, vp_f, poison[:, :qn].contiguous(), poison[:, :Cd].contiguous(), fold)
        assert int(tok[0]) == t, (pos, int(tok[0]), t)
        assert torch.equal(y_f, y_r), pos
        if ho:
            assert torch.equal(yh_f, yh_r) and torch.equal(ssq_f, ssq_r), pos
        assert torch.equal(kp_f, kp_r) and torch.equal(vp_f, vp_r), pos            # the new row, and nothing else in the pools


@pytest.fixture(scope="module")
def golden():
    return load_golden_lm()


@pytest.fixture(scope="module")
def sd(golden):
    return toy_state_dict(golden[1])


def _argmax_launches():
    from uniaudio2_amd._lib import lib
    return lib.ua2_debug_kernel_launches(b"argmax")


def _prompt(d, case, rows):
    tokens = torch.from_numpy(d[f"{case}_tokens"]).long()
    mask = torch.from_numpy(d[f"{case}_mask"]).bool()
    if tokens.dim() == 2:
        tokens, mask = tokens[None], mask[None]
    return tokens[rows].cuda(), mask[rows].cuda()


def _run(sd, dtype, tokens, mask, monkeypatch, fold, use_graph=False):
    """FRAMES greedy audio-feedback frames, one generate_frames call per frame.  Returns the frame log, the audio_logits and h_final
    buffers after every frame, the depth decoder's cache pools after the last, and the arg-max launches the frames issued (un-graphed
    frames issue theirs every time; a captured frame counts once, at capture)."""
    monkeypatch.delenv("UA2_NO_ARGMAX_FOLD", raising=False)
    if not fold:
        monkeypatch.setenv("UA2_NO_ARGMAX_FOLD", "1")
    B, L, _ = tokens.shape
    m = build_product_model(sd, dtype, batch=B)                 # the hook is read by ua2_stage3_create: one plan per setting
    m.reset_caches()
    pos = torch.arange(0, L, device="cuda").unsqueeze(0).repeat(B, 1)
    m.forward_prefix(tokens[:, :-1], labels=tokens[:, 1:, :-1], tokens_mask=mask, loss_mask=mask, input_pos=pos[:, :-1])
    m.begin_decode(tokens[:, -1:], mask[:, -1:], torch.tensor([L - 1], device="cuda"))
    log, logits, hfin = [], [], []
    n0 = _argmax_launches()
    for _ in range(FRAMES):
        log.append(m.generate_frames(1, B, 0, use_graph=use_graph).cpu().clone())
        logits.append(m.buffer("audio_logits", B).cpu().clone())
        hfin.append(m.buffer("h_final", B).cpu().clone())
    n = _argmax_launches() - n0
    kv = m.decoder.kv_cache
    pools = [t.cpu().clone() for t in list(kv.k) + list(kv.v)]
    return dict(log=torch.cat(log), logits=logits, hfin=hfin, pools=pools, launches=n)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_last_step_argmax_inside_the_feedback_kernel(golden, sd, dtype, monkeypatch):
    d, _ = golden
    tokens, mask = _prompt(d, "tts1", slice(0, 1))
    on = _run(sd, dtype, tokens, mask, monkeypatch, fold=True)
    off = _run(sd, dtype, tokens, mask, monkeypatch, fold=False)
    assert torch.equal(on["log"], off["log"])
    assert int(on["log"][:, :, 1:].min()) >= 0                  # every audio id of every frame was written
    for f in range(FRAMES):
        assert torch.equal(on["logits"][f], off["logits"][f]), f
        assert torch.equal(on["hfin"][f], off["hfin"][f]), f
    for a, b in zip(on["pools"], off["pools"]):
        assert torch.equal(a, b)
    # whole frames (text head included): text arg-max + 7 table gathers + the last step's arg-max = 9 launches; folded: the text's only
    assert off["launches"] == 9 * FRAMES
    assert on["launches"] == 1 * FRAMES
    # the captured frame (what the generators replay) bakes the descriptors: same log, logits and caches
    rep = _run(sd, dtype, tokens, mask, monkeypatch, fold=True, use_graph=True)
    assert torch.equal(rep["log"], off["log"])
    assert torch.equal(rep["logits"][-1], off["logits"][-1])
    for a, b in zip(rep["pools"], off["pools"]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_frames_of_two_rows_keep_their_launches(golden, sd, dtype, monkeypatch):
    d, _ = golden
    tokens, mask = _prompt(d, "tts2", slice(0, 2))
    on = _run(sd, dtype, tokens, mask, monkeypatch, fold=True)
    off = _run(sd, dtype, tokens, mask, monkeypatch, fold=False)
    assert on["launches"] == off["launches"] == 9 * FRAMES
    assert torch.equal(on["log"], off["log"])
    for r in range(2):                                          # row invariance: each row's ids are those of its own B = 1 run
        one = _run(sd, dtype, tokens[r:r + 1], mask[r:r + 1], monkeypatch, fold=True)
        assert torch.equal(one["log"][:, 0], on["log"][:, r]), r
