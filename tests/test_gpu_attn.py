"""GPU parity of the MFMA flash form of ua2_attn (prefill, dense encoders / DiT): against a torch fp32 softmax(q k^T) v on
the bf16 cache contents, against the row-by-row kernel (same arithmetic contract), and bit-for-bit invariance of a row's
result under re-grouping of the query rows.
The row-by-row (decode) form on its own — fp32 caches, windows, ring caches, every group size — is in tests/test_gpu_attn_decode.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _setup(nh, nkv, hs, lens, seed=0, causal=True):
    """A paged bf16 cache filled for sequences of the given lengths + one query row per (sequence, position)."""
    from uniaudio2_amd import ops
    g = torch.Generator().manual_seed(seed)
    B, maxp = len(lens), (max(lens) + 63) // 64
    k = torch.zeros(B * maxp, nkv, 64, hs, dtype=torch.bfloat16)
    v = torch.zeros_like(k)
    table = torch.randperm(B * maxp, generator=g).to(torch.int32).view(B, maxp)          # scattered pages
    K = [torch.randn(L, nkv, hs, generator=g) for L in lens]
    V = [torch.randn(L, nkv, hs, generator=g) for L in lens]
    for b, L in enumerate(lens):
        for t in range(L):
            pg = int(table[b, t // 64])
            k[pg, :, t % 64] = K[b][t].to(torch.bfloat16)
            v[pg, :, t % 64] = V[b][t].to(torch.bfloat16)
    pos = torch.cat([torch.arange(L) if causal else torch.full((L,), L - 1) for L in lens]).to(torch.int32)
    seq = torch.cat([torch.full((L,), b) for b, L in enumerate(lens)]).to(torch.int32)
    perm = torch.randperm(pos.numel(), generator=g)                                       # rows in arbitrary order
    pos, seq = pos[perm].contiguous(), seq[perm].contiguous()
    q = torch.randn(pos.numel(), nh * hs, generator=g)
    kc, vc, tc = k.cuda(), v.cuda(), table.cuda()
    geom = ops.kv_geom(kc, vc, tc, nh, nkv, hs)
    # fp32 reference on the bf16-rounded K/V
    ref = torch.zeros_like(q)
    G = nh // nkv
    for r in range(pos.numel()):
        b, p = int(seq[r]), int(pos[r])
        kk, vv = K[b][:p + 1].to(torch.bfloat16).float(), V[b][:p + 1].to(torch.bfloat16).float()
        for h in range(nh):
            s = (kk[:, h // G] @ q[r, h * hs:(h + 1) * hs]) / hs ** 0.5
            ref[r, h * hs:(h + 1) * hs] = torch.softmax(s, 0) @ vv[:, h // G]
    return dict(q=q.cuda(), pos=pos.cuda(), seq=seq.cuda(), geom=geom, keep=(kc, vc, tc), ref=ref, pos_h=pos, seq_h=seq)


@pytest.mark.parametrize("nh,nkv,hs,lens,causal", [(24, 8, 128, [196, 33, 70], True), (4, 2, 64, [12, 9, 130], True),
                                                   (24, 24, 64, [150, 150], False), (6, 6, 128, [90], False), (4, 2, 32, [67], True)])
def test_flash_attention_vs_torch_and_row_kernel(nh, nkv, hs, lens, causal):
    from uniaudio2_amd import ops
    s = _setup(nh, nkv, hs, lens, causal=causal)
    R = s["q"].shape[0]
    y_row = torch.empty_like(s["q"])
    ops.attn(dtype=torch.bfloat16, R=R, q=s["q"], row_pos=s["pos"], row_seq=s["seq"], kv=s["geom"], y=y_row)
    groups = ops.attn_groups(s["pos_h"].numpy(), s["seq_h"].numpy(), nh, nkv, "cuda")
    y = torch.empty_like(s["q"])
    ops.attn(dtype=torch.bfloat16, R=R, q=s["q"], row_pos=s["pos"], row_seq=s["seq"], kv=s["geom"], y=y, groups=groups)
    err = float((y.cpu() - s["ref"]).abs().max())
    err_row = float((y_row.cpu() - s["ref"]).abs().max())
    print(f"flash vs torch fp32: {err:.2e}; row-by-row kernel vs torch: {err_row:.2e}; flash vs row kernel: {float((y - y_row).abs().max()):.2e}")
    assert err < 2e-4 and float((y - y_row).abs().max()) < 2e-4


def test_flash_attention_eight_query_tiles_equal_four():
    """The dense (multi-head, head size 64) form the DiT uses takes 128 query rows per workgroup since round 4; a row's
    bits do not depend on how many rows share its workgroup."""
    from uniaudio2_amd import ops
    s = _setup(24, 24, 64, [150, 150, 77], causal=False, seed=5)
    R = s["q"].shape[0]
    outs = []
    for qt in (4, 8):
        groups = ops.attn_groups(s["pos_h"].numpy(), s["seq_h"].numpy(), 24, 24, "cuda", q_tiles=qt)
        assert groups[3] == qt and groups[0].shape[1] == qt * 16
        y = torch.zeros_like(s["q"])
        ops.attn(dtype=torch.bfloat16, R=R, q=s["q"], row_pos=s["pos"], row_seq=s["seq"], kv=s["geom"], y=y, groups=groups)
        outs.append(y)
    assert torch.equal(outs[0], outs[1])
    assert float((outs[1].cpu() - s["ref"]).abs().max()) < 2e-4


def test_flash_attention_bf16_q_and_weights_form():
    """UA2_ATTN_BF16_QP (the DiT's order-free plan): q and the softmax weights rounded to bf16 once, as torch SDPA under bf16
    autocast does — half the matrix work.  Against the fp32-grade form and the torch fp32 softmax: bf16-level agreement
    (2^-8 relative on the weights: the bar is 1e-2 on unit-scale outputs), deterministic, padding rows untouched; and the
    unmasked fast path of fully visible key blocks leaves the fp32-grade form's bits where they were (causal and dense)."""
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import ATTN_BF16_QP
    s = _setup(24, 24, 64, [150, 150, 77], causal=False, seed=5)
    R = s["q"].shape[0]
    groups = ops.attn_groups(s["pos_h"].numpy(), s["seq_h"].numpy(), 24, 24, "cuda", q_tiles=8)
    outs = []
    for flags in (0, ATTN_BF16_QP, ATTN_BF16_QP):
        y = torch.zeros_like(s["q"])
        ops.attn(dtype=torch.bfloat16, R=R, q=s["q"], row_pos=s["pos"], row_seq=s["seq"], kv=s["geom"], y=y, groups=groups, flags=flags)
        outs.append(y)
    assert torch.equal(outs[1], outs[2]) and not torch.equal(outs[0], outs[1])
    err = float((outs[1].cpu() - s["ref"]).abs().max())
    print(f"flash, bf16 q / weights vs torch fp32: {err:.2e} (fp32-grade form: {float((outs[0].cpu() - s['ref']).abs().max()):.2e})")
    assert err < 1e-2
    # the flag is ignored where the form is not built (4 query tiles): the fp32-grade bits
    g4 = ops.attn_groups(s["pos_h"].numpy(), s["seq_h"].numpy(), 24, 24, "cuda", q_tiles=4)
    y4 = torch.zeros_like(s["q"])
    ops.attn(dtype=torch.bfloat16, R=R, q=s["q"], row_pos=s["pos"], row_seq=s["seq"], kv=s["geom"], y=y4, groups=g4, flags=ATTN_BF16_QP)
    assert torch.equal(y4, outs[0])


@pytest.mark.parametrize("lens,causal", [([500, 129], False), ([200, 64, 65], True), ([1], False)])
def test_flash_attention_bf16_form_two_pages_per_iteration(lens, causal):
    """The DiT's instantiation walks 128 keys per loop iteration (round 6): whole pairs of pages, an odd last page (its partner re-reads
    the last page and is masked), a single key, causal rows whose last visible key falls anywhere inside a pair — against the torch
    fp32 softmax, at the bf16-weights bar."""
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import ATTN_BF16_QP
    s = _setup(24, 24, 64, lens, causal=causal, seed=11)
    R = s["q"].shape[0]
    groups = ops.attn_groups(s["pos_h"].numpy(), s["seq_h"].numpy(), 24, 24, "cuda", q_tiles=8)
    y = torch.full_like(s["q"], float("nan"))
    ops.attn(dtype=torch.bfloat16, R=R, q=s["q"], row_pos=s["pos"], row_seq=s["seq"], kv=s["geom"], y=y, groups=groups, flags=ATTN_BF16_QP)
    err = float((y.cpu() - s["ref"]).abs().max())
    assert err < 1e-2, err


def test_flash_attention_rows_do_not_depend_on_the_grouping():
    """Re-grouping the query rows (other tile compositions, padded groups, one row per group) leaves every row's bits
    unchanged: chunked prefill == one-pass prefill, a prompt alone == the same prompt inside a ragged batch."""
    from uniaudio2_amd import ops
    s = _setup(24, 8, 128, [100, 37], seed=3)
    R = s["q"].shape[0]
    pos, seq = s["pos_h"].numpy(), s["seq_h"].numpy()

    def run(groups):
        y = torch.zeros_like(s["q"])
        ops.attn(dtype=torch.bfloat16, R=R, q=s["q"], row_pos=s["pos"], row_seq=s["seq"], kv=s["geom"], y=y, groups=groups)
        return y

    base = run(ops.attn_groups(pos, seq, 24, 8, "cuda"))
    # (i) one row per group
    rows = torch.full((R, 32), -1, dtype=torch.int32)
    rows[:, 0] = torch.arange(R)
    single = (rows.cuda(), s["seq"].clone(), (s["pos"] + 1).to(torch.int32), 2)
    assert torch.equal(run(single), base)
    # (ii) rows of a sequence in reversed order, groups of 7 live rows scattered over the 32 slots
    order = np.lexsort((-pos, seq))
    rows, gseq, nkeys = [], [], []
    for c in range(0, R, 7):
        idx = order[c:c + 7]
        for sq in np.unique(seq[idx]):
            sel = idx[seq[idx] == sq]
            slot = np.full(32, -1)
            slot[np.arange(len(sel)) * 4 + 1] = sel
            rows.append(slot); gseq.append(sq); nkeys.append(int(pos[sel].max()) + 1)
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int32)).cuda()
    assert torch.equal(run((t(np.stack(rows)), t(gseq), t(nkeys), 2)), base)


def test_row_kernel_two_per_cu_form_equals_the_prefetch_form():
    """Round 6: launches of the row-by-row kernel with more workgroups than CUs (R * n_kv > 256) take the 128-register form without
    the one-step K / V prefetch (two workgroups per CU); fewer take the prefetch form.  Same arithmetic in the same order: a row's
    bits must not depend on which form its launch took — the whole batch in one launch against its rows in launches of 8."""
    from uniaudio2_amd import ops
    s = _setup(24, 8, 128, [196, 33, 70, 5, 64, 65], seed=3)
    R = s["q"].shape[0]
    assert R * 8 > 256
    y_all = torch.empty_like(s["q"])
    ops.attn(dtype=torch.bfloat16, R=R, q=s["q"], row_pos=s["pos"], row_seq=s["seq"], kv=s["geom"], y=y_all)
    y_few = torch.empty_like(s["q"])
    for r0 in range(0, R, 8):
        n = min(8, R - r0)                                              # 8 rows x 8 kv heads = 64 workgroups: the prefetch form
        ops.attn(dtype=torch.bfloat16, R=n, q=s["q"][r0:r0 + n].contiguous(), row_pos=s["pos"][r0:r0 + n].contiguous(),
                 row_seq=s["seq"][r0:r0 + n].contiguous(), kv=s["geom"], y=y_few[r0:r0 + n])
    assert torch.equal(y_all, y_few)
    assert float((y_all.cpu() - s["ref"]).abs().max()) < 2e-4
