"""ua2_sample_topk_rows (per-row sampler streams) against ONE-ROW launches of the existing ua2_sample_topk with the row's key in
the device seed word and its draw index in the counter: the reference of every comparison is the entry point this change leaves
alone, never the new code against itself."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

CE, EMB_OFF, STREAM_ID = 8, 3, 4
KEYS = [0x0123456789ABCDEF, 7, 0xFFFFFFFFFFFFFFFF, 0x80000000, 0xDEADBEEF00000001]
DRAWS = [0, 1, 2 ** 31 - 1, 2, 1]


def _s32(x):
    return x - (1 << 32) if x >= (1 << 31) else x


def _words(k):
    return [_s32(k & 0xFFFFFFFF), _s32(k >> 32)]


def _case(V, seed):
    """Rows 0-4: random logits, distinct keys, draws in {0, 1, 2, 2^31 - 1}; 5: a tie at the k-th value for every topk (pairs of
    equal values all the way down); 6: a forbid prefix that leaves one column; 7: all -inf (the fallback id: its first admitted
    column); 8: a copy of row 1 — logits, key and draw."""
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn(9, V, generator=g) * 0.7
    lg[2, ::4] = float("-inf")
    lg[5] = (torch.arange(V) // 2).float()[torch.randperm(V, generator=g)] * 0.05
    lg[7] = float("-inf")
    lg[8] = lg[1]
    forbid = torch.tensor([0, 3, 0, V // 2, 1, 0, V - 1, 2, 3], dtype=torch.int32)
    keys = KEYS + [11, 12, 13, KEYS[1]]
    draws = DRAWS + [5, 6, 7, DRAWS[1]]
    return lg, forbid, keys, draws


def _emb(V, dtype):
    g = torch.Generator().manual_seed(5)
    return torch.randn(V + EMB_OFF, CE, generator=g).to(dtype).cuda()


def _rows(code, lg, forbid, keys, draws, topk, T, emb):
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import check, lib
    M, V = lg.shape
    out = torch.full((M, 2), -1, dtype=torch.int32, device="cuda")
    nh = torch.zeros(M, CE, device="cuda")
    rk = torch.tensor([_words(k) for k in keys], dtype=torch.int32, device="cuda")
    rd = torch.tensor(draws, dtype=torch.int32, device="cuda")
    fb = forbid.cuda()
    check(lib.ua2_sample_topk_rows(code, M, lg.data_ptr(), V, V, topk, C.c_float(T), fb.data_ptr(), rk.data_ptr(), rd.data_ptr(), STREAM_ID,
                                   out.data_ptr(), 2, 1, emb.data_ptr(), EMB_OFF, CE, nh.data_ptr(), ops.stream()), "ua2_sample_topk_rows")
    assert torch.equal(rd.cpu(), torch.tensor(draws, dtype=torch.int32))          # the sampler reads the draws, it never advances them
    assert bool((out[:, 0] == -1).all())                                          # out_col 1 of out_ld 2 only
    return out[:, 1].cpu(), nh.cpu()


def _single(code, lg, forbid, keys, draws, topk, T, emb):
    """Row by row through the existing entry point: M = 1, by-value seed 0, counter = [draw, key lo, key hi]."""
    from uniaudio2_amd import ops
    from uniaudio2_amd._lib import check, lib
    M, V = lg.shape
    ids, nhs = [], []
    for m in range(M):
        row = lg[m:m + 1].contiguous()
        out = torch.full((1, 1), -1, dtype=torch.int32, device="cuda")
        nh = torch.zeros(1, CE, device="cuda")
        counter = torch.tensor([draws[m]] + _words(keys[m]), dtype=torch.int32, device="cuda")
        fb = forbid[m:m + 1].cuda()
        check(lib.ua2_sample_topk(code, 1, row.data_ptr(), V, V, topk, C.c_float(T), fb.data_ptr(), 0, counter.data_ptr(), STREAM_ID,
                                  out.data_ptr(), 1, 0, emb.data_ptr(), EMB_OFF, CE, nh.data_ptr(), 0, ops.stream()), "ua2_sample_topk")
        ids.append(out.cpu()[0, 0])
        nhs.append(nh.cpu()[0])
    return torch.stack(ids), torch.stack(nhs)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("V", [37, 1030])
def test_rows_equal_one_row_launches_of_the_shared_form(V, dtype):
    from uniaudio2_amd import ops
    code, T = ops.dtype_code(dtype), 0.9
    lg, forbid, keys, draws = _case(V, V)
    lg = lg.cuda()
    emb = _emb(V, dtype)
    for topk in (2, 5, V):
        ids, nh = _rows(code, lg, forbid, keys, draws, topk, T, emb)
        want, want_nh = _single(code, lg, forbid, keys, draws, topk, T, emb)
        assert torch.equal(ids, want), (topk, ids.tolist(), want.tolist())
        assert torch.equal(nh, want_nh), topk
        assert torch.equal(nh, emb[(ids.long() + EMB_OFF).cuda()].float().cpu())  # the gather is of the id that was written
        assert bool((ids >= forbid).all()) and bool((ids < V).all())
        assert int(ids[6]) == V - 1 and int(ids[7]) == 2                          # the single column; the all -inf row's fallback
        assert int(ids[8]) == int(ids[1])                                         # equal key, draw and logits: equal ids
        # permuting the rows permutes the ids
        perm = torch.tensor([4, 7, 0, 8, 2, 6, 1, 5, 3])
        pid, _ = _rows(code, lg[perm.cuda()].contiguous(), forbid[perm], [keys[i] for i in perm], [draws[i] for i in perm], topk, T, emb)
        assert torch.equal(pid, ids[perm]), topk
        # a row's key and draw are inputs: the next draw index moves some row (and equals the shared form at that index)
        nxt = [d + 1 if d < 2 ** 31 - 1 else 0 for d in draws]
        nid, _ = _rows(code, lg, forbid, keys, nxt, topk, T, emb)
        assert torch.equal(nid, _single(code, lg, forbid, keys, nxt, topk, T, emb)[0]), topk
        assert not torch.equal(nid, ids), topk


def test_rows_reject_bad_arguments():
    from uniaudio2_amd._lib import lib
    x = torch.zeros(4, 8, device="cuda")
    i = torch.zeros(8, dtype=torch.int32, device="cuda")
    call = lambda topk, T, rk: lib.ua2_sample_topk_rows(0, 4, x.data_ptr(), 8, 8, topk, C.c_float(T), None, rk, i.data_ptr(), 0, i.data_ptr(),
                                                        1, 0, None, 0, 0, None, None)
    assert call(9, 1.0, i.data_ptr()) != 0 and call(2, 0.0, i.data_ptr()) != 0 and call(2, 1.0, None) != 0
