"""Op-level Python wrappers over the C ABI (torch is only the owner of device memory and the
stream).  Each wrapper names the reference call site it stands in for; the arithmetic lives in
csrc/*.hip.  Used by the parity tests and by the module mirrors in llm_models/.
"""
import ctypes as C

import os

import torch

from . import _lib
from ._lib import (EPI_QKV_ROPE, EPI_RESIDUAL, EPI_STORE, EPI_SWIGLU, PRO_CAST, PRO_NORM, UA2_BF16,
                   UA2_F32, UA2_PAGE, AttnArgs, KvGeom, LinearArgs, check, lib)

_CODES = {torch.float32: UA2_F32, torch.bfloat16: UA2_BF16}


def dtype_code(dt):
    try:
        return _CODES[dt]
    except KeyError:
        raise ValueError(f"uniaudio2_amd supports torch.float32 and torch.bfloat16 weights, got {dt}")


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device-contiguous tensor expected"
    return t.data_ptr()


def packed_elems(dtype, N, K):
    return lib.ua2_packed_elems(dtype_code(dtype), N, K)


def pack_linear(weight, dtype, transposed=False, rope_head_size=0):
    """nn.Linear.weight [N,K] (or [K,N] with transposed=True) -> MFMA-fragment-ordered buffer of `dtype`."""
    assert weight.dim() == 2 and weight.is_cuda
    w = weight.contiguous()
    if w.dtype not in _CODES:
        w = w.float()
    N, K = (w.shape[1], w.shape[0]) if transposed else (w.shape[0], w.shape[1])
    out = torch.empty(packed_elems(dtype, N, K), dtype=dtype, device=w.device)
    check(lib.ua2_pack_linear(ptr(w), dtype_code(w.dtype), int(transposed), N, K, ptr(out), dtype_code(dtype),
                              rope_head_size, stream()), "ua2_pack_linear")
    return out


def w8_exponents(weight):
    """Per-row exponents of the fp8 weight-only contract (include/ua2hip.h): e = ceil(log2(amax / 448)) per output row of `weight`
    [N, K], 0 for an all-zero row, clamped to [-117, 120].  Computed without a logarithm: amax = m 2^x with m in [0.5, 1) and
    448 = 0.875 2^9.  Plain torch, any device."""
    amax = weight.detach().float().abs().amax(dim=1)
    m, x = torch.frexp(amax)
    e = torch.where(m <= 0.875, x - 9, x - 8)
    e = torch.where(amax > 0, e, torch.zeros_like(e))
    return e.clamp(-117, 120).to(torch.int32)


def quant_w8(weight):
    """(q, e): q [N, K] torch.float8_e4m3fn = RNE(weight * 2^-e), e [N] int32 — the quantiser of the fp8 contract in plain torch."""
    e = w8_exponents(weight)
    scaled = torch.ldexp(weight.detach().float(), -e.unsqueeze(1))
    return scaled.to(torch.float8_e4m3fn), e


def dequant_w8(weight):
    """W' = q * 2^e [N, K] fp32: the weight a plan with weight_dtype=torch.float8_e4m3fn computes with in place of `weight`
    (exactly representable in bf16).  Plain torch, any device: for tests and for looking at what the option costs."""
    q, e = quant_w8(weight)
    return torch.ldexp(q.float(), e.unsqueeze(1))


def pack_linear_w8(weight, transposed=False, rope_head_size=0):
    """nn.Linear.weight [N, K] (or [K, N] with transposed=True; K % 64 == 0) -> (q, exp, bf16_twin): the fp8 image in the decode
    kernel's burst order (uint8), the int8 exponents in packed column order (N padded to 16) and pack_linear(W', bfloat16)
    (ua2_pack_linear_w8)."""
    assert weight.dim() == 2 and weight.is_cuda
    w = weight.contiguous()
    if w.dtype not in _CODES:
        w = w.float()
    N, K = (w.shape[1], w.shape[0]) if transposed else (w.shape[0], w.shape[1])
    n16 = (N + 15) // 16 * 16
    q = torch.empty(max(lib.ua2_packed_bytes_w8(N, K), 1), dtype=torch.uint8, device=w.device)
    exp = torch.empty(n16, dtype=torch.int8, device=w.device)
    twin = torch.empty(packed_elems(torch.bfloat16, N, K), dtype=torch.bfloat16, device=w.device)
    check(lib.ua2_pack_linear_w8(ptr(w), dtype_code(w.dtype), int(transposed), N, K, ptr(q), ptr(exp), ptr(twin), rope_head_size,
                                 stream()), "ua2_pack_linear_w8")
    return q, exp, twin


def _image_refs(Ref, images):
    """The (r0, r1) ctypes arrays of `Ref` (W8Ref / L13Ref) that the launches on weight images take: images[i] = ((image, side array) of
    w0, the same of w1 or None).  r1 is None when no launch has a w1."""
    def ref(t):
        return Ref(ptr(t[0]), ptr(t[1])) if t is not None else Ref()
    n = len(images)
    r0 = (Ref * n)(*[ref(t[0]) for t in images])
    r1 = (Ref * n)(*[ref(t[1]) for t in images]) if any(t[1] is not None for t in images) else None
    return r0, r1


def linear_w8(args, w0, w1=None):
    """ua2_linear_w8: the launch `args` (ops.linear(..., launch=False); w0 / w1 = the bf16 twins) on the fp8 twins w0, w1 = (q, exp)."""
    check(lib.ua2_linear_w8(C.byref(args), *_image_refs(_lib.W8Ref, [(w0, w1)]), stream()), "ua2_linear_w8")


def linear_w8_many(args, w0, w1=None):
    """ua2_linear_w8_many: the many-row launch `args` (6 .. UA2_SKINNY_W8_MAX_ROWS rows, a workspace or x_packed; w0 / w1 = the bf16 twins)
    on the fp8 twins w0, w1 = (q, exp) through the weights-stationary kernel; raises where that kernel does not serve the launch."""
    check(lib.ua2_linear_w8_many(C.byref(args), *_image_refs(_lib.W8Ref, [(w0, w1)]), stream()), "ua2_linear_w8_many")


def pack_linear_l13(packed, N, K):
    """Packed bf16 weight (pack_linear(..., torch.bfloat16)) of an [N, K] Linear, K % 128 == 0 -> (image, base, escapes): the lossless
    13-bit image (uint8), the per-tile base bytes (uint8 [ceil(N / 16)]) and the escape count (int32 [1], on the device)
    (ua2_pack_linear_l13).  An image with escapes != 0 must not be handed to linear_l13."""
    assert packed.is_cuda and packed.dtype == torch.bfloat16 and packed.numel() == packed_elems(torch.bfloat16, N, K)
    nbytes = lib.ua2_packed_bytes_l13(N, K)
    if nbytes == 0:
        raise ValueError(f"no 13-bit image for K={K} (K % 128 != 0)")
    image = torch.empty(nbytes, dtype=torch.uint8, device=packed.device)
    base = torch.empty((N + 15) // 16, dtype=torch.uint8, device=packed.device)
    esc = torch.zeros(1, dtype=torch.int32, device=packed.device)
    check(lib.ua2_pack_linear_l13(ptr(packed), N, K, ptr(image), ptr(base), ptr(esc), stream()), "ua2_pack_linear_l13")
    return image, base, esc


def linear_l13(args, w0, w1=None):
    """ua2_linear_l13: the launch `args` (ops.linear(..., launch=False); w0 / w1 = the packed bf16 weights) on their 13-bit images
    w0, w1 = (image, base)."""
    check(lib.ua2_linear_l13(C.byref(args), *_image_refs(_lib.L13Ref, [(w0, w1)]), stream()), "ua2_linear_l13")


def kv_geom(k_pool, v_pool, page_table, n_head, n_kv, head_size, ring_pages=0):
    g = KvGeom()
    g.ring_pages = ring_pages
    g.k_pool, g.v_pool, g.page_table = ptr(k_pool), ptr(v_pool), ptr(page_table)
    g.max_pages = page_table.shape[-1] if page_table is not None else 0
    g.n_kv, g.n_head, g.head_size = n_kv, n_head, head_size
    return g


def linear(*, dtype, M, N, K, w0, prologue=PRO_CAST, epilogue=EPI_STORE, x=None, ldx=None, norm_w=None, eps=1e-5,
           w1=None, y=None, ldy=None, resid=None, ldr=None, part_max=None, part_idx=None,
           forbid=None, row_pos=None, row_seq=None, rope_cos=None, rope_sin=None, q_out=None, kv=None, launch=True,
           norm_b=None, norm_kind=0, out_scale=None, rope_mode=0, workspace=None, bias=None, bias1=None, act_kind=0,
           y_packed=None, x_packed=None, y_norm_w=None, y_h=None, ldh=0, y_ssq=None, x_h=None, x_ssq=None, split_ws=None, sum_order=0, y_ln=None, range_ws=None, fold=None):
    a = LinearArgs()
    a.dtype, a.prologue, a.epilogue = dtype_code(dtype), prologue, epilogue
    a.M, a.N, a.K = M, N, K
    # (PRO_CAST with x_h, EPI_SWIGLU with y_h: bf16 rows in x's / y's place, on x's / y's stride)
    a.x, a.ldx = ptr(x), (ldx if ldx is not None else (x.shape[-1] if x is not None else (x_h.shape[-1] if x_h is not None else 0)))
    a.norm_w, a.eps = ptr(norm_w), eps
    a.w0, a.w1 = ptr(w0), ptr(w1)
    a.y, a.ldy = ptr(y), (ldy if ldy is not None else (y.shape[-1] if y is not None else (y_h.shape[-1] if y_h is not None else 0)))
    a.resid, a.ldr = ptr(resid), (ldr if ldr is not None else (resid.shape[-1] if resid is not None else 0))
    a.part_max, a.part_idx, a.forbid = ptr(part_max), ptr(part_idx), ptr(forbid)
    a.row_pos, a.row_seq = ptr(row_pos), ptr(row_seq)
    a.rope_cos, a.rope_sin, a.q_out = ptr(rope_cos), ptr(rope_sin), ptr(q_out)
    a.norm_b, a.norm_kind, a.out_scale, a.rope_mode = ptr(norm_b), norm_kind, ptr(out_scale), rope_mode
    a.bias, a.bias1, a.act_kind = ptr(bias), ptr(bias1), act_kind
    a.y_packed, a.x_packed = ptr(y_packed), ptr(x_packed)
    a.y_norm_w, a.y_h, a.y_ssq, a.x_h, a.x_ssq = ptr(y_norm_w), ptr(y_h), ptr(y_ssq), ptr(x_h), ptr(x_ssq)
    a.ldh = ldh or (y_h.shape[-1] if y_h is not None else (x_h.shape[-1] if x_h is not None else 0))
    if workspace is not None:
        a.workspace, a.workspace_bytes = ptr(workspace), workspace.numel() * workspace.element_size()
    if split_ws is not None:
        a.split_ws, a.split_ws_bytes = ptr(split_ws), split_ws.numel() * split_ws.element_size()
    if range_ws is not None:       # scratch of the range split of row-invariant 33-64-row launches (ua2hip.h [v10]): same bits with and without
        a.range_ws, a.range_ws_bytes = ptr(range_ws), range_ws.numel() * range_ws.element_size()
    a.sum_order = sum_order
    if y_ln is not None:                 # (w, b, eps): LayerNorm hand-over of a RESIDUAL launch (ua2hip.h y_ln_w)
        a.y_ln_w, a.y_ln_b, a.y_ln_eps = ptr(y_ln[0]), ptr(y_ln[1]), float(y_ln[2])
    if kv is not None:
        a.kv = kv
    if fold is not None:                 # ua2_argmax_fold (PRO_LOCAL_ATTN): dict of its fields, tensors for the pointers
        f = a.fold
        f.part_max, f.part_idx, f.out_token = ptr(fold["part_max"]), ptr(fold["part_idx"]), ptr(fold["out_token"])
        f.n_part, f.limit, f.row_off, f.pos = fold["n_part"], fold["limit"], fold["row_off"], fold["pos"]
        f.tab_y, f.tab_q, f.tab_k, f.tab_v = ptr(fold["tab_y"]), ptr(fold["tab_q"]), ptr(fold["tab_k"]), ptr(fold["tab_v"])
    if not launch:
        return a
    check(lib.ua2_linear(C.byref(a), stream()), "ua2_linear")


def linear_workspace(dtype, M, K, device):
    """Scratch that lets ua2_linear take its large-M kernel for up to M rows of width K."""
    n = lib.ua2_linear_workspace_bytes(dtype_code(dtype), M, K)
    return torch.empty(n, dtype=torch.uint8, device=device)


def linear_chain_timed(args_list, iters):
    """Average milliseconds per launch of the given ua2_linear launches, back to back, HIP-event timed."""
    arr = (LinearArgs * len(args_list))(*args_list)
    ms = C.c_float(0.0)
    check(lib.ua2_linear_chain_timed(arr, len(args_list), iters, stream(), C.byref(ms)), "ua2_linear_chain_timed")
    return ms.value / (len(args_list) * iters)


def linear_l13_chain_timed(args_list, images, iters):
    """Average milliseconds per launch of the given launches through ua2_linear_l13, back to back, HIP-event timed: the image side of
    linear_chain_timed (same host path).  images[i] = ((image, base) of w0, (image, base) of w1 or None)."""
    n = len(args_list)
    arr = (LinearArgs * n)(*args_list)
    r0, r1 = _image_refs(_lib.L13Ref, images)
    ms = C.c_float(0.0)
    check(lib.ua2_linear_l13_chain_timed(arr, r0, r1, n, iters, stream(), C.byref(ms)), "ua2_linear_l13_chain_timed")
    return ms.value / (n * iters)


def linear_w8_many_chain_timed(args_list, twins, iters):
    """Average milliseconds per launch of the given launches through ua2_linear_w8_many, back to back, HIP-event timed: the fp8 side of
    linear_chain_timed (same host path).  twins[i] = ((q, exp) of w0, (q, exp) of w1 or None)."""
    n = len(args_list)
    arr = (LinearArgs * n)(*args_list)
    r0, r1 = _image_refs(_lib.W8Ref, twins)
    ms = C.c_float(0.0)
    check(lib.ua2_linear_w8_many_chain_timed(arr, r0, r1, n, iters, stream(), C.byref(ms)), "ua2_linear_w8_many_chain_timed")
    return ms.value / (n * iters)


def attn_groups(pos, seq, n_head, n_kv, device, q_tiles=None):
    """Row groups for the MFMA flash form of ua2_attn: pos, seq = host int sequences (position and page-table row of every
    query row of the launch).  Rows of one sequence, ordered by position, are cut into groups of q_tiles * 16
    (q_tiles = 2 with grouped-query heads, 4 otherwise; a caller whose head size has the wider instantiation may ask for 8:
    twice the query rows per staged K / V page).  -> (rows [n, q_tiles*16] int32, seq [n], nkeys [n], q_tiles), device."""
    import numpy as np
    pos, seq = np.asarray(pos, dtype=np.int64), np.asarray(seq, dtype=np.int64)
    qt = q_tiles or (2 if n_head > n_kv else 4)
    if n_head == n_kv and os.environ.get("UA2_ATTN_QTILES"):   # experiment hook (a row's bits do not depend on the grouping)
        qt = int(os.environ["UA2_ATTN_QTILES"])
    per = qt * 16
    order = np.lexsort((pos, seq))
    rows, gseq, nkeys = [], [], []
    start = 0
    while start < len(order):
        s0 = seq[order[start]]
        end = start
        while end < len(order) and seq[order[end]] == s0:
            end += 1
        for c in range(start, end, per):
            idx = order[c:min(c + per, end)]
            rows.append(np.concatenate([idx, np.full(per - len(idx), -1)]))
            gseq.append(s0)
            nkeys.append(int(pos[idx].max()) + 1)
        start = end
    to = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int32)).to(device)
    return to(np.stack(rows)).contiguous(), to(gseq), to(nkeys), qt


def attn(*, dtype, R, q, row_pos, row_seq, kv, y=None, window=0, groups=None, y_packed=None, flags=0, y_h=None):
    """y [R, n_head*hs] fp32 and / or y_packed: the same rows already in ua2_linear's operand order (its consumer then takes
    them as x_packed and needs no prep launch); y_h [R, ldh] bf16: the same rows row-major (the x_h of a one-row-tile O-projection)."""
    a = AttnArgs()
    a.y_h, a.ldh = ptr(y_h), (y_h.shape[-1] if y_h is not None else 0)
    a.flags = flags
    a.y_packed = ptr(y_packed)
    if groups is not None:
        a.group_rows, a.group_seq, a.group_nkeys = ptr(groups[0]), ptr(groups[1]), ptr(groups[2])
        a.n_groups, a.group_q_tiles = groups[0].shape[0], groups[3]
    a.y = ptr(y)
    a.window = window
    a.dtype, a.R = dtype_code(dtype), R
    a.q, a.row_pos, a.row_seq = ptr(q), ptr(row_pos), ptr(row_seq)
    a.kv = kv
    check(lib.ua2_attn(C.byref(a), stream()), "ua2_attn")


def attn_local(*, dtype, R, q, row_pos, row_seq, kv, y):
    """Short-context attention of the depth decoder (row_pos < 8, first cache page): y [R, n_head*head_size] fp32."""
    a = AttnArgs()
    a.dtype, a.R = dtype_code(dtype), R
    a.q, a.row_pos, a.row_seq, a.y, a.kv = ptr(q), ptr(row_pos), ptr(row_seq), ptr(y), kv
    check(lib.ua2_attn_local(C.byref(a), stream()), "ua2_attn_local")


def embed_frame(dtype, tokens, mask, audio_emb, wte, va):
    M, w = tokens.shape
    Cc = audio_emb.shape[1]
    a = torch.empty(M, Cc, dtype=torch.float32, device=tokens.device)
    t = torch.empty_like(a)
    check(lib.ua2_embed_frame(dtype_code(dtype), M, Cc, w - 1, va, ptr(tokens), ptr(mask), ptr(audio_emb), ptr(wte),
                              ptr(a), ptr(t), None, stream()), "ua2_embed_frame")
    return a, t


def rmsnorm_blend(x, w, eps, other=None, mask=None, col_a=-1, col_b=-1, want_n=False):
    M, Cc = x.shape
    o1 = torch.empty_like(x)
    o2 = torch.empty_like(x) if want_n else None
    check(lib.ua2_rmsnorm_blend(M, Cc, ptr(x), ptr(w), eps, ptr(other), ptr(mask),
                                mask.shape[1] if mask is not None else 0, col_a, col_b, ptr(o1), ptr(o2), None, stream()),
          "ua2_rmsnorm_blend")
    return (o1, o2) if want_n else o1


def argmax_embed(dtype, part_max, part_idx, out_tokens, out_col, emb=None, emb_row_offset=0, next_h=None):
    M, n_part = part_max.shape
    check(lib.ua2_argmax_embed(dtype_code(dtype), M, n_part, ptr(part_max), ptr(part_idx), ptr(out_tokens),
                               out_tokens.shape[1], out_col, ptr(emb), emb_row_offset,
                               emb.shape[1] if emb is not None else 0, ptr(next_h), stream()), "ua2_argmax_embed")


def rvq_encode(x, emb, embT=None):
    """x [N,D] fp32, emb [L,C,D] fp32 -> codes [N,L] int32, quantized [N,D] fp32 (core_vq.py:365-376)."""
    N, D = x.shape
    L, Cc, _ = emb.shape
    if embT is None:
        embT = emb.transpose(1, 2).contiguous()
    codes = torch.empty(N, L, dtype=torch.int32, device=x.device)
    q = torch.empty(N, D, dtype=torch.float32, device=x.device)
    ws = torch.empty(lib.ua2_rvq_workspace_bytes(N, L), dtype=torch.uint8, device=x.device)
    check(lib.ua2_rvq_encode(ptr(x), ptr(emb), ptr(embT), N, L, Cc, D, ptr(codes), ptr(q), ptr(ws), ws.numel(), stream()), "ua2_rvq_encode")
    return codes, q


def rvq_decode(codes, emb):
    """codes [N,L] int32, emb [L,C,D] -> [N,D] fp32 (core_vq.py:378-384)."""
    N, L = codes.shape
    _, Cc, D = emb.shape
    out = torch.empty(N, D, dtype=torch.float32, device=emb.device)
    check(lib.ua2_rvq_decode(ptr(codes), ptr(emb), N, L, Cc, D, ptr(out), stream()), "ua2_rvq_decode")
    return out


# ---- codec convolutions ------------------------------------------------------------------------

def pack_conv_weight(w):
    """nn.Conv1d weight [Cout, Cin, K] fp32 -> packed buffer for ua2_conv1d (Cin zero-padded to 16)."""
    Cout, Cin, K = w.shape
    cin_pad = (Cin + 15) // 16 * 16
    wp = torch.zeros(Cout, cin_pad, K, dtype=torch.float32, device=w.device)
    wp[:, :Cin] = w.float()
    return pack_linear(wp.view(Cout, cin_pad * K), torch.float32), K


def convtr_phase_rows(w, stride):
    """nn.ConvTranspose1d weight [Cin, Cout, K] -> [stride * Cout, Cin, M] phase filters of ua2_conv1d's phase mode:
    row phase*Cout + co, taps in descending order (x index q - m  <->  original tap phase + m*stride)."""
    Cin, Cout, K = w.shape
    M = (K + stride - 1) // stride
    wp = torch.zeros(stride, Cout, Cin, M, dtype=torch.float32, device=w.device)
    for ph in range(stride):
        for m in range(M):
            j = ph + m * stride
            if j < K:
                wp[ph, :, :, M - 1 - m] = w[:, :, j].float().t()
    return wp.view(stride * Cout, Cin, M), M


def pack_convtr_weight(w, stride):
    """Packed fp32 phase filters of a transposed conv for the exact ua2_conv1d (see convtr_phase_rows)."""
    rows, M = convtr_phase_rows(w, stride)
    return pack_conv_weight(rows)[0], M


def pack_conv_weight_x3(w_rows):
    """[rows, Cin, K] fp32 filter (rows = Cout, or phases * Cout for a transposed conv) -> (hi, lo) packed bf16 buffers for
    ua2_conv1d precision 1: reduction index (channel group of 32, tap, channel in group), Cin zero-padded to 32."""
    rows, Cin, K = w_rows.shape
    G = (Cin + 31) // 32
    wp = torch.zeros(rows, G * 32, K, dtype=torch.float32, device=w_rows.device)
    wp[:, :Cin] = w_rows.float()
    wk = wp.view(rows, G, 32, K).permute(0, 1, 3, 2).reshape(rows, G * K * 32).contiguous()
    hi = wk.to(torch.bfloat16)
    lo = (wk - hi.float()).contiguous()
    return pack_linear(hi.float().contiguous(), torch.bfloat16), pack_linear(lo, torch.bfloat16)


def conv1d_plan(B, Cin, Cout, Tin, Tout, K, *, stride=1, dilation=1, in_repeat=1, out_phases=1, out_trim_left=0, pre_act=0, post_act=0,
                precision=0, fused=False, residual=False):
    """What ua2_conv1d would launch for this problem (ua2_debug_conv1d_plan: the launcher's own selection code; nothing is launched and
    no device is needed): dict(kernel, ntt, rt, tpw, gpu, npg, nw), see include/ua2hip.h.  Reads UA2_CONV_PIPE as the launcher does."""
    from ._lib import Conv1dArgs
    a = Conv1dArgs()
    a.B, a.Cin, a.Cout, a.Tin, a.Tout = B, Cin, Cout, Tin, Tout
    a.K, a.stride, a.dilation = K, stride, dilation
    a.in_repeat, a.out_phases, a.out_trim_left = in_repeat, out_phases, out_trim_left
    a.pre_act, a.post_act, a.precision = pre_act, post_act, precision
    some = 64                              # pointers are only tested for NULL
    a.x = a.w = a.y = a.post_alpha = some
    a.post_alpha_n = 1
    if precision == 1:
        a.w_lo = some
    if fused:
        a.w2 = a.w2_lo = some
    if fused or residual:
        a.residual = some
    out = [C.c_int32() for _ in range(7)]
    check(lib.ua2_debug_conv1d_plan(C.byref(a), *[C.byref(o) for o in out]), "ua2_debug_conv1d_plan")
    return dict(zip(("kernel", "ntt", "rt", "tpw", "gpu", "npg", "nw"), (o.value for o in out)))


def conv1d(x, w_packed, K, Cout, *, stride=1, dilation=1, pad_left=0, Tout=None, bias=None, pre_act=0, pre_alpha=None,
           post_act=0, post_alpha=None, residual=None, in_repeat=1, out_phases=1, out_trim_left=0, w_lo=None, fused2=None, out=None):
    """`out`: an fp32, contiguous [B, Cout, Tout] tensor (or view) to write into instead of a fresh one."""
    from ._lib import Conv1dArgs
    B, Cin, Tin = x.shape
    a = Conv1dArgs()
    a.B, a.Cin, a.Cout, a.Tin, a.Tout = B, Cin, Cout, Tin, Tout
    a.K, a.stride, a.dilation, a.pad_left = K, stride, dilation, pad_left
    a.in_repeat, a.out_phases, a.out_trim_left = in_repeat, out_phases, out_trim_left
    a.pre_act, a.post_act = pre_act, post_act
    if out is None:
        y = torch.empty(B, Cout, Tout, dtype=torch.float32, device=x.device)
    else:
        assert out.shape == (B, Cout, Tout) and out.dtype == torch.float32 and out.is_contiguous() and out.device == x.device
        y = out
    a.x, a.w, a.bias = ptr(x), ptr(w_packed), ptr(bias)
    a.pre_alpha, a.post_alpha = ptr(pre_alpha), ptr(post_alpha)
    a.post_alpha_n = post_alpha.numel() if post_alpha is not None else 0
    a.residual, a.y = ptr(residual), ptr(y)
    if w_lo is not None:                  # bf16 x 3 form: (w_packed, w_lo) = pack_conv_weight_x3(...)
        a.w_lo, a.precision = ptr(w_lo), 1
    if fused2 is not None:                # (w2_hi, w2_lo, bias2, alpha2): the 1 x 1 conv + PReLU + residual of a residual unit, fused
        a.w2, a.w2_lo, a.bias2, a.alpha2 = ptr(fused2[0]), ptr(fused2[1]), ptr(fused2[2]), ptr(fused2[3])
    check(lib.ua2_conv1d(C.byref(a), stream()), "ua2_conv1d")
    return y


class TC:
    """Activation in the decode side's layout: two bf16 planes hi = RNE(x), lo = RNE(x - hi), each [B, T, C] (time-major,
    channels contiguous) — include/ua2hip.h, ua2_conv1d_tc.  `planes` is one (2, B, T, C) bf16 tensor."""

    def __init__(self, planes):
        assert planes.dim() == 4 and planes.shape[0] == 2 and planes.dtype == torch.bfloat16 and planes.is_contiguous()
        self.planes = planes

    @property
    def hi(self):
        return self.planes[0]

    @property
    def lo(self):
        return self.planes[1]

    @property
    def shape(self):                      # (B, C, T): what the fp32 tensor it stands for would report
        _, B, T, Cc = self.planes.shape
        return (B, Cc, T)

    @staticmethod
    def empty(B, Cc, T, device):
        return TC(torch.empty(2, B, T, Cc, dtype=torch.bfloat16, device=device))


def tc_w2_order(w2):
    """[Cout, C, 1] filter of a fused residual unit's 1 x 1 conv -> the same filter with its input channels in the K order the
    ua2_conv1d_tc kernels reduce in (csrc/ua2_convtc.hip, "tc_w2_order"): inside each group of 32, k' = 8 g + e holds channel
    4 g + e (e < 4) or 16 + 4 g + (e - 4) (e >= 4).  Pack the result with pack_conv_weight_x3 and pass it as `fused2`."""
    Cc = w2.shape[1]
    assert Cc % 32 == 0
    k = torch.arange(32)
    g, e = k // 8, k % 8
    ch = torch.where(e < 4, 4 * g + e, 16 + 4 * g + (e - 4))
    perm = (torch.arange(0, Cc, 32).view(-1, 1) + ch.view(1, -1)).reshape(-1).to(w2.device)
    return w2[:, perm].contiguous()


def tc_pack(x):
    """fp32 [B, C, T] -> TC (ua2_tc_pack)."""
    B, Cc, T = x.shape
    out = TC.empty(B, Cc, T, x.device)
    check(lib.ua2_tc_pack(ptr(x.contiguous()), ptr(out.hi), ptr(out.lo), B, Cc, T, stream()), "ua2_tc_pack")
    return out


def tc_unpack(t):
    """TC -> fp32 [B, C, T], x = hi + lo exactly (ua2_tc_unpack)."""
    B, Cc, T = t.shape
    y = torch.empty(B, Cc, T, dtype=torch.float32, device=t.planes.device)
    check(lib.ua2_tc_unpack(ptr(t.hi), ptr(t.lo), ptr(y), B, Cc, T, stream()), "ua2_tc_unpack")
    return y


def conv1d_tc(x, w_hi, w_lo, K, Cout, *, dilation=1, pad_left=0, Tout=None, bias=None, post_act=0, post_alpha=None, in_repeat=1,
              out_phases=1, out_trim_left=0, fused2=None, residual=None, out_f32=False, variant=0, out=None):
    """ua2_conv1d_tc: x a TC; (w_hi, w_lo) = pack_conv_weight_x3(filter rows).  Returns a TC, or fp32 [B, Cout, Tout] with
    out_f32 (the waveform).  fused2 = (w2_hi, w2_lo, bias2, alpha2): the 1 x 1 conv + PReLU + residual of a residual unit in
    the same launch (residual = x), with (w2_hi, w2_lo) = pack_conv_weight_x3(tc_w2_order(W2)); residual = a TC added after the
    activation (un-fused second conv).  variant: 0 automatic, 1 plain, 2 pipelined, 3 big-tile."""
    from ._lib import ConvTcArgs
    B, Cin, Tin = x.shape
    a = ConvTcArgs()
    a.B, a.Cin, a.Cout, a.Tin, a.Tout = B, Cin, Cout, Tin, Tout
    a.K, a.dilation, a.pad_left, a.in_repeat = K, dilation, pad_left, in_repeat
    a.out_phases, a.out_trim_left, a.post_act, a.variant = out_phases, out_trim_left, post_act, variant
    a.x_hi, a.x_lo, a.w, a.w_lo, a.bias = ptr(x.hi), ptr(x.lo), ptr(w_hi), ptr(w_lo), ptr(bias)
    a.post_alpha = ptr(post_alpha)
    a.post_alpha_n = post_alpha.numel() if post_alpha is not None else 0
    if fused2 is not None:
        a.w2, a.w2_lo, a.bias2, a.alpha2 = ptr(fused2[0]), ptr(fused2[1]), ptr(fused2[2]), ptr(fused2[3])
    if residual is not None:
        assert residual.shape == (B, Cout, Tout)
        a.res_hi, a.res_lo = ptr(residual.hi), ptr(residual.lo)
    dev = x.planes.device
    if out is not None:                   # write into the caller's fp32 tensor (out_f32) or planes (anything with .hi / .lo / .shape)
        assert tuple(out.shape) == (B, Cout, Tout)
        y = out
    if out_f32:
        if out is None:
            y = torch.empty(B, Cout, Tout, dtype=torch.float32, device=dev)
        assert y.dtype == torch.float32
        a.y_f32 = ptr(y)
    else:
        if out is None:
            y = TC.empty(B, Cout, Tout, dev)
        assert y.hi.dtype == torch.bfloat16 and y.lo.dtype == torch.bfloat16
        a.y_hi, a.y_lo = ptr(y.hi), ptr(y.lo)
    check(lib.ua2_conv1d_tc(C.byref(a), stream()), "ua2_conv1d_tc")
    return y


def dwconv1d(x, w, *, stride=1, dilation=1, pad_left=0, Tout=None, bias=None, transposed=False):
    """Depthwise conv / transposed conv: x [B,C,Tin] fp32, w [C,K] fp32 -> [B,C,Tout] (ua2_dwconv1d)."""
    B, Cc, Tin = x.shape
    K = w.shape[-1]
    y = torch.empty(B, Cc, Tout, dtype=torch.float32, device=x.device)
    check(lib.ua2_dwconv1d(ptr(x.contiguous()), ptr(w.contiguous()), ptr(bias), ptr(y), B, Cc, Tin, Tout, K, stride, dilation,
                           pad_left, int(transposed), stream()), "ua2_dwconv1d")
    return y


def avgpool1d(x, k):
    B, Cc, T = x.shape
    y = torch.empty(B, Cc, T // k, dtype=torch.float32, device=x.device)
    check(lib.ua2_avgpool1d(ptr(x), ptr(y), B * Cc, T, k, stream()), "ua2_avgpool1d")
    return y


# ---- codec neural stages: glue ops -----------------------------------------------------------------

def ew_fma(a, b=None, c=None, alpha=1.0, beta=0.0, out=None, n=None):
    """out[i] = alpha * a[i % na] * b[i % nb] + c[i % nc] + beta over n = max numel (ua2_ew_fma)."""
    ts = [t for t in (a, b, c) if t is not None]
    n = n or max(t.numel() for t in ts)
    if out is None:
        big = max(ts, key=lambda t: t.numel())
        out = torch.empty(big.shape, dtype=torch.float32, device=a.device)
    nz = lambda t: t.numel() if t is not None else 0
    check(lib.ua2_ew_fma(ptr(out), n, ptr(a), a.numel(), ptr(b), nz(b), ptr(c), nz(c), float(alpha), float(beta), stream()), "ua2_ew_fma")
    return out


def ew_act(x, act):
    out = torch.empty_like(x)
    check(lib.ua2_ew_act(ptr(out), ptr(x), x.numel(), act, stream()), "ua2_ew_act")
    return out


def gather_rows(x, idx):
    """x [N, C] fp32, idx [R] int32 (negative = zero row) -> [R, C]."""
    R, Cc = idx.numel(), x.shape[-1]
    out = torch.empty(R, Cc, dtype=torch.float32, device=x.device)
    check(lib.ua2_gather_rows(ptr(out), ptr(x), ptr(idx), R, Cc, stream()), "ua2_gather_rows")
    return out


def reason_merge(rec, reason, src, out=None, src_checked=False):
    """rec [R, D] + reason[src] -> [R, D] fp32 (ua2_reason_merge): feature_combine's `rec_feature + reasoning_feature` after
    the x2.5 nearest up-sampling (AudioDiffusion1D.py:440-456).  src [R] int32 on the device; out may be rec (in place).
    Unless the caller vouches for the table (src_checked=True, built once and checked on the host), it is checked here
    against reason's row count — one small device-to-host copy."""
    R, D = rec.shape
    if src.numel() != R or src.dtype != torch.int32 or reason.shape[-1] != D:
        raise ValueError(f"reason_merge: rec {tuple(rec.shape)}, reason {tuple(reason.shape)}, src {tuple(src.shape)} {src.dtype}")
    if not src_checked:
        lo, hi = (int(v) for v in src.aminmax())
        if lo < 0 or hi >= reason.shape[0]:
            raise ValueError(f"reason_merge: src entries in [{lo}, {hi}] but reason has {reason.shape[0]} rows")
    if out is None:
        out = torch.empty(R, D, dtype=torch.float32, device=rec.device)
    check(lib.ua2_reason_merge(ptr(out), ptr(rec), ptr(reason), ptr(src), R, D, stream()), "ua2_reason_merge")
    return out


def crossfade(seg, win, ovlp, target_len):
    """seg [n_seg, N >= win] fp32 decoded windows -> [target_len] joined waveform (ua2_crossfade): the float64 linear
    cross-fade of reason_tokenizer.py:210-224 (== reason_tokenizer.crossfade_concat bit for bit) and the crop."""
    n_seg, stride = seg.shape
    out = torch.empty(int(target_len), dtype=torch.float32, device=seg.device)
    check(lib.ua2_crossfade(ptr(out), ptr(seg), n_seg, stride, int(win), int(ovlp), int(target_len), stream()), "ua2_crossfade")
    return out


def time_film(params, x, batch_mask, rows_per_batch, gamma_scale):
    R, Cc = x.shape
    out = torch.empty_like(x)
    check(lib.ua2_time_film(ptr(out), ptr(params), ptr(x), ptr(batch_mask), R, rows_per_batch, Cc, float(gamma_scale), stream()),
          "ua2_time_film")
    return out


def layernorm_rows(x, w=None, b=None, eps=1e-5):
    R, Cc = x.shape
    out = torch.empty_like(x)
    check(lib.ua2_layernorm_rows(ptr(out), ptr(x), ptr(w), ptr(b), R, Cc, float(eps), stream()), "ua2_layernorm_rows")
    return out


def qknorm_rope_kv(dtype, qkv, row_pos, row_seq, kv, q_out, qw=None, qb=None, kw=None, kb=None, eps=1e-5, cos=None, sin=None,
                   rot_dim=0):
    check(lib.ua2_qknorm_rope_kv(dtype_code(dtype), ptr(qkv), qkv.shape[0], ptr(row_pos), ptr(row_seq), ptr(qw), ptr(qb), ptr(kw),
                                 ptr(kb), float(eps), ptr(cos), ptr(sin), rot_dim, ptr(q_out), C.byref(kv), stream()),
          "ua2_qknorm_rope_kv")


# ---- Whisper log-mel front end -------------------------------------------------------------------

LOGMEL_SAMPLES, LOGMEL_FFT, LOGMEL_HOP, LOGMEL_BINS, LOGMEL_MELS, LOGMEL_FRAMES = 480000, 400, 160, 201, 80, 3000
_LOGMEL_TABLES = {}


def logmel_tables_host():
    """(basis [400, 402], mel_fb [201, 80]) float64 on the host: the windowed DFT basis and the filter bank WhisperFeatureExtractor
    builds (periodic Hann window; mel_filter_bank(201, 80, 0, 8000, 16000, norm='slaney', mel_scale='slaney')), restated."""
    n = torch.arange(LOGMEL_FFT, dtype=torch.float64)
    hann = 0.5 - 0.5 * torch.cos(2 * torch.pi * n / LOGMEL_FFT)
    k = torch.arange(LOGMEL_BINS, dtype=torch.float64)
    ang = 2 * torch.pi * ((n[:, None] * k[None, :]) % LOGMEL_FFT) / LOGMEL_FFT      # exact integer reduction of n k mod 400
    basis = torch.cat([hann[:, None] * torch.cos(ang), hann[:, None] * torch.sin(ang)], 1)
    # Slaney scale: linear (200/3 Hz per mel) below 1 kHz, logarithmic (27 mels per factor 6.4) above
    logstep = torch.log(torch.tensor(6.4, dtype=torch.float64)) / 27.0
    to_mel = lambda f: torch.where(f >= 1000.0, 15.0 + torch.log(f.clamp(min=1e-300) / 1000.0) / logstep, 3.0 * f / 200.0)
    to_hz = lambda m: torch.where(m >= 15.0, 1000.0 * torch.exp(logstep * (m - 15.0)), 200.0 * m / 3.0)
    lo, hi = to_mel(torch.tensor([0.0, 8000.0], dtype=torch.float64))
    edges = to_hz(torch.linspace(float(lo), float(hi), LOGMEL_MELS + 2, dtype=torch.float64))
    freqs = torch.linspace(0.0, 8000.0, LOGMEL_BINS, dtype=torch.float64)
    diff = edges[1:] - edges[:-1]
    slopes = edges[None, :] - freqs[:, None]
    fb = torch.minimum(-slopes[:, :-2] / diff[:-1], slopes[:, 2:] / diff[1:]).clamp(min=0.0)
    fb = fb * (2.0 / (edges[2:] - edges[:-2]))[None, :]                                # norm='slaney'
    return basis, fb


def logmel(wav):
    """wav [B, N] fp32 at 16 kHz on the device -> log-mel [B, 80, 3000] fp32 (ua2_logmel: WhisperFeatureExtractor's numpy path)."""
    assert wav.dim() == 2 and wav.dtype == torch.float32
    wav = wav.contiguous()
    tabs = _LOGMEL_TABLES.get(wav.device)
    if tabs is None:
        basis, fb = logmel_tables_host()
        tabs = _LOGMEL_TABLES[wav.device] = (basis.float().contiguous().to(wav.device), fb.float().contiguous().to(wav.device))
    assert tuple(tabs[0].shape) == (LOGMEL_FFT, 2 * LOGMEL_BINS) and tuple(tabs[1].shape) == (LOGMEL_BINS, LOGMEL_MELS)
    B, N = wav.shape
    out = torch.empty(B, LOGMEL_MELS, LOGMEL_FRAMES, dtype=torch.float32, device=wav.device)
    ws = torch.empty(max(lib.ua2_logmel_workspace_bytes(B) // 4, 1), dtype=torch.float32, device=wav.device)
    check(lib.ua2_logmel(ptr(out), ptr(wav), B, N, ptr(tabs[0]), ptr(tabs[1]), ptr(ws), ws.numel() * 4, stream()), "ua2_logmel")
    return out


# ---- BEST-RQ (MusicFM 25 Hz) encoder: 2-D convolution stem, LayerNorm + rotary rows, mel front end -------------------

CONV2D_SMALL_CIN = 4          # ua2_conv2d: up to this many input channels the filter stays plain and one thread forms an output


def pack_conv2d_weight(w):
    """nn.Conv2d weight [Cout, Cin, 3, 3] fp32 -> the buffer ua2_conv2d takes: for Cin > 4 ua2_pack_linear(fp32) of the
    [Cout, G * 9 * 16] matrix with reduction index (group of 16 channels, tap, channel in group), Cin zero-padded to 16 G; for
    Cin <= 4 the plain filter."""
    Cout, Cin, kf, kt = w.shape
    assert (kf, kt) == (3, 3) and w.is_cuda
    w = w.detach().float().contiguous()
    if Cin <= CONV2D_SMALL_CIN:
        return w
    G = (Cin + 15) // 16
    wp = torch.zeros(Cout, G * 16, 9, dtype=torch.float32, device=w.device)
    wp[:, :Cin] = w.view(Cout, Cin, 9)
    wk = wp.view(Cout, G, 16, 9).permute(0, 1, 3, 2).reshape(Cout, G * 9 * 16).contiguous()
    return pack_linear(wk, torch.float32)


def conv2d(x, w_packed, Cout, *, stride=(1, 1), bias=None, residual=None, relu=False):
    """x [B, Cin, F, T] fp32 -> relu?(conv3x3(x, padding 1, stride) + bias (+ residual)) [B, Cout, Fo, To] (ua2_conv2d, exact fp32);
    w_packed = pack_conv2d_weight(filter)."""
    B, Cin, F, T = x.shape
    Fo, To = (F - 1) // stride[0] + 1, (T - 1) // stride[1] + 1
    y = torch.empty(B, Cout, Fo, To, dtype=torch.float32, device=x.device)
    if residual is not None:
        assert tuple(residual.shape) == (B, Cout, Fo, To)
    check(lib.ua2_conv2d(ptr(x), ptr(w_packed), ptr(bias), ptr(residual), ptr(y), B, Cin, Cout, F, T, int(stride[0]), int(stride[1]),
                         int(bool(relu)), stream()), "ua2_conv2d")
    return y


def layernorm_rope_rows(x, w, b, eps, cos, sin, row_pos, head_size):
    """x [R, C] -> [R, 2 C] = [rotate(LN(x)) | LN(x)] (ua2_layernorm_rope_rows); cos / sin [n_pos, head_size], row_pos [R] int32."""
    R, Cc = x.shape
    assert cos.shape == sin.shape and cos.shape[1] == head_size and row_pos.numel() == R and row_pos.dtype == torch.int32
    out = torch.empty(R, 2 * Cc, dtype=torch.float32, device=x.device)
    check(lib.ua2_layernorm_rope_rows(ptr(out), ptr(x), ptr(w), ptr(b), ptr(cos), ptr(sin), ptr(row_pos), cos.shape[0], R, Cc, head_size,
                                      float(eps), stream()), "ua2_layernorm_rope_rows")
    return out


MEL_SR, MEL_FFT, MEL_HOP, MEL_BINS, MEL_MELS, MEL_CUT = 24000, 2048, 240, 1025, 128, 960
MEL_MEAN, MEL_STD = 6.768444971712967, 18.417922652295623       # melspec_2048 statistics of musicfm_25hz.py:80
_MEL_TABLES = {}


def melspec_tables_host(n_mels=MEL_MELS):
    """(basis [2048, 2050], mel_fb [1025, n_mels]) float64 on the host: the periodic-Hann-windowed cos | sin basis of the 2048-point
    DFT and torchaudio's melscale_fbanks(1025, 0, 12000, n_mels, 24000, norm=None, mel_scale='htk'), restated."""
    n = torch.arange(MEL_FFT, dtype=torch.float64)
    hann = 0.5 - 0.5 * torch.cos(2 * torch.pi * n / MEL_FFT)
    k = torch.arange(MEL_BINS, dtype=torch.float64)
    ang = 2 * torch.pi * ((n[:, None] * k[None, :]) % MEL_FFT) / MEL_FFT              # exact integer reduction of n k mod 2048
    basis = torch.cat([hann[:, None] * torch.cos(ang), hann[:, None] * torch.sin(ang)], 1)
    freqs = torch.linspace(0.0, MEL_SR // 2, MEL_BINS, dtype=torch.float64)
    m_max = 2595.0 * torch.log10(torch.tensor(1.0 + (MEL_SR / 2) / 700.0, dtype=torch.float64))
    m_pts = torch.linspace(0.0, float(m_max), n_mels + 2, dtype=torch.float64)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - freqs[:, None]
    fb = torch.minimum(-slopes[:, :-2] / f_diff[:-1], slopes[:, 2:] / f_diff[1:]).clamp(min=0.0)
    return basis, fb


def mel_frames(wav):
    """wav [B, N] -> ([B * T, 2048] frames, T): cut to a multiple of 960 samples (musicfm_model.py:78), reflect-pad 1024 on both
    sides (center=True), frames of 2048 at hop 240, the last of the T + 1 dropped ([..., :-1]).  Data movement only."""
    B, N = wav.shape
    n = N // MEL_CUT * MEL_CUT
    if n <= MEL_FFT // 2:
        raise ValueError(f"melspec: {N} samples; the reflection of center=True needs more than {MEL_FFT // 2} after the cut to a multiple of {MEL_CUT}")
    x = wav[:, :n]
    h = MEL_FFT // 2
    x = torch.cat([x[:, 1:h + 1].flip(1), x, x[:, -h - 1:-1].flip(1)], 1)
    T = n // MEL_HOP
    return x.unfold(1, MEL_FFT, MEL_HOP)[:, :T].reshape(B * T, MEL_FFT).contiguous(), T


def melspec(wav, n_mels=MEL_MELS):
    """wav [B, N] fp32 at 24 kHz on the device -> normalised dB mel spectrogram [B, n_mels, T] fp32, T = (N // 960) * 4: MusicFM's
    MelSTFT(n_fft 2048, hop 240, is_db) + [..., :-1] + (x - mean) / std, as an exact-fp32 ua2_linear against the windowed DFT basis
    followed by ua2_melspec_db."""
    assert wav.dim() == 2 and wav.dtype == torch.float32 and wav.is_cuda
    tabs = _MEL_TABLES.get((wav.device, n_mels))
    if tabs is None:
        basis, fb = melspec_tables_host(n_mels)
        n_pad = (2 * MEL_BINS + 15) // 16 * 16
        wmat = torch.zeros(n_pad, MEL_FFT, dtype=torch.float32)
        wmat[:2 * MEL_BINS] = basis.t().float()
        tabs = _MEL_TABLES[(wav.device, n_mels)] = (pack_linear(wmat.to(wav.device), torch.float32), fb.float().contiguous().to(wav.device), n_pad)
    wpk, fb, n_pad = tabs
    frames, T = mel_frames(wav.contiguous())
    B, M = wav.shape[0], frames.shape[0]
    spec = torch.empty(M, n_pad, dtype=torch.float32, device=wav.device)
    ws = linear_workspace(torch.float32, M, MEL_FFT, wav.device) if M > 16 else None
    linear(dtype=torch.float32, M=M, N=n_pad, K=MEL_FFT, w0=wpk, x=frames, ldx=MEL_FFT, y=spec, ldy=n_pad, workspace=ws)
    out = torch.empty(B, n_mels, T, dtype=torch.float32, device=wav.device)
    check(lib.ua2_melspec_db(ptr(out), ptr(spec), ptr(fb), B, T, MEL_BINS, n_mels, n_pad, MEL_MEAN, MEL_STD, stream()), "ua2_melspec_db")
    return out


# ---- WavLM encoder: first conv layer, grouped positional conv, gated relative-position bias ------------------------------

def wavlm_conv0(x, w, gn_w, gn_b, stride, eps=1e-5):
    """x [B, N] fp32, w [C, K] -> gelu(GroupNorm_{groups = C}(conv1d(x, w, stride))) as [B, T0, C] time-major rows (ua2_wavlm_conv0)."""
    assert x.dim() == 2 and x.dtype == torch.float32 and w.dim() == 2
    B, N = x.shape
    Cc, K = w.shape
    n = lib.ua2_wavlm_conv0_workspace_bytes(B, N, Cc, K, int(stride))
    ws = torch.empty(max(n // 8, 1), dtype=torch.float64, device=x.device)
    T0 = (N - K) // int(stride) + 1 if N >= K else 0
    y = torch.empty(B, max(T0, 0), Cc, dtype=torch.float32, device=x.device)
    check(lib.ua2_wavlm_conv0(ptr(y), ptr(x.contiguous()), ptr(w.contiguous()), ptr(gn_w), ptr(gn_b), B, N, Cc, K, int(stride), float(eps),
                              ptr(ws), ws.numel() * 8, stream()), "ua2_wavlm_conv0")
    return y


def pack_conv1d_grouped_weight(w, groups):
    """nn.Conv1d(C, C, K, groups) weight [C, C / groups, K] fp32 (weight norm folded) -> the buffer ua2_conv1d_grouped takes:
    ua2_pack_linear(fp32) of the [C, K * C / groups] matrix with reduction index (tap, channel in the group)."""
    Cc, Cg, K = w.shape
    assert w.is_cuda and Cc % groups == 0 and Cg == Cc // groups
    wk = w.detach().float().permute(0, 2, 1).reshape(Cc, K * Cg).contiguous()
    return pack_linear(wk, torch.float32)


def conv1d_grouped(x, w_packed, B, T, groups, K, *, bias=None, resid=None, gelu=False, out=None):
    """x [B * T, C] rows -> resid + act(grouped conv over time, padding K // 2, T outputs) [B * T, C] (ua2_conv1d_grouped)."""
    Cc = x.shape[-1]
    assert x.shape[0] == B * T and x.dtype == torch.float32
    y = out if out is not None else torch.empty(B * T, Cc, dtype=torch.float32, device=x.device)
    check(lib.ua2_conv1d_grouped(ptr(y), ptr(x), ptr(w_packed), ptr(bias), ptr(resid), B, T, Cc, int(groups), int(K), int(bool(gelu)), stream()),
          "ua2_conv1d_grouped")
    return y


def relpos_gate(h, w, b, c, n_head):
    """h [R, n_head * hs], w [8, hs], b [8], c [n_head] -> gate [R, n_head] fp32 (ua2_relpos_gate)."""
    R, hs = h.shape[0], h.shape[1] // n_head
    g = torch.empty(R, n_head, dtype=torch.float32, device=h.device)
    check(lib.ua2_relpos_gate(ptr(g), ptr(h), ptr(w), ptr(b), ptr(c), R, n_head, hs, stream()), "ua2_relpos_gate")
    return g


def attn_relbias(*, dtype, R, q, row_pos, row_seq, kv, q_pos, gate, rel_tab, y=None, groups=None, y_packed=None):
    """ua2_attn_relbias: ops.attn with score + gate[r, h] * rel_tab[h][key - q_pos[r] + tab_half]; q pre-scaled; rel_tab [n_head, 2 tab_half + 1]."""
    a = AttnArgs()
    a.y_packed = ptr(y_packed)
    if groups is not None:
        a.group_rows, a.group_seq, a.group_nkeys = ptr(groups[0]), ptr(groups[1]), ptr(groups[2])
        a.n_groups, a.group_q_tiles = groups[0].shape[0], groups[3]
    a.y = ptr(y)
    a.dtype, a.R = dtype_code(dtype), R
    a.q, a.row_pos, a.row_seq = ptr(q), ptr(row_pos), ptr(row_seq)
    a.kv = kv
    assert rel_tab.dim() == 2 and rel_tab.shape[0] == kv.n_head and rel_tab.shape[1] % 2 == 1 and rel_tab.dtype == torch.float32
    assert q_pos.dtype == torch.int32 and q_pos.numel() == R and tuple(gate.shape) == (R, kv.n_head)
    check(lib.ua2_attn_relbias(C.byref(a), ptr(q_pos), ptr(gate), ptr(rel_tab), rel_tab.shape[1] // 2, stream()), "ua2_attn_relbias")
