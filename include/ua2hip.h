/*
 * ua2hip.h — C ABI of libua2hip.so: the MI355X (gfx950) kernels behind UniAudio 2.0's
 * audio-token generation hot path (BASELINE.json north_star).
 *
 * The reference (yangdongchao/UniAudio2) is pure Python/PyTorch and has no FFI of its own
 * (SURVEY.md §8b): each entry point below replaces a *PyTorch call site* of the reference,
 * cited as file:line relative to the reference root.  The binding a maintainer of the
 * reference would add is a ctypes stub; uniaudio2_amd/_lib.py is that stub.
 *
 * Conventions
 *   - plain C: raw DEVICE pointers (void*), explicit sizes, a hipStream_t passed as void*.
 *   - every function returns 0 on success, negative on error; ua2_last_error() gives text.
 *   - the caller owns every buffer; the library owns only the handles it returns.
 *   - stream-ordered, no hidden synchronisation, no device allocation inside calls.
 *   - dtype = storage/compute type of weights, embedding tables and the KV cache:
 *       UA2_F32  exact-fp32 path (f32-input MFMA), for id-level parity with the fp32 reference
 *       UA2_BF16 bf16 operands, fp32 accumulate (MFMA 16x16x32 bf16), fp32 residual stream
 *     Activations between kernels are always fp32.
 */
#ifndef UA2HIP_H
#define UA2HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UA2_VERSION 10

enum ua2_dtype { UA2_F32 = 0, UA2_BF16 = 1 };

/* A-operand producer fused into the GEMM (what the reference does right before the Linear). */
enum ua2_prologue {
  UA2_PRO_CAST = 0, /* x as is                                   (lit_model.py:511,595; model_new.py:617,631) */
  UA2_PRO_NORM = 1, /* RMSNorm(x)*w, fp32 math                    (lit_model.py:883-890 before :424 / :591)    */
  /* 2: reserved (round 1's merge of per-page attention partials; ua2_attn now writes the normalised row itself) */
  UA2_PRO_LOCAL_ATTN = 3, /* M == 1 only: the operand row IS the short-context attention of ua2_attn_local, computed
                       in the kernel (x = q [1, n_head*head_size], kv, row_pos, row_seq as for ua2_attn_local;
                       K == n_head*head_size).  Bit-identical to ua2_attn_local followed by UA2_PRO_CAST. */
  UA2_PRO_SCALED = 4  /* RMSNorm folded around the GEMM (UA2_BF16 only; the frame executor's form of lit_model.py:883-890
                       + :424 / :591):   y = rstd[m] * ( RNE_bf16(x (.) w) W^T ),   rstd = rsqrt(mean(x^2) + eps).
                       The operand RNE_bf16(x (.) w) is handed over by the PRODUCER of x (x_h: row-major bf16, launches of
                       one row tile; x_packed: fragment order, many-row launches) together with per-16-column sums of
                       squares of the fp32 x (x_ssq) — see y_norm_w below — so that no launch stands between the
                       producer and this GEMM, whatever the row count; the row scale is applied to the fp32 sums in
                       the epilogue.  Mathematically RMSNorm(x) W^T; numerically the bf16 rounding happens before
                       the row scale instead of after it (same relative error).  K % 32 == 0. */
};

/* What happens to the GEMM result (the ops the reference runs right after the Linear). */
enum ua2_epilogue {
  UA2_EPI_STORE = 0,    /* y = xW^T; optional per-tile (max,idx) partials for greedy sampling (model_new.py:146-187) */
  UA2_EPI_RESIDUAL = 1, /* y = resid + xW^T                          (lit_model.py:345,349)                    */
  UA2_EPI_SWIGLU = 2,   /* y = silu(xW1^T) * (xW2^T)                 (lit_model.py:592-594)                    */
  UA2_EPI_QKV_ROPE = 3, /* split q|k|v, RoPE on q,k (rope_mode), append k,v to the paged cache
                           (lit_model.py:431, 458-461, 778-807, 831-856; Moshi: transformer.py:386-396, rope.py:12-68) */
  UA2_EPI_GELU = 4      /* y = gelu(xW^T + b): exact erf form (Moshi FFN, transformer.py:559 F.gelu) or, with
                           act_kind = UA2_GELU_TANH, the tanh approximation (DiT FeedForward "gelu-approximate",
                           ReasoningCodec_film/models/model_config.json:4)                                        */
};

/* ua2_linear_args.act_kind: variant of the activation inside UA2_EPI_GELU / UA2_EPI_SWIGLU */
enum ua2_act_kind {
  UA2_ACT_DEFAULT = 0,          /* GELU: erf form; SWIGLU: silu(xW0^T) * (xW1^T)                                    */
  UA2_GELU_TANH = 1,            /* GELU: tanh approximation                                                         */
  UA2_GATE_SIGMOID_SECOND = 2   /* SWIGLU: (xW0^T + b0) * sigmoid(xW1^T + b1)  — the GLU of ReasoningCodec_film/
                                   modules/transformer.py:208-243 under power_normalized (proj output chunked x | gate) */
};

/* ua2_linear_args.sum_order */
enum ua2_sum_order { UA2_SUM_ORDER_INVARIANT = 0, UA2_SUM_ORDER_FREE = 1 };

/* flavours of UA2_PRO_NORM */
enum ua2_norm_kind {
  UA2_NORM_RMS_LIT = 0,   /* (x * rsqrt(mean(x^2) + eps)) * w           lit_model.py:883-890                     */
  UA2_NORM_RMS_MOSHI = 1, /* x * (alpha * rsqrt(eps + mean(x^2)))       llm_modules/transformer.py:34-46          */
  UA2_NORM_LAYERNORM = 2  /* (x - mean) * rsqrt(var + eps) * w + b      nn.LayerNorm (create_norm_fn :111-112).
                             Two passes over the row, both in one fixed order (the corrected two-pass form): mean = sum(x) / K;
                             then, with d = x - mean, var = mean(d^2) - (sum(d) / K)^2 — the CENTRED variance, not
                             mean(x^2) - mean^2, which cancels once |mean| >> std — and the operand is
                             ((x - mean) - sum(d) / K) * rsqrt(var + eps) * w + b: sum(d) / K is the rounding error the fp32
                             sum left in the mean. */
};
/* RoPE flavours of UA2_EPI_QKV_ROPE */
enum ua2_rope_mode {
  UA2_ROPE_HALF_SPLIT = 0,  /* rotate-half (lit_model.py:795-806); weight packed with rope_head_size          */
  UA2_ROPE_INTERLEAVED = 1, /* adjacent pairs (2i, 2i+1) (rope.py:46-66); weight packed without permutation  */
  UA2_ROPE_NONE = 2         /* positional_embedding='none'                                                   */
};

const char* ua2_last_error(void);
int ua2_version(void);
/* sizeof() of the ABI structs as this library was compiled, for a binding to check its own layout against:
 * which = 0 ua2_kv_geom, 1 ua2_linear_args, 2 ua2_attn_args, 3 ua2_conv1d_args, 4 ua2_gpt_desc, 5 ua2_stage3_desc,
 * 6 ua2_convtc_args, 7 ua2_beam_ngram; else 0. */
size_t ua2_struct_size(int which);

/* Number of elements (of `dtype`) in the packed form of an [N,K] Linear weight. */
size_t ua2_packed_elems(int dtype, int64_t N, int64_t K);

/* Re-tile a Linear weight into MFMA B-fragment order so that every wave load is one
 * contiguous 1 KiB line burst: out[N/16][K/KC][64 lanes][16 B].  `src` is [N,K] row-major
 * (nn.Linear.weight, lit_model.py:356-360) or, with transposed=1, [K,N] (audio_head[i],
 * model_new.py:349,632).  src_dtype is the dtype of `src`; dst dtype is `dtype`
 * (fp32 -> bf16 rounds to nearest even, as torch .to(bfloat16)).
 * rope_head_size > 0 (fused qkv weights consumed by UA2_EPI_QKV_ROPE): the rows of every head are
 * additionally permuted so that output tile r of a head carries dims [8r,8r+8) and their half-split
 * rotation partners [hs/2+8r, hs/2+8r+8): RoPE then closes inside one 16-column tile. */
int ua2_pack_linear(const void* src, int src_dtype, int transposed, int64_t N, int64_t K,
                    void* out, int dtype, int rope_head_size, void* stream);

/* ---- fp8 weight-only twins (OCP e4m3fn, never the fnuz encoding) of the decode kernel's weights; UA2_BF16 launches only ----------
 * Contract, per OUTPUT ROW n of W [N, K]: e[n] = ceil(log2(amax_n / 448)) (an all-zero row takes 0; clamped to [-117, 120] so that 2^e
 * and every nonzero |W'| are normal numbers), q[n, k] = RNE_e4m3fn(W[n, k] * 2^-e[n]) (|W 2^-e| <= 448: nothing saturates), and the
 * weight the model computes with is W' = q * 2^e — exactly representable in bf16.  A launch on the fp8 image gives, bit for bit, what
 * the bf16 launch gives on the packed bf16 form of W' (a power-of-two scale commutes with every fp32 rounding of the sums), so the fp8
 * image is a second, half-sized copy of a weight that the few-row decode kernel streams, and every many-row kernel keeps reading W'.
 *
 * ua2_pack_linear_w8: out_q = the fp8 image [N/16][K/64][64 lanes][16 B] — a lane's 16 bytes are its 8 B-fragment elements of chunk 2j
 * followed by its 8 of chunk 2j + 1 (a chunk = 32 of K; the lane <-> (column, k) map inside a chunk and the rope_head_size row
 * permutation are those of the bf16 form above), ua2_packed_bytes_w8 bytes; out_exp = int8 [N padded to 16] exponents in PACKED column
 * order, padding columns 0; out_bf16 (may be NULL) = the bf16 form above of W', written from the same q and e.  K % 64 != 0 is refused
 * (the caller then keeps that weight in bf16 alone); ua2_packed_bytes_w8 returns 0 for it. */
typedef struct {
  const void* q;         /* fp8 image */
  const int8_t* exp;     /* exponents, packed column order */
} ua2_w8_ref;
size_t ua2_packed_bytes_w8(int64_t N, int64_t K);
int ua2_pack_linear_w8(const void* src, int src_dtype, int transposed, int64_t N, int64_t K, void* out_q, int8_t* out_exp,
                       void* out_bf16, int rope_head_size, void* stream);

/* ---- [v10, addition] lossless 13-bit image of a packed bf16 weight; UA2_BF16 launches of the decode kernel only ----------------------
 * A bf16 weight is s | E[7:0] | m[6:0]; its sign and mantissa are close to uniform, its exponent is not: inside a 16-column tile nearly
 * every weight lies within 30 binades of the largest.  The image stores, for every element of ua2_pack_linear's bf16 form
 * [N/16][K/32][64 lanes][8 elements] (same lane <-> (column, k) map, K % 128 == 0):
 *   low byte  E[0] | m, raw;
 *   code q    4 bits: q = 0 means E[7:1] == 0 (exact +-0 and the lowest pair of binades), q = 1 .. 15 means E[7:1] == base + q;
 *   sign      1 bit;
 * and per tile one byte base = max(largest E[7:1] of the tile - 15, 0), in a side array [N/16] (packed tile order).  A weight with
 * 0 < E[7:1] <= base cannot be written: an ESCAPE.  ua2_pack_linear_l13 counts them; an image with escapes != 0 must not be used (its
 * escaped weights hold q = 0) and the weight stays on its bf16 form — there are no per-tile fallbacks.  With escapes == 0 the decode
 * s | (q ? base + q : 0) | low byte gives back every bf16 bit pattern (NaN payloads and infinities included), so a launch on the image
 * computes with the very B fragments of the bf16 launch: every sum, id and cache entry is unchanged.
 * Layout: per tile, K / 128 groups of 4 chunks, 3328 B each (13/16 of the bf16 form), four dense planes so that every wave load is
 * contiguous and every lane load aligned:
 *   [0, 2048)     low bytes: pair p of chunks (2p, 2p + 1) = [64 lanes][16 B]: the lane's 8 low bytes of chunk 2p, then of chunk 2p + 1;
 *   [2048, 3072)  codes: [64 lanes][4 chunks] dwords; byte b of a dword = q(element b) | q(element b + 4) << 4;
 *   [3072, 3328)  signs: [64 lanes] dwords; bit 8 b + 2 c + h = sign of element 4 h + b of chunk c of the group.
 * ua2_packed_bytes_l13 returns 0 for shapes without an image (K % 128 != 0).  ua2_pack_linear_l13 reads the PACKED bf16 form (device),
 * writes the image, the base bytes [ceil(N / 16)] and *escapes (one int32 on the device), stream-ordered. */
typedef struct {
  const void* image;     /* 13-bit image */
  const uint8_t* base;   /* per-tile base bytes */
} ua2_l13_ref;
size_t ua2_packed_bytes_l13(int64_t N, int64_t K);
int ua2_pack_linear_l13(const void* packed_bf16, int64_t N, int64_t K, void* out_image, uint8_t* out_base, int32_t* escapes, void* stream);

/* Geometry of the paged KV cache shared by the QKV epilogue and the attention kernel.
 * Pool layout (per layer): [n_pages][n_kv][UA2_PAGE][head_size] of `dtype`, K and V separate.
 * page_table[seq*max_pages + p] = page id holding positions [p*UA2_PAGE, (p+1)*UA2_PAGE). */
#define UA2_PAGE 64

typedef struct ua2_kv_geom {
  void* k_pool;
  void* v_pool;
  const int32_t* page_table;
  int32_t max_pages; /* per sequence */
  int32_t n_kv;      /* n_query_groups */
  int32_t n_head;
  int32_t head_size;
  int32_t ring_pages; /* 0: linear cache (page of position p = p / UA2_PAGE).  > 0: ring cache — position p lives in table column
                         (p / UA2_PAGE) % ring_pages (ring_pages a power of two), so a streaming session of any length re-uses ring_pages pages per sequence
                         (RingKVCache, llm_modules/transformer.py:211-278).  The caller guarantees ring_pages * UA2_PAGE exceeds
                         the attention window plus the positions written per launch; ua2_attn needs window > 0 with it. */
} ua2_kv_geom;

/* [v10, addition] Greedy sampling tail of the depth decoder folded into the launch that consumes it (B = 1 frames of the executor,
 * ua2_linear_args.fold).  Step i of the depth decoder ends in audio_head's per-16-column arg-max partials; with the plan's per-id tables
 * everything step i + 1 reads of the sampled id is a table row (projected embedding y, layer 0's q | k | v at position i + 1).  Instead of a
 * one-block launch that reduces the partials and copies those rows into buffers only the next launch reads, layer 0's O-projection
 * (UA2_PRO_LOCAL_ATTN, UA2_EPI_RESIDUAL, M == 1) reduces them itself, after an ordinary kernel boundary — no flags, counters or fences:
 *   id  = arg-max over (part_max, part_idx)[0 .. n_part) under "larger value, then lower index" (the all-NaN fallback and the clamp into
 *         [0, limit) of the stand-alone tails included), every workgroup for itself;   row = id + row_off;
 *   q   = tab_q[row], K / V of position `pos` = tab_k / tab_v[row], positions < pos from the sequence's cache page as always;
 *   y   = tab_y[row] + attention (.) W^T   (the residual comes from the table; `x` and `resid` are not read);
 *   workgroup 0 also stores id to *out_token and the K / V row into the cache page at position `pos` (later launches read them there).
 * part_max == NULL: off.  Same bits as the arg-max launch followed by the plain launch. */
typedef struct ua2_argmax_fold {
  const float* part_max;    /* [n_part] */
  const int32_t* part_idx;  /* [n_part] */
  int32_t n_part, limit;
  int32_t* out_token;
  int64_t row_off;
  int32_t pos;              /* 1 .. 7: position of this step's row (== row_pos[0]) */
  int32_t reserved;
  const float* tab_y;       /* [rows, N] fp32 */
  const float* tab_q;       /* [rows, K] fp32 */
  const void* tab_k;        /* [rows, n_kv * head_size] of the launch dtype */
  const void* tab_v;
} ua2_argmax_fold;

typedef struct ua2_linear_args {
  int32_t dtype, prologue, epilogue;
  int32_t M, N, K;        /* rows, out features, in features */
  const float* x;         /* CAST/NORM: [M, ldx] fp32 */
  int32_t ldx;
  const float* norm_w;    /* NORM: [K] fp32 */
  float eps;
  const void* w0;         /* packed weight */
  const void* w1;         /* SWIGLU: packed fc_2 */
  float* y;               /* STORE/RESIDUAL/SWIGLU: [M, ldy] fp32 (STORE: may be NULL if only partials wanted) */
  int32_t ldy;
  const float* resid;     /* RESIDUAL: [M, ldr], may alias y */
  int32_t ldr;
  float* part_max;        /* STORE, optional: [M, ceil(N/16)] */
  int32_t* part_idx;
  const int32_t* forbid;  /* optional [M]: columns < forbid[m] are excluded from the partial arg-max */
  const int32_t* row_pos; /* QKV_ROPE, LOCAL_ATTN: [M] absolute position of each row */
  const int32_t* row_seq; /* QKV_ROPE: [M] sequence (page-table row) of each row */
  const float* rope_cos;  /* QKV_ROPE: [max_pos, head_size/2] */
  const float* rope_sin;
  float* q_out;           /* QKV_ROPE: [M, n_head*head_size] fp32, rotated */
  ua2_kv_geom kv;         /* QKV_ROPE, LOCAL_ATTN */
  const float* norm_b;    /* NORM, LAYERNORM only: [K] bias */
  int32_t norm_kind;      /* enum ua2_norm_kind */
  const float* out_scale; /* RESIDUAL, optional [N]: y = resid + out_scale[n] * xW^T  (LayerScale, transformer.py:97) */
  int32_t rope_mode;      /* enum ua2_rope_mode */
  void* workspace;        /* optional device scratch of >= ua2_linear_workspace_bytes(dtype, M, K): enables the
                             large-M kernel (normalised operand rows packed once, 128-row tiles).  Results are
                             bit-identical with or without it; without it M > 16 streams the weights once per
                             16-row tile. */
  size_t workspace_bytes;
  /* Producer / consumer hand-over of the many-row operand, skipping the consumer's prep launch:
     y_packed (UA2_EPI_SWIGLU, UA2_EPI_GELU; N % chunk == 0): the result, rounded to `dtype`, also (or, with y == NULL, only) in the
       packed operand layout [ceil(M/16)][N/KC][64 lanes][16 B] of a following K = N launch;
     x_packed (UA2_PRO_CAST, M spanning more than one row tile): the operand already in that layout (K = this launch's K).
     Same bits as the unpacked route: the packed value is the same RNE cast the prep launch applies. */
  void* y_packed;
  const void* x_packed;
  const float* bias;      /* optional [N]: nn.Linear bias added to xW^T before the epilogue's activation / residual /
                             split (NULL for every Linear of the LM).  With UA2_EPI_QKV_ROPE only for weights packed
                             WITHOUT rope_head_size (rope_mode INTERLEAVED / NONE), where column n is source row n */
  const float* bias1;     /* SWIGLU: bias of w1 */
  int32_t act_kind;       /* enum ua2_act_kind */
  /* Scaled-norm hand-over (UA2_BF16).  Producer side — UA2_EPI_RESIDUAL / UA2_EPI_STORE with y_norm_w != NULL: besides
     y the launch writes, for the UA2_PRO_SCALED consumer that follows, RNE_bf16(y[m][n] * y_norm_w[n]) into y_h (row-major
     [M, ldh] bf16) and / or y_packed (fragment order, N % 32 == 0), and y_ssq[m][n / 16] = the sum of y[m][n]^2 over the
     16-column tile, added in a fixed butterfly order (xor 1, 2, 4, 8; the first level fused: an even column c contributes
     fma(y_c, y_c, RN(y_{c+1}^2))) — the same tree in every kernel, so a row's statistic does not depend on the row count.  N % 32 == 0 (the launcher enforces it: whole bf16 MFMA chunks of the consumer).
     Consumer side — UA2_PRO_SCALED: x_h (M <= the decode kernel's row tile) or x_packed, and x_ssq [M, K / 16]; eps as
     for UA2_PRO_NORM.  rstd[m] = rsqrt(sum_j x_ssq[m][j] / K + eps), j summed as 16 interleaved chains + butterfly.
     [v10, addition] bf16 operand rows without a norm (UA2_BF16, launches the decode kernel serves: up to ua2_gemv_rows_preferred rows).
     Producer side — UA2_EPI_SWIGLU with y_h != NULL (no y_norm_w): the result, rounded RNE to bf16, row-major [M, ldy] (y's stride, not ldh); y may then be
     NULL (the fp32 store disappears where nobody reads it).  Consumer side — UA2_PRO_CAST with x_h != NULL ([M, ldx] bf16: x's stride; K % 32 == 0,
     ldx % 8 == 0, x_h 16-byte aligned; x is not read): the operand row(s) are copied into the kernel's LDS tile as they are, instead of every
     workgroup loading the fp32 row and rounding it — the same RNE of the same value, done once: bit-identical to the launch on fp32 x.
     RESIDUAL and STORE epilogues; bf16 weights, their 13-bit images and fp8 twins.  Any other launch with these fields set (more rows,
     UA2_F32, another epilogue, x_packed beside x_h) is refused with a message. */
  const float* y_norm_w;
  void* y_h;
  int32_t ldh;            /* row stride (elements) of y_h / x_h */
  float* y_ssq;
  const void* x_h;
  const float* x_ssq;
  /* [v7] Optional scratch for a K split of UA2_EPI_RESIDUAL launches that take the tiled many-row kernel with a long K and a
     grid too small for the device (the codec DiT's FF2: 1000 x 1536, K = 6144 on 192 workgroups).  When given (and N % 64 == 0,
     no hand-over outputs, K >= 4096), the launcher may cut K into S <= 4 slabs — S a function of (M, N, K) AND of how many slabs
     split_ws_bytes holds: S = min(4, ceil(768 / workgroups(M, N)), split_ws_bytes / (M N 4)); a shorter last window of the DiT or a
     smaller scratch therefore means another S, i.e. another (equally valid) summation order — whose
     workgroups run side by side and write fp32 partial sums [S][M][N] here; a second launch forms
     y = resid + out_scale (.) ((((s0 + s1) + s2) + s3) + bias) in that fixed order.  Deterministic, but the last bits differ
     from the unsplit launch (one chain per slab instead of the decode kernel's ranges): callers that rely on the row-count
     invariance of ua2_linear (every launch of the LM) leave it NULL.  Needs S * M * N * 4 bytes (4 * M * N * 4 always suffices). */
  float* split_ws;
  size_t split_ws_bytes;
  /* [v8] Summation-order contract of the K sum (enum ua2_sum_order).  UA2_SUM_ORDER_INVARIANT (0, the default): a row's bits are
     those of the decode kernel whatever the row count or the kernel (`waves` partial chains over fixed K ranges, added in wave
     order) — every launch of the LM's fp32 plan and of its bf16 plan below 2048 rows.  UA2_SUM_ORDER_FREE: the order is the
     launcher's choice (one chain over K per slab on the 256-row-tile kernel of csrc/ua2_gemm2.hip; S slabs with split_ws) —
     deterministic for a given (M, N, K, scratch), fp32 rounding noise (~1e-6 relative) against the invariant form; for callers
     outside the LM's row-invariance contract (codec DiT, AudioThinking, Mimi) and, as a plan option, LM launches of >= 2048
     rows.  bf16 only; launches outside the fast kernel's forms silently take the invariant kernels. */
  int32_t sum_order;
  /* [v9] LayerNorm hand-over (UA2_SUM_ORDER_FREE, UA2_EPI_RESIDUAL, UA2_BF16; the codec DiT: attention.py:311-319 / :388-390 behind
     :345-349 / :401-405).  With y_ln_w != NULL the launch also writes, for the K = N GEMM that follows,
         y_packed = RNE_bf16( (y[m] - mean_m) * rstd_m * y_ln_w + y_ln_b ),   mean / rstd over the N columns of y[m] (eps = y_ln_eps),
     in fragment order — F.layer_norm(y) * w + b, the operand its consumer's UA2_PRO_NORM prep launch would build (the consumer then
     takes it as x_packed with UA2_PRO_CAST).  Where the launch runs as K slabs the combine forms it in the same pass (one launch
     instead of combine + prep); otherwise a row pass follows the GEMM.  Only the order-free kernel implements it (N % 4 == 0,
     N <= 2048): ua2_linear_order_free_accepts() tells a caller beforehand whether a launch will be taken; a launch that carries
     y_ln_w and is not is an error.  The statistics are the prep launch's two-pass form (centred variance, the mean carried in two
     parts) summed in this kernel's own order (fp32): same value as the prep launch's to rounding, not to the bit — the order-free
     contract. */
  const float* y_ln_w;
  const float* y_ln_b;
  float y_ln_eps;
  /* [v10] Optional scratch for the RANGE split of row-invariant launches (UA2_SUM_ORDER_INVARIANT, UA2_BF16, UA2_EPI_RESIDUAL, K = 8192,
     33-64 rows: the batched-decode down-projections, lit_model.py:591-595).  The decode kernel adds `waves` partial chains over fixed K
     ranges in range order; with range_ws a launch may run each range on its own workgroups (the range's operand staged once per
     workgroup, wide column groups) and add the partials [waves][ceil(M/16)][ceil(N/16)][256] in a second launch IN THAT ORDER from zero —
     the same sums, the same bits as without it (tests/test_gpu_invariance.py).  Needs waves * ceil(M/16)*16 * ceil(N/16)*16 * 4 bytes
     (16 ranges: 12.6 MB at 64 x 3072), 16-byte aligned; NULL = never.  Measured slower than the one-launch form in the LM's frame
     (profiles/r6_range_split.txt: 15.3 + 5.9 us against 20.4), so the frame executor leaves it NULL unless UA2_RANGE_SPLIT=1. */
  float* range_ws;
  size_t range_ws_bytes;
  ua2_argmax_fold fold;   /* [v10, addition] UA2_PRO_LOCAL_ATTN only; fold.part_max == NULL: off */
} ua2_linear_args;

int ua2_linear(const ua2_linear_args* a, void* stream);
/* The same launch with the weight(s) streamed from their fp8 twins (w1: the second matrix of a SWIGLU launch, else NULL); a->w0 / a->w1
 * still carry the bf16 forms of W'.  Served: UA2_BF16, K % 64 == 0, no more rows than the launchers give the decode kernel (5 by default; UA2_GEMV_MAX_ROWS), no x_packed,
 * the (prologue, epilogue) pairs of the decode frame — NORM or SCALED with QKV_ROPE / SWIGLU / STORE, CAST with RESIDUAL / STORE,
 * LOCAL_ATTN with RESIDUAL.  Anything else is an error (never a silent launch on the bf16 form).  Same grid, waves, chunk ranges and
 * summation order as the bf16 launch of that (N, K): bit-identical outputs.  Counted as "gemv_w8" by ua2_debug_kernel_launches. */
int ua2_linear_w8(const ua2_linear_args* a, const ua2_w8_ref* w0, const ua2_w8_ref* w1, void* stream);
/* [v10, addition] ua2_linear on the 13-bit images of a->w0 (and a->w1 for SWIGLU; both must be escape-free): the launches ua2_linear_w8
 * serves (UA2_BF16, up to ua2_gemv_rows_preferred rows, a prologue / epilogue pair of the decode frame, no x_packed, no argmax fold) with
 * K % 128 == 0; anything else is refused with a message.  Same grid, waves, chunk ranges and summation order as the bf16 launch and the
 * same B fragments: bit-identical outputs.  Counted as "gemv_l13" (and, a decode-kernel launch on bf16 weights, as "gemv") by
 * ua2_debug_kernel_launches. */
int ua2_linear_l13(const ua2_linear_args* a, const ua2_l13_ref* w0, const ua2_l13_ref* w1, void* stream);
/* [v10, addition] The many-row counterpart: one launch on the fp8 twins through the weights-stationary kernel (csrc/ua2_skinny.hip,
 * skinny2_kernel with W8 = true) — the batched decode frame, 6 .. UA2_SKINNY_W8_MAX_ROWS rows (default 64; 0 / "off" = never).  Served: UA2_BF16,
 * K % 64 == 0, more rows than the launchers give the decode kernel, a workspace (or x_packed), a Linear geometry of the released widths
 * (K = 2048 / 3072 / 8192 with a STORE / RESIDUAL / SWIGLU / QKV_ROPE epilogue), prologues NORM / CAST / SCALED (through x_packed).
 * Anything else — fewer or more rows, fp32, GELU, a toy shape, a forced tile variant without an fp8 form — is an error naming this entry
 * point, never a launch on the bf16 form.  Same grid, waves, K ranges, chunk order and range-order sum as the bf16 launch of that shape
 * (the exponent 2^e goes once on the reduced sum): bit-identical to ua2_linear on W' and, row by row, to ua2_linear_w8.  Counted as
 * "skinny2_w8" by ua2_debug_kernel_launches.  ua2_linear_w8 itself keeps refusing more rows than the decode kernel takes. */
int ua2_linear_w8_many(const ua2_linear_args* a, const ua2_w8_ref* w0, const ua2_w8_ref* w1, void* stream);
/* [v9] 1 when a launch with these arguments (sum_order = UA2_SUM_ORDER_FREE) will run on the order-free kernel (csrc/ua2_gemm2.hip) as it
 * stands — shape, alignment, the tile-count rule, scratch for K slabs; 0 when ua2_linear would take the row-invariant kernels instead.
 * Nothing is launched. */
int ua2_linear_order_free_accepts(const ua2_linear_args* a);
/* Bytes of ua2_linear_args.workspace that a launch with these M, K needs (the operand rows in MFMA
 * fragment order, rows padded to 16, K padded to the chunk size). */
size_t ua2_linear_workspace_bytes(int dtype, int64_t M, int64_t K);
/* Test hook, returns the previous setting.  0 (default): the launcher picks — row-tiled decode-regime
 * kernel for one row tile, large-M kernels when a workspace is supplied and M spans more than one.
 * 1: removed (round 1's general-M kernel), treated as 0.
 * 2: never the large-M kernels.  3: a large-M kernel whenever a workspace is supplied, even for M = 1
 * (4: always its skinny form, 5: always its 128-row tiled form).
 * Modes 0, 2, 3, 4 and 5 produce bit-identical results (tests/test_gpu_invariance.py). */
int ua2_debug_force_general_linear(int on);

/* Test hooks (ABI v9).  ua2_debug_kernel_launches: how many launches of a kernel family this process has issued so far —
 * "gemm2" (ua2_gemm2.hip, the order-free many-row GEMM), "gemm" (ua2_gemm.hip's tiled kernel), "skinny2", "skinny2_w8" (the weights-stationary kernel on fp8 weights), "gemv", "gemv_w8" (the decode kernel on fp8 weights), "gemv_l13" (the decode kernel on 13-bit images of its bf16 weights: such a launch counts under "gemv" as well), "rsplit" ([v10] the range split
 * of ua2_skinny.hip: main + combine count once), "text_flush" (calls of ua2_stage3_text_flush that issued their launches), "argmax" (launches of the two greedy tails: arg-max + embedding gather, arg-max + table gather), "score" (calls of ua2_stage3_score that issued their launches), "gemv_hot" / "attn_hot" (decode-kernel / ua2_attn row-by-row launches served by the form that takes its leading arguments as plain kernel parameters: counted besides their families); -1 for an unknown
 * name.  A test that claims "the order-free kernel ran" reads the counter on both sides of the call instead of trusting the
 * launcher's rules.  ua2_debug_refresh_env: the launchers read their UA2_* tuning / A-B environment variables ONCE (they used to
 * call getenv on every launch); a process that changes one of them afterwards (the tests do) calls this to have them read again. */
int64_t ua2_debug_kernel_launches(const char* family);
/* [v10, addition] Test hook: the decode kernel's launch geometry for an [N, K] weight of `dtype` and nt matrices per launch (2 = SWIGLU) —
 * workgroup waves and chunks per wave per round; *multi_round = 1 when a wave walks its range in several double-buffered rounds. */
int ua2_debug_gemv_geometry(int dtype, int32_t N, int32_t K, int32_t nt, int32_t* waves, int32_t* cpw, int32_t* multi_round);
void ua2_debug_refresh_env(void);

/* Measurement helper (bench.py roofline leg): launches args[0..n) back to back `iters` times on
 * `stream`, bracketed by hipEvents recorded on that same stream, waits for the stop event and
 * returns the elapsed milliseconds in *ms_out.  No other work is enqueued in between. */
int ua2_linear_chain_timed(const ua2_linear_args* args, int32_t n, int32_t iters, void* stream, float* ms_out);
/* [v10, addition] The same chain through ua2_linear_l13: launch i on the images w0[i] (and w1[i]; w1 may be NULL when no launch is a
 * SWIGLU one) — the image side of ua2_linear_chain_timed for tools/ubench/gemv_shapes.py. */
int ua2_linear_l13_chain_timed(const ua2_linear_args* args, const ua2_l13_ref* w0, const ua2_l13_ref* w1, int32_t n, int32_t iters, void* stream,
                               float* ms_out);
/* [v10, addition] The same chain through ua2_linear_w8_many: launch i on the fp8 twins w0[i] (and w1[i]; w1 may be NULL when no launch is a
 * SWIGLU one).  Same host path and the same events as ua2_linear_chain_timed, so the two figures of one shape can be compared
 * (tools/ubench/skinny_shapes.py --w8). */
int ua2_linear_w8_many_chain_timed(const ua2_linear_args* args, const ua2_w8_ref* w0, const ua2_w8_ref* w1, int32_t n, int32_t iters, void* stream,
                                   float* ms_out);

/* Decode/prefill attention over the paged cache: one query row per (row, head); one workgroup per (row, kv-head)
 * walks positions 0..row_pos (waves own contiguous ranges, online softmax, fixed-order merge in LDS) and writes the
 * normalised output.  Replaces repeat_interleave + masked SDPA (lit_model.py:478-481, 529-531): GQA without
 * materialising K/V per query head, causal mask = "positions <= row_pos". */
typedef struct ua2_attn_args {
  int32_t dtype;
  int32_t R;              /* query rows */
  const float* q;         /* [R, n_head*head_size] fp32 */
  const int32_t* row_pos; /* [R] */
  const int32_t* row_seq; /* [R] page-table row of each query row; NULL: row r is sequence r */
  ua2_kv_geom kv;
  float* y;               /* [R, n_head*head_size] fp32 normalised output (may be NULL when y_packed is given) */
  int32_t window;         /* > 0 = attend only to the last `window` positions (Moshi `context`,
                             transformer.py:405-406: delta < context); 0 = all positions <= row_pos */
  void* y_packed;         /* optional: the output rounded to `dtype` in the packed operand layout of the
                             O-projection (ua2_linear_args.x_packed), K = n_head*head_size */
  /* Grouped form (prefill of prompts, dense encoders, the DiT): when group_rows != NULL and dtype == UA2_BF16 the rows
     are processed by an MFMA flash kernel with LDS-staged K/V pages instead of row by row.  The host lists, per group,
     up to group_q_tiles * 16 query rows OF ONE SEQUENCE (row indices into q / row_pos, -1 = padding); rows outside every
     group are not computed.  Same arithmetic contract (bf16 K/V, fp32-grade q and softmax), a row's result independent
     of how rows are grouped. */
  const int32_t* group_rows;   /* [n_groups, group_q_tiles * 16] device */
  const int32_t* group_seq;    /* [n_groups] page-table row of the group's sequence */
  const int32_t* group_nkeys;  /* [n_groups] 1 + the largest row_pos in the group (keys visited: 0 .. nkeys-1) */
  int32_t n_groups;
  int32_t group_q_tiles;       /* 16-row tiles per group: 2 with grouped-query heads (n_head > n_kv), 4 with n_head == n_kv */
  int32_t flags;               /* [v8] UA2_ATTN_BF16_QP: the grouped form may round q and the softmax weights to bf16 once (no hi / lo
                                  split) — what torch SDPA under bf16 autocast computes (the codec's DiT, reason_tokenizer.py:265); half the
                                  matrix work.  Served at head size 64, 8 query tiles; ignored (the fp32-grade form runs) elsewhere. */
  void* y_h;                   /* [v10, addition] optional (ua2_attn's row-by-row form, UA2_BF16): the output rounded RNE to bf16, row-major
                                  [R, ldh] — the x_h of an O-projection of one row tile (ua2_linear_args.x_h under UA2_PRO_CAST).  y and
                                  y_packed may then both be NULL.  The grouped form, ua2_attn_local and ua2_attn_relbias refuse it. */
  int32_t ldh;                 /* row stride (elements) of y_h, >= n_head*head_size */
} ua2_attn_args;
#define UA2_ATTN_BF16_QP 1

int ua2_attn(const ua2_attn_args* a, void* stream);
/* Short-context form for the local (depth) decoder (model_new.py:629-641): every row attends to positions
 * 0..row_pos[r], row_pos[r] < 8, all in the first cache page of its sequence.  Uses q, row_pos, row_seq, kv, y
 * of ua2_attn_args ([R, n_head*head_size] fp32 out); exact-operation softmax in position order. */
int ua2_attn_local(const ua2_attn_args* a, void* stream);

/* Producer half of the scaled-norm hand-over (see ua2_linear_args.y_norm_w) for the row-wise kernels that feed a GPT's first
 * layer: besides its fp32 output `o` [M, C] the kernel writes RNE_bf16(o * norm_w) into h (row-major, stride ldh) and / or
 * packed (fragment order), and ssq [M, C / 16] (the same butterfly tree as the linear epilogues).  UA2_BF16; C % 32 == 0. */
typedef struct ua2_handover {
  const float* norm_w;   /* [C] weight of the RMSNorm the consumer folds */
  void* h;               /* [M, ldh] bf16, or NULL */
  int32_t ldh;
  void* packed;          /* [ceil(M/16)][C/32][64 lanes][16 B], or NULL */
  float* ssq;            /* [M, C / 16] */
} ua2_handover;

/* Frame embedding (model_new.py:594-600, 604, 665-673): for each row,
 * audio_sum = sum_i mask[i] * audio_emb[tok[i] + i*V_a]  (i = 0..n_cb-1, in order), text = wte[tok[n_cb]].
 * ho (optional): hand-over of audio_sum to the understanding expert's first layer. */
int ua2_embed_frame(int dtype, int32_t M, int32_t C, int32_t n_cb, int32_t va,
                    const int32_t* tokens /* [M, n_cb+1] */, const uint8_t* mask /* [M, n_cb+1] */,
                    const void* audio_emb, const void* wte, float* audio_sum /* [M,C] */, float* text /* [M,C] */,
                    const ua2_handover* ho, void* stream);

/* Final RMSNorm of a GPT + the step-mask blends (lit_model.py:164; model_new.py:607,610,613):
 *   n = RMSNorm(x)*w ; out1 = n*fa + other*fb ; out2 = n (optional)
 * fa = mask[m, col_a] if col_a >= 0 else 1 ; fb = mask[m, col_b] if other else 0. */
int ua2_rmsnorm_blend(int32_t M, int32_t C, const float* x, const float* w, float eps,
                      const float* other, const uint8_t* mask, int32_t mask_ld, int32_t col_a, int32_t col_b,
                      float* out1, float* out2, const ua2_handover* ho /* optional: hand-over of out1 */, void* stream);

/* The all-NaN rule of the sampling tails (ua2_argmax_embed, ua2_sample_topk, and the executor's internal arg-max + table gather):
 * a NaN score never wins a comparison, so a row whose partial maxima (arg-max) or race scores (top-k: a NaN row, or a row of -inf)
 * are all NaN has no winner.  Such a row takes its LOWEST CANDIDATE id — the lowest part_idx entry of the row for the arg-max
 * forms, the first admitted column (forbid[m], or 0) for ua2_sample_topk — and every tail clamps the id it chose into [0, limit)
 * before it is written to out_tokens and before any gather: limit = V for ua2_sample_topk, the vocabulary for the executor's
 * launches, 16 * n_part (the most ids the partials can describe) for the exported ua2_argmax_embed.  A NaN partial next to
 * finite ones simply loses.  The token written and the row gathered are always the same in-range value. */
/* Greedy sampling tail (model_new.py:146-187 with topk=1; lowest index wins ties) fused with
 * the next-step embedding gather (model_new.py:640,662-663):
 *   tok = argmax over the per-tile partials; out_tokens[m*out_ld + out_col] = tok;
 *   if emb: next_h[m,:] = emb[tok + emb_row_offset, :]  */
int ua2_argmax_embed(int dtype, int32_t M, int32_t n_part, const float* part_max, const int32_t* part_idx,
                     int32_t* out_tokens, int32_t out_ld, int32_t out_col,
                     const void* emb, int32_t emb_row_offset, int32_t C, float* next_h, void* stream);

/* [v10, addition] Cross-entropy tail of the teacher-forced pass (model_new.py:402-454 forward, :59-109 CrossEntropyAndAccuracy_*),
 * over the raw fp32 logits — forbid_prefix, guidance and the arg-max partials are never consulted.  Per row m, with
 * label = labels[m * label_ld + label_col]:
 *   nll[m * out_ld + out_col]  = lse(logits[m, :V]) - logits[m, label], the row maximum subtracted before the exponentials; 0 for
 *                                label == -1 (ignored).  A -inf target gives +inf; a row of -inf, or one that holds a NaN, gives NaN
 *                                (as F.cross_entropy does);
 *   pred[m * out_ld + out_col] = the arg-max, lowest index on ties, under the all-NaN rule and the clamp into [0, V) above;
 *   emb != NULL: emb_out[m, :C] = emb[emb_row0 + label, :] — the gather of ua2_argmax_embed, of the LABEL's row instead of the chosen
 *                id's (teacher forcing); label == -1 gathers row emb_row0.  The label is clamped into [0, V) before the gather; callers
 *                reject labels outside [-1, V) on the host.
 * One workgroup per row and one summation order per row whatever M is: a row's nll bits do not depend on the rows beside it. */
int ua2_xent_embed(int dtype, int32_t M, const float* logits, int32_t ld, int32_t V,
                   const int32_t* labels, int32_t label_ld, int32_t label_col,
                   float* nll, int32_t* pred, int32_t out_ld, int32_t out_col,
                   const void* emb, int64_t emb_row0, int32_t C, float* emb_out, void* stream);

/* Classifier-free guidance (model_new.py:618-622, 634-637) over `pairs` (conditional, unconditional) pairs of logit rows
 * (rows 2p, 2p + 1 of [2 pairs, ld] fp32; the reference has one pair, batched generation has one per utterance):
 * guided = l1 + (l0 - l1) * scale, written to BOTH rows of the pair, and the per-16-column arg-max partials of both rows
 * ([2 pairs, ceil(V/16)], same format and tie rule as UA2_EPI_STORE; columns < forbid[2p] excluded) rebuilt from it, so
 * ua2_argmax_embed / ua2_sample_topk run unchanged and both rows continue from the same token. */
int ua2_cfg_mix(float* logits, int32_t ld, int32_t V, float scale, const int32_t* forbid, float* part_max,
                int32_t* part_idx, int32_t pairs, void* stream);

/* Top-k sampling tail (model_new.py:146-187 with topk > 1: temperature, forbid_prefix, keep logits >= the
 * k-th largest, exponential-race multinomial draw) + next-step embedding gather.  Philox4x32-10 keyed by
 * (seed + device seed word, draw index, row, stream_id) where `counter` is a DEVICE int32[3]: [0] = draw index,
 * [1], [2] = low / high half of a 64-bit word added to `seed` (zeros for a purely by-value seed; the frame
 * executor keeps its seed there so that one captured graph serves every seed).  Reproducible under graph replay;
 * it does not reproduce torch's generator stream (parity with the reference is distributional).
 * The draw, stated so that it can be replayed on the host (tests/sampler_refs.py does, id by id): for every kept column c,
 *   r = Philox4x32-10(counter = (c, draw index, row part, stream_id), key = (lo, hi) of (seed + device seed word) mod 2^64),
 *   x = r[0] >> 8,  u = fminf(RN(x + 0.5f) * 2^-24, 1 - 2^-24)  (fp32; strictly inside (0, 1): RN(x + 0.5f) is 2^24 at x = 2^24 - 1,
 *   and u = 1.0f would make q = -0.0f and the score -inf for the very column that drew the smallest q),
 *   q = -logf(u),  score = expf(l_c - mx) / q with mx = the largest admitted l;  the id is the arg-max, the LOWEST column among
 *   equal scores.  Draw index and seed words are read as unsigned 32-bit values; the carry of the low into the high key half counts.
 * row_key_shift (0 or 1): the row part of the key is m >> row_key_shift — 1 makes the two rows of a guidance pair draw the
 * same numbers (they hold the same guided logits: both continue from one sample, model_new.py:622). */
int ua2_sample_topk(int dtype, int32_t M, const float* logits, int32_t ld, int32_t V, int32_t topk, float temperature,
                    const int32_t* forbid, uint64_t seed, const int32_t* counter, int32_t stream_id,
                    int32_t* out_tokens, int32_t out_ld, int32_t out_col, const void* emb, int32_t emb_row_offset,
                    int32_t C, float* next_h, int32_t row_key_shift, void* stream);

/* [v10, addition] The same tail with one random stream PER ROW, read from device memory: row_key [M][2] int32 = the row's 64-bit seed
 * (lo, hi), row_draw [M] int32 = the row's own draw index.  Philox4x32-10 keyed by (column, row_draw[m], 0, stream_id) under row_key[m]:
 * neither the row index nor a shared counter enters, so a row's ids depend on nothing but its logits, its key and its draw — row m is
 * bit-identical to a one-row ua2_sample_topk launch with seed 0, the device seed word row_key[m] and the draw index row_draw[m].
 * Rows that hold equal (key, draw, logits) — the two rows of a guidance pair — draw equal ids.  Radix select, exponential race, forbid
 * prefix, the all-NaN rule and the gather are ua2_sample_topk's (one device function).  Nothing is written to row_key / row_draw. */
int ua2_sample_topk_rows(int dtype, int32_t M, const float* logits, int32_t ld, int32_t V, int32_t topk, float temperature,
                         const int32_t* forbid, const int32_t* row_key, const int32_t* row_draw, int32_t stream_id,
                         int32_t* out_tokens, int32_t out_ld, int32_t out_col, const void* emb, int32_t emb_row_offset,
                         int32_t C, float* next_h, void* stream);

/* [v10, addition] Nucleus (top-p) sampling: ua2_sample_topk / ua2_sample_topk_rows with one more filter between the top-k threshold and
 * the race (llm_utils/sampling.py:66-82 sample_top_p, :85-105 sample_token(..., top_k, top_p)).  Per row, with l_c = logits[c] / T over
 * the columns c in [forbid, V), K = the top-k kept set exactly as above (key(l_c) >= the k-th largest key; topk = V admits every
 * column), mx = max l_c and e_c = expf(l_c - mx), the very values the race computes:
 *   the nucleus keeps column c of K iff the mass of the columns of K whose value is STRICTLY GREATER than l_c is at most top_p times
 *   the mass of K.
 * This is the reference's `mask = probs_sum - probs_sort > p` without the sort, with one departure: columns that tie at the threshold
 * value are all kept (the tie rule of the top-k filter), where torch.sort would split the tie arbitrarily — probabilities
 * [.4, .2, .2, .1, .1] under top_p = .5 keep 3 columns here, 2 there.  The race then runs over the nucleus with the same Philox counter
 * per column (column, draw, row part, stream_id) and the same score e_c / q: a row whose top-k-only id lies in the nucleus draws the
 * same id, and pure nucleus sampling is topk = V.
 * The masses are summed in integers, so that the kept set — and with it the row's id — is a function of the row's logits alone, not of
 * thread scheduling, atomic order or launch geometry:
 *   q_c = (uint64) floor(e_c * 2^40), 0 for a NaN or non-finite e_c;  Z = sum of q_c over K (at most 2^57 for V <= 2^17: a larger V is
 *   refused);  P = (uint64) floor((double) top_p * 2^32);  S_gt(c) = sum of q_j over the j of K with key(l_j) > key(l_c);
 *   c is kept iff S_gt(c) * 2^32 <= P * Z, compared exactly in 128 bits.
 * Z == 0 (a row of -inf or NaN): no nucleus filter, the all-NaN rule above decides.  A NaN column (the largest key, mass 0) next to
 * finite ones stays admitted and loses the race, as in ua2_sample_topk.
 * top_p == 0 and top_p >= 1 mean OFF: ids and gathered rows are bit-identical to the top-k launch (with keep_count == NULL it IS that
 * launch).  top_p outside [0, 1] or NaN, or V > 131072, is an error and nothing is launched.
 * keep_count: optional [M] int32 (NULL = off) — the number of columns of row m that entered the race (the nucleus size; |K| when off).
 * The threshold value is found by a weighted 4-pass radix select on the keys (256 buckets of uint64 mass per pass, native LDS 64-bit
 * adds, runs of equal buckets summed per thread and per wave first); one 1024-thread workgroup per row, like the top-k tail. */
int ua2_sample_topp(int dtype, int32_t M, const float* logits, int32_t ld, int32_t V, int32_t topk, float temperature,
                    const int32_t* forbid, uint64_t seed, const int32_t* counter, int32_t stream_id,
                    int32_t* out_tokens, int32_t out_ld, int32_t out_col, const void* emb, int32_t emb_row_offset,
                    int32_t C, float* next_h, int32_t row_key_shift, float top_p, int32_t* keep_count, void* stream);
/* [v10, addition] ... with one random stream per row (ua2_sample_topk_rows): row m equals a one-row ua2_sample_topp launch with that key
 * and draw, bit for bit; nothing is written to row_key / row_draw. */
int ua2_sample_topp_rows(int dtype, int32_t M, const float* logits, int32_t ld, int32_t V, int32_t topk, float temperature,
                         const int32_t* forbid, const int32_t* row_key, const int32_t* row_draw, int32_t stream_id,
                         int32_t* out_tokens, int32_t out_ld, int32_t out_col, const void* emb, int32_t emb_row_offset,
                         int32_t C, float* next_h, float top_p, int32_t* keep_count, void* stream);

/* [v10, addition] Repetition penalty over a window of the ids a sampler has produced: the four tails above (top-k / nucleus x shared
 * stream / per-row streams) behind ONE entry point, each optionally penalised.  Not in the reference (an opt-in extension; its effect on
 * audio quality is NOT measured: no trained checkpoint ships).  The rule is the CTRL / Hugging Face RepetitionPenaltyLogitsProcessor
 * rule restricted to a window, stated so that a host can replay it exactly.
 *
 * The form of the launch: row_key / row_draw non-NULL = per-row streams (ua2_sample_topk_rows: seed, counter, row_key_shift unused),
 * else the shared stream (ua2_sample_topk: seed, counter, row_key_shift); 0 < top_p < 1 = the nucleus filter, top_p == 0 = off;
 * keep_count as in ua2_sample_topp.  Every other field up to keep_count is the argument of that name of the four entries.
 *
 * History ring of row m: ring = rep_hist + m * rep_hist_ld (rep_cap int32 slots), n = rep_len[m * rep_len_ld] = the number of ids
 * appended to the ring so far (a negative n reads as 0).  Entry j (j = 0 the oldest id ever appended) lives in ring[j % rep_cap]; the
 * entries still stored are j in [max(0, n - rep_cap), n).  An append of id writes ring[n % rep_cap] = id and rep_len becomes n + 1 (it
 * counts every append and does not saturate; n < 2^31 - 1 is the caller's to keep, by starting the row anew).  A row starts with
 * rep_len = 0; the slots need no initial value.
 *
 * The penalty: S = the set of distinct ids in [0, V) among entries j in [n - min(n, rep_window), n).  For c in S the sampler reads
 *   l'_c = (l_c < 0) ? l_c * rep_penalty : l_c / rep_penalty
 * in place of the fp32 logit l_c = logits[m * ld + c]: one IEEE-754 round-to-nearest fp32 multiply or divide, applied ONCE per distinct
 * id however often it occurs in the window; -0.0, +0.0, -inf and NaN follow from the expression (-0.0 and +0.0 take the divide, NaN
 * stays NaN).  Columns outside S read l_c.  The penalty comes before the temperature division; everything downstream is the tail of
 * that form on l' — forbid prefix (a penalised column below it stays forbidden), top-k threshold on key(l' / T), nucleus filter, the
 * Philox race under the same counters, tie rule, all-NaN rule, embedding gather.  The logits buffer is only read.
 * After the draw the id written to out_tokens is appended to the row's ring (if 0 <= id < V, which the tail's clamp guarantees).
 *
 * Equivalence: the launch on (logits, history) is bit for bit the launch of the same form on logits whose columns in S hold l' — equal
 * ids, equal gathered next_h rows.  Row invariance: a block reads and writes only its own row's ring and counter, so a row's id depends
 * on its logits, its key and draw and its own history alone; the two rows of a guidance pair (equal logits, keys, histories) draw and
 * append equal ids.
 *
 * rep_hist == NULL, or rep_penalty == 1: OFF — the call IS the existing launch of that form, and a supplied history is neither read nor
 * written.  With rep_hist != NULL: rep_penalty must be finite and > 0 and 1 <= rep_window <= 512; when penalised also V <= 131072 (the
 * V-bit membership set in LDS: 16 KB), rep_len != NULL, rep_cap >= rep_window, rep_hist_ld >= rep_cap, rep_len_ld >= 1.  Anything else is
 * an error and nothing is launched.  One 1024-thread workgroup per row: the set is filled with LDS atomic ORs (which de-duplicates), and
 * every pass of the tail reads its logit through the same helper. */
typedef struct {
  int32_t dtype, M;
  const float* logits;
  int32_t ld, V, topk;
  float temperature;
  const int32_t* forbid;
  uint64_t seed;                    /* shared stream */
  const int32_t* counter;
  int32_t row_key_shift, stream_id;
  const int32_t *row_key, *row_draw;   /* per-row streams: both non-NULL */
  int32_t* out_tokens;
  int32_t out_ld, out_col;
  const void* emb;
  int32_t emb_row_offset, C;
  float* next_h;
  float top_p;
  int32_t reserved;
  int32_t* keep_count;
  float rep_penalty;                /* theta; 1 = off */
  int32_t rep_window, rep_cap, rep_hist_ld, rep_len_ld, reserved2;
  int32_t* rep_hist;                /* NULL = off */
  int32_t* rep_len;
} ua2_sample_args;
int ua2_sample_penalized(const ua2_sample_args* a, void* stream);

/* n-gram repeat filter of the text loop (evaluation/asr_task.py:329-432 generate_asr_with_ngram_sampling, :407-432).  Row r
 * (r < R): candidate c = out[r * ld], generated ids H = hist[r * cap ...], L = hist_len[r] of them.  c is replaced by `fallback`
 * when the n-gram (last n - 1 ids of H, c) already occurs in H; the final id is appended to H when L < cap and hist_len[r] becomes
 * L + 1.  Nothing is written at or past cap; a row with L > cap passes c through unfiltered (its suffix is no longer stored).
 * 2 <= n <= 16.  One 256-thread workgroup per row. */
int ua2_ngram_filter(int32_t* out, int32_t ld, int32_t R, int32_t n, int32_t fallback,
                     int32_t* hist, int32_t* hist_len, int32_t cap, void* stream);

/* ---- beam search over the text head (entry points added under ABI v10) -------------------------------------
 * The W <= 8 hypotheses ("slots") of a beam are rows 0 .. W - 1 of a decode frame.  All state lives in caller-owned device buffers:
 *   score [W] fp32, fin [W] (0 live, 1 finished, 2 dead = holds no hypothesis), len [W] text ids so far, parent [W] (written by a step),
 *   ctrl [4]: [0] steps run, [1] the step at which all W slots were first finished (-1 until then), [2..3] unused,
 *   cand_logp / cand_id [W, 8]: scratch between the two launches of a step,
 *   log [log_cap, W, 4] int32: per step and slot (parent, text id or -1, score bits, fin) — the host recovers a hypothesis's text by
 *   walking the log backwards; a step at or past log_cap is not logged,
 *   lp_inv [lp_n] fp32: 1 / lp(L), lp(L) = ((5 + L) / 6) ** length_penalty, computed by the host in float64 (index clamped to lp_n - 1).
 * Start: score = (0, -inf, ..), fin = (0, 2, ..), len = 0, ctrl = (0, -1, 0, 0). */
typedef struct ua2_beam_state {
  float* score;
  int32_t* fin;
  int32_t* len;
  int32_t* parent;
  int32_t* ctrl;
  float* cand_logp;
  int32_t* cand_id;
  int32_t* log;
  int32_t log_cap;
  const float* lp_inv;
  int32_t lp_n;
} ua2_beam_state;
/* One step of the rule on logits [W, ld] fp32 (V columns used, W <= V <= ld).  Slots in slot order: a finished slot contributes
 * itself; a live slot its W largest logits (NaN ordered as -inf; lowest id first among equals) in rank order with
 * logp = (x - m) - logf(S), m the row maximum, S = sum of expf(x - m) as 1024 strided partial sums (column c in partial c % 1024,
 * ascending c) joined by a fixed halving tree — the launch geometry (one 1024-thread workgroup per live row) is part of the contract.
 * Column eos: the slot finishes, len unchanged, score + logp * lp_inv[len]; any other column k: len + 1, score + logp * lp_inv[len + 1],
 * text id k (one rounded fp32 product, one rounded fp32 sum).  The new beam = the W candidates of highest score, equal scores in
 * candidate order.  Writes score / fin / len / parent, token[j * token_ld] = the id slot j feeds back (0 for a finished slot;
 * every id clamped into [0, V)), the log record, ctrl.  An eos outside [0, V) never matches.  Two launches. */
int ua2_beam_step(const float* logits, int32_t ld, int32_t V, int32_t W, int32_t eos, const ua2_beam_state* st,
                  int32_t* token, int32_t token_ld, void* stream);
/* One K or V pool of a paged cache for the fork: [pages, n_kv, 64, head_bytes / element size]; table = index of its page table. */
typedef struct ua2_beam_pool {
  void* pool;
  int32_t table;
  int32_t n_kv;
  int32_t head_bytes;   /* bytes of one position of one head: a multiple of 16 */
  int32_t reserved;
} ua2_beam_pool;
/* The K/V fork behind a step (or, parent == NULL: all parents 0, the start).  Page tables [table_rows, max_pages] in the static layout
 * (sequence b owns pages b * max_pages ..), table_rows >= 2 W; every pool holds table_rows * max_pages pages.  Slot j (row j of the
 * tables), n = row_pos[j] + pos_add the next position it writes (pos_add 0: before the first frame, 1: behind a frame's trunk),
 * c = n / 64, p = parent[j] (clamped into [0, W)):
 *   table[j][col < c] = OLD table[p][col]   (full pages are shared, never written again),
 *   table[j][c] = page ((n & 1) * W + j) * max_pages + c   (its own page of page set n & 1: the sets alternate from step to step, so
 *                 the pages read and the pages written by one call are disjoint),
 *   positions [0, n % 64) of OLD table[p][c] are copied to that page in every pool (16-byte accesses; nothing when n % 64 == 0 or the
 *   two pages are the same).  A position at or past 64 * max_pages changes no column and copies nothing.
 * pools: DEVICE array of n_pools descriptors (bf16 and fp32 pools alike: bytes are copied); tables: host array of n_tables <= 3 device
 * pointers.  Two launches (copy, then tables). */
int ua2_beam_reorder(int32_t W, const int32_t* parent, const int32_t* row_pos, int32_t pos_add, const ua2_beam_pool* pools,
                     int32_t n_pools, int32_t* const* tables, int32_t n_tables, int32_t table_rows, int32_t max_pages, void* stream);
/* Several beams in one frame (added under ABI v10 like the entry points above, which are their G = 1 case: same kernels, same bits).
 * G >= 1 groups (utterances) of W <= 8 slots, G * W <= 64; group g's slot j is row r = g * W + j of the frame.  The structs keep their
 * layout; group g's state lies at fixed strides from the base pointers of ua2_beam_state:
 *   score / fin / len / parent + 8 g,  ctrl + 4 g,  cand_logp / cand_id + 64 g,  log + g * log_cap * W * 4  (its [log_cap, W, 4] log);
 * lp_inv, lp_n, log_cap and eos are shared.  Every group starts as a single beam does.
 * ua2_beam_step_groups: logits [G * W, ld], token rows g * W + j.  One 1024-thread workgroup per live row (the contract of the
 *   log-sum-exp above), then one workgroup per group that reads and writes only that group's state, token rows and log; group g's
 *   ctrl[1] latches the step at which all ITS slots were first finished.  A group whose slots are all finished is a fixed point of the
 *   step, so it can keep running beside live ones.  A group's result does not depend on the other groups.
 * ua2_beam_reorder_groups: parent strided 8 per group, values local to the group (0 .. W - 1; NULL: slot 0 of each group);
 *   row_pos [G * W].  With R = G * W the two page sets are R-based: row r's own page for position n is
 *   ((n & 1) * R + r) * max_pages + n / 64, and the parent of row g * W + j is row g * W + parent[8 g + j].  The table launch runs one
 *   workgroup per group over its W rows (shared memory W * max_pages * 4 <= 48 KB); a group touches only its own table rows and
 *   its own rows of the two page sets.  Checked before any launch: 1 <= W <= 8, G >= 1, G * W <= 64, table_rows >= 2 G W. */
int ua2_beam_step_groups(const float* logits, int32_t ld, int32_t V, int32_t W, int32_t G, int32_t eos, const ua2_beam_state* st,
                         int32_t* token, int32_t token_ld, void* stream);
int ua2_beam_reorder_groups(int32_t W, int32_t G, const int32_t* parent, const int32_t* row_pos, int32_t pos_add,
                            const ua2_beam_pool* pools, int32_t n_pools, int32_t* const* tables, int32_t n_tables,
                            int32_t table_rows, int32_t max_pages, void* stream);
/* The step under a no-repeat-n-gram ban (added under ABI v10 like the entry points above; opt-in — the reference's
 * `_apply_ngram_constraint`, evaluation/asr_task.py:602-628, bans an always-empty set, and the entry points above reproduce that).
 *   n: 0 = off, or 2 .. 16;  cap: ids one history holds (>= 1);
 *   hist [G][2][8][cap] int32, caller-owned: per group two sets of 8 histories.  A step reads set (ctrl[0] & 1) of its group — slot
 *   j's text ids h[0 .. L), L = len[j] — and writes the other set: for every new LIVE slot t the history of parent[t] plus the new id.
 *   Finished and dead slots keep no history.  Start: len = 0, so the content of hist does not matter.
 * The rule, for a live slot with L >= n:  p = h[L - n + 1 .. L),  ban = { h[i + n - 1] : 0 <= i <= L - n, h[i .. i + n - 1) == p }
 * (the EOS id is never part of a history, hence never banned); the banned columns count as -inf in the row maximum, in S and in the
 * top-W selection — mask, then softmax.  Everything else is the contract of ua2_beam_step above, so
 *   - a banned step on a row x owes bit for bit what ua2_beam_step_groups owes on x with the banned columns overwritten by -inf;
 *   - a group's result depends only on its own rows and histories.
 * Finished and dead slots read no logits and ban nothing.  L < n bans nothing; a slot with L > cap is not filtered (like
 * ua2_ngram_filter); nothing is written at or past cap; history ids are clamped into [0, V) before they index anything.  The logits
 * are read-only: the ban is a bitmap over the V columns in shared memory ((V + 31) / 32 words <= 48 KB).
 * ng == NULL or ng->n == 0: exactly ua2_beam_step_groups (the same two launches).  Checked before any launch: n in {0, 2 .. 16},
 * cap >= 1, hist non-NULL when n >= 2.  Two launches (1024 threads per live row; 256 per group: the copy of the histories). */
typedef struct ua2_beam_ngram {
  int32_t n;
  int32_t cap;
  int32_t* hist;
} ua2_beam_ngram;
int ua2_beam_step_groups_ngram(const float* logits, int32_t ld, int32_t V, int32_t W, int32_t G, int32_t eos, const ua2_beam_state* st,
                               const ua2_beam_ngram* ng, int32_t* token, int32_t token_ld, void* stream);

/* ---- codec: residual vector quantisation ------------------------------------------------ */

/* Nearest-codeword search, level by level on the residual (core_vq.py:179-185, 365-376; the live codec's
 * ResidualVQ calls AudioDiffusion1D.py:388,529,535,544).  x [N,D] fp32 in codebook space (after any
 * project_in), emb [L,C,D] fp32, embT [L,D,C] = the same codebooks k-major (coalesced scan).
 * codes [N,L] int32; quantized [N,D] = sum of the chosen codewords (may be NULL).
 * d2 = sum_k fma(x_k-e_k, x_k-e_k, .), k ascending; lowest index wins ties (= oracle/rvq_oracle.c bit for bit).
 * workspace (optional, >= ua2_rvq_workspace_bytes(N, L) bytes of device scratch): lets a launch with few vectors (one
 * clip) split each level's codebook over several workgroups per group of 8 vectors (candidates merged by 64-bit atomic
 * min, lowest index on ties); same codes and sums with or without it.  The workgroups of a split launch wait for each
 * other with BOUNDED spins; if one expires (a peer held back by another stream / process) the launch raises a device
 * flag and a second, self-contained launch behind it on the same stream — a no-op when the flag is clean — recomputes
 * every vector: rc 0 always means oracle-exact codes.  ua2_rvq_fallbacks counts how often that happened (health counter;
 * synchronous copy from the device).  The second launch is enqueued on EVERY split encode (its workgroups read the flag and
 * return when it is clean: ~2 us of launch + boundary per encode against the 51 us search — measured, profiles/r3_rvq.txt — the
 * price of never needing a host round trip to learn whether the spin expired).  Env UA2_RVQ_SPIN_LIMIT overrides the spin bound (tests force the path with 0). */
int ua2_rvq_encode(const float* x, const float* emb, const float* embT, int64_t N, int32_t L, int32_t C, int32_t D,
                   int32_t* codes, float* quantized, void* workspace, size_t workspace_bytes, void* stream);
size_t ua2_rvq_workspace_bytes(int64_t N, int32_t L);
int ua2_rvq_fallbacks(uint32_t* out);
/* Lookup + sum over levels (core_vq.py:378-384; AudioDiffusion1D.py:577-583 get_output_from_indices). */
int ua2_rvq_decode(const int32_t* codes, const float* emb, int64_t N, int32_t L, int32_t C, int32_t D, float* out,
                   void* stream);

/* ---- codec: 1-D convolutions -------------------------------------------------------------- */

enum ua2_act { UA2_ACT_NONE = 0, UA2_ACT_PRELU = 1, UA2_ACT_ELU = 2, UA2_ACT_TANH = 3, UA2_ACT_ROUND9 = 4 };

/* out[b][co][t] = post( bias[co] + sum_{ci,j} W[co][ci][j] * pre(x[b][ci][(t*stride + j*dilation - pad_left)/in_repeat]) )
 *                 (+ residual[b][co][t]),   zero outside [0, Tin*in_repeat).
 * Covers scalar24k.py Conv1d :36-74 (causal: pad_left = d(k-1); else symmetric) and conv.py StreamingConv1d
 * :232-254 (pad_left = k_eff - stride, right pad implied by Tout); PReLU/ELU/tanh/round9 fused before or
 * after; in_repeat = repeat-upsampling (scalar24k.py:136-138).
 * Transposed conv (scalar24k.py:76-112, conv.py:306-329): out_phases = stride P, `w` holds the P phase
 * filters stacked (rows phase*Cout + co, taps of a phase in descending order: ua2 host helper
 * pack_convtr_weight), K = taps per phase, pad_left = K - 1, stride = dilation = 1; result written to
 * y[co][t*P + phase - out_trim_left], Tout = final (trimmed) length.
 * w: ua2_pack_linear(fp32) of the [rows, Cin_pad*K] matrix, Cin padded with zeros to a multiple of 16.
 * precision = 1 ("bf16 x 3"): every fp32 operand is split into two bf16 halves and the product taken as
 * Wh Xh + Wh Xl + Wl Xh on the bf16 MFMA with fp32 accumulation (~2^-16 relative per product instead of exact; 5x the
 * matrix rate).  w / w_lo then hold the hi / lo halves, each ua2_pack_linear(bf16) of the [rows, G*K*32] matrix whose
 * reduction index is (channel group of 32, tap, channel in group), Cin zero-padded to a multiple of 32 (host helper
 * ops.pack_conv_weight_x3). */
typedef struct ua2_conv1d_args {
  int32_t B, Cin, Cout, Tin, Tout;
  int32_t K, stride, dilation, pad_left;
  int32_t in_repeat, out_phases, out_trim_left;
  int32_t pre_act, post_act;       /* enum ua2_act */
  const float* x;                  /* [B, Cin, Tin] fp32 */
  const void* w;                   /* packed fp32 */
  const float* bias;               /* [Cout] or NULL */
  const float* pre_alpha;          /* PReLU slope for pre_act (1 value) or NULL */
  const float* post_alpha;         /* PReLU slope(s) for post_act */
  int32_t post_alpha_n;            /* 1 or Cout */
  const float* residual;           /* [B, Cout, Tout] or NULL, added after post_act (scalar24k.py:151) */
  float* y;                        /* [B, Cout, Tout] */
  const void* w_lo;                /* precision 1: packed bf16 low halves of the filter */
  int32_t precision;               /* 0 = exact fp32 (f32-input MFMA), 1 = bf16 x 3 */
  /* precision 1, optional: fused residual unit (scalar24k.py:143-151) — y = residual + PReLU(alpha2, W2 h + bias2) with
     h = post_act(conv(x) + bias) kept on chip; W2 a 1 x 1 conv [Cout, Cout] packed like w / w_lo (pack_conv_weight_x3 of
     [Cout, Cout, 1]).  Needs Cin == Cout in {32, 64, 128}, stride 1, Tin == Tout, residual. */
  const void* w2;
  const void* w2_lo;
  const float* bias2;              /* [Cout] or NULL */
  const float* alpha2;             /* PReLU slope (1 value) of the second activation, NULL = 0 (ReLU) */
} ua2_conv1d_args;

int ua2_conv1d(const ua2_conv1d_args* a, void* stream);
/* [v10, addition] Test hook: what ua2_conv1d would launch for *a — the launcher's own selection code, nothing launched, no pointer of
 * *a dereferenced (they are only tested for NULL, as by ua2_conv1d; a geometry ua2_conv1d rejects is rejected here with the same message).
 * Reads UA2_CONV_PIPE exactly as the launcher does.  kernel: 0 = exact fp32, 1 = bf16 x 3 plain, 2 = bf16 x 3 pipelined.  ntt: 16-step
 * time tiles per wave.  rt: wave row-groups per workgroup (exact kernel: 4).  Pipelined kernel: tpw = consecutive time tiles per
 * workgroup, gpu = channel groups per unit, npg = instantiated position groups, nw = waves per workgroup (8: the fused 128-channel
 * unit).  Other kernels: tpw = 1, npg = 0, nw = 4; gpu = 0 (exact) or the row tiles per wave, RPW (plain bf16 x 3). */
int ua2_debug_conv1d_plan(const ua2_conv1d_args* a, int32_t* kernel, int32_t* ntt, int32_t* rt, int32_t* tpw, int32_t* gpu,
                          int32_t* npg, int32_t* nw);
/* ---- codec decode side: convolutions on "time-major split planes" (round 4) --------------------------------------
 * Between the layers of the waveform DECODER (scalar24k.py:403-407: ScalarModel.decode = Conv1d -> N x ResDecoderBlock
 * [ConvTranspose1d up-sampler -> 5 dilated ResidualUnits, :143-151] -> PostProcessor -> Conv1d) activations travel as two
 * bf16 planes hi = RNE(x), lo = RNE(x - hi) (16 significant bits, the same 4 bytes per element as fp32), each laid out
 * [B][T][C] — time-major, channels contiguous — instead of fp32 [B][C][T].  The layout is what the bf16 x 3 matrix-pipe
 * form consumes (an MFMA B fragment = 8 consecutive channels of one time step), so a layer's input window goes from L2
 * to LDS by LDS-DMA (global_load_lds, no register staging, no conversion, no transposing LDS writes) and the epilogue of
 * every layer emits the next layer's operand.  C must be a multiple of 32 (channel groups of the MFMA K dimension).
 * Arithmetic per output: the ua2_conv1d precision-1 sum (chunks = (channel group, tap) ascending; per chunk Wl*Xh, Wh*Xl,
 * Wh*Xh), bias added once, PReLU with single roundings, residual x = hi + lo (exact in fp32) added last, then the hi / lo
 * split.  Three kernels with identical bits (`variant`): 1 = plain (any K <= 32, reference of the bit-identity test),
 * 2 = software-pipelined LDS-DMA form (K in {1, 2, 7}), 3 = big-tile form (fused residual units of 32 / 64 channels: one 512- / 1024-step
 * tile per 8-wave workgroup), 0 = automatic (big-tile for those units, pipelined otherwise, plain as the fallback). */
typedef struct ua2_convtc_args {
  int32_t B, Cin, Cout, Tin, Tout;
  int32_t K, dilation, pad_left;   /* stride is 1 on the decode side */
  int32_t in_repeat;               /* input row of window position p is p / in_repeat (repeat-upsampling, scalar24k.py:136-140) */
  int32_t out_phases, out_trim_left; /* transposed conv as out_phases phase filters: packed row n = phase * Cout + co lands at
                                      y[t * out_phases + phase - out_trim_left][co] (see ua2_conv1d) */
  int32_t post_act;                /* UA2_ACT_NONE or UA2_ACT_PRELU */
  int32_t variant;                 /* 0 auto (fused 32- / 64-channel residual units: the big-tile kernel; everything else the pipelined one,
                                      the plain one for shapes outside both), 1 plain, 2 pipelined, 3 big-tile (error if the shape is outside
                                      the requested kernel's instantiations).  All three give identical bits. */
  const uint16_t* x_hi;            /* [B, Tin, Cin] bf16 */
  const uint16_t* x_lo;
  const void* w;                   /* ops.pack_conv_weight_x3 of the [rows, Cin, K] filter: hi ... */
  const void* w_lo;                /* ... and lo halves */
  const float* bias;               /* [Cout] or NULL */
  const float* post_alpha;         /* PReLU slope(s) */
  int32_t post_alpha_n;            /* 1 or Cout */
  /* fused residual unit (scalar24k.py:143-151): y = x + PReLU(alpha2, W2 h + bias2), h = post_act(conv(x) + bias) kept on
     chip; needs Cin == Cout in {32, 64, 128}, out_phases == 1, in_repeat == 1, Tin == Tout.  The residual is the input. */
  const void* w2;
  const void* w2_lo;
  const float* bias2;
  const float* alpha2;             /* 1 value; NULL = slope 0 */
  /* separate residual (the un-fused second conv of a wide residual unit): added after the activation */
  const uint16_t* res_hi;          /* [B, Tout, Cout] bf16 or NULL */
  const uint16_t* res_lo;
  /* output: planes, or fp32 [B, Cout, Tout] (the waveform: last layer) — exactly one of (y_hi & y_lo) / y_f32 */
  uint16_t* y_hi;
  uint16_t* y_lo;
  float* y_f32;
} ua2_convtc_args;

int ua2_conv1d_tc(const ua2_convtc_args* a, void* stream);
/* fp32 [B, C, T] -> planes [B, T, C] (hi, lo) and back (x = hi + lo, exact).  C % 2 == 0. */
int ua2_tc_pack(const float* x, uint16_t* hi, uint16_t* lo, int32_t B, int32_t C, int32_t T, void* stream);
int ua2_tc_unpack(const uint16_t* hi, const uint16_t* lo, float* y, int32_t B, int32_t C, int32_t T, void* stream);

/* torch.nn.AvgPool1d(kernel_size=k) over the last axis of [rows, Tin] (scalar24k.py:118). */
int ua2_avgpool1d(const float* x, float* y, int64_t rows, int32_t Tin, int32_t k, void* stream);

/* Depthwise (groups == channels) 1-D convolution / transposed convolution, exact fp32, taps in ascending order:
 *   conv:   y[b,c,t] = bias[c] + sum_j w[c,j] * x[b,c, t*stride + j*dilation - pad_left]      (zero outside)
 *   convtr: y[b,c,t] = bias[c] + sum_{ti*stride + j == t + pad_left} w[c,j] * x[b,c,ti]        (pad_left = left trim)
 * Replaces the channel-wise resamplers of tools/tokenizer/MimiCodec/model/modules/resample.py:13-119
 * (nn.Conv1d / nn.ConvTranspose1d with groups = dimension). x [B,C,Tin], w [C,K], y [B,C,Tout]. */
int ua2_dwconv1d(const float* x, const float* w, const float* bias, float* y, int32_t B, int32_t C, int32_t Tin,
                 int32_t Tout, int32_t K, int32_t stride, int32_t dilation, int32_t pad_left, int32_t transposed,
                 void* stream);

/* ---- codec: glue of the neural stages (flow-matching DiT, AudioThinking encoder) ------------------------------- */

enum ua2_ew_act { UA2_EW_IDENTITY = 0, UA2_EW_SILU = 1, UA2_EW_SIGMOID = 2, UA2_EW_TANH = 3 };

/* out[i] = alpha * a[i % na] * (b ? b[i % nb] : 1) + (c ? c[i % nc] : 0) + beta, i < n (modulo = broadcast of a shorter
 * operand over rows).  The broadcast multiply-adds of the DiT and the Euler solver: adaLN modulation vectors
 * (models/attention.py:308-311), gated residuals (:345-349, 401-405), ProjectLayer's k^-0.5 (transformer_1d_flow.py:31),
 * guidance and the Euler step (AudioDiffusion1D.py:104,116-123).  out may alias a, b or c. */
int ua2_ew_fma(float* out, int64_t n, const float* a, int64_t na, const float* b, int64_t nb, const float* c, int64_t nc,
               float alpha, float beta, void* stream);
/* out[i] = act(x[i]) (SiLU of adaLN-single, transformer_1d_flow.py:113; nn.SiLU of TimestepEmbedding). */
int ua2_ew_act(float* out, const float* x, int64_t n, int32_t act, void* stream);
/* out[r, :] = in[idx[r], :], zeros where idx[r] < 0; C % 4 == 0.  Nearest-neighbour interpolation along time
 * (AudioDiffusion1D.py:450,512,590) and the cls-token interleave / extraction (:458-486) with host-built index lists. */
int ua2_gather_rows(float* out, const float* in, const int32_t* idx, int64_t R, int32_t C, void* stream);
/* time_film (AudioDiffusion1D.py:428-438): params [R, 2C] = (delta_gamma | beta); out = (1 + gamma_scale * tanh(dg)) * x
 * + beta; rows of a batch element with batch_mask[b] != 0 (the reference's `torch.rand(B,1,1) < 0.2` draw, passed in so
 * that runs are reproducible) pass x through unchanged.  R = B * rows_per_batch. */
int ua2_time_film(float* out, const float* params, const float* x, const uint8_t* batch_mask, int64_t R,
                  int32_t rows_per_batch, int32_t C, float gamma_scale, void* stream);
/* F.layer_norm over the last axis of [R, C]; w, b optional (NULL = elementwise_affine=False, transformer_1d_flow.py:252). */
int ua2_layernorm_rows(float* out, const float* x, const float* w, const float* b, int64_t R, int32_t C, float eps, void* stream);
/* out[r, :] = rec[r, :] + reason[src[r], :] in fp32 (one rounding), r < rows; D % 4 == 0, out / rec / reason 16-byte aligned,
 * out may equal rec.  feature_combine of the reasoning-conditioned decode (AudioDiffusion1D.py:440-456): the reason_adaptor
 * rows up-sampled x2.5 by nearest neighbour (src = the host-built index table, every entry a valid row of `reason`) and
 * added to the summed RVQ look-ups. */
int ua2_reason_merge(float* out, const float* rec, const float* reason, const int32_t* src, int64_t rows, int32_t D, void* stream);
/* Linear cross-fade + crop of n_seg decoded windows (reason_tokenizer.py:210-224): window k (row k of seg, seg_stride
 * floats apart, first `win` samples used) starts at k * (win - ovlp); in the ovlp samples shared with window k - 1 the
 * result is (float)((double)old * (1 - ramp[i]) + (double)new * ramp[i]), ramp = np.linspace(0, 1, ovlp), without fused
 * multiply-adds — the host's float64 blend bit for bit.  out [target_len], target_len <= (n_seg - 1) * (win - ovlp) + win;
 * requires 0 < ovlp <= win - ovlp and seg_stride >= win. */
int ua2_crossfade(float* out, const float* seg, int32_t n_seg, int64_t seg_stride, int64_t win, int64_t ovlp, int64_t target_len,
                  void* stream);
/* Whisper log-mel front end (reason_tokenizer.py:67-72: WhisperFeatureExtractor(feature_size=80), numpy path).  wav [B, n_samples]
 * fp32 at 16 kHz -> out [B, 80, 3000] fp32.  Per clip: truncate / zero-pad to 480 000 samples, reflect-pad 200 on both sides,
 * frames of 400 at hop 160, periodic Hann window, power of the 201 real-DFT bins, 80 x 201 Slaney mel filter bank,
 * log10(max(., 1e-10)), the last of the 3001 frames dropped, max(x, max over the clip - 8), (x + 4) / 4.
 * basis [400, 402] fp32: row n = (hann[n] cos(2 pi n k / 400), k < 201 | hann[n] sin(2 pi n k / 400), k < 201); mel_fb [201, 80] fp32;
 * both built once on the host in float64 (the kernel carries no tables).  fp32 accumulation throughout; the clip maximum is a
 * second launch over per-workgroup maxima (no atomics): a clip's bits depend neither on scheduling nor on the batch it is in.
 * ws: scratch of the size the _workspace_bytes function below reports for B. */
size_t ua2_logmel_workspace_bytes(int32_t B);
int ua2_logmel(float* out, const float* wav, int32_t B, int64_t n_samples, const float* basis, const float* mel_fb, float* ws,
               size_t ws_bytes, void* stream);
/* ---- BEST-RQ (MusicFM 25 Hz) encoder: modules/our_MERT_BESTRQ/mert_fairseq/models/musicfm/ (entry points added under ABI v10) ----
 * ua2_conv2d: nn.Conv2d(kernel 3 x 3, padding 1, stride (stride_f, stride_t), each 1 or 2) of the stem's Res2dModule (modules/conv.py:
 * 20-42), exact fp32 on the f32 matrix pipe (the arithmetic class of ua2_conv1d precision 0), with the epilogue
 *     y = act( conv(x) + bias (+ residual) ),   act 0 = none, 1 = ReLU.
 * x [B, Cin, F, T] fp32, y and residual [B, Cout, Fo, To] fp32 with Fo = (F - 1) / stride_f + 1, To = (T - 1) / stride_t + 1.
 * Eval-mode BatchNorm2d is folded by the caller: w' = w g / sqrt(var + eps), b' = (b - mean) g / sqrt(var + eps) + beta.
 * w: for Cin > 4 the filter as ua2_pack_linear(fp32) of the [Cout, G * 9 * 16] matrix whose reduction index is (group of 16 input
 * channels, tap kf * 3 + kt, channel in the group), Cin zero-padded to 16 G (host helper ops.pack_conv2d_weight); for Cin <= 4 (the
 * first layer, Cin = 1) the plain [Cout, Cin, 3, 3] fp32 filter, summed as one fma chain.  Any F, T, Cin, Cout (partial tiles are
 * masked, never mis-tiled); every load index is clamped into the buffer and the zero padding is a select on the loaded value.  A clip's
 * output does not depend on the batch it is in. */
int ua2_conv2d(const float* x, const void* w, const float* bias, const float* residual, float* y, int32_t B, int32_t Cin, int32_t Cout,
               int32_t F, int32_t T, int32_t stride_f, int32_t stride_t, int32_t act, void* stream);
/* LayerNorm + the conformer's rotary step (transformers Wav2Vec2ConformerSelfAttention._apply_rotary_embedding: the LayerNorm-ed
 * hidden states are rotated BEFORE linear_q / linear_k, linear_v reads them un-rotated).  out [R, 2 C]: columns [0, C) =
 * n cos + rotate_half(n) sin per head of head_size (rotate_half = (-second half, first half)), columns [C, 2 C) = n, with
 * n = F.layer_norm(x[r]) * w + b (the sums of ua2_layernorm_rows).  cos_t / sin_t [n_pos, head_size] fp32 = cos / sin of
 * cat(freqs, freqs), built on the host; row r uses table row row_pos[r] (clamped to n_pos - 1).  C % head_size == 0, C <= 8192. */
int ua2_layernorm_rope_rows(float* out, const float* x, const float* w, const float* b, const float* cos_t, const float* sin_t,
                            const int32_t* row_pos, int32_t n_pos, int64_t R, int32_t C, int32_t head_size, float eps, void* stream);
/* Tail of the MusicFM mel front end (modules/features.py MelSTFT(is_db=True), musicfm_25hz.py:199-233): spec [B * T, ld] fp32 holds per
 * frame the real parts of the n_bins DFT bins in columns [0, n_bins) and the imaginary parts in [n_bins, 2 n_bins) (a ua2_linear
 * product of the frames with the windowed basis); out[b][m][t] = (10 log10(max(sum_k (re^2 + im^2) mel_fb[k][m], 1e-10)) - mean) / std.
 * mel_fb [n_bins, n_mels] fp32 (torchaudio melscale_fbanks, htk, norm None), built on the host.  fp32 throughout. */
int ua2_melspec_db(float* out, const float* spec, const float* mel_fb, int32_t B, int32_t T, int32_t n_bins, int32_t n_mels, int32_t ld,
                   float mean, float stdv, void* stream);
/* ---- WavLM encoder: transformers WavLMModel, base architecture (feat_extract_norm "group", post-norm layers, gated relative-position
 * bias), as AudioDiffusion1D.py:355-366 calls it (entry points added under ABI v10) ----
 * First feature-extractor layer: Conv1d(1 -> C, kernel K, stride, no bias) + GroupNorm(num_groups = C) + exact-erf GELU.
 * x [B, N] fp32, w [C, K] fp32, y [B, T0, C] fp32 TIME-MAJOR with T0 = (N - K) / stride + 1:
 *     y[b][t][c] = gelu((conv[b][t][c] - mean[b][c]) * rsqrt(var[b][c] + eps) * gn_w[c] + gn_b[c]),
 * conv = one fp32 fma chain over the taps in ascending order, mean / var (biased) over the T0 frames of clip b.  The statistics are
 * sums and sums of squares in double over fixed chunks of 256 frames (a constant of the kernel: independent of B and of the grid),
 * the chunks added in chunk order in double; a single frame has variance exactly 0.  Three launches; 16-byte stores along C.
 * C % 4 == 0, K <= 16, stride <= 32.  ws: 8-byte aligned scratch of the size the _workspace_bytes function reports. */
size_t ua2_wavlm_conv0_workspace_bytes(int32_t B, int64_t N, int32_t C, int32_t K, int32_t stride);
int ua2_wavlm_conv0(float* y, const float* x, const float* w, const float* gn_w, const float* gn_b, int32_t B, int64_t N, int32_t C,
                    int32_t K, int32_t stride, float eps, void* ws, size_t ws_bytes, void* stream);
/* Grouped 1-D convolution over time-major rows (WavLMPositionalConvEmbedding: k 128, 16 groups, padding 64, the last step of an
 * even kernel dropped by WavLMSamePadLayer):
 *     y[b][t][co] = resid[b][t][co] + act( bias[co] + sum_{k, ci} W[co][ci][k] * x[b][t + k - K / 2][group(co) * C / groups + ci] ),
 * x beyond both ends = 0, T outputs for T inputs (odd and even K), act 0 = none, 1 = exact-erf GELU, bias and resid optional.
 * x, y, resid [B * T, C] fp32.  Exact fp32 on the f32 matrix pipe (the arithmetic class of ua2_conv1d precision 0).
 * w: ua2_pack_linear(fp32) of the [C, K * C / groups] matrix whose reduction index is (tap, channel in the group) (host helper
 * ops.pack_conv1d_grouped_weight); weight norm is folded by the caller.  The reduction runs in ascending index order: the order of
 * summation is a function of (C, groups, K) only.  (C / groups) % 16 == 0 is required (an error otherwise); any T, also T < K / 2.
 * Every load index is clamped into the buffer and the zero padding is a select on the loaded value. */
int ua2_conv1d_grouped(float* y, const float* x, const void* w, const float* bias, const float* resid, int32_t B, int32_t T, int32_t C,
                       int32_t groups, int32_t K, int32_t act, void* stream);
/* Gate of WavLM's gated relative-position bias (WavLMAttention: gru_rel_pos_linear Linear(head_size, 8), gru_rel_pos_const).
 * h [R, n_head * head_size] fp32 = the layer's input rows, w [8, head_size], b [8], c [n_head]; g [R, n_head] fp32:
 *     p = w h[r, head] + b;  a = sigmoid(p0 + p1 + p2 + p3);  bb = sigmoid(p4 + p5 + p6 + p7);  g = a (bb c[head] - 1) + 2.
 * One fma chain per projection, dims ascending; head_size % 4 == 0, <= 128. */
int ua2_relpos_gate(float* g, const float* h, const float* w, const float* b, const float* c, int64_t R, int32_t n_head, int32_t head_size,
                    void* stream);
/* Dense attention with the gated relative-position bias over the paged K/V of `a` (n_head == n_kv, head size 64 or 128): row r attends
 * keys 0 .. a->row_pos[r] with
 *     score = q . k + gate[r][h] * rel_tab[h][clamp(kpos - q_pos[r] + tab_half, 0, 2 tab_half)]
 * (q arrives scaled by head_size^-0.5, as WavLM scales it), online softmax, normalised fp32 output to a->y and / or a->y_packed.
 * rel_tab [n_head, 2 tab_half + 1] fp32: entry d + tab_half holds the bias of relative position d = key - query (built on the host from
 * rel_attn_embed by the transformers bucket rule); gate [R, n_head] from the gate entry point above; q_pos [R] int32.
 * dtype UA2_BF16 needs the row groups of ua2_attn_args and runs the MFMA flash form (bf16 K/V, fp32-grade q and softmax, LDS-staged
 * 64-key pages combined in page order, the head's table row staged in LDS once per workgroup, the bias added to the fp32 score tile
 * before the running maximum; group_q_tiles 4 or 8 at head size 64, 4 at 128); a row's result does not depend on the grouping.
 * dtype UA2_F32 is the parity form: row by row, the arithmetic of ua2_attn's fp32 kernel plus the bias term (with an all-zero table:
 * its bits). */
int ua2_attn_relbias(const ua2_attn_args* a, const int32_t* q_pos, const float* gate, const float* rel_tab, int32_t tab_half, void* stream);
/* q/k LayerNorm over the head dim + partial rotary embedding + K/V append to the paged cache for the x-transformers
 * style attention of the AudioThinking encoder (modules/transformer.py:447-485, 146-170).  qkv [R, 3*n_head*hs] =
 * (q | k | v); q_out [R, n_head*hs] fp32; cos_t / sin_t [max_pos, rot_dim/2]; norm weights NULL = no q/k norm;
 * rot_dim 0 = no rotary.  Multi-head only (kv->n_kv == kv->n_head). */
int ua2_qknorm_rope_kv(int dtype, const float* qkv, int64_t R, const int32_t* row_pos, const int32_t* row_seq,
                       const float* q_norm_w, const float* q_norm_b, const float* k_norm_w, const float* k_norm_b, float eps,
                       const float* cos_t, const float* sin_t, int32_t rot_dim, float* q_out, const ua2_kv_geom* kv, void* stream);

/* ---- whole-frame executor -------------------------------------------------------------- */

typedef struct ua2_gpt_desc {
  int32_t n_layer, n_embd, n_head, n_kv, head_size, inter;
  float eps;
  /* per layer arrays of device pointers (host arrays of length n_layer) */
  const void* const* qkv;    /* packed [ (n_head+2*n_kv)*hs, n_embd ] */
  const void* const* proj;   /* packed [ n_embd, n_head*hs ] */
  const void* const* fc1;    /* packed [ inter, n_embd ] */
  const void* const* fc2;
  const void* const* mlp_proj; /* packed [ n_embd, inter ] */
  const float* const* norm1;
  const float* const* norm2;
  const float* ln_f;
  const float* rope_cos;     /* [max_pos, hs/2] */
  const float* rope_sin;
  void* const* k_pool;       /* per layer */
  void* const* v_pool;
  const int32_t* page_table;
  int32_t max_pages;
} ua2_gpt_desc;

typedef struct ua2_stage3_desc {
  int32_t dtype;
  int32_t n_cb;         /* audio_num_codebooks (8) */
  int32_t va;           /* audio_semantic_vocab_size + audio_reason_vocab_size */
  int32_t vt;           /* text vocab (lm_head rows) */
  int32_t max_rows;     /* capacity in rows of the trunk (prefill chunk / decode batch) */
  int32_t max_batch;    /* capacity in rows of the heads (lm_head + local decoder), <= max_rows */
  ua2_gpt_desc und, backbone, gen, decoder;
  const void* wte;      /* [vt, C] */
  const void* audio_emb;/* [va*n_cb, C] */
  const void* lm_head;  /* packed [vt, C] */
  const void* projection; /* packed [Cd, C] */
  const void* const* audio_head; /* n_cb packed [va, Cd] */
  /* sequence state (device) */
  int32_t* tokens;      /* [max_rows, n_cb+1] current input frame(s) */
  uint8_t* mask;        /* [max_rows, n_cb+1] */
  int32_t* row_pos;     /* [max_rows] */
  int32_t* row_seq;     /* [max_rows] */
  int32_t* dec_pos;     /* [n_cb, max_rows]: row i filled with i — positions of the local decoder's step i */
  int32_t* dec_seq;     /* [max_rows] = 0,1,2,...: page-table rows of the local decoder's 8-slot caches */
  int32_t* forbid;      /* [max_rows] forbid_prefix per row */
  int32_t* out_tokens;  /* [max_rows, n_cb+1] sampled [text, a0..a7] */
  int32_t* frame_log;   /* [log_frames, max_rows, n_cb+1] */
  int32_t* counters;    /* [4]: [0] frame index (log slot), [1] sampling draw index, [2..3] sampler seed (lo, hi) */
  int32_t log_frames;
  /* scratch (device, fp32 unless noted) — sizes in ua2_stage3_scratch_floats() */
  float* scratch;
  size_t scratch_floats;
} ua2_stage3_desc;

typedef struct ua2_stage3 ua2_stage3;

/* [round 6] Per-plan tables of the depth decoder (model_new.py:630-641).  `self.projection(_embed_audio(i, sample))` and layer 0's
 * q | k | v of that row at position i + 1 are functions of the sampled id alone; ua2_stage3_create builds them for all (n_cb - 1) * va
 * ids by running the frame's own launches on the null stream (a row's bits do not depend on the rows beside it), synchronises, and the
 * frame's arg-max gathers the rows instead of launching the two GEMVs per step (greedy frames of row-invariant plans; top-k sampling and
 * the order-free opt-in keep the launches).  Bit-identical ids and logits (tests/test_gpu_lm.py); the tables live in `scratch`:
 * ua2_stage3_scratch_floats() includes (n_cb - 1) * va * (Cd fp32 + Cd bf16 + Cd / 16 fp32 + q fp32 + k + v) — 1.9 GB at the released
 * sizes.  Environment, read when a plan is sized and created: UA2_NO_PROJ_TABLE=1 (neither table), UA2_NO_QKV_TABLE=1 (projection only). */
size_t ua2_stage3_scratch_floats(const ua2_stage3_desc* d);
int ua2_stage3_create(const ua2_stage3_desc* d, ua2_stage3** out);
void ua2_stage3_destroy(ua2_stage3* h);
/* Sampling mode of the heads: topk == 1 -> greedy (default); topk > 1 -> ua2_sample_topk with this temperature / seed.
 * The seed is written to counters[2..3] on `stream` (stream-ordered with the frames that follow); topk / temperature
 * select the captured graph, the seed does not. */
int ua2_stage3_set_sampling(ua2_stage3* h, int32_t topk, float temperature, uint64_t seed, void* stream);
/* [v10, addition] Per-row sampler streams (ua2_sample_topk_rows).  row_key [max_batch][2], row_draw [max_batch]: device arrays owned by
 * the caller, alive while set.  While set, every sampler of a top-k frame (the text sampler — of mode 1 too — and the n_cb audio samplers,
 * with the stream ids they have without it) draws row m under row_key[m] at row_draw[m], and the frame's one draw-index launch advances
 * row_draw[0 .. R) instead of counters[1]; the seed of ua2_stage3_set_sampling and counters[1] are then neither read nor written.  The
 * two rows of a guidance pair get the same key from the caller and advance together.  Greedy frames (topk == 1) neither read nor advance
 * the streams.  NULL, NULL = off (the default).  The pointers are baked into recorded frames: a change of either drops them, on / off
 * selects among them. */
int ua2_stage3_set_row_streams(ua2_stage3* h, int32_t* row_key, int32_t* row_draw);
/* [v10, addition] Nucleus filter of the heads' samplers (ua2_sample_topp above): with topk > 1 and 0 < top_p < 1 every sampler of a frame —
 * the text sampler and the n_cb audio samplers, shared stream or per-row streams, guided pairs included — runs the nucleus tail; 0
 * (the default) and 1 are off and the frame is the top-k frame it was.  top_p outside [0, 1] or NaN is an error.  Greedy frames
 * (topk == 1, the per-id tables and the arg-max fold with them), ua2_stage3_text_flush and beam frames ignore it.  top_p's bits select
 * the captured graph next to topk / temperature: a changed value never replays a frame recorded under another. */
int ua2_stage3_set_top_p(ua2_stage3* h, float top_p);
/* [v10, addition] Repetition penalty of the heads' samplers (ua2_sample_penalized above; not in the reference, effect on audio quality NOT
 * measured).  hist [max_batch][1 + n_cb][window] int32 and len [max_batch][1 + n_cb] int32 are device buffers owned by the caller, alive
 * while set: the ring of row m and sampler stream s (0 = the text head, 1 + i = audio codebook i) is hist + (m * (1 + n_cb) + s) * window
 * (rep_cap = rep_window = window) and its counter len[m * (1 + n_cb) + s], with the layout stated there.  The caller zeroes the counters
 * of a row that starts.  While set and topk > 1, EVERY sampler launch of a frame — the text sampler of any mode that runs it and the n_cb
 * audio samplers, shared stream or per-row streams, with or without the nucleus filter, guided pairs included (ua2_cfg_mix comes first:
 * the guided logits are penalised) — runs penalised against its own stream's history and appends its id.  Greedy frames (topk == 1: the
 * per-id tables, the arg-max fold, the partials of the GEMM epilogue), ua2_stage3_text_flush, beam frames (mode 3) and ua2_stage3_score
 * ignore it and leave the histories alone.  penalty must be finite and > 0, 1 <= window <= 512, and the heads' vocabularies at most
 * 131072 columns; penalty == 1 or NULL buffers clear it.  penalty's bits and window select the captured graph next to top_p's; the
 * buffer pointers are baked into recorded frames, so a change of either drops them. */
int ua2_stage3_set_rep_penalty(ua2_stage3* h, float penalty, int32_t window, int32_t* hist, int32_t* len);
/* Row groups (ua2_attn_args.group_*; device tables owned by the caller, alive until replaced) for the attention of the
 * NEXT ua2_stage3_trunk call (they are cleared when it returns): prefill rows of one sequence then share LDS-staged K/V
 * pages on the MFMA flash kernel.  ua2_stage3_frame (decode) never uses groups. */
int ua2_stage3_set_prefill_groups(ua2_stage3* h, const int32_t* group_rows, const int32_t* group_seq, const int32_t* group_nkeys,
                                  int32_t n_groups, int32_t group_q_tiles);
/* rows > 0 (UA2_BF16 plans; default 0 = off): launches of the four GPTs (trunk and depth decoder) with at least `rows` rows — prefill chunks of
 * batches (BASELINE config 3: 32 x 195 rows), decode frames of >= `rows` sequences — set ua2_linear_args.sum_order =
 * UA2_SUM_ORDER_FREE: the 256-row-tile GEMM with one chain over K (csrc/ua2_gemm2.hip), 10-25 % faster per launch at >= 2048
 * rows.  The price is the row-invariance contract ACROSS that threshold: a sequence prefilled alone (few rows) and inside a big
 * batch (>= rows) then differs by fp32 summation noise in its K/V cache, i.e. by bf16-level noise in later logits — the same
 * class of difference the MFMA prefill attention already has against decode rows.  Below the threshold nothing changes. */
int ua2_stage3_set_order_free_rows(ua2_stage3* h, int32_t rows);
/* fp8 weights for the plan's few-row launches (UA2_BF16 plans).  table[i] = {w: a packed weight pointer exactly as the desc gave it (a
 * layer's qkv / proj / fc1 / fc2 / mlp_proj, projection, lm_head, audio_head[i]) — it must hold the bf16 form of W' —, q / exp: its fp8
 * twin from ua2_pack_linear_w8}.  Launches of the frame that go to the decode kernel — exactly those that would go to it in the plain bf16 plan: by default up to 5 rows
 * (UA2_GEMV_MAX_ROWS), and a weight whose (N, K) geometry has no fp8 form stays on its bf16 form — then stream the fp8 image of every
 * weight that has an entry (a SWIGLU launch: of both); prefill chunks, larger batches and the plan's tables keep reading W' — the same
 * function, the same bits.  lm_head then runs as a launch of its own (the rider kernel has no fp8 form).  The table is copied; the
 * images stay owned by the caller and alive as long as the plan uses them.  n = 0 clears.  Every call drops the captured frame graphs.
 * An entry whose pointer is not a weight of the plan, or a plan of another dtype, is an error. */
typedef struct {
  const void* w;
  const void* q;
  const int8_t* exp;
} ua2_w8_entry;
int ua2_stage3_set_w8(ua2_stage3* h, const ua2_w8_entry* table, int32_t n);
/* [v10, addition] Lossless 13-bit weight images (ua2_pack_linear_l13 above).  ua2_stage3_create packs, for a UA2_BF16 plan, an image of
 * every Linear weight a decode frame streams — the layers of the three trunk GPTs and of the depth decoder, projection, the audio heads;
 * not lm_head — and keeps those without an escape; the handle owns them (about 13/16 of the plan's weight bytes in extra device memory).
 * The frame's few-row launches that the decode kernel serves (up to ua2_gemv_rows_preferred rows; not the argmax-fold launch, not launches
 * that carry riders, not the one form the image makes longer — a 16-chunk single burst on fewer than 160 workgroups, the depth decoder's
 * down-projection at the released sizes —) then stream the image of a weight that has one: the same bits as the bf16 form, fewer bytes.  Everything else — prefill,
 * larger batches, the plan's tables, UA2_F32 plans — reads the bf16 form.  fp8 twins (ua2_stage3_set_w8), when attached, take precedence.
 * On by default; UA2_NO_LOSSLESS=1 in the environment when the plan is created packs nothing.  ua2_stage3_set_lossless switches a plan that
 * has images and drops the captured frame graphs.  ua2_stage3_lossless_stats reports what creation found: how many matrices compress
 * depends on the weights (the escape count of each) and is measured, never assumed. */
typedef struct {
  int32_t on;                     /* images in use by the frame's launches */
  int32_t with_image;             /* matrices with an escape-free image */
  int32_t without_image;          /* matrices on bf16 alone: K % 128 != 0, an escape, or no memory for the images */
  int32_t with_escapes;           /* ... of those, the ones with at least one escape */
  int64_t bf16_bytes_per_frame;   /* weight bytes one B = 1 frame streams from these matrices in bf16 (depth decoder: once per codebook) */
  int64_t image_bytes_per_frame;  /* ... and with every image in use */
  int64_t extra_device_bytes;     /* device memory the images take */
  float build_ms;                 /* host time of packing them */
  int32_t reserved;
} ua2_lossless_info;
int ua2_stage3_set_lossless(ua2_stage3* h, int32_t on);
int ua2_stage3_lossless_stats(const ua2_stage3* h, ua2_lossless_info* out);
/* n-gram repeat filter of the text-feedback frames: with n >= 2 every feedback of mode 1 (ua2_stage3_frame with or without
 * UA2_FRAME_SKIP_AUDIO_EXPERTS, and the standalone feedback) first runs the n-gram filter above over the text ids of its R rows,
 * so the frame log and the fed-back text id carry the filtered id.  hist [max_batch, cap] / hist_len [max_batch] int32 are
 * device buffers owned by the caller, like the rest of the decode state.  n <= 1 turns the filter off.  The captured frame graphs
 * are keyed on n (switching the filter off and on again re-uses them); a new fallback, new buffers or a new cap drop them.
 * Modes 0 and 2 are never filtered. */
int ua2_stage3_set_ngram(ua2_stage3* h, int32_t n, int32_t fallback, int32_t* hist, int32_t* hist_len, int32_t cap);
/* Beam search of the text loop (feedback mode 3 of the frame entry point below).  W >= 1 attaches the caller-owned state (copied by
 * value; the buffers stay alive while attached), the EOS id and the device array of the n_pools K / V pools of the three trunk
 * GPTs (table index 0 = understanding expert, 1 = backbone, 2 = generation expert; their page tables, of max_batch rows, are the
 * plan's).  Needs 1 <= W <= 8, 2 W <= max_batch (the pages of sequences W .. 2W - 1 are the second page set of the fork) and the
 * three tables of one width.  W = 0 clears.  New buffers, a new W or a new EOS drop the captured frame graphs. */
int ua2_stage3_set_beam(ua2_stage3* h, int32_t W, int32_t eos, const ua2_beam_state* st, const ua2_beam_pool* pools, int32_t n_pools);
/* The same for G groups of W slots (ua2_beam_step_groups; ua2_stage3_set_beam is G = 1): mode 3 frames then have R = G * W rows.  Needs
 * G >= 1, G * W <= 64 and 2 G W <= max_batch.  A new G drops the captured frame graphs as a new W does. */
int ua2_stage3_set_beam_groups(ua2_stage3* h, int32_t W, int32_t G, int32_t eos, const ua2_beam_state* st, const ua2_beam_pool* pools,
                               int32_t n_pools);
/* The no-repeat-n-gram ban of the attached beam (ua2_beam_step_groups_ngram; opt-in): mode 3 frames then run the step under it.  Valid
 * only while a beam is attached; ng is copied by value and hist ([G][2][8][cap] for the attached G) stays alive while set.  NULL or
 * n == 0 = off.  Checked as ua2_beam_step_groups_ngram checks it.  A call that changes anything drops the captured frame graphs;
 * every ua2_stage3_set_beam[_groups] call clears the ban, so it is set after the beam is attached and gone once it is detached. */
int ua2_stage3_set_beam_ngram(ua2_stage3* h, const ua2_beam_ngram* ng);
/* cfg_scale > 1: frames of (conditional, unconditional) row pairs — rows 2p, 2p + 1; an even row count — sample from the guided
 * logits (ua2_cfg_mix); feedback mode 2 continues every row from its pair's conditional row. */
int ua2_stage3_set_cfg(ua2_stage3* h, float cfg_scale);

/* model_new.py:594-613 (embed-merge -> U-expert -> backbone -> G-expert -> blend) for R rows
 * described by tokens/mask/row_pos/row_seq.  Used for prefill (forward_prefix, :456-497; the
 * discarded lm_head/local-decoder work :498-506 is skipped) and as the first half of a frame. */
int ua2_stage3_trunk(ua2_stage3* h, int32_t R, void* stream);
/* model_new.py:617-641: lm_head + greedy text sample, then the 8-step local decoder.  [r6] On bf16 plans of up to 6 rows lm_head has no
 * launch of its own: its column tiles ride on workgroups past the grid of the local decoder's down-projection launches (which fill
 * half of the CUs; csrc/ua2_gemv.hip gemv_rider_kernel) and the text sample is taken behind the decoder — the same logits and ids
 * bit for bit (lm_head reads only the trunk's output, :617 vs :629-640).  UA2_NO_RIDER=1: lm_head as a launch, as before. */
int ua2_stage3_heads(ua2_stage3* h, int32_t R, void* stream);
/* Feedback for the next frame, on device (evaluation/tts_task.py:259-280 mode 0 "audio";
 * evaluation/asr_task.py:668-682 mode 1 "text"; mode 2 = "audio" with every row continuing from row 0's
 * sample, the classifier-free-guidance pair of tts_task.py:256-258,278-280): logs out_tokens, builds the next input frame,
 * row_pos += 1, applies the reason_eos -> forbid_prefix switch (tts_task.py:263-266). */
int ua2_stage3_feedback(ua2_stage3* h, int32_t R, int32_t mode, int32_t reason_eos, int32_t reason_card, void* stream);
/* trunk + heads + feedback (mode < 0: no feedback), captured once into a hipGraph and replayed
 * (use_graph != 0).
 * mode | UA2_FRAME_SKIP_TEXT_HEAD (audio-feedback modes 0 and 2 only): the frame skips lm_head and the text sample — in those
 * loops the text id is fed back under a zero mask and collected into a list the generators never read
 * (evaluation/tts_task.py:259,274-277; model_new.py:617 computes it every frame), so the audio ids are bit-identical with and
 * without it; the frame log's text column holds -1 for such frames and the next frame's (masked) text token is 0. */
#define UA2_FRAME_SKIP_TEXT_HEAD 16
/* mode 1 | UA2_FRAME_SKIP_AUDIO_EXPERTS [round 6]: every row of the frame is a TEXT step of a text-only continuation (the loops of
 * evaluation/asr_task.py:666-682 and its twins from their second frame on: the fed-back masks are (audio 0, text 1) and no audio step ever
 * follows).  There audio_step_mask = 0 multiplies both experts' outputs (model_new.py:607 backbone_input, :613 h_final) and nothing reads
 * their caches again, so the frame does not run audio_understanding_expert / audio_generation_expert (5 of the trunk's 33 layers at the
 * released sizes): text ids bit-identical (tests/test_gpu_lm.py).  The CALLER vouches for the precondition — the first frame after a prefill
 * (it consumes the prompt's last token, usually an audio step) and any sequence that will see an audio step later must run without it:
 * the skipped positions of the experts' caches are left unwritten. */
#define UA2_FRAME_SKIP_AUDIO_EXPERTS 32
/* mode 0 | UA2_FRAME_DEFER_TEXT_HEAD (feedback mode 0 only; not together with UA2_FRAME_SKIP_TEXT_HEAD): the frame is a
 * UA2_FRAME_SKIP_TEXT_HEAD frame — no lm_head, no rider, no text sample, -1 in the log's text column, 0 as the next frame's masked text
 * token — that also keeps its R rows of h_final (fp32) in slot counters[0] % cap_frames of a stash ring of the plan, cap_frames =
 * ua2_stage3_defer_rows() / R.  In that loop the text id has no consumer inside the model (it is fed back under a zero mask), so the
 * text ids of different frames depend neither on each other nor on anything else the loop computes: ua2_stage3_text_flush computes
 * them for up to UA2_DEFER_CAP_ROWS stashed rows with ONE pass over lm_head's weights instead of one pass per frame.  At R <= 4 the
 * copy is part of the feedback kernel (no launch is added to the frame); more rows take one small copy launch.  The flag and
 * cap_frames select the captured graph. */
#define UA2_FRAME_DEFER_TEXT_HEAD 64
#define UA2_DEFER_CAP_ROWS 64
/* mode 3 (with or without UA2_FRAME_SKIP_AUDIO_EXPERTS, under mode 1's precondition): a beam-search frame of R = G * W rows — trunk,
 * lm_head, the beam step on its fp32 logits, the K/V fork, then the text feedback of mode 1 with the ids the step chose (tokens
 * (0 x n_cb, id), masks (0.., 1), row_pos += 1; the frame log's text column holds them).  Checked before any launch: a beam is
 * attached (the set_beam calls above) and R equals its G * W; no classifier-free guidance, no n-gram filter, top-k = 1.  The caller keeps the step
 * count within the state's log and length-penalty tables and every position within the caches.  With ua2_stage3_set_beam_ngram set the
 * step is ua2_beam_step_groups_ngram under that ban (the greedy loop's n-gram filter stays excluded). */
int ua2_stage3_frame(ua2_stage3* h, int32_t R, int32_t mode, int32_t reason_eos, int32_t reason_card,
                     int32_t use_graph, void* stream);
/* Rows of the stash ring in use: UA2_DEFER_CAP_ROWS, or UA2_DEFER_ROWS=n from the environment (clamped to 1 .. UA2_DEFER_CAP_ROWS; tests and
 * sweeps), or 0 under UA2_NO_DEFER_TEXT_HEAD=1 (A/B: callers then run every frame undeferred).  Read once; ua2_debug_refresh_env re-reads. */
int32_t ua2_stage3_defer_rows(void);
/* The text ids of frames frame0 .. frame0 + n - 1 (log slots: the values counters[0] had when the UA2_FRAME_DEFER_TEXT_HEAD frames of R
 * rows ran), stream-ordered behind them: lm_head over the n * R stashed rows — the launch ua2_stage3_heads builds for it, under
 * UA2_SUM_ORDER_INVARIANT, through the same launcher, so a row's logits and arg-max partials carry the bits of its per-frame launch
 * whichever kernel serves the row count — then the arg-max per row (tie and all-NaN rules of ua2_argmax_embed) into
 * frame_log[((frame0 + j) * max_rows + m) * (n_cb + 1) + 0] for frame0 + j < log_frames.  The window must not wrap the ring
 * (frame0 % cap_frames + n <= cap_frames): callers flush whenever a frame fills the last slot and once more at the end of a run of
 * deferred frames, before the ring is written again.  Greedy, unguided plans (top-k = 1, no classifier-free guidance); the logits of a
 * flush are scratch — "text_logits" keeps what the last undeferred frame wrote.  Counted as "text_flush" by ua2_debug_kernel_launches. */
int ua2_stage3_text_flush(ua2_stage3* h, int32_t R, int32_t frame0, int32_t n, void* stream);
/* [v10, addition] Teacher-forced scoring (model_new.py:402-454 forward + the cross-entropies of :59-109) of the R rows the preceding
 * ua2_stage3_trunk(h, R) ran (R <= max_batch; its h_final is still in the plan's buffer): lm_head into "text_logits" and the text tail,
 * then per codebook i the projection of the step's input (h_final at i = 0, the embedding of LABEL i - 1 after that), the local decoder
 * at position i, audio_head[i] into "audio_logits" and ua2_xent_embed on label column i, which gathers audio_emb[i * va + label] for
 * step i + 1.  These are the launches ua2_stage3_heads issues on its plain path (same prologues, hand-overs and summation orders; no
 * riders, per-id tables, arg-max fold, graph, guidance or sampler; forbid_prefix ignored), so on the row-invariant plans a
 * teacher-forced row carries the bits of the decode frame that saw the same ids.  Every row runs the local decoder; rows whose next step
 * is text pass -1 labels.  labels (device) / nll / pred: [R, n_cb + 1] in the token layout a0 .. a(n_cb-1), text; label -1 = ignored
 * (nll 0), pred is always written.  Afterwards "text_logits" / "audio_logits" hold the chunk's raw logits.  Touches none of out_tokens,
 * frame_log, counters, the sampler state, the n-gram history or the beam state; refused while a beam is attached.  Counted as "score" by
 * ua2_debug_kernel_launches. */
int ua2_stage3_score(ua2_stage3* h, int32_t R, const int32_t* labels, float* nll, int32_t* pred, void* stream);
/* Expose intermediate buffers for tests: name in {"h_final","text_logits","audio_logits"}. */
float* ua2_stage3_buffer(ua2_stage3* h, const char* name);

#ifdef __cplusplus
}
#endif
#endif /* UA2HIP_H */
