// ua2_linear: Y[M,N] = epilogue( prologue(X)[M,K] * W[N,K]^T ) — weight packing, argument validation and dispatch.
//
// Replaces the nn.Linear call sites of the reference's decode frame together with the op right before and
// right after each of them (include/ua2hip.h lists the file:line of every
// fused piece).  The kernels live in ua2_gemv.hip (decode regime: one row tile, activations staged in LDS,
// the weight streamed once as non-temporal 1 KiB fragment bursts) and ua2_gemm.hip (many rows: packed
// operand, skinny or 128-row tiled MFMA GEMM); all of them give the same bits per row.
//   * the weight is pre-tiled here into MFMA B-fragment order (ua2_pack_linear): every wave load is one
//     contiguous 1 KiB burst (64 lanes x 16 B);
//   * M rows ride in the 16-row A operand of mfma_f32_16x16x32_bf16 (bf16 operands, fp32 accumulate) or
//     mfma_f32_16x16x4_f32 (exact fp32).
#include <algorithm>

#include "ua2_common.h"
#include "ua2_linear_common.h"

namespace {

// ---- packing ------------------------------------------------------------------------------

template <int SRC, int DST>
__global__ void pack_kernel(const void* __restrict__ src, void* __restrict__ out, int transposed, int64_t N, int64_t K,
                            int64_t total, int rope_hs) {
  constexpr int KC = Elem<DST>::KC, EPL = Elem<DST>::EPL;
  const int64_t nchunks = (K + KC - 1) / KC;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int e = (int)(idx % EPL);
    const int lane = (int)((idx / EPL) % 64);
    const int64_t chunk = (idx / (EPL * 64)) % nchunks;
    const int64_t tile = idx / (EPL * 64 * nchunks);
    int64_t n = tile * 16 + (lane & 15);
    if (rope_hs > 0) {  // packed column -> source row: [8r, 8r+8) then [hs/2+8r, hs/2+8r+8) per tile r of a head
      const int64_t h = n / rope_hs, within = n - h * rope_hs;
      const int64_t r = within / 16, c = within % 16;
      n = h * rope_hs + (c < 8 ? r * 8 + c : rope_hs / 2 + r * 8 + (c - 8));
    }
    const int64_t k = chunk * KC + (lane >> 4) * EPL + e;
    float v = 0.f;
    if (n < N && k < K) v = load_elem<SRC>(src, transposed ? (size_t)(k * N + n) : (size_t)(n * K + k));
    store_elem<DST>(out, (size_t)idx, v);
  }
}

// ---- fp8 (OCP e4m3fn) weight-only packing: include/ua2hip.h ua2_pack_linear_w8 -----------------------------------------------
// packed column -> source row (the bf16 pack's map: rope_hs > 0 permutes the rows of every head)
__device__ __forceinline__ int64_t w8_src_row(int64_t n, int rope_hs) {
  if (rope_hs <= 0) return n;
  const int64_t h = n / rope_hs, within = n - h * rope_hs;
  const int64_t r = within / 16, c = within % 16;
  return h * rope_hs + (c < 8 ? r * 8 + c : rope_hs / 2 + r * 8 + (c - 8));
}

// e = ceil(log2(amax / 448)) without a logarithm: amax = m 2^x with m in [0.5, 1) and 448 = 0.875 2^9, so amax 2^-e <= 448 first holds
// at e = x - 9 (m <= 0.875) or x - 8.  Zero rows take 0; clamped to [-117, 120] so that both 2^e and the smallest nonzero |W'| = 2^(e - 9)
// are normal numbers of fp32 and bf16.
__device__ __forceinline__ int w8_exponent(float amax) {
  if (!(amax > 0.f)) return 0;
  int x;
  const float m = frexpf(amax, &x);
  const int e = (m <= 0.875f) ? x - 9 : x - 8;
  return min(max(e, -117), 120);
}

// RNE of a finite |v| <= 448 to OCP e4m3fn (bias 7, subnormals m / 8 2^-6, no infinities): the code byte, sign included
__device__ __forceinline__ unsigned f2e4m3(float v) {
  const unsigned sign = (__float_as_uint(v) >> 24) & 0x80u;
  const float x = fminf(fabsf(v), 448.f);
  if (x < 0.015625f) return sign | (unsigned)rintf(x * 512.f);       // below 2^-6: multiples of 2^-9 (8 = the smallest normal)
  unsigned u = __float_as_uint(x);
  u += 0x7ffffu + ((u >> 20) & 1u);                                    // round the 23-bit fraction to 3 bits, ties to even
  return sign | ((((u >> 23) - 120u) << 3) | ((u >> 20) & 7u));
}
__device__ __forceinline__ float e4m32f(unsigned b) {
  const unsigned E = (b >> 3) & 15u, m = b & 7u;
  const float mag = E ? __uint_as_float(((E + 120u) << 23) | (m << 20)) : (float)m * 0.001953125f;
  return (b & 0x80u) ? -mag : mag;
}

// one wave per packed column: amax over the source row -> exponent (columns past N: 0)
template <int SRC>
__global__ void w8_exp_kernel(const void* __restrict__ src, int8_t* __restrict__ out_exp, int transposed, int64_t N, int64_t K, int64_t n16, int rope_hs) {
  const int lane = threadIdx.x & 63;
  const int64_t np = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (np >= n16) return;
  const int64_t n = w8_src_row(np, rope_hs);
  float amax = 0.f;
  if (n < N)
    for (int64_t k = lane; k < K; k += 64) amax = fmaxf(amax, fabsf(load_elem<SRC>(src, transposed ? (size_t)(k * N + n) : (size_t)(n * K + k))));
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
  if (lane == 0) out_exp[np] = (int8_t)w8_exponent(amax);
}

// one thread per fp8 byte of the image [N/16][K/64][64 lanes][16 B]; the bf16 twin W' = q 2^e goes out from the same q and e
template <int SRC>
__global__ void w8_pack_kernel(const void* __restrict__ src, const int8_t* __restrict__ exps, uint8_t* __restrict__ out_q,
                               unsigned short* __restrict__ out_bf16, int transposed, int64_t N, int64_t K, int64_t total, int rope_hs) {
  const int64_t nbursts = K / 64;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int e = (int)(idx & 7), half = (int)((idx >> 3) & 1), lane = (int)((idx >> 4) & 63);
    const int64_t burst = (idx >> 10) % nbursts, tile = (idx >> 10) / nbursts;
    const int64_t chunk = 2 * burst + half;
    const int64_t np = tile * 16 + (lane & 15), n = w8_src_row(np, rope_hs);
    const int64_t k = chunk * 32 + (lane >> 4) * 8 + e;
    const int ex = exps[np];
    float v = 0.f;
    if (n < N) v = load_elem<SRC>(src, transposed ? (size_t)(k * N + n) : (size_t)(n * K + k));
    const unsigned q = f2e4m3(__fmul_rn(v, __uint_as_float((unsigned)(127 - ex) << 23)));
    out_q[idx] = (uint8_t)q;
    if (out_bf16) out_bf16[((tile * (2 * nbursts) + chunk) * 64 + lane) * 8 + e] = f2bf(__fmul_rn(e4m32f(q), __uint_as_float((unsigned)(127 + ex) << 23)));
  }
}

// ---- lossless 13-bit image of a packed bf16 weight: include/ua2hip.h ua2_pack_linear_l13 ------------------------------------------
// one workgroup per 16-column tile: the largest E[7:1] of the tile -> its base byte, then the weights below the window -> the escape count
__global__ __launch_bounds__(256) void l13_base_kernel(const unsigned short* __restrict__ w, uint8_t* __restrict__ out_base, int32_t* __restrict__ escapes,
                                                       int64_t tile_elems) {
  __shared__ int red[4];
  const unsigned short* t = w + (size_t)blockIdx.x * tile_elems;
  int mx = 0;
  for (int64_t i = threadIdx.x; i < tile_elems; i += 256) mx = max(mx, (t[i] >> 8) & 0x7f);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) mx = max(mx, __shfl_xor(mx, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  const int base = max(max(max(red[0], red[1]), max(red[2], red[3])) - 15, 0);
  int esc = 0;
  for (int64_t i = threadIdx.x; i < tile_elems; i += 256) {
    const int e7 = (t[i] >> 8) & 0x7f;
    esc += (e7 != 0 && e7 <= base) ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) esc += __shfl_xor(esc, o);
  if ((threadIdx.x & 63) == 0 && esc) atomicAdd(escapes, esc);
  if (threadIdx.x == 0) out_base[blockIdx.x] = (uint8_t)base;
}

// one thread per (tile, group of 4 chunks, lane): its 4 x 16 B of the bf16 image -> its share of the group's four planes
__global__ __launch_bounds__(256) void l13_pack_kernel(const u32x4* __restrict__ w, const uint8_t* __restrict__ bases, u32x4* __restrict__ out,
                                                       int64_t groups_per_tile, int64_t total) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int lane = (int)(idx & 63);
    const int64_t grp = idx >> 6, tile = grp / groups_per_tile;
    const int base = bases[tile];
    unsigned lo[8], code[4], sign = 0u;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const u32x4 v = w[(grp * 4 + c) * 64 + lane];
      unsigned la = 0u, lb = 0u, cd = 0u;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const unsigned b = (v[e >> 1] >> ((e & 1) * 16)) & 0xffffu;
        const int e7 = (int)((b >> 8) & 0x7fu);
        const unsigned q = (unsigned)min(max(e7 - base, 0), 15);          // 0: E[7:1] == 0 (an escape lands here too: such an image is never used)
        const int by = e & 3, h = e >> 2;
        if (h == 0) la |= (b & 0xffu) << (8 * by); else lb |= (b & 0xffu) << (8 * by);
        cd |= q << (8 * by + 4 * h);
        sign |= (b >> 15) << (8 * by + 2 * c + h);
      }
      lo[2 * c] = la; lo[2 * c + 1] = lb; code[c] = cd;
    }
    u32x4* g = out + grp * 208;
    g[lane] = u32x4{lo[0], lo[1], lo[2], lo[3]};
    g[64 + lane] = u32x4{lo[4], lo[5], lo[6], lo[7]};
    g[128 + lane] = u32x4{code[0], code[1], code[2], code[3]};
    reinterpret_cast<unsigned*>(g + 192)[lane] = sign;
  }
}

}  // namespace

static int g_force_general = 0;

int ua2_linear_launch(const ua2_linear_args& a, hipStream_t s, const Ua2Weights* w8) {
  const Ua2WDemand demand = w8 ? w8->demand : UA2_W_OFFERED;
  const bool w8_many = demand == UA2_W_STATIONARY;
  const auto decode_rows = [&] { return a.dtype == UA2_BF16 && !a.x_packed && a.K > 0 && a.M <= ua2_gemv_rows_preferred(a.dtype, a.K); };
  switch (demand) {      // a kernel asked for by name: the launch is one it serves, or an error
    case UA2_W_OFFERED: break;
    case UA2_W_STATIONARY:
      UA2_CHECK(ua2_gemm_w8_serves(a, *w8),
                "ua2_linear_w8_many: not a launch the fp8 weights-stationary kernel serves (UA2_BF16, K %% 64 == 0, %d to %d rows [UA2_SKINNY_W8_MAX_ROWS], "
                "a released Linear geometry with a STORE / RESIDUAL / SWIGLU / QKV_ROPE epilogue, workspace or x_packed, a built variant)",
                a.K > 0 ? ua2_gemv_rows_preferred(UA2_BF16, a.K) + 1 : 0, ua2_skinny_w8_max_rows());
      break;
    case UA2_W_DECODE:
      if (w8->form == UA2_W_L13)
        UA2_CHECK(decode_rows() && ua2_gemv_l13_ok(a),
                  "ua2_linear_l13: not a launch the decode kernel serves on a 13-bit image (UA2_BF16, K %% 128 == 0, up to %d rows, a prologue / epilogue pair of the decode frame, no x_packed, no argmax fold)",
                  a.K > 0 ? ua2_gemv_rows_preferred(UA2_BF16, a.K) : 0);
      else
        UA2_CHECK(decode_rows() && ua2_gemv_w8_ok(a),
                  "ua2_linear_w8: not a launch the fp8 decode kernel serves (UA2_BF16, K %% 64 == 0, up to %d rows, a prologue / epilogue pair of the decode frame, no x_packed)",
                  a.K > 0 ? ua2_gemv_rows_preferred(UA2_BF16, a.K) : 0);
      break;
  }
  UA2_CHECK(a.M > 0 && a.N > 0 && a.K > 0, "ua2_linear: empty problem M=%d N=%d K=%d", a.M, a.N, a.K);
  UA2_CHECK(a.w0 != nullptr, "ua2_linear: w0 is NULL");
  const int epl = a.dtype == UA2_BF16 ? 8 : 4;
  UA2_CHECK(a.K % epl == 0, "ua2_linear: K=%d must be a multiple of %d", a.K, epl);
  if (a.prologue == UA2_PRO_LOCAL_ATTN) {
    const int kc = a.dtype == UA2_BF16 ? 32 : 16;
    UA2_CHECK(a.M == 1 && a.epilogue == UA2_EPI_RESIDUAL, "ua2_linear: LOCAL_ATTN is the M == 1 O-projection only (use ua2_attn_local + CAST otherwise)");
    UA2_CHECK(a.x && a.row_pos && a.kv.k_pool && a.kv.v_pool && a.kv.page_table && a.kv.n_kv > 0 && a.kv.n_head % a.kv.n_kv == 0 &&
                  (a.kv.head_size == 32 || a.kv.head_size == 64 || a.kv.head_size == 128) &&
                  a.kv.n_head % (128 / a.kv.head_size) == 0 && a.K == a.kv.n_head * a.kv.head_size && a.K % kc == 0,
              "ua2_linear: bad LOCAL_ATTN arguments");
    UA2_CHECK(a.resid != nullptr && a.y != nullptr, "ua2_linear: RESIDUAL needs resid, y");
    if (a.fold.part_max) {   // ua2_argmax_fold
      const ua2_argmax_fold& f = a.fold;
      UA2_CHECK(f.part_idx && f.n_part > 0 && f.limit > 0 && f.out_token && f.tab_y && f.tab_q && f.tab_k && f.tab_v && f.row_off >= 0,
                "ua2_linear: argmax fold: missing partials / tables / out_token");
      UA2_CHECK(f.pos >= 1 && f.pos < 8 && !a.out_scale && a.kv.ring_pages == 0 && !w8,
                "ua2_linear: argmax fold needs 1 <= pos < 8, a linear cache, no out_scale and no fp8 twin");
    }
    const int rc = ua2_gemv_try_launch(a, s, w8);
    UA2_CHECK(rc <= 0, "ua2_linear: LOCAL_ATTN problem outside the decode kernel's range%s", a.fold.part_max ? " (argmax fold: rounds of 4 or 8 chunks per wave)" : "");
    return rc;
  }
  if (a.y_norm_w) {   // producer half of the scaled-norm hand-over
    UA2_CHECK(a.dtype == UA2_BF16 && (a.epilogue == UA2_EPI_RESIDUAL || a.epilogue == UA2_EPI_STORE) && a.N % 32 == 0 && a.y_ssq &&
                  (a.y_h || a.y_packed) && (!a.y_h || a.ldh % 8 == 0),
              "ua2_linear: y_norm_w hand-over needs UA2_BF16, a RESIDUAL / STORE epilogue, N %% 32 == 0, y_ssq and y_h (ldh %% 8 == 0) or y_packed");
  }
  if (a.y_ln_w)     // LayerNorm hand-over: the order-free kernel's form only (ua2_linear_order_free_accepts tells a caller beforehand)
    UA2_CHECK(a.dtype == UA2_BF16 && a.sum_order == UA2_SUM_ORDER_FREE && a.epilogue == UA2_EPI_RESIDUAL && a.y_packed && !a.y_norm_w && a.N % 32 == 0,
              "ua2_linear: y_ln_w needs UA2_BF16, UA2_SUM_ORDER_FREE, a RESIDUAL epilogue, y_packed and N %% 32 == 0");
  if (a.prologue == UA2_PRO_SCALED) {
    UA2_CHECK(a.dtype == UA2_BF16 && a.K % 32 == 0 && a.K <= 4096 && a.x_ssq && (a.x_h || a.x_packed) && (!a.x_h || a.ldh % 8 == 0),
              "ua2_linear: UA2_PRO_SCALED needs UA2_BF16, K %% 32 == 0, K <= 4096, x_ssq and x_h (ldh %% 8 == 0) or x_packed");
    UA2_CHECK(a.epilogue == UA2_EPI_QKV_ROPE || a.epilogue == UA2_EPI_SWIGLU || a.epilogue == UA2_EPI_STORE,
              "ua2_linear: UA2_PRO_SCALED serves the QKV_ROPE, SWIGLU and STORE epilogues");
    // The tiled kernel's staged no-rotation head-size-64 q|k|v epilogue (the DiT's) writes the un-scaled sums: no caller
    // pairs it with the scaled hand-over, and the ABI refuses the pair instead of returning un-normalised q / k / v.
    UA2_CHECK(a.epilogue != UA2_EPI_QKV_ROPE || a.rope_mode != UA2_ROPE_NONE,
              "ua2_linear: UA2_PRO_SCALED with a QKV_ROPE epilogue needs a rotation mode (UA2_ROPE_NONE is served by the NORM / CAST prologues)");
  }
  // bf16 operand rows without a norm (include/ua2hip.h, beside y_norm_w): the decode kernel's launches only, or an error
  const bool x_rows = a.prologue == UA2_PRO_CAST && a.x_h, y_rows = a.epilogue == UA2_EPI_SWIGLU && a.y_h;
  if (x_rows)
    UA2_CHECK(decode_rows() && a.K % 32 == 0 && a.ldx % 8 == 0 && a.ldx >= a.K && (reinterpret_cast<uintptr_t>(a.x_h) & 15) == 0 &&
                  (a.epilogue == UA2_EPI_RESIDUAL || a.epilogue == UA2_EPI_STORE) && !w8_many,
              "ua2_linear: UA2_PRO_CAST with x_h needs UA2_BF16, up to %d rows, K %% 32 == 0, ldx %% 8 == 0, ldx >= K, a 16-byte aligned x_h, "
              "no x_packed and a RESIDUAL / STORE epilogue", a.K > 0 ? ua2_gemv_rows_preferred(UA2_BF16, a.K) : 0);
  if (y_rows)
    UA2_CHECK(decode_rows() && !a.y_norm_w && a.ldy >= a.N && !w8_many && (a.prologue == UA2_PRO_NORM || a.prologue == UA2_PRO_SCALED || a.prologue == UA2_PRO_CAST),
              "ua2_linear: UA2_EPI_SWIGLU with y_h needs UA2_BF16, up to %d rows, ldy >= N, no y_norm_w and no x_packed",
              a.K > 0 ? ua2_gemv_rows_preferred(UA2_BF16, a.K) : 0);
  if (a.x_packed) {   // operand handed over in fragment order by its producer: only the many-row kernels read it
    UA2_CHECK((a.prologue == UA2_PRO_CAST || a.prologue == UA2_PRO_SCALED) && g_force_general != 2,
              "ua2_linear: x_packed needs PRO_CAST / PRO_SCALED and the many-row kernels");
    const int rc = ua2_gemm_try_launch(a, s, w8_many ? 0 : (g_force_general >= 4 ? g_force_general : 3), w8);
    UA2_CHECK(rc <= 0, "%s: x_packed launch not applicable", w8_many ? "ua2_linear_w8_many" : "ua2_linear");
    return rc;
  }
  if (a.prologue == UA2_PRO_SCALED) {   // row-major hand-over: one row tile, the decode kernel
    UA2_CHECK(a.M <= ua2_gemv_rows_per_tile(a.dtype, a.K), "ua2_linear: x_h serves launches of one row tile (M=%d): hand over x_packed", a.M);
    const int rc = ua2_gemv_try_launch(a, s, w8);
    UA2_CHECK(rc <= 0, "ua2_linear: UA2_PRO_SCALED launch outside the decode kernel's range");
    return rc;
  }
  UA2_CHECK(a.prologue == UA2_PRO_CAST || a.prologue == UA2_PRO_NORM, "ua2_linear: bad prologue %d", a.prologue);
  UA2_CHECK(x_rows || (a.x != nullptr && a.ldx % 4 == 0), "ua2_linear: x NULL or ldx %% 4 != 0");
  if (a.prologue == UA2_PRO_NORM)
    UA2_CHECK(a.norm_w != nullptr && (a.norm_kind != UA2_NORM_LAYERNORM || a.norm_b != nullptr) && a.norm_kind >= 0 && a.norm_kind <= 2,
              "ua2_linear: norm_w / norm_b / norm_kind invalid");
  if (a.epilogue == UA2_EPI_GELU) {
    UA2_CHECK(a.y != nullptr || a.y_packed != nullptr, "ua2_linear: GELU needs y or y_packed");
    UA2_CHECK(!a.y_packed || a.N % (a.dtype == UA2_BF16 ? 32 : 16) == 0, "ua2_linear: y_packed needs N %% chunk == 0");
  }
  UA2_CHECK(!a.bias || a.epilogue != UA2_EPI_QKV_ROPE || a.rope_mode != UA2_ROPE_HALF_SPLIT,
            "ua2_linear: bias with the half-split QKV layout is not supported (columns are permuted at pack time)");
  UA2_CHECK(a.act_kind >= 0 && a.act_kind <= 2, "ua2_linear: bad act_kind %d", a.act_kind);
  if (a.epilogue == UA2_EPI_SWIGLU) {
    UA2_CHECK(a.w1 != nullptr && (a.y != nullptr || a.y_packed != nullptr || y_rows), "ua2_linear: SWIGLU needs w1 and y, y_packed or y_h");
    UA2_CHECK(!a.y_packed || a.N % (a.dtype == UA2_BF16 ? 32 : 16) == 0, "ua2_linear: y_packed needs N %% chunk == 0");
  } else if (a.epilogue != UA2_EPI_GELU) {
    UA2_CHECK(!a.y_packed || a.y_norm_w || a.y_ln_w, "ua2_linear: y_packed is a SWIGLU / GELU output (or, with y_norm_w / y_ln_w, a RESIDUAL / STORE hand-over)");
  }
  if (a.epilogue == UA2_EPI_RESIDUAL) UA2_CHECK(a.resid != nullptr && a.y != nullptr, "ua2_linear: RESIDUAL needs resid, y");
  if (a.epilogue == UA2_EPI_STORE) UA2_CHECK(a.y != nullptr || a.part_max != nullptr, "ua2_linear: STORE needs y or part_max");
  if (a.epilogue == UA2_EPI_QKV_ROPE) {
    UA2_CHECK(a.kv.head_size % (a.rope_mode == UA2_ROPE_HALF_SPLIT ? 32 : 16) == 0 &&
                  a.N == (a.kv.n_head + 2 * a.kv.n_kv) * a.kv.head_size && a.rope_mode >= 0 && a.rope_mode <= 2,
              "ua2_linear: QKV_ROPE needs head_size %% 32 == 0 (16 when not half-split) and N == (n_head+2*n_kv)*head_size");
    UA2_CHECK(a.row_pos && (a.rope_mode == UA2_ROPE_NONE || (a.rope_cos && a.rope_sin)) && a.q_out && a.kv.k_pool && a.kv.v_pool &&
                  a.kv.page_table,
              "ua2_linear: QKV_ROPE pointer arguments missing");
    UA2_CHECK(a.kv.ring_pages == 0 || (a.kv.ring_pages & (a.kv.ring_pages - 1)) == 0, "ua2_linear: ring_pages=%d must be a power of two", a.kv.ring_pages);
  }
  if (a.dtype != UA2_BF16 && a.dtype != UA2_F32) {
    ua2_set_error("ua2_linear: bad dtype %d", a.dtype);
    return -1;
  }
  if (w8_many) {    // by name: the weights-stationary kernel on the fp8 image or an error (ua2_gemm_w8_serves above said it takes the launch)
    const int rc = ua2_gemm_try_launch(a, s, 0, w8);
    UA2_CHECK(rc <= 0, "ua2_linear_w8_many: the fp8 weights-stationary kernel did not take the launch");
    return rc;
  }
  if (g_force_general != 2 && demand != UA2_W_DECODE && !x_rows && !y_rows) {      // (bf16 operand rows: the decode kernel alone reads / writes them)
    const int rc = ua2_gemm_try_launch(a, s, g_force_general >= 3 ? g_force_general : 0, w8);  // many rows: packed operand, 128-row tiles
    if (rc <= 0) return rc;
  }
  const int rc = ua2_gemv_try_launch(a, s, w8);  // decode regime: LDS-staged activations, all loads up front
  UA2_CHECK(rc <= 0, "ua2_linear: prologue %d / epilogue %d / K=%d is outside the built kernels (a row must fit the LDS operand tile)",
            a.prologue, a.epilogue, a.K);
  return rc;
}

extern "C" int ua2_debug_force_general_linear(int on) {
  const int old = g_force_general;
  g_force_general = (on == 1) ? 0 : on;   // mode 1 (the round-1 general-M kernel) no longer exists
  return old;
}

extern "C" int ua2_linear(const ua2_linear_args* a, void* stream) {
  UA2_CHECK(a != nullptr, "ua2_linear: NULL args");
  return ua2_linear_launch(*a, (hipStream_t)stream);
}

// The event-timed loop of the *_chain_timed exports: launch(0) .. launch(n - 1) back to back, iters times.  The events are destroyed on
// every path (a refused launch, a failed HIP call).
template <class LaunchFn>
static int chain_timed(int32_t n, int32_t iters, hipStream_t s, float* ms_out, LaunchFn&& launch) {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  const auto run = [&]() -> int {
    UA2_HIP(hipEventCreate(&e0));
    UA2_HIP(hipEventCreate(&e1));
    UA2_HIP(hipEventRecord(e0, s));
    for (int it = 0; it < iters; ++it)
      for (int i = 0; i < n; ++i)
        if (int rc = launch(i)) return rc;
    UA2_HIP(hipEventRecord(e1, s));
    UA2_HIP(hipEventSynchronize(e1));
    UA2_HIP(hipEventElapsedTime(ms_out, e0, e1));
    return 0;
  };
  const int rc = run();
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  return rc;
}

extern "C" int ua2_linear_chain_timed(const ua2_linear_args* args, int32_t n, int32_t iters, void* stream,
                                      float* ms_out) {
  UA2_CHECK(args && n > 0 && iters > 0 && ms_out, "ua2_linear_chain_timed: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  return chain_timed(n, iters, s, ms_out, [&](int i) { return ua2_linear_launch(args[i], s); });
}

// A launch on weight images asked for by name (`name`: the entry point; `what`: what its messages call an image).  Ref = ua2_w8_ref /
// ua2_l13_ref: the image and its side array.
template <class Ref>
static int linear_by_name(const char* name, const char* what, Ua2WForm form, Ua2WDemand demand, const ua2_linear_args* a, const Ref* w0,
                          const Ref* w1, hipStream_t s) {
  Ua2Weights w;
  w.form = form; w.demand = demand;
  if (w0) { const auto& [q, e] = *w0; w.img.q0 = q; w.img.e0 = e; }
  if (w1) { const auto& [q, e] = *w1; w.img.q1 = q; w.img.e1 = e; }
  UA2_CHECK(a != nullptr && w.complete(UA2_EPI_STORE), "%s: NULL args or %s of w0", name, what);
  UA2_CHECK(w.complete(a->epilogue), "%s: SWIGLU needs the %s of w1", name, what);
  return ua2_linear_launch(*a, s, &w);
}
static int linear_w8_many(const ua2_linear_args* a, const ua2_w8_ref* w0, const ua2_w8_ref* w1, hipStream_t s) {
  return linear_by_name("ua2_linear_w8_many", "fp8 twin", UA2_W_FP8, UA2_W_STATIONARY, a, w0, w1, s);
}
static int linear_l13(const ua2_linear_args* a, const ua2_l13_ref* w0, const ua2_l13_ref* w1, hipStream_t s) {
  return linear_by_name("ua2_linear_l13", "image", UA2_W_L13, UA2_W_DECODE, a, w0, w1, s);
}

extern "C" size_t ua2_packed_elems(int dtype, int64_t N, int64_t K) {
  const int kc = dtype == UA2_BF16 ? 32 : 16, epl = dtype == UA2_BF16 ? 8 : 4;
  return (size_t)((N + 15) / 16) * (size_t)((K + kc - 1) / kc) * 64 * epl;
}

extern "C" int ua2_pack_linear(const void* src, int src_dtype, int transposed, int64_t N, int64_t K, void* out,
                               int dtype, int rope_head_size, void* stream) {
  UA2_CHECK(src && out && N > 0 && K > 0, "ua2_pack_linear: bad arguments");
  UA2_CHECK(rope_head_size == 0 || (rope_head_size % 32 == 0 && N % rope_head_size == 0),
            "ua2_pack_linear: rope_head_size=%d must divide N and be a multiple of 32", rope_head_size);
  const int64_t total = (int64_t)ua2_packed_elems(dtype, N, K);
  const int threads = 256;
  const int blocks = (int)((total + threads - 1) / threads < 65535 * 16 ? (total + threads - 1) / threads : 65535 * 16);
  hipStream_t s = (hipStream_t)stream;
  if (src_dtype == UA2_F32 && dtype == UA2_F32)
    hipLaunchKernelGGL((pack_kernel<UA2_F32, UA2_F32>), dim3(blocks), dim3(threads), 0, s, src, out, transposed, N, K, total, rope_head_size);
  else if (src_dtype == UA2_F32 && dtype == UA2_BF16)
    hipLaunchKernelGGL((pack_kernel<UA2_F32, UA2_BF16>), dim3(blocks), dim3(threads), 0, s, src, out, transposed, N, K, total, rope_head_size);
  else if (src_dtype == UA2_BF16 && dtype == UA2_BF16)
    hipLaunchKernelGGL((pack_kernel<UA2_BF16, UA2_BF16>), dim3(blocks), dim3(threads), 0, s, src, out, transposed, N, K, total, rope_head_size);
  else if (src_dtype == UA2_BF16 && dtype == UA2_F32)
    hipLaunchKernelGGL((pack_kernel<UA2_BF16, UA2_F32>), dim3(blocks), dim3(threads), 0, s, src, out, transposed, N, K, total, rope_head_size);
  else {
    ua2_set_error("ua2_pack_linear: bad dtypes %d -> %d", src_dtype, dtype);
    return -1;
  }
  UA2_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t ua2_packed_bytes_w8(int64_t N, int64_t K) {
  if (N <= 0 || K <= 0 || K % 64) return 0;
  return (size_t)((N + 15) / 16) * 16 * (size_t)K;
}

extern "C" int ua2_pack_linear_w8(const void* src, int src_dtype, int transposed, int64_t N, int64_t K, void* out_q, int8_t* out_exp,
                                  void* out_bf16, int rope_head_size, void* stream) {
  UA2_CHECK(src && out_q && out_exp && N > 0 && K > 0, "ua2_pack_linear_w8: bad arguments");
  UA2_CHECK(K % 64 == 0, "ua2_pack_linear_w8: K=%lld must be a multiple of 64 (two 32-wide chunks per fp8 burst)", (long long)K);
  UA2_CHECK(rope_head_size == 0 || (rope_head_size % 32 == 0 && N % rope_head_size == 0),
            "ua2_pack_linear_w8: rope_head_size=%d must divide N and be a multiple of 32", rope_head_size);
  UA2_CHECK(src_dtype == UA2_F32 || src_dtype == UA2_BF16, "ua2_pack_linear_w8: bad source dtype %d", src_dtype);
  hipStream_t s = (hipStream_t)stream;
  const int64_t n16 = (N + 15) / 16 * 16, total = n16 * K;
  const int eblocks = (int)((n16 + 3) / 4);
  const int blocks = (int)std::min<int64_t>((total + 255) / 256, 65535 * 16);
  if (src_dtype == UA2_F32) {
    hipLaunchKernelGGL(w8_exp_kernel<UA2_F32>, dim3(eblocks), dim3(256), 0, s, src, out_exp, transposed, N, K, n16, rope_head_size);
    hipLaunchKernelGGL(w8_pack_kernel<UA2_F32>, dim3(blocks), dim3(256), 0, s, src, out_exp, (uint8_t*)out_q, (unsigned short*)out_bf16, transposed, N, K, total, rope_head_size);
  } else {
    hipLaunchKernelGGL(w8_exp_kernel<UA2_BF16>, dim3(eblocks), dim3(256), 0, s, src, out_exp, transposed, N, K, n16, rope_head_size);
    hipLaunchKernelGGL(w8_pack_kernel<UA2_BF16>, dim3(blocks), dim3(256), 0, s, src, out_exp, (uint8_t*)out_q, (unsigned short*)out_bf16, transposed, N, K, total, rope_head_size);
  }
  UA2_LAUNCH_CHECK();
  return 0;
}

extern "C" int ua2_linear_w8(const ua2_linear_args* a, const ua2_w8_ref* w0, const ua2_w8_ref* w1, void* stream) {
  return linear_by_name("ua2_linear_w8", "fp8 twin", UA2_W_FP8, UA2_W_DECODE, a, w0, w1, (hipStream_t)stream);
}

extern "C" size_t ua2_packed_bytes_l13(int64_t N, int64_t K) {
  if (N <= 0 || K <= 0 || K % 128) return 0;
  return (size_t)((N + 15) / 16) * (size_t)(K / 128) * 3328;
}

extern "C" int ua2_pack_linear_l13(const void* packed_bf16, int64_t N, int64_t K, void* out_image, uint8_t* out_base, int32_t* escapes, void* stream) {
  UA2_CHECK(packed_bf16 && out_image && out_base && escapes && N > 0 && K > 0, "ua2_pack_linear_l13: bad arguments");
  UA2_CHECK(K % 128 == 0, "ua2_pack_linear_l13: K=%lld must be a multiple of 128 (groups of four 32-wide chunks)", (long long)K);
  hipStream_t s = (hipStream_t)stream;
  const int64_t tiles = (N + 15) / 16, groups = K / 128, total = tiles * groups * 64;
  UA2_HIP(hipMemsetAsync(escapes, 0, sizeof(int32_t), s));
  hipLaunchKernelGGL(l13_base_kernel, dim3((unsigned)tiles), dim3(256), 0, s, (const unsigned short*)packed_bf16, out_base, escapes, 16 * K);
  hipLaunchKernelGGL(l13_pack_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 65535 * 16)), dim3(256), 0, s, (const u32x4*)packed_bf16,
                     out_base, (u32x4*)out_image, groups, total);
  UA2_LAUNCH_CHECK();
  return 0;
}

extern "C" int ua2_linear_l13(const ua2_linear_args* a, const ua2_l13_ref* w0, const ua2_l13_ref* w1, void* stream) {
  return linear_l13(a, w0, w1, (hipStream_t)stream);
}

extern "C" int ua2_linear_l13_chain_timed(const ua2_linear_args* args, const ua2_l13_ref* w0, const ua2_l13_ref* w1, int32_t n, int32_t iters,
                                          void* stream, float* ms_out) {
  UA2_CHECK(args && w0 && n > 0 && iters > 0 && ms_out, "ua2_linear_l13_chain_timed: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  return chain_timed(n, iters, s, ms_out, [&](int i) { return linear_l13(&args[i], &w0[i], w1 ? &w1[i] : nullptr, s); });
}

extern "C" int ua2_linear_w8_many(const ua2_linear_args* a, const ua2_w8_ref* w0, const ua2_w8_ref* w1, void* stream) {
  return linear_w8_many(a, w0, w1, (hipStream_t)stream);
}

extern "C" int ua2_linear_w8_many_chain_timed(const ua2_linear_args* args, const ua2_w8_ref* w0, const ua2_w8_ref* w1, int32_t n, int32_t iters,
                                              void* stream, float* ms_out) {
  UA2_CHECK(args && w0 && n > 0 && iters > 0 && ms_out, "ua2_linear_w8_many_chain_timed: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  return chain_timed(n, iters, s, ms_out, [&](int i) { return linear_w8_many(&args[i], &w0[i], w1 ? &w1[i] : nullptr, s); });
}
