// Top-k sampling tail of a frame (model_new.py:146-187 sample_topk / audio_sample_topk with topk > 1):
//   logits / T  ->  [:forbid_prefix] = -inf  ->  keep logits >= k-th largest (ties at the threshold are
//   all kept, `logits < topk_value` is what gets removed, :150,182)  ->  softmax  ->  arg-max(probs / q),
//   q ~ Exp(1) (:141-143, the "exponential race" = one multinomial draw)  ->  int32 id,
// fused with the next-step embedding gather (:640,662-663) like ua2_argmax_embed.
//
// The k-th largest value is found exactly with a 4-pass radix select (8 bits per pass) on the
// order-preserving integer image of the fp32 logits, one workgroup per row (the row is L2-resident:
// 513 KB for the text head); softmax normalisation is dropped (it does not move the arg-max).
// Randomness: counter-based Philox4x32-10 keyed by (seed + the 64-bit device word counter[1..2], draw index
// counter[0] from the device frame counter, row, stream) — reproducible under hipGraph replay and independent of launch geometry.  It cannot
// reproduce torch's generator stream; parity with the reference is distributional (tests).
//
// Nucleus (top-p) filter (llm_utils/sampling.py:66-82 sample_top_p; include/ua2hip.h ua2_sample_topp has the contract): among the
// top-k kept columns, keep column c iff the mass of the kept columns of strictly greater value is at most top_p of the kept mass.
// The masses are integers, q_c = floor(expf(l_c - mx) * 2^40), so their sums do not depend on the order the threads add them in; the
// threshold value is found by a second, WEIGHTED 4-pass radix select on the same keys (256 buckets of uint64 mass per pass), and the
// race then runs over key >= max(k-th key, threshold key).  Ties at the threshold value are all kept, like the top-k filter's.
// The filter is a template parameter: the top-k-only kernels are the code they were.
//
// Repetition penalty (include/ua2hip.h ua2_sample_penalized has the contract; not in the reference): the columns named by the last
// min(len, W) ids of the row's history ring read l' = (l < 0) ? l * theta : l / theta in place of l, once per distinct id, before the
// temperature division; the drawn id is appended to the ring.  The distinct ids are a V-bit set in LDS (16 KB at V = 131072) filled
// with LDS atomic ORs; every pass reads its logit through one helper (lv), so the select, the maximum, the nucleus masses and the race
// see one value.  One more template parameter: the four kernels above it keep their code, and the set exists in the penalised ones only.
#include "ua2_common.h"

namespace {

__device__ __forceinline__ unsigned key_of(float f) {   // monotone: larger float -> larger key; -0.0 and +0.0 share one key
  unsigned u = __float_as_uint(f);                       // (`logits < topk_value` keeps -0.0 at a +0.0 threshold: they compare equal)
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ void philox4x32(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                           unsigned (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// The repetition penalty of a penalised launch (ua2_sample_args.rep_*): row m's ring is hist + m * hist_ld, its counter len[m * len_ld]
struct RepArgs {
  float theta;
  int window, cap;
  int32_t* hist;
  int hist_ld;
  int32_t* len;
  int len_ld;
};

// One row of the tail: block m of either kernel below.  (draw, row_part, seed) is the row's random stream — Philox counter
// (column, draw, row_part, stream_id) under the 64-bit key `seed`; everything else is the row's data.
// TOPP: the nucleus form — nucleus != 0 filters with P = floor(top_p * 2^32); keep_count (optional) [M] = columns that entered the race
// REP: the penalised form — the columns of the ring's last min(len, window) ids are read penalised, and the id is appended
template <int DT, bool TOPP = false, bool REP = false>
__device__ __forceinline__ void sample_topk_row(const float* __restrict__ logits, int ld, int V, int topk, float temperature,
                                                const int32_t* __restrict__ forbid, unsigned long long seed, unsigned draw,
                                                unsigned row_part, int stream_id, int32_t* __restrict__ out_tokens, int out_ld,
                                                int out_col, const void* __restrict__ emb, int emb_off, int C,
                                                float* __restrict__ next_h, int nucleus = 0, unsigned long long P = 0ull,
                                                int32_t* __restrict__ keep_count = nullptr, RepArgs rep = RepArgs{}) {
  __shared__ unsigned hist[256];
  __shared__ unsigned sel_prefix, sel_remaining;
  __shared__ float red_v[16];
  __shared__ int red_i[16];
  __shared__ int tok_s;
  const int m = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const float* row = logits + (size_t)m * ld;
  const int fb = forbid ? max(forbid[m], 0) : 0;
  // lv(c): the logit of column c as the sampler reads it — row[c], or its penalised value when c is in the set
  [[maybe_unused]] unsigned* rep_set = nullptr;
  [[maybe_unused]] int rep_n = 0;
  if constexpr (REP) {
    __shared__ unsigned rep_bits[(1 << 17) / 32];          // bit c: column c is among the last min(len, window) ids (V <= 131072: the launcher checks)
    rep_set = rep_bits;
    const int32_t* ring = rep.hist + (size_t)m * rep.hist_ld;
    rep_n = max(rep.len[(size_t)m * rep.len_ld], 0);
    for (int i = tid; i < (V + 31) / 32; i += nt) rep_bits[i] = 0u;
    __syncthreads();
    for (int j = rep_n - min(rep_n, rep.window) + tid; j < rep_n; j += nt) {
      const int id = ring[j % rep.cap];                    // entry j of the history lives in slot j % cap
      if (id >= 0 && id < V) atomicOr(&rep_bits[id >> 5], 1u << (id & 31));
    }
    __syncthreads();
  }
  auto lv = [&](int c) -> float {
    const float l = row[c];
    if constexpr (REP) {
      if ((rep_set[c >> 5] >> (c & 31)) & 1u) return l < 0.f ? l * rep.theta : l / rep.theta;
    }
    return l;
  };
  // ---- exact k-th largest key among columns [fb, V) -------------------------------------------
  if (tid == 0) { sel_prefix = 0u; sel_remaining = (unsigned)topk; }
  for (int pass = 3; pass >= 0; --pass) {
    if (tid < 256) hist[tid] = 0u;
    __syncthreads();
    const unsigned prefix = sel_prefix, shift = pass * 8;
    const unsigned mask_hi = (pass == 3) ? 0u : (0xffffffffu << (shift + 8));
    for (int c = fb + tid; c < V; c += nt) {
      const unsigned k = key_of(lv(c) / temperature);
      if ((k & mask_hi) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned rem = sel_remaining;
      int b = 255;
      for (; b > 0; --b) {                       // walk buckets from the largest digit down
        if (hist[b] >= rem) break;
        rem -= hist[b];
      }
      sel_prefix = prefix | ((unsigned)b << shift);
      sel_remaining = rem;
    }
    __syncthreads();
  }
  const unsigned kth = sel_prefix;               // key of the k-th largest scaled logit
  // ---- exponential race among the kept columns ------------------------------------------------
  float mx = -INFINITY;
  for (int c = fb + tid; c < V; c += nt) mx = fmaxf(mx, lv(c) / temperature);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  if ((tid & 63) == 0) red_v[tid >> 6] = mx;
  __syncthreads();
  mx = red_v[0];
  for (int w = 1; w < (nt >> 6); ++w) mx = fmaxf(mx, red_v[w]);
  __syncthreads();
  unsigned thr = kth;                            // the race admits key >= thr
  int kept = 0;
  if constexpr (TOPP) {
    // ---- nucleus: lowest value v* whose strictly-greater kept mass S_gt satisfies S_gt * 2^32 <= P * Z ------------------------
    __shared__ unsigned long long mass[256];
    __shared__ unsigned long long nu_above, nu_pz_lo, nu_pz_hi;   // mass above the selected prefix; P * Z as 128 bits
    __shared__ unsigned nu_prefix;
    __shared__ int nu_on;
    if (tid == 0) { nu_prefix = 0u; nu_above = 0ull; nu_on = nucleus; }
    for (int pass = 3; pass >= 0 && nucleus; --pass) {
      if (tid < 256) mass[tid] = 0ull;
      __syncthreads();
      if (!nu_on) break;                         // Z == 0 (a row of -inf or NaN): no filter, the all-NaN rule decides
      const unsigned prefix = nu_prefix, shift = pass * 8;
      const unsigned mask_hi = (pass == 3) ? 0u : (0xffffffffu << (shift + 8));
      // a thread sums runs of columns that share a bucket before it touches LDS: neighbouring logits mostly share the top byte,
      // and a flat row shares all four
      int rb = -1;
      unsigned long long rs = 0ull;
      for (int c = fb + tid; c < V; c += nt) {
        const float l = lv(c) / temperature;
        const unsigned k = key_of(l);
        if (k < kth || (k & mask_hi) != prefix) continue;
        const float e = expf(l - mx);
        const unsigned long long q = (e == e && e < INFINITY) ? (unsigned long long)(e * 1099511627776.0f) : 0ull;   // floor(e * 2^40)
        if (q == 0ull) continue;
        const int b = (int)((k >> shift) & 255u);
        if (b != rb) {
          if (rs) atomicAdd(&mass[rb], rs);
          rb = b; rs = 0ull;
        }
        rs += q;
      }
      const int b0 = __shfl(rb, 0);
      if (__all(rb == b0)) {                     // the wave ends on one bucket (always on a flat row): one add per wave
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) rs += __shfl_xor(rs, o);
        if ((tid & 63) == 0 && rs) atomicAdd(&mass[b0], rs);
      } else if (rs) {
        atomicAdd(&mass[rb], rs);
      }
      __syncthreads();
      if (tid < 64) {
        // The lowest bucket that holds mass and whose top value is kept (mass above it * 2^32 <= P * Z; the mass above only grows on
        // the way down, so the kept buckets are the leading ones).  One wave: lane j owns buckets 255 - 4j .. 252 - 4j, a shuffle scan
        // over the lanes gives the mass above each — 256 dependent LDS reads of one thread otherwise, as long as the pass itself.
        unsigned long long m4[4], tot = 0ull;
#pragma unroll
        for (int i = 0; i < 4; ++i) { m4[i] = mass[255 - 4 * tid - i]; tot += m4[i]; }
        unsigned long long inc = tot;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const unsigned long long t = __shfl_up(inc, o);
          if (tid >= o) inc += t;
        }
        unsigned long long pz_lo = nu_pz_lo, pz_hi = nu_pz_hi;
        int on = nu_on;
        if (pass == 3) {                         // the first pass's buckets hold every kept column: their total is Z
          const unsigned long long Z = __shfl(inc, 63);
          pz_lo = P * Z; pz_hi = __umul64hi(P, Z);
          on = Z != 0ull;
          if (tid == 0) { nu_pz_lo = pz_lo; nu_pz_hi = pz_hi; nu_on = on; }
        }
        unsigned long long acc = nu_above + (inc - tot), cand_acc = 0ull;
        int cand = 256;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const unsigned long long a_hi = acc >> 32, a_lo = acc << 32;         // acc * 2^32 (acc <= 2^57)
          if (m4[i] != 0ull && !(a_hi > pz_hi || (a_hi == pz_hi && a_lo > pz_lo))) { cand = 255 - 4 * tid - i; cand_acc = acc; }
          acc += m4[i];
        }
        int sel = cand;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) sel = min(sel, __shfl_xor(sel, o));
        if (on && sel < 256 && cand == sel) {    // (on: the top bucket that holds mass always qualifies, so sel < 256; one lane owns it)
          nu_prefix = prefix | ((unsigned)sel << shift);
          nu_above = cand_acc;
        }
      }
      __syncthreads();
    }
    if (nucleus && nu_on) thr = max(kth, nu_prefix);
  }
  float bv = -INFINITY;
  int bi = UA2_TOK_NONE;
  for (int c = fb + tid; c < V; c += nt) {
    const float l = lv(c) / temperature;
    if (key_of(l) < thr) continue;               // removed: strictly below the k-th value (and, TOPP, below the nucleus threshold)
    if constexpr (TOPP) ++kept;
    unsigned r[4];
    philox4x32((unsigned)c, draw, row_part, (unsigned)stream_id, (unsigned)seed, (unsigned)(seed >> 32), r);
    // (0, 1): x + 0.5 rounds to even from x = 2^23 on and reaches 2^24 at x = 2^24 - 1 — u == 1.0f, q == -0.0f, score == -inf for the
    // column that drew the SMALLEST q — so the product is held at the largest fp32 below 1 (include/ua2hip.h; one draw in 2^24 changes)
    const float u = fminf(((float)(r[0] >> 8) + 0.5f) * (1.0f / 16777216.0f), 0x1.fffffep-1f);
    const float q = -logf(u);                                                // Exp(1)
    const float score = expf(l - mx) / q;                                    // probs / q up to the softmax constant
    if (score > bv || (score == bv && c < bi)) { bv = score; bi = c; }
  }
  // every kept column scored NaN (a NaN or all -inf row): the lowest column the row may sample (ua2_row_token)
  const int tok = ua2_row_token(bv, bi, V, red_v, red_i, &tok_s, [&] { return (tid == 0 && fb < V) ? fb : UA2_TOK_NONE; });
  if (tid == 0) out_tokens[(size_t)m * out_ld + out_col] = tok;
  if constexpr (REP) {
    if (tid == 0 && tok >= 0 && tok < V) {       // every thread read the ring and the counter before the barriers of ua2_row_token
      rep.hist[(size_t)m * rep.hist_ld + rep_n % rep.cap] = tok;
      rep.len[(size_t)m * rep.len_ld] = rep_n + 1;
    }
  }
  if constexpr (TOPP) {
    if (keep_count) {                            // red_i is free again: ua2_row_token's last reader is behind its barriers
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) kept += __shfl_xor(kept, o);
      if ((tid & 63) == 0) red_i[tid >> 6] = kept;
      __syncthreads();
      if (tid == 0) {
        int n = 0;
        for (int w = 0; w < (nt >> 6); ++w) n += red_i[w];
        keep_count[m] = n;
      }
    }
  }
  if (emb) {
    const size_t er = (size_t)tok + (size_t)emb_off;
    for (int c = tid; c < C; c += nt) next_h[(size_t)m * C + c] = load_elem<DT>(emb, er * C + c);
  }
}

// shared stream: one seed and one draw index for the launch, the row index (m >> row_key_shift) tells the rows apart
template <int DT>
__global__ __launch_bounds__(1024) void sample_topk_kernel(const float* __restrict__ logits, int ld, int V, int topk,
                                                           float temperature, const int32_t* __restrict__ forbid,
                                                           unsigned long long seed, const int32_t* __restrict__ counter,
                                                           int stream_id, int32_t* __restrict__ out_tokens, int out_ld,
                                                           int out_col, const void* __restrict__ emb, int emb_off, int C,
                                                           float* __restrict__ next_h, int row_key_shift) {
  // device-resident part of the key (ua2_stage3_set_sampling writes it): added to the by-value seed
  seed += (unsigned long long)(unsigned)counter[1] | ((unsigned long long)(unsigned)counter[2] << 32);
  sample_topk_row<DT>(logits, ld, V, topk, temperature, forbid, seed, (unsigned)counter[0], (unsigned)((int)blockIdx.x >> row_key_shift),
                      stream_id, out_tokens, out_ld, out_col, emb, emb_off, C, next_h);
}

// per-row streams: row m draws under its own key row_key[m] = (lo, hi) at its own index row_draw[m]; neither the row index nor
// a shared counter enters, so the row's ids are those of a one-row launch of the kernel above with that key and that index
template <int DT>
__global__ __launch_bounds__(1024) void sample_topk_rows_kernel(const float* __restrict__ logits, int ld, int V, int topk,
                                                                float temperature, const int32_t* __restrict__ forbid,
                                                                const int32_t* __restrict__ row_key, const int32_t* __restrict__ row_draw,
                                                                int stream_id, int32_t* __restrict__ out_tokens, int out_ld,
                                                                int out_col, const void* __restrict__ emb, int emb_off, int C,
                                                                float* __restrict__ next_h) {
  const int m = blockIdx.x;
  const unsigned long long seed = (unsigned long long)(unsigned)row_key[2 * m] | ((unsigned long long)(unsigned)row_key[2 * m + 1] << 32);
  sample_topk_row<DT>(logits, ld, V, topk, temperature, forbid, seed, (unsigned)row_draw[m], 0u, stream_id, out_tokens, out_ld, out_col,
                      emb, emb_off, C, next_h);
}

// the two kernels above with the nucleus filter (sample_topk_row<DT, true>): the same streams, the same race
template <int DT>
__global__ __launch_bounds__(1024) void sample_topp_kernel(const float* __restrict__ logits, int ld, int V, int topk,
                                                           float temperature, const int32_t* __restrict__ forbid,
                                                           unsigned long long seed, const int32_t* __restrict__ counter,
                                                           int stream_id, int32_t* __restrict__ out_tokens, int out_ld,
                                                           int out_col, const void* __restrict__ emb, int emb_off, int C,
                                                           float* __restrict__ next_h, int row_key_shift, int nucleus,
                                                           unsigned long long P, int32_t* __restrict__ keep_count) {
  seed += (unsigned long long)(unsigned)counter[1] | ((unsigned long long)(unsigned)counter[2] << 32);
  sample_topk_row<DT, true>(logits, ld, V, topk, temperature, forbid, seed, (unsigned)counter[0], (unsigned)((int)blockIdx.x >> row_key_shift),
                            stream_id, out_tokens, out_ld, out_col, emb, emb_off, C, next_h, nucleus, P, keep_count);
}

template <int DT>
__global__ __launch_bounds__(1024) void sample_topp_rows_kernel(const float* __restrict__ logits, int ld, int V, int topk,
                                                                float temperature, const int32_t* __restrict__ forbid,
                                                                const int32_t* __restrict__ row_key, const int32_t* __restrict__ row_draw,
                                                                int stream_id, int32_t* __restrict__ out_tokens, int out_ld,
                                                                int out_col, const void* __restrict__ emb, int emb_off, int C,
                                                                float* __restrict__ next_h, int nucleus, unsigned long long P,
                                                                int32_t* __restrict__ keep_count) {
  const int m = blockIdx.x;
  const unsigned long long seed = (unsigned long long)(unsigned)row_key[2 * m] | ((unsigned long long)(unsigned)row_key[2 * m + 1] << 32);
  sample_topk_row<DT, true>(logits, ld, V, topk, temperature, forbid, seed, (unsigned)row_draw[m], 0u, stream_id, out_tokens, out_ld, out_col,
                            emb, emb_off, C, next_h, nucleus, P, keep_count);
}

// the four kernels above under the repetition penalty (sample_topk_row<DT, TOPP, true>), as one template: ROWS picks the per-row streams
// (row_key / row_draw) over the shared one (seed / counter / row_key_shift); the streams, the filters and the race are theirs
template <int DT, bool TOPP, bool ROWS>
__global__ __launch_bounds__(1024) void sample_pen_kernel(const float* __restrict__ logits, int ld, int V, int topk, float temperature,
                                                          const int32_t* __restrict__ forbid, unsigned long long seed,
                                                          const int32_t* __restrict__ counter, int row_key_shift,
                                                          const int32_t* __restrict__ row_key, const int32_t* __restrict__ row_draw,
                                                          int stream_id, int32_t* __restrict__ out_tokens, int out_ld, int out_col,
                                                          const void* __restrict__ emb, int emb_off, int C, float* __restrict__ next_h,
                                                          int nucleus, unsigned long long P, int32_t* __restrict__ keep_count, RepArgs rep) {
  const int m = blockIdx.x;
  unsigned draw, row_part;
  if constexpr (ROWS) {
    seed = (unsigned long long)(unsigned)row_key[2 * m] | ((unsigned long long)(unsigned)row_key[2 * m + 1] << 32);
    draw = (unsigned)row_draw[m]; row_part = 0u;
  } else {
    seed += (unsigned long long)(unsigned)counter[1] | ((unsigned long long)(unsigned)counter[2] << 32);
    draw = (unsigned)counter[0]; row_part = (unsigned)(m >> row_key_shift);
  }
  sample_topk_row<DT, TOPP, true>(logits, ld, V, topk, temperature, forbid, seed, draw, row_part, stream_id, out_tokens, out_ld, out_col, emb,
                                  emb_off, C, next_h, nucleus, P, keep_count, rep);
}

// row_draw[0 .. R) += 1: the per-row form of the executor's one draw-index bump per sampled frame
__global__ void bump_rows_kernel(int32_t* __restrict__ row_draw, int R) {
  for (int m = threadIdx.x; m < R; m += blockDim.x) row_draw[m] = (int32_t)((unsigned)row_draw[m] + 1u);
}

}  // namespace

extern "C" int ua2_sample_topk(int dtype, int32_t M, const float* logits, int32_t ld, int32_t V, int32_t topk,
                               float temperature, const int32_t* forbid, uint64_t seed, const int32_t* counter,
                               int32_t stream_id, int32_t* out_tokens, int32_t out_ld, int32_t out_col, const void* emb,
                               int32_t emb_row_offset, int32_t C, float* next_h, int32_t row_key_shift, void* stream) {
  UA2_CHECK(M > 0 && logits && V > 0 && out_tokens && counter && row_key_shift >= 0 && row_key_shift <= 1, "ua2_sample_topk: bad arguments");
  UA2_CHECK(temperature > 0.f, "temperature must be > 0");                       // model_new.py:165-166
  UA2_CHECK(topk >= 1 && topk <= V, "topk must be in 1..%d", V);                 // :177-178 (per-row forbid checked by the host)
  UA2_CHECK(!emb || next_h, "ua2_sample_topk: next_h is NULL");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == UA2_BF16)
    hipLaunchKernelGGL((sample_topk_kernel<UA2_BF16>), dim3(M), dim3(1024), 0, s, logits, ld, V, topk, temperature, forbid,
                       (unsigned long long)seed, counter, stream_id, out_tokens, out_ld, out_col, emb, emb_row_offset, C, next_h, row_key_shift);
  else if (dtype == UA2_F32)
    hipLaunchKernelGGL((sample_topk_kernel<UA2_F32>), dim3(M), dim3(1024), 0, s, logits, ld, V, topk, temperature, forbid,
                       (unsigned long long)seed, counter, stream_id, out_tokens, out_ld, out_col, emb, emb_row_offset, C, next_h, row_key_shift);
  else {
    ua2_set_error("ua2_sample_topk: bad dtype %d", dtype);
    return -1;
  }
  UA2_LAUNCH_CHECK();
  return 0;
}

extern "C" int ua2_sample_topk_rows(int dtype, int32_t M, const float* logits, int32_t ld, int32_t V, int32_t topk, float temperature,
                                    const int32_t* forbid, const int32_t* row_key, const int32_t* row_draw, int32_t stream_id,
                                    int32_t* out_tokens, int32_t out_ld, int32_t out_col, const void* emb, int32_t emb_row_offset,
                                    int32_t C, float* next_h, void* stream) {
  UA2_CHECK(M > 0 && logits && V > 0 && out_tokens && row_key && row_draw, "ua2_sample_topk_rows: bad arguments");
  UA2_CHECK(temperature > 0.f, "temperature must be > 0");
  UA2_CHECK(topk >= 1 && topk <= V, "topk must be in 1..%d", V);
  UA2_CHECK(!emb || next_h, "ua2_sample_topk_rows: next_h is NULL");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == UA2_BF16)
    hipLaunchKernelGGL((sample_topk_rows_kernel<UA2_BF16>), dim3(M), dim3(1024), 0, s, logits, ld, V, topk, temperature, forbid, row_key,
                       row_draw, stream_id, out_tokens, out_ld, out_col, emb, emb_row_offset, C, next_h);
  else if (dtype == UA2_F32)
    hipLaunchKernelGGL((sample_topk_rows_kernel<UA2_F32>), dim3(M), dim3(1024), 0, s, logits, ld, V, topk, temperature, forbid, row_key,
                       row_draw, stream_id, out_tokens, out_ld, out_col, emb, emb_row_offset, C, next_h);
  else {
    ua2_set_error("ua2_sample_topk_rows: bad dtype %d", dtype);
    return -1;
  }
  UA2_LAUNCH_CHECK();
  return 0;
}

// top_p of the nucleus entries: 0 and >= 1 are off, anything outside [0, 1] (NaN included) is refused; P = floor(top_p * 2^32)
static int topp_arguments(const char* who, int32_t V, float top_p, int* nucleus, unsigned long long* P) {
  UA2_CHECK(top_p >= 0.f && top_p <= 1.f, "%s: top_p must be in [0, 1] (0 and 1 = off), got %g", who, (double)top_p);
  UA2_CHECK(V <= (1 << 17), "%s: V = %d: the integer masses of the nucleus filter are sized for V <= 131072", who, V);
  *nucleus = (top_p > 0.f && top_p < 1.f) ? 1 : 0;
  *P = *nucleus ? (unsigned long long)((double)top_p * 4294967296.0) : 0ull;
  return 0;
}

extern "C" int ua2_sample_topp(int dtype, int32_t M, const float* logits, int32_t ld, int32_t V, int32_t topk, float temperature,
                               const int32_t* forbid, uint64_t seed, const int32_t* counter, int32_t stream_id, int32_t* out_tokens,
                               int32_t out_ld, int32_t out_col, const void* emb, int32_t emb_row_offset, int32_t C, float* next_h,
                               int32_t row_key_shift, float top_p, int32_t* keep_count, void* stream) {
  int nucleus = 0;
  unsigned long long P = 0ull;
  if (int rc = topp_arguments("ua2_sample_topp", V, top_p, &nucleus, &P)) return rc;
  if (!nucleus && !keep_count)                   // off and nothing to count: the top-k launch itself
    return ua2_sample_topk(dtype, M, logits, ld, V, topk, temperature, forbid, seed, counter, stream_id, out_tokens, out_ld, out_col, emb,
                           emb_row_offset, C, next_h, row_key_shift, stream);
  UA2_CHECK(M > 0 && logits && V > 0 && out_tokens && counter && row_key_shift >= 0 && row_key_shift <= 1, "ua2_sample_topp: bad arguments");
  UA2_CHECK(temperature > 0.f, "temperature must be > 0");
  UA2_CHECK(topk >= 1 && topk <= V, "topk must be in 1..%d", V);
  UA2_CHECK(!emb || next_h, "ua2_sample_topp: next_h is NULL");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == UA2_BF16)
    hipLaunchKernelGGL((sample_topp_kernel<UA2_BF16>), dim3(M), dim3(1024), 0, s, logits, ld, V, topk, temperature, forbid,
                       (unsigned long long)seed, counter, stream_id, out_tokens, out_ld, out_col, emb, emb_row_offset, C, next_h, row_key_shift,
                       nucleus, P, keep_count);
  else if (dtype == UA2_F32)
    hipLaunchKernelGGL((sample_topp_kernel<UA2_F32>), dim3(M), dim3(1024), 0, s, logits, ld, V, topk, temperature, forbid,
                       (unsigned long long)seed, counter, stream_id, out_tokens, out_ld, out_col, emb, emb_row_offset, C, next_h, row_key_shift,
                       nucleus, P, keep_count);
  else {
    ua2_set_error("ua2_sample_topp: bad dtype %d", dtype);
    return -1;
  }
  UA2_LAUNCH_CHECK();
  return 0;
}

extern "C" int ua2_sample_topp_rows(int dtype, int32_t M, const float* logits, int32_t ld, int32_t V, int32_t topk, float temperature,
                                    const int32_t* forbid, const int32_t* row_key, const int32_t* row_draw, int32_t stream_id,
                                    int32_t* out_tokens, int32_t out_ld, int32_t out_col, const void* emb, int32_t emb_row_offset,
                                    int32_t C, float* next_h, float top_p, int32_t* keep_count, void* stream) {
  int nucleus = 0;
  unsigned long long P = 0ull;
  if (int rc = topp_arguments("ua2_sample_topp_rows", V, top_p, &nucleus, &P)) return rc;
  if (!nucleus && !keep_count)
    return ua2_sample_topk_rows(dtype, M, logits, ld, V, topk, temperature, forbid, row_key, row_draw, stream_id, out_tokens, out_ld, out_col,
                                emb, emb_row_offset, C, next_h, stream);
  UA2_CHECK(M > 0 && logits && V > 0 && out_tokens && row_key && row_draw, "ua2_sample_topp_rows: bad arguments");
  UA2_CHECK(temperature > 0.f, "temperature must be > 0");
  UA2_CHECK(topk >= 1 && topk <= V, "topk must be in 1..%d", V);
  UA2_CHECK(!emb || next_h, "ua2_sample_topp_rows: next_h is NULL");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == UA2_BF16)
    hipLaunchKernelGGL((sample_topp_rows_kernel<UA2_BF16>), dim3(M), dim3(1024), 0, s, logits, ld, V, topk, temperature, forbid, row_key,
                       row_draw, stream_id, out_tokens, out_ld, out_col, emb, emb_row_offset, C, next_h, nucleus, P, keep_count);
  else if (dtype == UA2_F32)
    hipLaunchKernelGGL((sample_topp_rows_kernel<UA2_F32>), dim3(M), dim3(1024), 0, s, logits, ld, V, topk, temperature, forbid, row_key,
                       row_draw, stream_id, out_tokens, out_ld, out_col, emb, emb_row_offset, C, next_h, nucleus, P, keep_count);
  else {
    ua2_set_error("ua2_sample_topp_rows: bad dtype %d", dtype);
    return -1;
  }
  UA2_LAUNCH_CHECK();
  return 0;
}

template <int DT>
static void launch_penalized(const ua2_sample_args& a, bool topp, bool rows, int nucleus, unsigned long long P, const RepArgs& rep, hipStream_t s) {
#define UA2_PEN_LAUNCH(TOPP, ROWS)                                                                                                         \
  hipLaunchKernelGGL((sample_pen_kernel<DT, TOPP, ROWS>), dim3(a.M), dim3(1024), 0, s, a.logits, a.ld, a.V, a.topk, a.temperature, a.forbid, \
                     (unsigned long long)a.seed, a.counter, a.row_key_shift, a.row_key, a.row_draw, a.stream_id, a.out_tokens, a.out_ld,    \
                     a.out_col, a.emb, a.emb_row_offset, a.C, a.next_h, nucleus, P, a.keep_count, rep)
  if (topp && rows) UA2_PEN_LAUNCH(true, true);
  else if (topp) UA2_PEN_LAUNCH(true, false);
  else if (rows) UA2_PEN_LAUNCH(false, true);
  else UA2_PEN_LAUNCH(false, false);
#undef UA2_PEN_LAUNCH
}

extern "C" int ua2_sample_penalized(const ua2_sample_args* a, void* stream) {
  UA2_CHECK(a != nullptr, "ua2_sample_penalized: NULL arguments");
  const bool rows = a->row_key || a->row_draw;
  bool penal = false;
  if (a->rep_hist) {                             // every range is checked before any launch, the off value of theta included
    UA2_CHECK(a->rep_penalty > 0.f && a->rep_penalty < INFINITY, "ua2_sample_penalized: rep_penalty must be finite and > 0 (1 = off), got %g",
              (double)a->rep_penalty);
    UA2_CHECK(a->rep_window >= 1 && a->rep_window <= 512, "ua2_sample_penalized: rep_window must be in 1..512, got %d", a->rep_window);
    penal = a->rep_penalty != 1.f;
  }
  if (!penal) {                                  // off: the existing launch, and the history is left alone
    const bool topp = a->top_p != 0.f || a->keep_count;
    if (rows && topp)
      return ua2_sample_topp_rows(a->dtype, a->M, a->logits, a->ld, a->V, a->topk, a->temperature, a->forbid, a->row_key, a->row_draw, a->stream_id,
                                  a->out_tokens, a->out_ld, a->out_col, a->emb, a->emb_row_offset, a->C, a->next_h, a->top_p, a->keep_count, stream);
    if (rows)
      return ua2_sample_topk_rows(a->dtype, a->M, a->logits, a->ld, a->V, a->topk, a->temperature, a->forbid, a->row_key, a->row_draw, a->stream_id,
                                  a->out_tokens, a->out_ld, a->out_col, a->emb, a->emb_row_offset, a->C, a->next_h, stream);
    if (topp)
      return ua2_sample_topp(a->dtype, a->M, a->logits, a->ld, a->V, a->topk, a->temperature, a->forbid, a->seed, a->counter, a->stream_id,
                             a->out_tokens, a->out_ld, a->out_col, a->emb, a->emb_row_offset, a->C, a->next_h, a->row_key_shift, a->top_p,
                             a->keep_count, stream);
    return ua2_sample_topk(a->dtype, a->M, a->logits, a->ld, a->V, a->topk, a->temperature, a->forbid, a->seed, a->counter, a->stream_id,
                           a->out_tokens, a->out_ld, a->out_col, a->emb, a->emb_row_offset, a->C, a->next_h, a->row_key_shift, stream);
  }
  UA2_CHECK(a->V <= (1 << 17), "ua2_sample_penalized: V = %d: the membership set of the penalty is sized for V <= 131072", a->V);
  UA2_CHECK(a->rep_len && a->rep_cap >= a->rep_window && a->rep_hist_ld >= a->rep_cap && a->rep_len_ld >= 1,
            "ua2_sample_penalized: the history needs rep_len, rep_cap >= rep_window, rep_hist_ld >= rep_cap and rep_len_ld >= 1");
  int nucleus = 0;
  unsigned long long P = 0ull;
  if (int rc = topp_arguments("ua2_sample_penalized", a->V, a->top_p, &nucleus, &P)) return rc;
  UA2_CHECK(a->M > 0 && a->logits && a->V > 0 && a->out_tokens, "ua2_sample_penalized: bad arguments");
  UA2_CHECK(rows ? (a->row_key && a->row_draw) : (a->counter && a->row_key_shift >= 0 && a->row_key_shift <= 1),
            "ua2_sample_penalized: row_key and row_draw go together; the shared stream needs counter and row_key_shift in 0..1");
  UA2_CHECK(a->temperature > 0.f, "temperature must be > 0");
  UA2_CHECK(a->topk >= 1 && a->topk <= a->V, "topk must be in 1..%d", a->V);
  UA2_CHECK(!a->emb || a->next_h, "ua2_sample_penalized: next_h is NULL");
  const RepArgs rep{a->rep_penalty, a->rep_window, a->rep_cap, a->rep_hist, a->rep_hist_ld, a->rep_len, a->rep_len_ld};
  const bool topp = nucleus || a->keep_count;
  if (a->dtype == UA2_BF16) launch_penalized<UA2_BF16>(*a, topp, rows, nucleus, P, rep, (hipStream_t)stream);
  else if (a->dtype == UA2_F32) launch_penalized<UA2_F32>(*a, topp, rows, nucleus, P, rep, (hipStream_t)stream);
  else {
    ua2_set_error("ua2_sample_penalized: bad dtype %d", a->dtype);
    return -1;
  }
  UA2_LAUNCH_CHECK();
  return 0;
}

int ua2_row_draw_bump(int32_t* row_draw, int32_t R, hipStream_t stream) {
  UA2_CHECK(row_draw && R > 0, "ua2_row_draw_bump: bad arguments");
  hipLaunchKernelGGL(bump_rows_kernel, dim3(1), dim3(64), 0, stream, row_draw, R);
  UA2_LAUNCH_CHECK();
  return 0;
}

// ---- n-gram repeat filter of the text loop (evaluation/asr_task.py:329-432 generate_asr_with_ngram_sampling) ----------------
// Row r holds the generated text ids H = hist[r*cap .. r*cap + L), L = hist_len[r], and the frame's candidate c = out[r*ld].
// c is banned when (H[L-n+1 .. L) , c) already occurs as an n-gram of H (_should_reject_ngram :407-415 over the n-grams that
// _update_ngrams_simple :424-432 collects); a banned c becomes `fallback` (_get_fallback_token :417-421).  The final id is
// appended and hist_len becomes L + 1 (EOS included: the loops stop there and discard every later frame).  One workgroup per
// row; its threads test the start positions i in [0, L - n] in parallel.  Nothing is written at or past cap: a row with
// L >= cap keeps its stored history, and a row with L > cap (whose suffix is no longer stored) passes c through unfiltered —
// the host refuses to run a frame whose result it keeps into that state (Model_stage3.generate_frames).
__global__ __launch_bounds__(256) void ngram_filter_kernel(int32_t* __restrict__ out, int ld, int n, int fallback,
                                                           int32_t* __restrict__ hist, int32_t* __restrict__ hist_len, int cap) {
  const int r = blockIdx.x, tid = threadIdx.x;
  int32_t* h = hist + (size_t)r * cap;
  const int L = max(hist_len[r], 0);
  const int32_t c = out[(size_t)r * ld];
  int hit = 0;
  if (L <= cap && L >= n) {                      // L == n - 1: no n-gram in H yet, nothing to match
    const int32_t* suf = h + (L - n + 1);        // the last n - 1 ids
    for (int i = tid; i <= L - n; i += blockDim.x) {
      bool eq = h[i + n - 1] == c;
      for (int j = 0; eq && j < n - 1; ++j) eq = h[i + j] == suf[j];
      hit |= eq ? 1 : 0;
    }
  }
  hit = __syncthreads_or(hit);                   // every thread has read c and H before thread 0 writes
  if (tid == 0) {
    const int32_t id = hit ? fallback : c;
    out[(size_t)r * ld] = id;
    if (L < cap) h[L] = id;
    hist_len[r] = L + 1;
  }
}

extern "C" int ua2_ngram_filter(int32_t* out, int32_t ld, int32_t R, int32_t n, int32_t fallback, int32_t* hist,
                                int32_t* hist_len, int32_t cap, void* stream) {
  UA2_CHECK(out && hist && hist_len && R > 0 && ld >= 1 && cap >= 1, "ua2_ngram_filter: bad arguments");
  UA2_CHECK(n >= 2 && n <= 16, "ua2_ngram_filter: n must be in 2..16, got %d", n);
  hipLaunchKernelGGL(ngram_filter_kernel, dim3(R), dim3(256), 0, (hipStream_t)stream, out, ld, n, fallback, hist, hist_len, cap);
  UA2_LAUNCH_CHECK();
  return 0;
}
