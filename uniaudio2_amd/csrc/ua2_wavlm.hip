// WavLM encoder of the codec's tokenizer (include/ua2hip.h, "WavLM encoder"): the pieces that are WavLM's own —
//
//   ua2_wavlm_conv0      first feature-extractor layer: Conv1d(1 -> C, k, stride, no bias) + GroupNorm(groups = channels, i.e. a
//                        normalisation of every channel over time) + exact-erf GELU, written time-major [B, T0, C]
//   ua2_conv1d_grouped   the positional convolution: grouped Conv1d(C, C, K, padding K / 2, groups) (+ bias, GELU, residual), exact
//                        fp32 on v_mfma_f32_16x16x4_f32, time-major rows in and out
//   ua2_relpos_gate      the gate of the gated relative-position bias (gru_rel_pos_linear, gru_rel_pos_const)
//   ua2_attn_relbias     dense attention over the paged K/V with score = q k + gate[row, head] * rel_tab[head][key - query]
//
// Every load index is clamped into its buffer before the load and padding / masking is a select on the loaded value (the rule
// ua2_conv2d documents).  No atomics; nothing crosses the batch axis of a grid, so a clip has the same bits alone and in a batch.
#include "ua2_common.h"

namespace {

__device__ __forceinline__ float gelu_erf(float x) {
  return __fmul_rn(__fmul_rn(0.5f, x), __fadd_rn(1.0f, erff(__fmul_rn(x, 0.70710678118654752440f))));
}

// ---- ua2_wavlm_conv0 ------------------------------------------------------------------------------------------------------
// Three launches over fixed chunks of kC0Chunk output frames (a constant: the statistics do not depend on B or on the grid):
//   conv0_stats_kernel   per (clip, chunk, channel): sum and sum of squares of the chunk's conv values in double: four runs of 64
//                        frames, each accumulated in frame order by one thread, added in run order
//   conv0_merge_kernel   per (clip, channel): the chunks' partials added in chunk order in double -> mean, 1 / sqrt(var + eps)
//   conv0_apply_kernel   the conv values again (the same fma chain, taps ascending: the same bits), normalised, GELU, 16-byte stores
//                        along C
constexpr int kC0Chunk = 256;
constexpr int kC0MaxK = 16;

struct Conv0P {
  const float* x; const float* w; const float* gn_w; const float* gn_b; float* y; double* part; float* stat;
  long long N, T0;
  int B, C, K, stride, nch;
  float eps;
};

__device__ __forceinline__ float conv0_value(const float* wr, const float* xw, int K) {
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < kC0MaxK; ++k)
    if (k < K) acc = fmaf(wr[k], xw[k], acc);
  return acc;
}

// the samples of frames f0 .. f0 + nfr - 1: x[f0 * stride .. f0 * stride + (nfr - 1) * stride + K - 1]
__device__ __forceinline__ void conv0_stage(const Conv0P& a, int b, long long f0, int nfr, float* xw) {
  const int nx = (nfr - 1) * a.stride + a.K;
  const long long s0 = f0 * a.stride;
  for (int i = threadIdx.x; i < nx; i += blockDim.x) {
    const long long si = s0 + i;
    const long long sic = si < a.N ? si : a.N - 1;
    const float v = a.x[(size_t)b * a.N + sic];
    xw[i] = si < a.N ? v : 0.f;
  }
}

// workgroup = (chunk of 256 frames, 64 channels, clip); thread (channel, run r of 64 frames): the run's sums in frame order, the four
// runs added in run order — a function of the chunk alone
__global__ __launch_bounds__(256) void conv0_stats_kernel(const Conv0P a) {
  extern __shared__ __attribute__((aligned(16))) float xw[];
  __shared__ double red[4][64][2];
  const int chunk = blockIdx.x, b = blockIdx.z;
  const int cl = threadIdx.x & 63, run = threadIdx.x >> 6;
  const int c = blockIdx.y * 64 + cl, cc = min(c, a.C - 1);
  const long long f0 = (long long)chunk * kC0Chunk;
  const int nf = (int)min((long long)kC0Chunk, a.T0 - f0);
  conv0_stage(a, b, f0, kC0Chunk, xw);
  __syncthreads();
  float wr[kC0MaxK];
#pragma unroll
  for (int k = 0; k < kC0MaxK; ++k) wr[k] = a.w[(size_t)cc * a.K + min(k, a.K - 1)];
  double s = 0.0, ss = 0.0;
  const int fe = min(nf, run * 64 + 64);
  for (int f = run * 64; f < fe; ++f) {
    const float v = conv0_value(wr, xw + f * a.stride, a.K);
    s += (double)v;
    ss += (double)v * (double)v;
  }
  red[run][cl][0] = s;
  red[run][cl][1] = ss;
  __syncthreads();
  if (run == 0 && c < a.C) {
    double* p = a.part + (((size_t)b * a.nch + chunk) * a.C + c) * 2;
    p[0] = ((red[0][cl][0] + red[1][cl][0]) + red[2][cl][0]) + red[3][cl][0];
    p[1] = ((red[0][cl][1] + red[1][cl][1]) + red[2][cl][1]) + red[3][cl][1];
  }
}

__global__ __launch_bounds__(256) void conv0_merge_kernel(const Conv0P a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.B * a.C) return;
  const int b = i / a.C, c = i - b * a.C;
  double s = 0.0, ss = 0.0;
  for (int ch = 0; ch < a.nch; ++ch) {
    const double* p = a.part + (((size_t)b * a.nch + ch) * a.C + c) * 2;
    s += p[0];
    ss += p[1];
  }
  const double mean = s / (double)a.T0;
  double var = ss / (double)a.T0 - mean * mean;      // biased variance; one frame: exactly 0
  var = var > 0.0 ? var : 0.0;
  a.stat[(size_t)i * 2] = (float)mean;
  a.stat[(size_t)i * 2 + 1] = (float)(1.0 / sqrt(var + (double)a.eps));
}

// workgroup = (kC0Apply frames, clip): the filter and the four per-channel constants of the clip in LDS, 16-byte stores along C
constexpr int kC0Apply = 64;

__global__ __launch_bounds__(256) void conv0_apply_kernel(const Conv0P a) {
  extern __shared__ __attribute__((aligned(16))) float sm0[];
  const int nx = (kC0Apply - 1) * a.stride + a.K;
  float* xw = sm0;                       // [nx]
  float* ws = sm0 + ((nx + 3) & ~3);     // [C][K]
  float* cs = ws + a.C * a.K;            // [C][4]: mean, rstd, gn_w, gn_b
  const int b = blockIdx.y;
  const long long f0 = (long long)blockIdx.x * kC0Apply;
  const int nf = (int)min((long long)kC0Apply, a.T0 - f0);
  conv0_stage(a, b, f0, kC0Apply, xw);
  for (int i = threadIdx.x; i < a.C * a.K; i += blockDim.x) ws[i] = a.w[i];
  for (int c = threadIdx.x; c < a.C; c += blockDim.x) {
    cs[c * 4] = a.stat[((size_t)b * a.C + c) * 2];
    cs[c * 4 + 1] = a.stat[((size_t)b * a.C + c) * 2 + 1];
    cs[c * 4 + 2] = a.gn_w[c];
    cs[c * 4 + 3] = a.gn_b[c];
  }
  __syncthreads();
  const int c4n = a.C / 4;
  for (int idx = threadIdx.x; idx < nf * c4n; idx += blockDim.x) {
    const int f = idx / c4n, c = (idx - f * c4n) * 4;
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float wr[kC0MaxK];
#pragma unroll
      for (int k = 0; k < kC0MaxK; ++k) wr[k] = ws[(c + j) * a.K + min(k, a.K - 1)];
      const float v = conv0_value(wr, xw + f * a.stride, a.K);
      const float4 q = *reinterpret_cast<const float4*>(cs + (c + j) * 4);
      const float n = __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(v, q.x), q.y), q.z), q.w);
      o[j] = gelu_erf(n);
    }
    *reinterpret_cast<float4*>(a.y + ((size_t)b * a.T0 + f0 + f) * a.C + c) = make_float4(o[0], o[1], o[2], o[3]);
  }
}

// ---- ua2_conv1d_grouped -----------------------------------------------------------------------------------------------------
// Implicit GEMM on v_mfma_f32_16x16x4_f32.  Workgroup = 4 waves = one channel group's (up to kGRT) 16-row tiles x 128 output
// steps of one clip; wave w owns steps 32 w .. 32 w + 31 (two 16-step tiles) of every row tile, so a value read from LDS feeds
// kGRT MFMAs.  The group's input window (128 + K - 1 steps x C / groups channels) is staged once, channel-major with a pitch of
// 4 mod 16 floats (the four lane groups of a B-operand read fall on disjoint bank quarters).  Reduction index = (tap, channel in
// the group): one packed chunk of 16 is one tap over 16 channels, chunks ascending — a function of (C, groups, K) only.
constexpr int kGRT = 3, kGNT = 2;
constexpr int kGBT = 4 * 16 * kGNT;      // output steps per workgroup

struct GConvP {
  const float* x; const u32x4* w; const float* bias; const float* resid; float* y;
  int B, T, C, Cg, K, pad, act, Wp, ntg, rb;
};

__global__ __launch_bounds__(256) void gconv_kernel(const GConvP a) {
  extern __shared__ __attribute__((aligned(16))) float xs[];   // [Cg][Wp]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tl = lane & 15, g = lane >> 4;
  const int t0 = blockIdx.x * kGBT;
  const int gr = blockIdx.y / a.rb, rblk = blockIdx.y - gr * a.rb;
  const int b = blockIdx.z;
  const int W = kGBT + a.K - 1;
  for (int idx = tid; idx < W * a.Cg; idx += 256) {
    const int wi = idx / a.Cg, ci = idx - wi * a.Cg;
    const int ti = t0 - a.pad + wi;
    const int tic = min(max(ti, 0), a.T - 1);                   // never load through unclamped arithmetic
    const float v = a.x[((size_t)b * a.T + tic) * a.C + gr * a.Cg + ci];
    xs[ci * a.Wp + wi] = (ti >= 0 && ti < a.T) ? v : 0.f;
  }
  __syncthreads();
  const int cpk = a.Cg / 16;                // chunks per tap
  const int nchunks = a.K * cpk;
  const u32x4* wp[kGRT];
  bool live[kGRT];
#pragma unroll
  for (int q = 0; q < kGRT; ++q) {
    const int tq = rblk * kGRT + q;
    live[q] = tq < a.ntg;                   // wave-uniform
    wp[q] = a.w + (size_t)(gr * a.ntg + min(tq, a.ntg - 1)) * nchunks * 64 + lane;
  }
  f32x4 acc[kGRT][kGNT];
#pragma unroll
  for (int q = 0; q < kGRT; ++q)
#pragma unroll
    for (int nt = 0; nt < kGNT; ++nt) acc[q][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  u32x4 wn[kGRT];
#pragma unroll
  for (int q = 0; q < kGRT; ++q) wn[q] = wp[q][0];
  int k = 0, cb = 0;
  for (int c = 0; c < nchunks; ++c) {
    f32x4 wa[kGRT];
#pragma unroll
    for (int q = 0; q < kGRT; ++q) wa[q] = __builtin_bit_cast(f32x4, wn[q]);
    if (c + 1 < nchunks) {                  // one chunk ahead
#pragma unroll
      for (int q = 0; q < kGRT; ++q) wn[q] = wp[q][(size_t)(c + 1) * 64];
    }
    const int base = (cb * 16 + g * 4) * a.Wp + k + wave * (16 * kGNT) + tl;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma unroll
      for (int nt = 0; nt < kGNT; ++nt) {
        const float xv = xs[base + e * a.Wp + nt * 16];
#pragma unroll
        for (int q = 0; q < kGRT; ++q)
          if (live[q]) acc[q][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[q][e], xv, acc[q][nt], 0, 0, 0);
      }
    }
    if (++cb == cpk) { cb = 0; ++k; }
  }
  // epilogue: D[row = (lane >> 4) * 4 + r][col = lane & 15]: four consecutive channels per lane
#pragma unroll
  for (int q = 0; q < kGRT; ++q) {
    if (!live[q]) continue;
    const int co = (gr * a.ntg + rblk * kGRT + q) * 16 + g * 4;
    float4 bias = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.bias) bias = *reinterpret_cast<const float4*>(a.bias + co);
#pragma unroll
    for (int nt = 0; nt < kGNT; ++nt) {
      const int t = t0 + wave * (16 * kGNT) + nt * 16 + tl;
      if (t >= a.T) continue;
      const size_t o = ((size_t)b * a.T + t) * a.C + co;
      float v[4] = {__fadd_rn(acc[q][nt][0], bias.x), __fadd_rn(acc[q][nt][1], bias.y), __fadd_rn(acc[q][nt][2], bias.z),
                    __fadd_rn(acc[q][nt][3], bias.w)};
      if (a.act) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = gelu_erf(v[r]);
      }
      if (a.resid) {
        const float4 rr = *reinterpret_cast<const float4*>(a.resid + o);
        v[0] = __fadd_rn(rr.x, v[0]); v[1] = __fadd_rn(rr.y, v[1]); v[2] = __fadd_rn(rr.z, v[2]); v[3] = __fadd_rn(rr.w, v[3]);
      }
      *reinterpret_cast<float4*>(a.y + o) = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
}

// ---- ua2_relpos_gate --------------------------------------------------------------------------------------------------------
constexpr int kGateMaxHS = 128;

__global__ __launch_bounds__(256) void relpos_gate_kernel(float* g, const float* h, const float* w, const float* bv, const float* cv,
                                                          long long R, int H, int hs) {
  __shared__ float ws[8 * kGateMaxHS];
  for (int i = threadIdx.x; i < 8 * hs; i += 256) ws[i] = w[i];
  __syncthreads();
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= R * H) return;
  const int head = (int)(i % H);
  const float* hp = h + (size_t)i * hs;               // row r, head: (r * H + head) * hs
  float p[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) p[j] = 0.f;
  for (int d = 0; d < hs; d += 4) {                   // one fma chain per projection, dims ascending
    const float4 v = *reinterpret_cast<const float4*>(hp + d);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      p[j] = fmaf(ws[j * hs + d], v.x, p[j]);
      p[j] = fmaf(ws[j * hs + d + 1], v.y, p[j]);
      p[j] = fmaf(ws[j * hs + d + 2], v.z, p[j]);
      p[j] = fmaf(ws[j * hs + d + 3], v.w, p[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) p[j] = __fadd_rn(p[j], bv[j]);
  const float sa = __fadd_rn(__fadd_rn(__fadd_rn(p[0], p[1]), p[2]), p[3]);
  const float sb = __fadd_rn(__fadd_rn(__fadd_rn(p[4], p[5]), p[6]), p[7]);
  const float ga = 1.0f / (1.0f + expf(-sa)), gb = 1.0f / (1.0f + expf(-sb));
  g[i] = __fadd_rn(__fmul_rn(ga, __fsub_rn(__fmul_rn(gb, cv[head]), 1.0f)), 2.0f);
}

// ---- ua2_attn_relbias, fp32 parity form --------------------------------------------------------------------------------------
// The row-by-row kernel of ua2_attn (ua2_attn.hip attn_fused_kernel, fp32, one query head per kv head) restated with the bias term:
// the same split of the keys over 8 waves, the same 16-lane DPP sums, the same merge order — with an all-zero table the result has
// the bits of ua2_attn on q * sqrt(head_size).  q arrives pre-scaled.
constexpr int kRbWaves = 8;

template <int CTRL>
__device__ __forceinline__ float rb_dpp_add(float v) {
  return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
template <int LPR>
__device__ __forceinline__ float rb_group_sum(float v) {
  v = rb_dpp_add<0xB1>(v);
  v = rb_dpp_add<0x4E>(v);
  if constexpr (LPR >= 8) v = rb_dpp_add<0x141>(v);
  if constexpr (LPR >= 16) v = rb_dpp_add<0x140>(v);
  if constexpr (LPR >= 32) v += __shfl_xor(v, 16);
  return v;
}
__device__ __forceinline__ float rb_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }

struct RelBias {
  const int32_t* q_pos; const float* gate; const float* tab; int half;
};

template <int HS>
__global__ __launch_bounds__(kRbWaves * 64, 2) void attn_relbias_rows_kernel(const ua2_attn_args a, const RelBias rb) {
  constexpr int EPL = 4, BYTES = 4;
  constexpr int LPR = HS / EPL, RPW = 64 / LPR;
  constexpr int UNR = 2;
  constexpr int NS = kRbWaves * RPW;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int r = blockIdx.x, kvh = blockIdx.y;
  float* st_m = sm;                    // [NS]
  float* st_l = st_m + NS;             // [NS]
  float* st_o = st_l + NS;             // [NS][HS]
  const int pos = a.row_pos[r];
  const int seq = a.row_seq ? a.row_seq[r] : r;
  const int n = pos + 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sub = lane % LPR, rin = lane / LPR;
  const int32_t* ptab = a.kv.page_table + (size_t)seq * a.kv.max_pages;
  const int chunk = ((n + kRbWaves * RPW - 1) / (kRbWaves * RPW)) * RPW;
  const int j0 = wave * chunk, j1 = min(n, j0 + chunk);
  const float gate = rb.gate[(size_t)r * a.kv.n_head + kvh];
  const int qp = rb.q_pos[r];
  const float* trow = rb.tab + (size_t)kvh * (2 * rb.half + 1);

  float q[EPL];
  {
    const float4 t = *reinterpret_cast<const float4*>(a.q + ((size_t)r * a.kv.n_head + kvh) * HS + sub * EPL);
    q[0] = t.x; q[1] = t.y; q[2] = t.z; q[3] = t.w;
  }
  float m_run = -INFINITY, l_run = 0.f, o_run[EPL];
#pragma unroll
  for (int e = 0; e < EPL; ++e) o_run[e] = 0.f;

  for (int jb = j0; jb < j1; jb += UNR * RPW) {
    u32x4 kraw[UNR], vraw[UNR];
    float bias[UNR];
    bool ok[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int j = jb + u * RPW + rin;
      ok[u] = j < j1;
      const int jc = ok[u] ? j : j0;              // clamp: unconditional loads, masked in the math
      const size_t off = ((((size_t)ptab[ua2_page_slot(a.kv, jc)] * a.kv.n_kv + kvh) * UA2_PAGE + (jc % UA2_PAGE)) * HS +
                          (size_t)sub * EPL) * BYTES;
      kraw[u] = *reinterpret_cast<const u32x4*>((const char*)a.kv.k_pool + off);
      vraw[u] = *reinterpret_cast<const u32x4*>((const char*)a.kv.v_pool + off);
      bias[u] = trow[min(max(jc - qp + rb.half, 0), 2 * rb.half)];
    }
    float s[UNR];
    float gmax = -INFINITY;
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      float d = 0.f;
#pragma unroll
      for (int e = 0; e < EPL; ++e) d += q[e] * __uint_as_float(kraw[u][e]);
      d = rb_group_sum<LPR>(d);
      d = d + gate * bias[u];
      s[u] = ok[u] ? d : -INFINITY;
      gmax = fmaxf(gmax, s[u]);
    }
    {
      const float m_new = fmaxf(m_run, gmax);
      const float resc = (m_new == -INFINITY) ? 1.f : rb_exp(m_run - m_new);
      m_run = m_new;
      l_run *= resc;
#pragma unroll
      for (int e = 0; e < EPL; ++e) o_run[e] *= resc;
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const float p = ok[u] ? rb_exp(s[u] - m_run) : 0.f;
      l_run += p;
#pragma unroll
      for (int e = 0; e < EPL; ++e) o_run[e] += p * __uint_as_float(vraw[u][e]);
    }
  }
  const int sidx = wave * RPW + rin;
  if (sub == 0) { st_m[sidx] = m_run; st_l[sidx] = l_run; }
  *reinterpret_cast<float4*>(st_o + (size_t)sidx * HS + sub * EPL) = make_float4(o_run[0], o_run[1], o_run[2], o_run[3]);
  __syncthreads();
  float* wgt = st_l;
  if (wave == 0) {
    const float mw = (lane < NS) ? st_m[lane] : -INFINITY;
    const float lw = (lane < NS) ? st_l[lane] : 0.f;
    float mx = mw;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    const float f = (mw == -INFINITY) ? 0.f : rb_exp(mw - mx);
    float den = f * lw;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) den += __shfl_xor(den, o);
    const float inv = 1.0f / den;
    if (lane < NS) wgt[lane] = f * inv;
  }
  __syncthreads();
  for (int d = tid; d < HS; d += kRbWaves * 64) {
    float acc = 0.f;
#pragma unroll 8
    for (int w = 0; w < NS; ++w) acc += wgt[w] * st_o[(size_t)w * HS + d];
    if (a.y) a.y[((size_t)r * a.kv.n_head + kvh) * HS + d] = acc;
    if (a.y_packed) store_packed_operand<UA2_F32>(a.y_packed, r, kvh * HS + d, a.kv.n_head * HS / Elem<UA2_F32>::KC, acc);
  }
}

// ---- ua2_attn_relbias, bf16 MFMA flash form ------------------------------------------------------------------------------------
// The grouped kernel of ua2_attn (ua2_attn.hip attn_flash_kernel, one query head per kv head, hi / lo split q and p, one 64-key page
// per step, pages in page order) with the head's table row staged in LDS once per workgroup and gate * table added to the fp32 score
// tile before the running maximum.  Scores live in the log2 domain there (q carries log2 e), so the gate carries it too.
template <int HS, int QT>
__global__ __launch_bounds__(64 * QT) void attn_relbias_flash_kernel(const ua2_attn_args a, const RelBias rb) {
  constexpr int NW = QT;
  constexpr int KPI = UA2_PAGE;
  constexpr int DC = HS / 32;
  constexpr int DTL = HS / 16;
  constexpr int KROW = HS * 2 + 16;
  constexpr int VROW = HS * 2 + 32;
  extern __shared__ __attribute__((aligned(16))) char smf[];
  constexpr int IMG = KPI * (KROW + VROW);
  float* tab_s = reinterpret_cast<float*>(smf + 2 * IMG);      // [2 half + 1]
  const int grp = blockIdx.x, head = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qt = wave;
  const int ql = lane & 15, g = lane >> 4;
  const int row = a.group_rows[(size_t)grp * (QT * 16) + qt * 16 + ql];
  const int seq = a.group_seq[grp];
  const int nkeys = a.group_nkeys[grp];
  const int rowc = max(row, 0);
  const int qpos = row >= 0 ? a.row_pos[rowc] : -1;
  const int qp = rb.q_pos[rowc];
  const float gate = row >= 0 ? __fmul_rn(rb.gate[(size_t)rowc * a.kv.n_head + head], 1.44269504088896340736f) : 0.f;
  const int32_t* ptab = a.kv.page_table + (size_t)seq * a.kv.max_pages;
  const int ntab = 2 * rb.half + 1;
  for (int i = tid; i < ntab; i += 64 * NW) tab_s[i] = rb.tab[(size_t)head * ntab + i];

  u32x4 qh[DC], qlo[DC];
  {
    const float sc = 1.44269504088896340736f;                 // q arrives scaled by head_size^-0.5
#pragma unroll
    for (int dc = 0; dc < DC; ++dc) {
      float f[8];
      if (row >= 0) {
        const float* qptr = a.q + ((size_t)row * a.kv.n_head + head) * HS + dc * 32 + g * 8;
        const float4 t0 = *reinterpret_cast<const float4*>(qptr), t1 = *reinterpret_cast<const float4*>(qptr + 4);
        f[0] = t0.x; f[1] = t0.y; f[2] = t0.z; f[3] = t0.w; f[4] = t1.x; f[5] = t1.y; f[6] = t1.z; f[7] = t1.w;
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = 0.f;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        unsigned hi, lo;
        split_pair(__fmul_rn(f[2 * e], sc), __fmul_rn(f[2 * e + 1], sc), hi, lo);
        qh[dc][e] = hi;
        qlo[dc][e] = lo;
      }
    }
  }
  float m_run = -INFINITY, l_run = 0.f;
  f32x4 o[DTL];
#pragma unroll
  for (int dt = 0; dt < DTL; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nkb = (nkeys + UA2_PAGE - 1) / UA2_PAGE;
  constexpr int PPP = UA2_PAGE * HS / 8;
  constexpr int NP = (PPP + 64 * NW - 1) / (64 * NW);
  u32x4 kk[NP], vv[NP];
  auto request = [&](int kb) {
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      const int i = tid + u * 64 * NW;
      if (i < PPP) {
        const int pg = min(kb, nkb - 1);
        const size_t base = (((size_t)ptab[ua2_page_slot(a.kv, pg * UA2_PAGE)] * a.kv.n_kv + head) * UA2_PAGE) * HS;
        kk[u] = reinterpret_cast<const u32x4*>(reinterpret_cast<const unsigned short*>(a.kv.k_pool) + base)[i];
        vv[u] = reinterpret_cast<const u32x4*>(reinterpret_cast<const unsigned short*>(a.kv.v_pool) + base)[i];
      }
    }
  };
  if (nkb > 0) request(0);
  for (int kb = 0; kb < nkb; ++kb) {
    char* k_lds = smf + (kb & 1) * IMG;
    char* v_lds = k_lds + KPI * KROW;
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      const int i = tid + u * 64 * NW;
      if (i < PPP) {
        const int key = i / (HS / 8), oct = i % (HS / 8);
        *reinterpret_cast<u32x4*>(k_lds + key * KROW + oct * 16) = kk[u];
        *reinterpret_cast<u32x4*>(v_lds + key * VROW + oct * 16) = vv[u];
      }
    }
    __syncthreads();                          // also publishes the table row (first pass)
    if (kb + 1 < nkb) request(kb + 1);
    f32x4 st[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      st[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int dc = 0; dc < DC; ++dc) {
        const bf16x8 kf = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(k_lds + (kt * 16 + ql) * KROW + dc * 64 + g * 16));
        st[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, __builtin_bit_cast(bf16x8, qlo[dc]), st[kt], 0, 0, 0);
        st[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, __builtin_bit_cast(bf16x8, qh[dc]), st[kt], 0, 0, 0);
      }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kpos = kb * KPI + kt * 16 + 4 * g + r;
        const float bias = tab_s[min(max(kpos - qp + rb.half, 0), 2 * rb.half)];
        const float sv = __fadd_rn(st[kt][r], __fmul_rn(gate, bias));
        st[kt][r] = (kpos > qpos) ? -INFINITY : sv;           // mask by select: stale cache slots never leak
        mx = fmaxf(mx, st[kt][r]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m_run, mx);
    const float alpha = (m_new == -INFINITY) ? 1.f : __builtin_amdgcn_exp2f(m_run - m_new);
    float ps = 0.f;
    u32x4 ph[2], pl[2];
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
      float pv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float sv = st[2 * kc + (e >> 2)][e & 3];
        pv[e] = (sv == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(sv - m_new);
        ps += pv[e];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        unsigned hi, lo;
        split_pair(pv[2 * e], pv[2 * e + 1], hi, lo);
        ph[kc][e] = hi;
        pl[kc][e] = lo;
      }
    }
    ps += __shfl_xor(ps, 16);
    ps += __shfl_xor(ps, 32);
    l_run = l_run * alpha + ps;
    m_run = m_new;
#pragma unroll
    for (int dt = 0; dt < DTL; ++dt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) o[dt][r] *= alpha;
    }
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
#pragma unroll
      for (int dt = 0; dt < DTL; ++dt) {
        typedef short tr4 __attribute__((ext_vector_type(4)));
        typedef __attribute__((address_space(3))) tr4* lds_tr4;
        const char* vr = v_lds + (size_t)(kc * 32 + 4 * g + (ql >> 2)) * VROW + (dt * 16 + 4 * (ql & 3)) * 2;
        const tr4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr4)vr);
        const tr4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr4)(vr + 16 * VROW));
        const uint2 v0 = __builtin_bit_cast(uint2, t0), v1 = __builtin_bit_cast(uint2, t1);
        const bf16x8 vf = __builtin_bit_cast(bf16x8, u32x4{v0.x, v0.y, v1.x, v1.y});
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, __builtin_bit_cast(bf16x8, pl[kc]), o[dt], 0, 0, 0);
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, __builtin_bit_cast(bf16x8, ph[kc]), o[dt], 0, 0, 0);
      }
    }
  }
  if (row < 0 || l_run == 0.f) return;
  const float inv = 1.0f / l_run;
#pragma unroll
  for (int dt = 0; dt < DTL; ++dt) {
    const int d0 = dt * 16 + 4 * g;
    const float4 out = make_float4(o[dt][0] * inv, o[dt][1] * inv, o[dt][2] * inv, o[dt][3] * inv);
    if (a.y) *reinterpret_cast<float4*>(a.y + ((size_t)row * a.kv.n_head + head) * HS + d0) = out;
    if (a.y_packed) {
      const int nch = a.kv.n_head * HS / Elem<UA2_BF16>::KC;
      store_packed_operand<UA2_BF16>(a.y_packed, row, head * HS + d0, nch, out.x);
      store_packed_operand<UA2_BF16>(a.y_packed, row, head * HS + d0 + 1, nch, out.y);
      store_packed_operand<UA2_BF16>(a.y_packed, row, head * HS + d0 + 2, nch, out.z);
      store_packed_operand<UA2_BF16>(a.y_packed, row, head * HS + d0 + 3, nch, out.w);
    }
  }
}

template <int HS>
void launch_relbias_rows(const ua2_attn_args& a, const RelBias& rb, hipStream_t s) {
  constexpr int NS = kRbWaves * (64 / (HS / 4));
  const size_t smem = (size_t)(2 * NS + NS * HS) * sizeof(float);
  hipLaunchKernelGGL(attn_relbias_rows_kernel<HS>, dim3(a.R, a.kv.n_head), dim3(kRbWaves * 64), smem, s, a, rb);
}

template <int HS, int QT>
void launch_relbias_flash(const ua2_attn_args& a, const RelBias& rb, hipStream_t s) {
  constexpr auto kern = attn_relbias_flash_kernel<HS, QT>;
  ua2_allow_big_lds<kern>();
  const size_t smem = 2 * ((size_t)UA2_PAGE * (HS * 2 + 16) + (size_t)UA2_PAGE * (HS * 2 + 32)) + (size_t)(2 * rb.half + 1) * sizeof(float);
  hipLaunchKernelGGL(kern, dim3(a.n_groups, a.kv.n_head), dim3(64 * QT), smem, s, a, rb);
}

}  // namespace

extern "C" size_t ua2_wavlm_conv0_workspace_bytes(int32_t B, int64_t N, int32_t C, int32_t K, int32_t stride) {
  if (B <= 0 || C <= 0 || K <= 0 || stride <= 0 || N < K) return 0;
  const int64_t T0 = (N - K) / stride + 1;
  const int64_t nch = (T0 + kC0Chunk - 1) / kC0Chunk;
  return (size_t)B * nch * C * 2 * sizeof(double) + (size_t)B * C * 2 * sizeof(float);
}

extern "C" int ua2_wavlm_conv0(float* y, const float* x, const float* w, const float* gn_w, const float* gn_b, int32_t B, int64_t N,
                               int32_t C, int32_t K, int32_t stride, float eps, void* ws, size_t ws_bytes, void* stream) {
  UA2_CHECK(y && x && w && gn_w && gn_b && ws, "ua2_wavlm_conv0: NULL argument");
  UA2_CHECK(B > 0 && B <= 65535 && C > 0 && C % 4 == 0 && K > 0 && K <= kC0MaxK && stride > 0 && stride <= 32 && N >= K,
            "ua2_wavlm_conv0: B=%d (1..65535) N=%lld C=%d (a multiple of 4) K=%d (1..%d, <= N) stride=%d (1..32)", B, (long long)N, C, K,
            kC0MaxK, stride);
  UA2_CHECK(((uintptr_t)ws & 7) == 0, "ua2_wavlm_conv0: the workspace must be 8-byte aligned");
  const size_t need = ua2_wavlm_conv0_workspace_bytes(B, N, C, K, stride);
  UA2_CHECK(ws_bytes >= need, "ua2_wavlm_conv0: workspace of %zu bytes, %zu needed", ws_bytes, need);
  Conv0P a;
  a.x = x; a.w = w; a.gn_w = gn_w; a.gn_b = gn_b; a.y = y;
  a.N = N; a.T0 = (N - K) / stride + 1;
  a.B = B; a.C = C; a.K = K; a.stride = stride; a.eps = eps;
  const int64_t nch = (a.T0 + kC0Chunk - 1) / kC0Chunk;
  UA2_CHECK(nch < (1ll << 31), "ua2_wavlm_conv0: %lld frames exceed the grid", (long long)a.T0);
  a.nch = (int)nch;
  a.part = reinterpret_cast<double*>(ws);
  a.stat = reinterpret_cast<float*>(a.part + (size_t)B * nch * C * 2);
  const int nx = (kC0Chunk - 1) * stride + K, nxa = (kC0Apply - 1) * stride + K;
  const size_t smem_apply = ((size_t)((nxa + 3) & ~3) + (size_t)C * K + (size_t)C * 4) * sizeof(float);
  UA2_CHECK(smem_apply <= 64 * 1024, "ua2_wavlm_conv0: C * K = %d does not fit the filter's LDS image", C * K);
  UA2_CHECK((C + 63) / 64 <= 65535 && (a.T0 + kC0Apply - 1) / kC0Apply < (1ll << 31), "ua2_wavlm_conv0: C=%d or %lld frames exceed the grid", C, (long long)a.T0);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(conv0_stats_kernel, dim3(a.nch, (C + 63) / 64, B), dim3(256), (size_t)nx * sizeof(float), s, a);
  hipLaunchKernelGGL(conv0_merge_kernel, dim3((B * C + 255) / 256), dim3(256), 0, s, a);
  hipLaunchKernelGGL(conv0_apply_kernel, dim3((unsigned)((a.T0 + kC0Apply - 1) / kC0Apply), B), dim3(256), smem_apply, s, a);
  UA2_LAUNCH_CHECK();
  return 0;
}

extern "C" int ua2_conv1d_grouped(float* y, const float* x, const void* w, const float* bias, const float* resid, int32_t B, int32_t T,
                                  int32_t C, int32_t groups, int32_t K, int32_t act, void* stream) {
  UA2_CHECK(y && x && w, "ua2_conv1d_grouped: NULL argument");
  UA2_CHECK(B > 0 && B <= 65535 && T > 0 && C > 0 && K > 0 && K <= 4096, "ua2_conv1d_grouped: B=%d (1..65535) T=%d C=%d K=%d", B, T, C, K);
  UA2_CHECK(groups > 0 && C % groups == 0 && (C / groups) % 16 == 0,
            "ua2_conv1d_grouped: C=%d groups=%d: the channels per group (C / groups) must be a multiple of 16", C, groups);
  UA2_CHECK(act == 0 || act == 1, "ua2_conv1d_grouped: act=%d (0 none, 1 erf-GELU)", act);
  UA2_CHECK((int64_t)T * C < (1ll << 31), "ua2_conv1d_grouped: a clip's tensor exceeds 2^31 elements");
  GConvP a;
  a.x = x; a.w = reinterpret_cast<const u32x4*>(w); a.bias = bias; a.resid = resid; a.y = y;
  a.B = B; a.T = T; a.C = C; a.Cg = C / groups; a.K = K; a.pad = K / 2; a.act = act;
  const int W = kGBT + K - 1;
  a.Wp = (W + 11) / 16 * 16 + 4;
  a.ntg = a.Cg / 16;
  a.rb = (a.ntg + kGRT - 1) / kGRT;
  const size_t smem = (size_t)a.Cg * a.Wp * sizeof(float);
  UA2_CHECK(smem <= 64 * 1024, "ua2_conv1d_grouped: the window of %d channels x %d steps does not fit LDS (64 KiB)", a.Cg, W);
  UA2_CHECK((int64_t)groups * a.rb <= 65535, "ua2_conv1d_grouped: groups=%d exceeds the grid", groups);
  hipLaunchKernelGGL(gconv_kernel, dim3((T + kGBT - 1) / kGBT, groups * a.rb, B), dim3(256), smem, (hipStream_t)stream, a);
  UA2_LAUNCH_CHECK();
  return 0;
}

extern "C" int ua2_relpos_gate(float* g, const float* h, const float* w, const float* b, const float* c, int64_t R, int32_t n_head,
                               int32_t head_size, void* stream) {
  UA2_CHECK(g && h && w && b && c, "ua2_relpos_gate: NULL argument");
  UA2_CHECK(R > 0 && n_head > 0 && head_size > 0 && head_size % 4 == 0 && head_size <= kGateMaxHS && R * n_head < (1ll << 31),
            "ua2_relpos_gate: R=%lld n_head=%d head_size=%d (a multiple of 4, <= %d)", (long long)R, n_head, head_size, kGateMaxHS);
  hipLaunchKernelGGL(relpos_gate_kernel, dim3((unsigned)((R * n_head + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, h, w, b, c,
                     (long long)R, n_head, head_size);
  UA2_LAUNCH_CHECK();
  return 0;
}

extern "C" int ua2_attn_relbias(const ua2_attn_args* ap, const int32_t* q_pos, const float* gate, const float* rel_tab, int32_t tab_half,
                                void* stream) {
  UA2_CHECK(ap != nullptr, "ua2_attn_relbias: NULL args");
  const ua2_attn_args& a = *ap;
  UA2_CHECK(a.R > 0, "ua2_attn_relbias: R=%d", a.R);
  UA2_CHECK(a.q && a.row_pos && (a.y || a.y_packed) && a.kv.k_pool && a.kv.v_pool && a.kv.page_table && q_pos && gate && rel_tab,
            "ua2_attn_relbias: NULL pointer argument");
  UA2_CHECK(!a.y_h, "ua2_attn_relbias: y_h is an output of ua2_attn's row-by-row form");
  UA2_CHECK(a.kv.n_kv > 0 && a.kv.n_head == a.kv.n_kv, "ua2_attn_relbias: n_head=%d n_kv=%d (multi-head only)", a.kv.n_head, a.kv.n_kv);
  UA2_CHECK(a.kv.n_head <= 65535, "ua2_attn_relbias: n_head=%d exceeds the grid", a.kv.n_head);
  UA2_CHECK(a.kv.ring_pages == 0 && a.window <= 0, "ua2_attn_relbias: ring caches and windows are not served");
  UA2_CHECK(tab_half >= 0 && tab_half < (1 << 20), "ua2_attn_relbias: tab_half=%d", tab_half);
  UA2_CHECK(a.kv.head_size == 64 || a.kv.head_size == 128, "ua2_attn_relbias: head_size %d not supported (64, 128)", a.kv.head_size);
  UA2_CHECK(!a.y_packed || (a.kv.n_head * a.kv.head_size) % (a.dtype == UA2_BF16 ? 32 : 16) == 0,
            "ua2_attn_relbias: y_packed needs n_head*head_size %% chunk == 0");
  const RelBias rb{q_pos, gate, rel_tab, tab_half};
  hipStream_t s = (hipStream_t)stream;
  const int hs = a.kv.head_size;
  if (a.dtype == UA2_BF16) {
    UA2_CHECK(a.group_rows && a.n_groups > 0 && a.group_seq && a.group_nkeys,
              "ua2_attn_relbias: the bf16 form needs row groups (group_rows / group_seq / group_nkeys)");
    UA2_CHECK((size_t)(2 * tab_half + 1) * sizeof(float) <= 64 * 1024, "ua2_attn_relbias: a table row of %d entries does not fit LDS", 2 * tab_half + 1);
    const int qt = a.group_q_tiles;
    if (hs == 64 && qt == 4) launch_relbias_flash<64, 4>(a, rb, s);
    else if (hs == 64 && qt == 8) launch_relbias_flash<64, 8>(a, rb, s);
    else if (hs == 128 && qt == 4) launch_relbias_flash<128, 4>(a, rb, s);
    else {
      ua2_set_error("ua2_attn_relbias: no grouped kernel for head_size %d, q tiles %d (64: 4 or 8, 128: 4)", hs, qt);
      return -1;
    }
  } else if (a.dtype == UA2_F32) {
    if (hs == 64) launch_relbias_rows<64>(a, rb, s);
    else launch_relbias_rows<128>(a, rb, s);
  } else {
    ua2_set_error("ua2_attn_relbias: bad dtype %d", a.dtype);
    return -1;
  }
  UA2_LAUNCH_CHECK();
  return 0;
}
