// Row-wise glue of the BEST-RQ (MusicFM 25 Hz) encoder (include/ua2hip.h): the conformer's LayerNorm + rotary step and the tail
// of its mel front end.
//
//   layernorm_rope_kernel   transformers' Wav2Vec2ConformerSelfAttention rotates the LayerNorm-ed hidden states BEFORE linear_q /
//                           linear_k (rotate-half over each head's head_size, cos / sin of cat(freqs, freqs)) while linear_v reads
//                           the un-rotated rows — UA2_EPI_QKV_ROPE rotates after the projection and cannot express it.  One
//                           workgroup per row writes out[r] = [ rotate(LN(x[r])) | LN(x[r]) ] (width 2 C): the operand of ONE
//                           ua2_linear launch with the block weight [[Wq, 0], [Wk, 0], [0, Wv]].  The LayerNorm is
//                           layernorm_rows_kernel's (ua2_codec.hip), sum for sum; the rotation is x cos + rotate_half(x) sin with
//                           two roundings of the products and one of the sum, as torch evaluates it.
//   melspec_db_kernel       per frame: power of the 1025 DFT bins (the real | imaginary halves of a ua2_linear product against the
//                           windowed basis), the 1025 x n_mels HTK filter bank as two chains per mel (bins below / from 512, low
//                           half first), 10 log10(max(., 1e-10)) and (x - mean) / std, written as [B, n_mels, T].
#include "ua2_common.h"

namespace {

__global__ __launch_bounds__(256) void layernorm_rope_kernel(float* __restrict__ out, const float* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ b, const float* __restrict__ cos_t,
                                                             const float* __restrict__ sin_t, const int32_t* __restrict__ row_pos, int n_pos,
                                                             int C, int hs, float eps) {
  extern __shared__ float ln[];                        // [C]
  __shared__ float red[4];
  const int64_t r = blockIdx.x;
  const float* xr = x + (size_t)r * C;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float s = 0.f;
  for (int c = tid; c < C; c += 256) s += xr[c];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  const float mean = (((red[0] + red[1]) + red[2]) + red[3]) / (float)C;
  __syncthreads();
  float q = 0.f;
  for (int c = tid; c < C; c += 256) { const float d = xr[c] - mean; q += d * d; }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) q += __shfl_xor(q, o);
  if (lane == 0) red[wave] = q;
  __syncthreads();
  const float rstd = 1.0f / sqrtf((((red[0] + red[1]) + red[2]) + red[3]) / (float)C + eps);
  float* orow = out + (size_t)r * 2 * C;
  for (int c = tid; c < C; c += 256) {
    float v = (xr[c] - mean) * rstd;
    if (w) v *= w[c];
    if (b) v += b[c];
    ln[c] = v;
    orow[C + c] = v;
  }
  __syncthreads();
  const int pos = min(max(row_pos[r], 0), n_pos - 1);  // the table row is clamped before it is used in a load
  const float* cr = cos_t + (size_t)pos * hs;
  const float* sr = sin_t + (size_t)pos * hs;
  const int half = hs >> 1;
  for (int c = tid; c < C; c += 256) {
    const int j = c % hs;
    const float partner = j < half ? -ln[c + half] : ln[c - half];
    orow[c] = __fadd_rn(__fmul_rn(ln[c], cr[j]), __fmul_rn(partner, sr[j]));
  }
}

__global__ __launch_bounds__(256) void melspec_db_kernel(float* __restrict__ out, const float* __restrict__ spec, const float* __restrict__ fb,
                                                         int T, int n_bins, int n_mels, int ld, float mean, float stdv) {
  extern __shared__ float pw[];                        // [n_bins]
  __shared__ float part[256];
  const int tid = threadIdx.x;
  const int t = blockIdx.x, clip = blockIdx.y;
  const float* row = spec + ((size_t)clip * T + t) * ld;
  for (int k = tid; k < n_bins; k += 256) {
    const float re = row[k], im = row[n_bins + k];
    pw[k] = fmaf(re, re, __fmul_rn(im, im));
  }
  __syncthreads();
  const int split = n_bins / 2;
  for (int m0 = 0; m0 < n_mels; m0 += 128) {
    const int m = m0 + (tid & 127), h = tid >> 7;
    float acc = 0.f;
    if (m < n_mels) {
      const int k0 = h ? split : 0, k1 = h ? n_bins : split;
      for (int k = k0; k < k1; ++k) acc = fmaf(pw[k], fb[(size_t)k * n_mels + m], acc);
    }
    __syncthreads();
    part[tid] = acc;
    __syncthreads();
    if (h == 0 && m < n_mels) {
      const float p = __fadd_rn(part[tid], part[tid + 128]);
      const float db = p <= 1e-10f ? -100.f : __fmul_rn(10.f, log10f(p));      // 10 log10(max(., 1e-10)): the floor is -100 exactly
      out[((size_t)clip * n_mels + m) * T + t] = __fdiv_rn(__fsub_rn(db, mean), stdv);
    }
  }
}

}  // namespace

extern "C" int ua2_layernorm_rope_rows(float* out, const float* x, const float* w, const float* b, const float* cos_t, const float* sin_t,
                                       const int32_t* row_pos, int32_t n_pos, int64_t R, int32_t C, int32_t head_size, float eps, void* stream) {
  UA2_CHECK(out && x && cos_t && sin_t && row_pos, "ua2_layernorm_rope_rows: NULL argument");
  UA2_CHECK(R > 0 && R < (1ll << 31) && C > 0 && n_pos > 0, "ua2_layernorm_rope_rows: R=%lld C=%d n_pos=%d", (long long)R, C, n_pos);
  UA2_CHECK(head_size > 0 && head_size % 2 == 0 && C % head_size == 0 && C <= 8192,
            "ua2_layernorm_rope_rows: C=%d (<= 8192) must be a multiple of the even head_size=%d", C, head_size);
  hipLaunchKernelGGL(layernorm_rope_kernel, dim3((unsigned)R), dim3(256), (size_t)C * sizeof(float), (hipStream_t)stream, out, x, w, b, cos_t,
                     sin_t, row_pos, n_pos, C, head_size, eps);
  UA2_LAUNCH_CHECK();
  return 0;
}

extern "C" int ua2_melspec_db(float* out, const float* spec, const float* mel_fb, int32_t B, int32_t T, int32_t n_bins, int32_t n_mels,
                              int32_t ld, float mean, float stdv, void* stream) {
  UA2_CHECK(out && spec && mel_fb, "ua2_melspec_db: NULL argument");
  UA2_CHECK(B > 0 && B <= 65535 && T > 0 && n_bins > 1 && n_bins <= 8192 && n_mels > 0 && ld >= 2 * n_bins && stdv > 0.f,
            "ua2_melspec_db: B=%d (1..65535) T=%d n_bins=%d (2..8192) n_mels=%d ld=%d (>= 2 n_bins) std=%g", B, T, n_bins, n_mels, ld, (double)stdv);
  hipLaunchKernelGGL(melspec_db_kernel, dim3((unsigned)T, B), dim3(256), (size_t)n_bins * sizeof(float), (hipStream_t)stream, out, spec, mel_fb, T,
                     n_bins, n_mels, ld, mean, stdv);
  UA2_LAUNCH_CHECK();
  return 0;
}
