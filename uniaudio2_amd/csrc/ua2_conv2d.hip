// 3 x 3 two-dimensional convolution of the BEST-RQ (MusicFM 25 Hz) stem (include/ua2hip.h, ua2_conv2d): nn.Conv2d(k 3, padding 1,
// stride (s_f, s_t) in {1, 2}^2) with the eval-mode BatchNorm2d folded into weight and bias on the host, the residual add and the
// ReLU of Res2dModule (modules/our_MERT_BESTRQ/mert_fairseq/models/musicfm/modules/conv.py:20-42) in the epilogue:
//
//   y[b][co][fo][to] = act( bias[co] + sum_{ci, kf, kt} W[co][ci][kf][kt] * x[b][ci][fo s_f + kf - 1][to s_t + kt - 1] (+ residual) )
//
// Exact fp32, the arithmetic class of conv1d_kernel (ua2_conv.hip): an implicit GEMM on v_mfma_f32_16x16x4_f32.  Two kernels:
//
//   conv2d_kernel        Cin > kSmallCin.  Reduction index = (group of 16 input channels, tap (kf, kt), channel in the group): one
//                        packed chunk of 16 is ONE tap over 16 channels.  Workgroup = 4 waves = 128 output channels x one output
//                        frequency row x 64 output time steps; wave w owns channels 32 w .. 32 w + 31 (two row tiles) and four
//                        16-step time tiles, so every activation value read from LDS feeds two MFMAs.  Per channel group the three
//                        input rows of the window ((64 - 1) s_t + 3 steps) are staged once in LDS: every index (channel, frequency,
//                        time) is clamped into the buffer BEFORE the load and the zero padding is a select on the loaded value.
//                        The weight comes pre-tiled (ua2_pack_linear fp32 over the [Cout, G * 9 * 16] matrix, Cin zero-padded to
//                        16: ops.pack_conv2d_weight), one 16-byte load per lane per chunk, fetched one chunk ahead.
//                        Any F, T, Cin, Cout: partial tiles are masked at the store, the weight tile index is clamped.
//   conv2d_small_kernel  Cin <= kSmallCin (the stem's first layer, Cin = 1: 9 multiply-adds per output): one thread per output, an
//                        fma chain over (ci, kf, kt) ascending; `w` is the plain [Cout, Cin, 3, 3] filter.
//
// A clip's output does not depend on the batch it is in: the grid's z axis is the clip and nothing crosses it.
#include "ua2_common.h"

namespace {

constexpr int kSmallCin = 4;
constexpr int kNTT = 4, kRPW = 2;
constexpr int kBT = 16 * kNTT;          // output time steps per workgroup
constexpr int kBR = 4 * 16 * kRPW;      // output channels per workgroup
constexpr int kCIG = 16;                // input channels per staging group

struct Conv2dP {
  const float* x; const void* w; const float* bias; const float* residual; float* y;
  int B, Cin, Cout, F, T, Fo, To, sf, st, act, ntt;
};

__global__ __launch_bounds__(256) void conv2d_kernel(const Conv2dP a) {
  extern __shared__ __attribute__((aligned(16))) float xs[];      // [kCIG][3][Wp]
  const int st = a.st;
  const int Wt = (kBT - 1) * st + 3, Wp = Wt + 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tl = lane & 15, g = lane >> 4;
  const int fo = blockIdx.x / a.ntt, t0 = (blockIdx.x - fo * a.ntt) * kBT;
  const int r0 = blockIdx.y * kBR + wave * (16 * kRPW);
  const int b = blockIdx.z;
  const int ngroups = (a.Cin + kCIG - 1) / kCIG;
  const int nchunks = ngroups * 9;
  const int ntile_rows = (a.Cout + 15) / 16;
  const bool wave_active = r0 < a.Cout;
  const u32x4* wp[kRPW];
#pragma unroll
  for (int q = 0; q < kRPW; ++q) {
    const int tile = min(r0 / 16 + q, ntile_rows - 1);            // a wave's second tile may lie past the last: clamped load, masked store
    wp[q] = reinterpret_cast<const u32x4*>(a.w) + (size_t)tile * nchunks * 64 + lane;
  }
  f32x4 acc[kRPW][kNTT];
#pragma unroll
  for (int q = 0; q < kRPW; ++q)
#pragma unroll
    for (int nt = 0; nt < kNTT; ++nt) acc[q][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  u32x4 wn[kRPW];
#pragma unroll
  for (int q = 0; q < kRPW; ++q) wn[q] = wave_active ? wp[q][0] : u32x4{0u, 0u, 0u, 0u};
  const int tin0 = t0 * st - 1, fin0 = fo * a.sf - 1;

  for (int cg = 0; cg < ngroups; ++cg) {
    __syncthreads();
    for (int row = wave; row < kCIG * 3; row += 4) {               // (channel in group, kf): one staged row per wave per step
      const int cl = row / 3, kf = row - cl * 3;
      const int ci = cg * kCIG + cl, fi = fin0 + kf;
      const bool row_ok = ci < a.Cin && fi >= 0 && fi < a.F;
      const int cic = min(ci, a.Cin - 1), fic = min(max(fi, 0), a.F - 1);
      const float* src = a.x + (((size_t)b * a.Cin + cic) * a.F + fic) * a.T;
      for (int wi = lane; wi < Wt; wi += 64) {
        const int ti = tin0 + wi;
        const int tic = min(max(ti, 0), a.T - 1);                  // never load through unclamped arithmetic
        const float v = src[tic];
        xs[row * Wp + wi] = (row_ok && ti >= 0 && ti < a.T) ? v : 0.f;
      }
    }
    __syncthreads();
    if (wave_active) {
      for (int j = 0; j < 9; ++j) {
        const int chunk = cg * 9 + j;
        f32x4 wa[kRPW];
#pragma unroll
        for (int q = 0; q < kRPW; ++q) wa[q] = __builtin_bit_cast(f32x4, wn[q]);
        if (chunk + 1 < nchunks) {                                 // one chunk ahead
#pragma unroll
          for (int q = 0; q < kRPW; ++q) wn[q] = wp[q][(size_t)(chunk + 1) * 64];
        }
        const int kf = j / 3, kt = j - kf * 3;
        const int base = (g * 4 * 3 + kf) * Wp + kt + tl * st;     // channel g * 4 + e of the group: + e * 3 * Wp
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
          for (int nt = 0; nt < kNTT; ++nt) {
            const float xv = xs[base + e * 3 * Wp + nt * 16 * st];
#pragma unroll
            for (int q = 0; q < kRPW; ++q) acc[q][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[q][e], xv, acc[q][nt], 0, 0, 0);
          }
        }
      }
    }
  }
  if (!wave_active) return;
  // epilogue: D[row = (lane >> 4) * 4 + r][col = lane & 15]
#pragma unroll
  for (int q = 0; q < kRPW; ++q)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = r0 + q * 16 + g * 4 + r;
      if (co >= a.Cout) continue;
      const float bias = a.bias ? a.bias[co] : 0.f;
      const size_t orow = (((size_t)b * a.Cout + co) * a.Fo + fo) * a.To;
#pragma unroll
      for (int nt = 0; nt < kNTT; ++nt) {
        const int t = t0 + nt * 16 + tl;
        if (t >= a.To) continue;
        float v = __fadd_rn(acc[q][nt][r], bias);
        if (a.residual) v = __fadd_rn(v, a.residual[orow + t]);
        if (a.act) v = fmaxf(v, 0.f);
        a.y[orow + t] = v;
      }
    }
}

__global__ __launch_bounds__(256) void conv2d_small_kernel(const Conv2dP a) {
  const int to = blockIdx.x * 256 + threadIdx.x;
  const int fo = blockIdx.y % a.Fo, co = blockIdx.y / a.Fo, b = blockIdx.z;
  if (to >= a.To) return;
  const float* w = reinterpret_cast<const float*>(a.w) + (size_t)co * a.Cin * 9;
  float acc = 0.f;
  for (int ci = 0; ci < a.Cin; ++ci)
#pragma unroll
    for (int kf = 0; kf < 3; ++kf) {
      const int fi = fo * a.sf + kf - 1;
      const int fic = min(max(fi, 0), a.F - 1);
      const float* src = a.x + (((size_t)b * a.Cin + ci) * a.F + fic) * a.T;
#pragma unroll
      for (int kt = 0; kt < 3; ++kt) {
        const int ti = to * a.st + kt - 1;
        const int tic = min(max(ti, 0), a.T - 1);
        const float v = src[tic];
        acc = fmaf(w[(ci * 3 + kf) * 3 + kt], (fi >= 0 && fi < a.F && ti >= 0 && ti < a.T) ? v : 0.f, acc);
      }
    }
  const size_t o = (((size_t)b * a.Cout + co) * a.Fo + fo) * a.To + to;
  float v = __fadd_rn(acc, a.bias ? a.bias[co] : 0.f);
  if (a.residual) v = __fadd_rn(v, a.residual[o]);
  if (a.act) v = fmaxf(v, 0.f);
  a.y[o] = v;
}

}  // namespace

extern "C" int ua2_conv2d(const float* x, const void* w, const float* bias, const float* residual, float* y, int32_t B, int32_t Cin,
                          int32_t Cout, int32_t F, int32_t T, int32_t stride_f, int32_t stride_t, int32_t act, void* stream) {
  UA2_CHECK(x && w && y, "ua2_conv2d: NULL argument");
  UA2_CHECK(B > 0 && B <= 65535 && Cin > 0 && Cout > 0 && F > 0 && T > 0, "ua2_conv2d: B=%d (1..65535) Cin=%d Cout=%d F=%d T=%d", B, Cin, Cout, F, T);
  UA2_CHECK((stride_f == 1 || stride_f == 2) && (stride_t == 1 || stride_t == 2), "ua2_conv2d: stride (%d, %d): each of 1, 2", stride_f, stride_t);
  UA2_CHECK(act == 0 || act == 1, "ua2_conv2d: act=%d (0 none, 1 ReLU)", act);
  Conv2dP a;
  a.x = x; a.w = w; a.bias = bias; a.residual = residual; a.y = y;
  a.B = B; a.Cin = Cin; a.Cout = Cout; a.F = F; a.T = T; a.sf = stride_f; a.st = stride_t; a.act = act;
  a.Fo = (F - 1) / stride_f + 1;
  a.To = (T - 1) / stride_t + 1;
  UA2_CHECK((int64_t)Cin * F * T < (1ll << 31) && (int64_t)Cout * a.Fo * a.To < (1ll << 31), "ua2_conv2d: a clip's tensor exceeds 2^31 elements");
  hipStream_t s = (hipStream_t)stream;
  if (Cin <= kSmallCin) {
    UA2_CHECK((int64_t)Cout * a.Fo <= 65535, "ua2_conv2d: Cout * Fo = %lld exceeds the grid (65535)", (long long)Cout * a.Fo);
    a.ntt = 0;
    hipLaunchKernelGGL(conv2d_small_kernel, dim3((a.To + 255) / 256, Cout * a.Fo, B), dim3(256), 0, s, a);
  } else {
    a.ntt = (a.To + kBT - 1) / kBT;
    UA2_CHECK((Cout + kBR - 1) / kBR <= 65535, "ua2_conv2d: Cout=%d exceeds the grid", Cout);
    const size_t smem = (size_t)kCIG * 3 * ((kBT - 1) * stride_t + 4) * sizeof(float);
    hipLaunchKernelGGL(conv2d_kernel, dim3((unsigned)((int64_t)a.Fo * a.ntt), (Cout + kBR - 1) / kBR, B), dim3(256), smem, s, a);
  }
  UA2_LAUNCH_CHECK();
  return 0;
}
