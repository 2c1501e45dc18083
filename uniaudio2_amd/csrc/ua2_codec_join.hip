// Joins of the reasoning-conditioned decode (ReasoningTokenizer.token2audio, reason_tokenizer.py:132-226):
//   * the reasoning features added to the summed RVQ look-ups after the x2.5 nearest up-sampling
//     (AudioDiffusion1D.py:440-456 feature_combine), one launch instead of a gather into a temporary plus an add;
//   * the linear cross-fade of the decoded 30-s windows and the final crop (reason_tokenizer.py:210-224), on the device.
#include "ua2_common.h"

namespace {

// out[r, :] = rec[r, :] + reason[src[r], :]   fp32, one rounding (torch's `qsum + gathered`).  One thread per float4;
// out may alias rec (each thread reads its own float4 of rec before it writes it).
__global__ void reason_merge_kernel(float* out, const float* rec, const float* __restrict__ reason, const int32_t* __restrict__ src,
                                    int64_t n4, int32_t D4) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / D4;
    const int32_t c = (int32_t)(i - r * D4);
    const float4 a = reinterpret_cast<const float4*>(rec)[i];
    const float4 b = reinterpret_cast<const float4*>(reason)[(int64_t)src[r] * D4 + c];
    float4 y;
    y.x = __fadd_rn(a.x, b.x);
    y.y = __fadd_rn(a.y, b.y);
    y.z = __fadd_rn(a.z, b.z);
    y.w = __fadd_rn(a.w, b.w);
    reinterpret_cast<float4*>(out)[i] = y;
  }
}

// Window k of the joined waveform starts at k * hop (hop = win - ovlp >= ovlp).  Output sample j belongs to window
// k = min(j / hop, n_seg - 1) at offset i = j - k * hop; when k > 0 and i < ovlp it is in the overlap with window k - 1
// (its offset i + hop) and takes the host's float64 blend
//   (float)((double)old * (1 - ramp[i]) + (double)new * ramp[i]),   ramp = np.linspace(0, 1, ovlp)
// rounded operation by operation (no fused multiply-add: the host computes the two products and the sum with three
// roundings), so the result equals crossfade_concat bit for bit.  Every sample reads at most two window samples.
__global__ void crossfade_kernel(float* __restrict__ out, const float* __restrict__ seg, int32_t n_seg, int64_t seg_stride, int64_t hop,
                                 int64_t ovlp, int64_t target_len, double step) {
  // hipcc contracts multiply-adds by default, and __dmul_rn / __dadd_rn do not prevent it (their bodies are outside any
  // pragma; the gfx950 assembly showed v_fmac_f64).  Plain operators under this pragma give v_mul_f64 + v_add_f64.
#pragma clang fp contract(off)
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < target_len; j += (int64_t)gridDim.x * blockDim.x) {
    int64_t k = j / hop;
    if (k > n_seg - 1) k = n_seg - 1;
    const int64_t i = j - k * hop;
    const float cur = seg[k * seg_stride + i];
    if (k > 0 && i < ovlp) {
      const float old = seg[(k - 1) * seg_stride + i + hop];
      // np.linspace: i * step, the last entry set to `stop` (num > 1)
      const double ramp = (ovlp > 1 && i == ovlp - 1) ? 1.0 : (double)i * step;
      const double a = (double)old * (1.0 - ramp);
      const double b = (double)cur * ramp;
      out[j] = (float)(a + b);
    } else {
      out[j] = cur;
    }
  }
}

unsigned grid_for(int64_t n, int block) {
  const int64_t g = (n + block - 1) / block;
  return (unsigned)(g < 65536 ? g : 65536);
}

}  // namespace

extern "C" int ua2_reason_merge(float* out, const float* rec, const float* reason, const int32_t* src, int64_t rows, int32_t D,
                                void* stream) {
  UA2_CHECK(out && rec && reason && src && rows > 0 && D > 0 && D % 4 == 0, "ua2_reason_merge: bad arguments (D %% 4 == 0)");
  UA2_CHECK(((uintptr_t)out | (uintptr_t)rec | (uintptr_t)reason) % 16 == 0, "ua2_reason_merge: out / rec / reason must be 16-byte aligned");
  const int64_t n4 = rows * (D / 4);
  hipLaunchKernelGGL(reason_merge_kernel, dim3(grid_for(n4, 256)), dim3(256), 0, (hipStream_t)stream, out, rec, reason, src, n4, D / 4);
  UA2_LAUNCH_CHECK();
  return 0;
}

extern "C" int ua2_crossfade(float* out, const float* seg, int32_t n_seg, int64_t seg_stride, int64_t win, int64_t ovlp,
                             int64_t target_len, void* stream) {
  UA2_CHECK(out && seg && n_seg > 0 && win > 0 && ovlp > 0 && 2 * ovlp <= win && seg_stride >= win && target_len > 0,
            "ua2_crossfade: bad arguments (0 < ovlp <= win - ovlp, seg_stride >= win)");
  const int64_t hop = win - ovlp;
  const int64_t joined = (int64_t)(n_seg - 1) * hop + win;
  UA2_CHECK(target_len <= joined, "ua2_crossfade: target_len %lld exceeds the joined length %lld", (long long)target_len, (long long)joined);
  const double step = ovlp > 1 ? 1.0 / (double)(ovlp - 1) : 0.0;        // np.linspace: (stop - start) / (num - 1)
  hipLaunchKernelGGL(crossfade_kernel, dim3(grid_for(target_len, 256)), dim3(256), 0, (hipStream_t)stream, out, seg, n_seg, seg_stride, hop,
                     ovlp, target_len, step);
  UA2_LAUNCH_CHECK();
  return 0;
}
