// Whisper log-mel front end (include/ua2hip.h, ua2_logmel): transformers' WhisperFeatureExtractor numpy path
// (feature_extraction_whisper.py `_np_extract_fbank_features` over audio_utils.spectrogram) as two launches.
//
//   logmel_kernel    one workgroup = 16 consecutive frames of one clip.  The 2800 samples they span are staged in LDS once
//                    (zero padding / truncation to 480 000 samples and the 200-sample reflection of center=True resolved per
//                    sample, every index clamped before the load); thread k < 201 forms bin k of the 400-point real DFT of the
//                    16 frames against the host-built fp32 basis (Hann window folded in), as four chains of 100 terms added in
//                    order; the 201 powers of a frame go through LDS to the 80 x 201 mel filter bank, then
//                    log10(max(., 1e-10)).  The workgroup's maximum goes to ws[clip][workgroup].
//   logmel_finish    per clip: the maximum of its 188 workgroup maxima (max is exact in any order: no atomics, nothing depends
//                    on scheduling), then max(x, clip_max - 8) and (x + 4) / 4 in place.
//
// A clip's values do not depend on the batch it is in: the grid's y axis is the clip and nothing crosses it.
#include "ua2_common.h"

namespace {

constexpr int kSamples = 480000;   // 30 s at 16 kHz: the extractor's n_samples (longer clips are truncated, shorter ones zero-padded)
constexpr int kFft = 400, kHop = 160, kBins = 201, kMels = 80, kFrames = 3000;   // frame 3000 of the 3001 is dropped (log_spec[:, :-1])
constexpr int kFT = 16;                                  // frames per workgroup
constexpr int kSpan = (kFT - 1) * kHop + kFft;           // 2800 samples
constexpr int kBlocks = (kFrames + kFT - 1) / kFT;       // 188 workgroups per clip
constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void logmel_kernel(const float* __restrict__ wav, const int64_t n_samples,
                                                          const float* __restrict__ basis, const float* __restrict__ fb,
                                                          float* __restrict__ out, float* __restrict__ ws) {
  __shared__ float xs[kSpan];
  __shared__ float pw[kFT][kBins + 3];
  __shared__ float red[kThreads];
  const int tid = threadIdx.x, clip = blockIdx.y, f0 = blockIdx.x * kFT;
  const int nf = min(kFT, kFrames - f0);
  const int nvalid = (int)(n_samples < (int64_t)kSamples ? n_samples : (int64_t)kSamples);
  const float* w = wav + (int64_t)clip * n_samples;
  for (int i = tid; i < kSpan; i += kThreads) {
    const int p = f0 * kHop + i - kFft / 2;              // position in the 480 000-sample clip before reflection
    int idx = p < 0 ? -p : (p >= kSamples ? 2 * (kSamples - 1) - p : p);   // np.pad(mode="reflect")
    idx = min(max(idx, 0), kSamples - 1);                // never load through unclamped arithmetic
    xs[i] = idx < nvalid ? w[idx] : 0.f;                 // zero padding up to 480 000
  }
  __syncthreads();
  if (tid < kBins) {
    float re[kFT], im[kFT];
#pragma unroll
    for (int f = 0; f < kFT; ++f) re[f] = im[f] = 0.f;
    const float* bc = basis + tid;
    const float* bs = basis + kBins + tid;
    for (int seg = 0; seg < kFft; seg += 100) {          // four chains of 100 terms, added in order
      float pr[kFT], pi[kFT];
#pragma unroll
      for (int f = 0; f < kFT; ++f) pr[f] = pi[f] = 0.f;
      for (int n = seg; n < seg + 100; ++n) {
        const float c = bc[n * (2 * kBins)], s = bs[n * (2 * kBins)];
#pragma unroll
        for (int f = 0; f < kFT; ++f) {
          const float x = xs[f * kHop + n];
          pr[f] = fmaf(x, c, pr[f]);
          pi[f] = fmaf(x, s, pi[f]);
        }
      }
#pragma unroll
      for (int f = 0; f < kFT; ++f) { re[f] += pr[f]; im[f] += pi[f]; }
    }
#pragma unroll
    for (int f = 0; f < kFT; ++f) pw[f][tid] = fmaf(re[f], re[f], im[f] * im[f]);
  }
  __syncthreads();
  float mx = -INFINITY;
  for (int o = tid; o < kFT * kMels; o += kThreads) {
    const int f = o / kMels, m = o - f * kMels;
    float acc = 0.f;
    for (int k = 0; k < kBins; ++k) acc = fmaf(pw[f][k], fb[k * kMels + m], acc);
    const float v = acc <= 1e-10f ? -10.f : log10f(acc);  // log10(max(., 1e-10)); the floor is -10 exactly, as in float64
    if (f < nf) {
      out[((int64_t)clip * kMels + m) * kFrames + f0 + f] = v;
      mx = fmaxf(mx, v);
    }
  }
  red[tid] = mx;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]);
    __syncthreads();
  }
  if (tid == 0) ws[clip * kBlocks + blockIdx.x] = red[0];
}

__global__ __launch_bounds__(kThreads) void logmel_finish_kernel(float* __restrict__ out, const float* __restrict__ ws) {
  __shared__ float red[kThreads];
  const int tid = threadIdx.x, clip = blockIdx.y;
  red[tid] = tid < kBlocks ? ws[clip * kBlocks + tid] : -INFINITY;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]);
    __syncthreads();
  }
  const float lo = red[0] - 8.f;
  float* o = out + (int64_t)clip * kMels * kFrames;
  for (int i = blockIdx.x * kThreads + tid; i < kMels * kFrames; i += gridDim.x * kThreads)
    o[i] = (fmaxf(o[i], lo) + 4.f) * 0.25f;
}

}  // namespace

static_assert(kBlocks <= kThreads, "logmel_finish_kernel reduces one maximum per thread");

extern "C" size_t ua2_logmel_workspace_bytes(int32_t B) { return B > 0 ? (size_t)B * kBlocks * sizeof(float) : 0; }

extern "C" int ua2_logmel(float* out, const float* wav, int32_t B, int64_t n_samples, const float* basis, const float* mel_fb,
                          float* ws, size_t ws_bytes, void* stream) {
  UA2_CHECK(out && wav && basis && mel_fb && ws, "ua2_logmel: NULL argument");
  UA2_CHECK(B > 0 && B <= 65535 && n_samples > 0, "ua2_logmel: B=%d (1..65535), n_samples=%lld (> 0)", B, (long long)n_samples);
  UA2_CHECK(ws_bytes >= ua2_logmel_workspace_bytes(B), "ua2_logmel: workspace of %zu bytes, %zu needed", ws_bytes, ua2_logmel_workspace_bytes(B));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(logmel_kernel, dim3(kBlocks, B), dim3(kThreads), 0, s, wav, n_samples, basis, mel_fb, out, ws);
  UA2_LAUNCH_CHECK();
  hipLaunchKernelGGL(logmel_finish_kernel, dim3(64, B), dim3(kThreads), 0, s, out, (const float*)ws);
  UA2_LAUNCH_CHECK();
  return 0;
}
