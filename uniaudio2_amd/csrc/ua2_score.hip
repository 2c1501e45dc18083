// Cross-entropy tail of the teacher-forced pass (llm_models/model_new.py:402-454 forward with :59-109 CrossEntropyAndAccuracy_*):
//   nll  = lse(logits[m, :V]) - logits[m, label]     (the row maximum subtracted before the exponentials)
//   pred = arg-max, lowest index on ties             (all-NaN / clamp rule of the sampling tails: ua2_row_token)
//   next_h[m, :] = emb[emb_row0 + label, :]          (teacher forcing: the LABEL's embedding feeds the next codebook step,
//                                                     where ua2_argmax_embed gathers the row of the id it chose)
// over the raw fp32 logits: no forbid_prefix, no guidance, no arg-max partials.
//
// One workgroup of 1024 threads per row.  Thread t owns columns t, t + 1024, ...; a row is reduced by 64-lane xor butterflies and
// then the 16 wave results in wave order — one summation order per row whatever M is, so a row's bits do not depend on its
// neighbours.  The row (513 KB for the text head) is read twice and stays in L2 between the passes.
#include "ua2_common.h"

namespace {

constexpr int kXentThreads = 1024;

template <int DT>
__global__ __launch_bounds__(kXentThreads) void xent_embed_kernel(const float* __restrict__ logits, int ld, int V,
                                                                  const int32_t* __restrict__ labels, int label_ld, int label_col,
                                                                  float* __restrict__ nll, int32_t* __restrict__ pred, int out_ld, int out_col,
                                                                  const void* __restrict__ emb, long long emb_row0, int C,
                                                                  float* __restrict__ emb_out) {
  __shared__ float red_v[kXentThreads / 64];
  __shared__ int red_i[kXentThreads / 64];
  __shared__ int tok_s;
  const int m = blockIdx.x, tid = threadIdx.x;
  const float* row = logits + (size_t)m * ld;
  // ---- arg-max (larger value, then lower index; a NaN never wins) ------------------------------------------------------------
  float bv = -INFINITY;
  int bi = UA2_TOK_NONE;
  for (int c = tid; c < V; c += kXentThreads) {
    const float v = row[c];
    if (v > bv || (v == bv && c < bi)) { bv = v; bi = c; }
  }
  const int tok = ua2_row_token(bv, bi, V, red_v, red_i, &tok_s, [&] { return tid == 0 ? 0 : UA2_TOK_NONE; });
  // the row maximum: the winner's value (an all-NaN row reads a NaN here and ends as NaN, like every row that holds one)
  const float mx = row[tok];
  // ---- sum of exp(x - max): a NaN entry, or -inf - -inf on a row of -inf, makes the sum NaN as F.cross_entropy does ----------
  float sum = 0.f;
  for (int c = tid; c < V; c += kXentThreads) sum += expf(row[c] - mx);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
  __syncthreads();                      // ua2_row_token's readers of red_v are done
  if ((tid & 63) == 0) red_v[tid >> 6] = sum;
  __syncthreads();
  const int lab_raw = labels[(size_t)m * label_ld + label_col];
  const int lab = min(max(lab_raw, 0), V - 1);      // -1 (ignored) gathers row 0; the host rejects everything outside [-1, V)
  if (tid == 0) {
    float s = red_v[0];
    for (int w = 1; w < kXentThreads / 64; ++w) s += red_v[w];
    // lse - x[label] = log(sum) - (x[label] - max): the large common term never enters a rounding
    nll[(size_t)m * out_ld + out_col] = lab_raw < 0 ? 0.f : logf(s) - (row[lab] - mx);
    pred[(size_t)m * out_ld + out_col] = tok;
  }
  if (emb) {
    const size_t er = (size_t)(emb_row0 + lab);
    for (int c = tid; c < C; c += kXentThreads) emb_out[(size_t)m * C + c] = load_elem<DT>(emb, er * C + c);
  }
}

}  // namespace

extern "C" int ua2_xent_embed(int dtype, int32_t M, const float* logits, int32_t ld, int32_t V, const int32_t* labels, int32_t label_ld,
                              int32_t label_col, float* nll, int32_t* pred, int32_t out_ld, int32_t out_col, const void* emb,
                              int64_t emb_row0, int32_t C, float* emb_out, void* stream) {
  UA2_CHECK(M > 0 && logits && V > 0 && ld >= V && labels && nll && pred, "ua2_xent_embed: bad arguments");
  UA2_CHECK(label_ld >= 1 && label_col >= 0 && label_col < label_ld && out_ld >= 1 && out_col >= 0 && out_col < out_ld,
            "ua2_xent_embed: label column %d of %d / output column %d of %d", label_col, label_ld, out_col, out_ld);
  UA2_CHECK(!emb || (emb_out && C > 0 && emb_row0 >= 0), "ua2_xent_embed: the gather needs emb_out, C > 0 and emb_row0 >= 0");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == UA2_BF16)
    hipLaunchKernelGGL((xent_embed_kernel<UA2_BF16>), dim3(M), dim3(kXentThreads), 0, s, logits, ld, V, labels, label_ld, label_col, nll, pred,
                       out_ld, out_col, emb, (long long)emb_row0, C, emb_out);
  else if (dtype == UA2_F32)
    hipLaunchKernelGGL((xent_embed_kernel<UA2_F32>), dim3(M), dim3(kXentThreads), 0, s, logits, ld, V, labels, label_ld, label_col, nll, pred,
                       out_ld, out_col, emb, (long long)emb_row0, C, emb_out);
  else {
    ua2_set_error("ua2_xent_embed: bad dtype %d", dtype);
    return -1;
  }
  UA2_LAUNCH_CHECK();
  return 0;
}
