// Beam search over the text head, on the device (DESIGN.md §2 "beam search", §4; the rule is a corrected restatement of the
// reference's evaluation/asr_task.py:438-576, whose own function cannot run).
//
// The W hypotheses of a beam are W rows of one decode frame; G beams ("groups": one per utterance) share a frame, group g's slot j
// being row g * W + j (rows = sequences 0 .. G * W - 1; G = 1 is the single search).  Per frame:
//   ua2_beam_step[_groups]     beam_topw_kernel    one 1024-thread workgroup per LIVE row over its fp32 logits: row maximum, sum of
//                                                  exp(x - m), the W best columns (value descending, id ascending), their log-softmax
//                              beam_select_kernel  one workgroup per group: the <= W * W + W candidates in candidate order, the
//                                                  length-normalised scores, the W best (stable), the new per-slot state, parents,
//                                                  fed-back ids, one log record
//   ua2_beam_reorder[_groups]  beam_copy_kernel    the K/V fork: a slot's copy of its parent's partial 64-position page, every pool
//                              beam_table_kernel   one workgroup per group: the page tables — shared full pages inherited from the
//                                                  parent, the new partial page
// A group's state lies at fixed strides from the base pointers of ua2_beam_state (8 slots, 4 ctrl words, 64 candidates, log_cap * W
// log records per group); a group reads and writes only its own state, token rows, log and table rows.
// Nothing is permuted on the device but page-table entries and at most one partial page per pool and slot; the text of a hypothesis
// is recovered on the host by walking the step log backwards.
//   ua2_beam_step_groups_ngram  beam_topw_ngram_kernel / beam_select_ngram_kernel: the same step under the no-repeat-n-gram ban
//                                                  (opt-in).  The step itself needs a slot's text, and walking the log
//                                                  would be one dependent load per id, so under the ban every group keeps two sets of
//                                                  8 histories of `cap` ids: a step reads set ctrl[0] & 1 and writes the other one.
//                                                  The ban is a bitmap over V in shared memory: the logits stay read-only.  The
//                                                  kernels without the ban are instantiations of the same bodies with the ban
//                                                  compiled out: their code is what it was.
//
// Reproducibility: the workgroup size of beam_topw_kernel (1024) is part of the contract — the sum of exponentials is 1024 strided
// partial sums (column c goes to thread c % 1024, ascending c) joined by the fixed halving tree below, so a row's log-sum-exp has
// the same bits whatever else runs.  The top-W selection is an arg-max over a total order (value, then lower id), so it does not
// depend on geometry at all.
#include "ua2_common.h"

namespace {

constexpr int kBeamMaxW = 8;
constexpr int kBeamMaxRows = 64;
constexpr int kTopwThreads = 1024;
constexpr int kTopwBatch = 16;
constexpr int kMaxCand = kBeamMaxW * kBeamMaxW + kBeamMaxW;

__device__ __forceinline__ bool beam_better(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }
__device__ __forceinline__ float beam_finite_or_ninf(float x) { return x == x ? x : -INFINITY; }   // a NaN is ordered as -inf

// The no-repeat-n-gram ban of a step (ua2_beam_step_groups_ngram): what the ban variants of the two kernels read besides the state
struct BeamBan {
  int n, cap;
  int32_t* hist;                                  // [G][2][8][cap]: set ctrl[0] & 1 of a group is read by a step, the other one written
};

// one column of a row as the passes below see it: a NaN is -inf, and under the ban so is a column whose bit is set
template <bool kBan>
__device__ __forceinline__ float beam_column(const float* __restrict__ row, int c, const uint32_t* ban) {
  const float x = beam_finite_or_ninf(row[c]);
  if constexpr (kBan) return ((ban[c >> 5] >> (c & 31)) & 1u) ? -INFINITY : x;
  return x;
}

// fin: 0 live, 1 finished, 2 dead (a slot that holds no hypothesis: slots 1 .. W - 1 before the first step)
// kBan: `ban` is a bitmap over the V columns in shared memory, filled by the caller (beam_topw_ngram_kernel) behind a barrier; the
// three passes are the same code for both values, so a banned row owes the bits of the row with -inf in the banned columns
template <bool kBan>
__device__ __forceinline__ void beam_topw_row(const float* __restrict__ logits, int ld, int V, int W, int j, const uint32_t* ban,
                                              float* __restrict__ cand_logp, int32_t* __restrict__ cand_id) {
  __shared__ float red[kTopwThreads];
  __shared__ float wv[kTopwThreads / 64];
  __shared__ int wi[kTopwThreads / 64];
  const int tid = threadIdx.x;
  const float* row = logits + (size_t)blockIdx.x * ld;
  float lv[kBeamMaxW];
  int li[kBeamMaxW];
#pragma unroll
  for (int k = 0; k < kBeamMaxW; ++k) { lv[k] = -INFINITY; li[k] = UA2_TOK_NONE; }
  float m = -INFINITY;
  // kTopwBatch independent loads in flight per thread (one load per iteration leaves the pass latency-bound: ~125 dependent
  // round trips at the released vocabulary), then the columns in ascending order as before
  for (int base = tid; base < V; base += kTopwBatch * kTopwThreads) {
    float xs[kTopwBatch];
#pragma unroll
    for (int u = 0; u < kTopwBatch; ++u) {
      const int c = base + u * kTopwThreads;
      xs[u] = c < V ? beam_column<kBan>(row, c, ban) : -INFINITY;
    }
#pragma unroll
    for (int u = 0; u < kTopwBatch; ++u) {
      const int c = base + u * kTopwThreads;
      const float x = xs[u];
      if (c >= V) continue;
      m = fmaxf(m, x);
      if (beam_better(x, c, lv[kBeamMaxW - 1], li[kBeamMaxW - 1])) {
        float cv = x;
        int ci = c;
        // the exchange as selects, not as a branch per entry: the branching form lost a column that TIED with entry 0 on its
        // value and won on its id (only an -inf / NaN column against the empty list can, ids being ascending) in the generated
        // code of the first column of an outer iteration, so a row with fewer than W finite entries named the wrong -inf columns
#pragma unroll
        for (int k = 0; k < kBeamMaxW; ++k) {
          const bool b = beam_better(cv, ci, lv[k], li[k]);
          const float tv = lv[k]; const int ti = li[k];
          lv[k] = b ? cv : tv; li[k] = b ? ci : ti;
          cv = b ? tv : cv; ci = b ? ti : ci;
        }
      }
    }
  }
  red[tid] = m;
  __syncthreads();
  for (int s = kTopwThreads / 2; s >= 1; s >>= 1) {
    if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]);
    __syncthreads();
  }
  m = red[0];
  __syncthreads();
  float part = 0.f;
  if (m > -INFINITY)
    for (int base = tid; base < V; base += kTopwBatch * kTopwThreads) {
      float xs[kTopwBatch];
#pragma unroll
      for (int u = 0; u < kTopwBatch; ++u) {
        const int c = base + u * kTopwThreads;
        xs[u] = c < V ? beam_column<kBan>(row, c, ban) : -INFINITY;
      }
#pragma unroll
      for (int u = 0; u < kTopwBatch; ++u)                 // ascending c, one rounded sum per column
        if (base + u * kTopwThreads < V) part += expf(xs[u] - m);
    }
  red[tid] = part;
  __syncthreads();
  for (int s = kTopwThreads / 2; s >= 1; s >>= 1) {       // the fixed tree: red[t] += red[t + s], s = 512, 256, .., 1
    if (tid < s) red[tid] = red[tid] + red[tid + s];
    __syncthreads();
  }
  const float logS = logf(red[0]);
  for (int r = 0; r < W; ++r) {
    float bv = lv[0];
    int bi = li[0];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float ov = __shfl_xor(bv, o);
      const int oi = __shfl_xor(bi, o);
      if (beam_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if ((tid & 63) == 0) { wv[tid >> 6] = bv; wi[tid >> 6] = bi; }
    __syncthreads();
    bv = wv[0]; bi = wi[0];
    for (int w = 1; w < kTopwThreads / 64; ++w)
      if (beam_better(wv[w], wi[w], bv, bi)) { bv = wv[w]; bi = wi[w]; }
    if (bi != UA2_TOK_NONE && bi == li[0]) {      // the one thread that held the winner moves on to its next entry
#pragma unroll
      for (int k = 0; k + 1 < kBeamMaxW; ++k) { lv[k] = lv[k + 1]; li[k] = li[k + 1]; }
      lv[kBeamMaxW - 1] = -INFINITY; li[kBeamMaxW - 1] = UA2_TOK_NONE;
    }
    if (tid == 0) {
      // a row without a finite entry has no distribution: every candidate scores -inf
      cand_logp[j * kBeamMaxW + r] = (m > -INFINITY) ? (bv - m) - logS : -INFINITY;
      cand_id[j * kBeamMaxW + r] = min(max(bi, 0), V - 1);
    }
    __syncthreads();                              // wv / wi are rewritten by the next round
  }
}

__global__ __launch_bounds__(kTopwThreads) void beam_topw_kernel(const float* __restrict__ logits, int ld, int V, int W,
                                                                 const int32_t* __restrict__ fin, float* __restrict__ cand_logp,
                                                                 int32_t* __restrict__ cand_id) {
  const int j = (blockIdx.x / W) * kBeamMaxW + blockIdx.x % W;   // row g * W + slot -> the slot's place in its group's state
  if (fin[j] != 0) return;                       // the whole workgroup: finished and dead slots produce no candidates from logits
  beam_topw_row<false>(logits, ld, V, W, j, nullptr, cand_logp, cand_id);
}

// The step under the no-repeat-n-gram ban.  How the ban is applied: a bitmap over the V columns in shared memory ((V + 31) / 32
// words: 16 KB at the released vocabulary), so the logits stay read-only.  The workgroup of a live row with L = len ids h[0 .. L) in
// its group's read set compares the L - n + 1 windows h[i .. i + n - 1) with the prefix h[L - n + 1 .. L), the windows strided over the
// 1024 threads, and sets the bit of h[i + n - 1] (clamped into [0, V)) where they are equal; then the passes of beam_topw_row run.
// L < n bans nothing; L > cap is not filtered (the history no longer holds the suffix), like ua2_ngram_filter.
__global__ __launch_bounds__(kTopwThreads) void beam_topw_ngram_kernel(const float* __restrict__ logits, int ld, int V, int W,
                                                                       const int32_t* __restrict__ fin, const int32_t* __restrict__ len,
                                                                       const int32_t* __restrict__ ctrl, BeamBan bn,
                                                                       float* __restrict__ cand_logp, int32_t* __restrict__ cand_id) {
  extern __shared__ uint32_t ban[];
  const int tid = threadIdx.x, g = blockIdx.x / W, slot = blockIdx.x % W;
  const int j = g * kBeamMaxW + slot;
  if (fin[j] != 0) return;                       // finished and dead slots read no logits and ban nothing
  for (int w = tid; w < (V + 31) / 32; w += kTopwThreads) ban[w] = 0u;
  __syncthreads();
  const int L = len[j], n = bn.n;
  if (L >= n && L <= bn.cap) {
    const int32_t* h = bn.hist + ((size_t)(g * 2 + (ctrl[g * 4] & 1)) * kBeamMaxW + slot) * bn.cap;
    const int32_t* p = h + (L - n + 1);
    for (int i = tid; i <= L - n; i += kTopwThreads) {
      bool same = true;
      for (int k = 0; k < n - 1; ++k) same = same && h[i + k] == p[k];
      if (same) {
        const int c = min(max(h[i + n - 1], 0), V - 1);
        atomicOr(&ban[c >> 5], 1u << (c & 31));
      }
    }
  }
  __syncthreads();
  beam_topw_row<true>(logits, ld, V, W, j, ban, cand_logp, cand_id);
}

// kBan: behind the selection the whole workgroup writes the histories of the new live slots into the set the step did not read —
// slot t's = its parent's in the read set plus the new id (two slots may swap parents in one step: hence two sets)
template <bool kBan>
__device__ __forceinline__ void beam_select_group(int W, int V, int eos, ua2_beam_state st, int32_t* __restrict__ token, int token_ld,
                                                  BeamBan bn) {
  __shared__ float cs[kMaxCand];
  __shared__ int cpar[kMaxCand], ctok[kMaxCand], cfin[kMaxCand], clen[kMaxCand], taken[kMaxCand];
  __shared__ float sscore[kBeamMaxW];
  __shared__ int sfin[kBeamMaxW], slen[kBeamMaxW];
  const int tid = threadIdx.x, g = blockIdx.x;
  st.score += g * kBeamMaxW; st.fin += g * kBeamMaxW; st.len += g * kBeamMaxW; st.parent += g * kBeamMaxW;
  st.ctrl += g * 4; st.cand_logp += g * kBeamMaxW * kBeamMaxW; st.cand_id += g * kBeamMaxW * kBeamMaxW;
  st.log += (size_t)g * st.log_cap * W * 4;
  token += (size_t)g * W * token_ld;
  if (tid < W) { sfin[tid] = st.fin[tid]; sscore[tid] = st.score[tid]; slen[tid] = max(st.len[tid], 0); }
  __syncthreads();
  // candidate order: slots in slot order, a live slot's W columns in rank order.  Thread (j, r) = j * 8 + r fills the candidate of
  // slot j, rank r at its place in that order (a finished slot has the one candidate, a dead slot none): the loads run side by side
  int n = 0;
  for (int i = 0; i < W; ++i) n += sfin[i] == 0 ? W : (sfin[i] == 1 ? 1 : 0);
  {
    const int j = tid / kBeamMaxW, r = tid % kBeamMaxW;
    if (j < W && r < W) {
      int at = r;
      for (int i = 0; i < j; ++i) at += sfin[i] == 0 ? W : (sfin[i] == 1 ? 1 : 0);
      const int f = sfin[j], L = slen[j];
      const float sc = sscore[j];
      if (f == 1 && r == 0) {
        cs[at] = beam_finite_or_ninf(sc); cpar[at] = j; ctok[at] = -1; cfin[at] = 1; clen[at] = L; taken[at] = 0;
      } else if (f == 0) {
        const int k = st.cand_id[j * kBeamMaxW + r];
        const float lp = beam_finite_or_ninf(st.cand_logp[j * kBeamMaxW + r]);
        const bool is_eos = k == eos;
        const int Ln = is_eos ? L : L + 1;        // the EOS id is not part of the text
        // score + logp / lp(len): the host's float64 1 / lp as fp32, one rounded product, one rounded sum.  __fmul_rn / __fadd_rn
        // are a plain * and + here, which the default -ffp-contract=fast fused into one v_fmac_f32 (a single rounding): the
        // contraction is switched off for this statement instead
        float s;
        {
#pragma clang fp contract(off)
          const float prod = lp * st.lp_inv[min(Ln, st.lp_n - 1)];
          s = sc + prod;
        }
        cs[at] = beam_finite_or_ninf(s); cpar[at] = j; ctok[at] = is_eos ? -1 : k; cfin[at] = is_eos ? 1 : 0; clen[at] = Ln; taken[at] = 0;
      }
    }
  }
  __syncthreads();
  __shared__ int npar[kBeamMaxW], ntok[kBeamMaxW], nfin[kBeamMaxW], nlen[kBeamMaxW], nset;   // the selection, for the copy (kBan)
  if (!kBan && tid != 0) return;
  if (tid == 0) {
    const int step = st.ctrl[0];
    bool all_fin = true;
    for (int t = 0; t < W; ++t) {                   // the W best; equal scores in candidate order (a stable descending sort)
      int best = -1;
      for (int i = 0; i < n; ++i)
        if (!taken[i] && (best < 0 || cs[i] > cs[best])) best = i;
      float s = -INFINITY;
      int par = t, tok = -1, f = 2, L = 0;          // fewer candidates than slots (never after the first step): a dead slot
      if (best >= 0) { taken[best] = 1; s = cs[best]; par = cpar[best]; tok = ctok[best]; f = cfin[best]; L = clen[best]; }
      all_fin = all_fin && f == 1;
      // every read of the old state is done (the candidates hold copies): write the new one
      st.score[t] = s; st.fin[t] = f; st.len[t] = L; st.parent[t] = par;
      token[(size_t)t * token_ld] = f == 0 ? min(max(tok, 0), V - 1) : 0;
      if (step >= 0 && step < st.log_cap) {
        int32_t* rec = st.log + ((size_t)step * W + t) * 4;
        rec[0] = par; rec[1] = f == 0 ? min(max(tok, 0), V - 1) : -1; rec[2] = __float_as_int(s); rec[3] = f;
      }
      if constexpr (kBan) { npar[t] = par; ntok[t] = min(max(tok, 0), V - 1); nfin[t] = f; nlen[t] = L; }
    }
    if (all_fin && st.ctrl[1] < 0) st.ctrl[1] = step;
    st.ctrl[0] = step + 1;
    if constexpr (kBan) nset = step & 1;
  }
  if constexpr (kBan) {
    __syncthreads();
    int32_t* sets = bn.hist + (size_t)g * 2 * kBeamMaxW * bn.cap;
    for (int t = 0; t < W; ++t) {
      if (nfin[t] != 0) continue;                 // finished and dead slots need no history
      const int Lp = nlen[t] - 1;                 // a live candidate is its parent's text plus one id
      const int32_t* src = sets + ((size_t)nset * kBeamMaxW + min(max(npar[t], 0), W - 1)) * bn.cap;
      int32_t* dst = sets + ((size_t)(nset ^ 1) * kBeamMaxW + t) * bn.cap;
      for (int i = tid; i < min(Lp, bn.cap); i += blockDim.x) dst[i] = src[i];
      if (tid == 0 && Lp >= 0 && Lp < bn.cap) dst[Lp] = ntok[t];     // nothing at or past cap
    }
  }
}

__global__ __launch_bounds__(64) void beam_select_kernel(int W, int V, int eos, ua2_beam_state st, int32_t* __restrict__ token, int token_ld) {
  beam_select_group<false>(W, V, eos, st, token, token_ld, BeamBan{});
}

constexpr int kSelectNgramThreads = 256;           // the copy of up to W * cap words is spread over them; the selection uses the first 64
__global__ __launch_bounds__(kSelectNgramThreads) void beam_select_ngram_kernel(int W, int V, int eos, ua2_beam_state st,
                                                                                int32_t* __restrict__ token, int token_ld, BeamBan bn) {
  beam_select_group<true>(W, V, eos, st, token, token_ld, bn);
}

struct BeamTables {
  int32_t* t[3];
};

// row r's private page for the column of position n: the static page (row, column) of page set n & 1 — set 0 = the pages of
// sequences 0 .. R - 1, set 1 = those of sequences R .. 2R - 1 (the static layout: sequence b owns pages [b * max_pages, ..));
// R = G * W rows, so a group owns W rows of either set and the groups' pages are disjoint
__device__ __forceinline__ int beam_own_page(int n, int r, int R, int max_pages) { return (((n & 1) * R) + r) * max_pages + (n >> 6); }

__global__ __launch_bounds__(256) void beam_copy_kernel(int W, int R, const int32_t* __restrict__ parent, const int32_t* __restrict__ row_pos,
                                                        int pos_add, const ua2_beam_pool* __restrict__ pools, BeamTables T,
                                                        int table_rows, int max_pages) {
  const ua2_beam_pool P = pools[blockIdx.x];
  const int r = blockIdx.y, g = r / W, j = r - g * W;
  const int n = row_pos[r] + pos_add;              // the next position the slot writes
  if (n < 0) return;
  const int c = n >> 6, fill = n & 63;
  if (fill == 0 || c >= max_pages) return;         // the position opens a new page: nothing to carry over
  const int p = g * W + (parent ? min(max(parent[g * kBeamMaxW + j], 0), W - 1) : 0);   // the parent's row: within the group
  const int32_t* tab = T.t[min(max(P.table, 0), 2)];
  const int src = min(max(tab[p * max_pages + c], 0), table_rows * max_pages - 1);
  const int dst = beam_own_page(n, r, R, max_pages);   // < 2 R * max_pages <= table_rows * max_pages (c < max_pages, r < R)
  if (src == dst) return;                          // the start, slot 0: the prompt's page is already its own
  const size_t head_bytes = (size_t)P.head_bytes, page_bytes = (size_t)P.n_kv * UA2_PAGE * head_bytes;
  const char* s = (const char*)P.pool + (size_t)src * page_bytes;
  char* d = (char*)P.pool + (size_t)dst * page_bytes;
  const int nvec = (int)(fill * head_bytes / 16);  // the filled positions of one head: contiguous
  for (int v = threadIdx.x; v < P.n_kv * nvec; v += blockDim.x) {
    const int h = v / nvec, o = v - h * nvec;
    const size_t off = (size_t)h * UA2_PAGE * head_bytes + (size_t)o * 16;
    *reinterpret_cast<uint4*>(d + off) = *reinterpret_cast<const uint4*>(s + off);
  }
}

// one workgroup per group, its rows g * W .. g * W + W - 1 of every table: read everything, barrier, write — a slot's new row is
// its parent's OLD row
__global__ __launch_bounds__(256) void beam_table_kernel(int W, int R, const int32_t* __restrict__ parent, const int32_t* __restrict__ row_pos,
                                                         int pos_add, BeamTables T, int n_tables, int max_pages) {
  extern __shared__ int32_t old[];
  const int cells = W * max_pages, g = blockIdx.x;
  for (int t = 0; t < n_tables; ++t) {
    int32_t* tab = T.t[t] + (size_t)g * W * max_pages;
    for (int e = threadIdx.x; e < cells; e += blockDim.x) old[e] = tab[e];
    __syncthreads();
    for (int e = threadIdx.x; e < cells; e += blockDim.x) {
      const int j = e / max_pages, col = e - j * max_pages;
      const int n = row_pos[g * W + j] + pos_add;
      if (n < 0) continue;
      const int c = n >> 6;
      const int p = parent ? min(max(parent[g * kBeamMaxW + j], 0), W - 1) : 0;
      if (col < c) tab[e] = old[p * max_pages + col];
      else if (col == c) tab[e] = beam_own_page(n, g * W + j, R, max_pages);
    }
    __syncthreads();
  }
}

int check_state(const ua2_beam_state* st, int W, int G, const char* who) {
  UA2_CHECK(W >= 1 && W <= kBeamMaxW, "%s: beam width must be in 1..%d, got %d", who, kBeamMaxW, W);
  UA2_CHECK(G >= 1 && G * W <= kBeamMaxRows, "%s: %d groups of %d slots: need 1 <= G and G * W <= %d rows", who, G, W, kBeamMaxRows);
  UA2_CHECK(st && st->score && st->fin && st->len && st->parent && st->ctrl && st->cand_logp && st->cand_id && st->log && st->lp_inv,
            "%s: NULL state buffer", who);
  UA2_CHECK(st->log_cap >= 1 && st->lp_n >= 2, "%s: log capacity %d / %d length-penalty entries", who, st->log_cap, st->lp_n);
  return 0;
}

}  // namespace

extern "C" int ua2_beam_step_groups(const float* logits, int32_t ld, int32_t V, int32_t W, int32_t G, int32_t eos, const ua2_beam_state* st,
                                    int32_t* token, int32_t token_ld, void* stream) {
  if (int rc = check_state(st, W, G, "ua2_beam_step")) return rc;
  UA2_CHECK(logits && token && token_ld >= 1, "ua2_beam_step: NULL logits / token buffer");
  UA2_CHECK(V >= W && ld >= V, "ua2_beam_step: need W <= V <= ld (W=%d V=%d ld=%d)", W, V, ld);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(beam_topw_kernel, dim3(G * W), dim3(kTopwThreads), 0, s, logits, ld, V, W, st->fin, st->cand_logp, st->cand_id);
  UA2_LAUNCH_CHECK();
  hipLaunchKernelGGL(beam_select_kernel, dim3(G), dim3(64), 0, s, W, V, eos, *st, token, token_ld);
  UA2_LAUNCH_CHECK();
  return 0;
}

extern "C" int ua2_beam_step_groups_ngram(const float* logits, int32_t ld, int32_t V, int32_t W, int32_t G, int32_t eos,
                                          const ua2_beam_state* st, const ua2_beam_ngram* ng, int32_t* token, int32_t token_ld, void* stream) {
  if (!ng) return ua2_beam_step_groups(logits, ld, V, W, G, eos, st, token, token_ld, stream);
  UA2_CHECK(ng->n == 0 || (ng->n >= 2 && ng->n <= 16), "ua2_beam_step_groups_ngram: no_repeat_ngram_size must be 0 (off) or in 2..16, got %d", ng->n);
  UA2_CHECK(ng->cap >= 1, "ua2_beam_step_groups_ngram: history capacity %d", ng->cap);
  UA2_CHECK(ng->n == 0 || ng->hist, "ua2_beam_step_groups_ngram: NULL history buffer");
  if (ng->n == 0) return ua2_beam_step_groups(logits, ld, V, W, G, eos, st, token, token_ld, stream);
  if (int rc = check_state(st, W, G, "ua2_beam_step_groups_ngram")) return rc;
  UA2_CHECK(logits && token && token_ld >= 1, "ua2_beam_step_groups_ngram: NULL logits / token buffer");
  UA2_CHECK(V >= W && ld >= V, "ua2_beam_step_groups_ngram: need W <= V <= ld (W=%d V=%d ld=%d)", W, V, ld);
  const size_t ban_bytes = (size_t)((V + 31) / 32) * sizeof(uint32_t);
  UA2_CHECK(ban_bytes <= 48 * 1024, "ua2_beam_step_groups_ngram: a vocabulary of %d does not fit the ban bitmap (48 KB)", V);
  hipStream_t s = (hipStream_t)stream;
  const BeamBan bn{ng->n, ng->cap, ng->hist};
  hipLaunchKernelGGL(beam_topw_ngram_kernel, dim3(G * W), dim3(kTopwThreads), ban_bytes, s, logits, ld, V, W, st->fin, st->len, st->ctrl, bn,
                     st->cand_logp, st->cand_id);
  UA2_LAUNCH_CHECK();
  hipLaunchKernelGGL(beam_select_ngram_kernel, dim3(G), dim3(kSelectNgramThreads), 0, s, W, V, eos, *st, token, token_ld, bn);
  UA2_LAUNCH_CHECK();
  return 0;
}

extern "C" int ua2_beam_step(const float* logits, int32_t ld, int32_t V, int32_t W, int32_t eos, const ua2_beam_state* st,
                             int32_t* token, int32_t token_ld, void* stream) {
  return ua2_beam_step_groups(logits, ld, V, W, 1, eos, st, token, token_ld, stream);
}

extern "C" int ua2_beam_reorder_groups(int32_t W, int32_t G, const int32_t* parent, const int32_t* row_pos, int32_t pos_add,
                                       const ua2_beam_pool* pools, int32_t n_pools, int32_t* const* tables, int32_t n_tables,
                                       int32_t table_rows, int32_t max_pages, void* stream) {
  UA2_CHECK(W >= 1 && W <= kBeamMaxW, "ua2_beam_reorder: beam width must be in 1..%d, got %d", kBeamMaxW, W);
  UA2_CHECK(G >= 1 && G * W <= kBeamMaxRows, "ua2_beam_reorder: %d groups of %d slots: need 1 <= G and G * W <= %d rows", G, W, kBeamMaxRows);
  const int R = G * W;
  UA2_CHECK(row_pos && tables && n_tables >= 1 && n_tables <= 3 && n_pools >= 0 && (n_pools == 0 || pools), "ua2_beam_reorder: bad arguments");
  UA2_CHECK(pos_add == 0 || pos_add == 1, "ua2_beam_reorder: pos_add must be 0 (start) or 1 (end of a frame)");
  UA2_CHECK(table_rows >= 2 * R, "ua2_beam_reorder: %d beam(s) of %d need page tables of %d sequences, got %d", G, W, 2 * R, table_rows);
  UA2_CHECK(max_pages >= 1 && (size_t)W * max_pages * sizeof(int32_t) <= 48 * 1024, "ua2_beam_reorder: max_pages=%d out of range", max_pages);
  UA2_CHECK((int64_t)table_rows * max_pages <= 0x7fffffff, "ua2_beam_reorder: %d x %d pages overflow a page index", table_rows, max_pages);
  BeamTables T{};
  for (int t = 0; t < n_tables; ++t) {
    UA2_CHECK(tables[t] != nullptr, "ua2_beam_reorder: table %d is NULL", t);
    T.t[t] = tables[t];
  }
  for (int t = n_tables; t < 3; ++t) T.t[t] = tables[0];
  hipStream_t s = (hipStream_t)stream;
  if (n_pools > 0) {
    hipLaunchKernelGGL(beam_copy_kernel, dim3(n_pools, R), dim3(256), 0, s, W, R, parent, row_pos, pos_add, pools, T, table_rows, max_pages);
    UA2_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(beam_table_kernel, dim3(G), dim3(256), (size_t)W * max_pages * sizeof(int32_t), s, W, R, parent, row_pos, pos_add, T,
                     n_tables, max_pages);
  UA2_LAUNCH_CHECK();
  return 0;
}

extern "C" int ua2_beam_reorder(int32_t W, const int32_t* parent, const int32_t* row_pos, int32_t pos_add, const ua2_beam_pool* pools,
                                int32_t n_pools, int32_t* const* tables, int32_t n_tables, int32_t table_rows, int32_t max_pages,
                                void* stream) {
  return ua2_beam_reorder_groups(W, 1, parent, row_pos, pos_add, pools, n_pools, tables, n_tables, table_rows, max_pages, stream);
}
