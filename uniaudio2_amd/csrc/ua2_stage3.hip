// Whole-frame executor for Model_stage3's inference methods (llm_models/model_new.py:456-507
// forward_prefix, :568-645 generate_frame) and the generators' per-frame feedback
// (evaluation/tts_task.py:259-280, evaluation/asr_task.py:668-682).
//
// One C call issues every kernel of a frame on the caller's stream; all per-frame state
// (input tokens, step masks, positions, forbid_prefix, sampled ids, the frame log) lives in
// device memory, so the launch sequence is identical from frame to frame and is captured once
// into a hipGraph and replayed: no host round trip between the 350-odd kernels of a frame and
// none between frames (the reference synchronises twice per frame, tts_task.py:261,263).
#include <chrono>
#include <map>
#include <stdlib.h>
#include <string.h>
#include <tuple>
#include <vector>

#include "ua2_common.h"
#include "ua2_linear_common.h"

namespace {
// What a recorded frame bakes in beyond the plan's own state (the setters drop the graphs with theirs).  mode: without its flag bits;
// defer_slots: frame slots of the stash ring, 0 = not deferring; ngram_n: mode 1 only; row_streams, topp_bits, rep_bits, rep_window: top-k frames only (topp_bits 0 / rep_window 0 = off)
struct FrameKey {
  int rows, mode, skip_text, skip_experts, defer_slots, ngram_n, eos, card, topk, temp_bits, cfg_bits, row_streams, topp_bits, rep_bits, rep_window;
  auto tied() const { return std::tie(rows, mode, skip_text, skip_experts, defer_slots, ngram_n, eos, card, topk, temp_bits, cfg_bits, row_streams, topp_bits, rep_bits, rep_window); }
  bool operator<(const FrameKey& o) const { return tied() < o.tied(); }
};
}  // namespace

struct ua2_stage3 {
  ua2_stage3_desc d;
  // deep copies of the per-layer pointer arrays
  std::vector<const void*> ptrs[4][5];
  std::vector<const float*> norms[4][2];
  std::vector<void*> pools[4][2];
  std::vector<const void*> audio_head;
  // scratch carve
  float *xa, *text, *xb, *hbuf, *xg, *hfin, *q, *act, *yattn, *xd, *curr_h;
  float *text_logits, *audio_logits, *pmax_t, *pmax_a;
  int32_t *pidx_t, *pidx_a;
  // deferred text head (UA2_FRAME_DEFER_TEXT_HEAD / ua2_stage3_text_flush): a ring of UA2_DEFER_CAP_ROWS h_final rows (fp32, as lm_head's
  // UA2_PRO_CAST prologue reads them) and the flush launch's own logits, arg-max partials and operand scratch — the per-frame
  // text_logits / pmax_t / gemm_ws hold max_batch (max_rows) rows and keep what the last undeferred frame wrote
  float *defer_stash = nullptr, *defer_logits = nullptr, *defer_pmax = nullptr;
  int32_t* defer_pidx = nullptr;
  void* defer_ws = nullptr;
  size_t defer_ws_bytes = 0;
  void* gemm_ws;               // operand scratch of the large-M linear kernel (max_rows x widest K)
  size_t gemm_ws_bytes;
  void* act_ws;                // packed SwiGLU output handed straight to the down-projection (max_rows x widest intermediate)
  // scaled-norm hand-over of the residual stream (UA2_PRO_SCALED, bf16): every producer of x also writes RNE_bf16(x (.) w_next)
  // for the RMSNorm + Linear that follows (row-major for launches of one row tile, fragment order otherwise) and the
  // per-16-column sums of squares — no prep launch and no in-kernel statistics between a residual update and its consumer
  void *xh, *xpk;
  float* ssq;
  // Projected-embedding table of the depth decoder (round 6; model_new.py:631 self.projection(ci_embed), :640 ci_embed = _embed_audio(i, ci_sample)):
  // row i * va + id = what the projection launch of step i + 1 would write for sample id of codebook i — y (fp32), and under the scaled
  // plan RNE_bf16(y (.) norm_1 of the decoder's layer 0) and the per-16-column sums of squares.  Built at create time by the very launches
  // the frame would run; the frame's arg-max gathers the row instead of launching the GEMV (ua2_misc.hip argmax_gather_kernel).
  float* ptab_y = nullptr;
  void* ptab_h = nullptr;
  float* ptab_ssq = nullptr;
  bool ptab_ho = false;
  // ... and layer 0's q | k | v of the depth decoder for the same rows (step i + 1 runs at position i + 1 whatever the frame: RoPE included):
  // q fp32 [qn], k / v [n_kv * head_size] of the plan dtype — the frame's arg-max writes q into the q buffer and k / v into the caches,
  // and layer 0's q|k|v launch of steps 1 .. n_cb - 1 disappears as well
  float* ptab_q = nullptr;
  void *ptab_k = nullptr, *ptab_v = nullptr;
  float* range_ws = nullptr;   // range-split scratch of the row-invariant 33-64-row down-projections (ua2_linear_args.range_ws): same bits
  size_t range_ws_bytes = 0;
  float* split_ws = nullptr;   // K-slab scratch of the order-free GEMM (ua2_linear_args.split_ws): handed to launches under UA2_SUM_ORDER_FREE only
  size_t split_ws_bytes = 0;
  bool scaled = false;
  // B = 1 greedy frames with both per-id tables: no arg-max launches inside the depth decoder.  The arg-max + table gather after steps
  // 0 .. n_cb - 2 is done by the launch that consumes it, layer 0's O-projection of the next step (ua2_argmax_fold); the arg-max of the
  // LAST step runs inside feedback_kernel's one block (its embedding gather has no reader: there is no further step).  Each consumer
  // redoes a tiny reduction after an ordinary kernel boundary: no flags, no counters, nothing to spin on.  UA2_NO_ARGMAX_FOLD=1, read
  // when the plan is created: off (A/B; one process can hold both plans)
  bool argmax_fold = false;
  // Launches of one row tile of the decode kernel (bf16 plans, up to ua2_gemv_rows_preferred rows): the SwiGLU launch and the trunk's attention
  // hand their result to the down- / O-projection as bf16 rows (ua2_linear_args.y_h / x_h under UA2_PRO_CAST, ua2_attn_args.y_h) — the RNE
  // cast once in the producer instead of in every workgroup of the consumer, and no fp32 row in between.  The rows lie where the many-row
  // form's packed operand would (act_ws, gemm_ws).  Same bits.  UA2_NO_ROW_OPERAND=1, read when the plan is created: off (A/B)
  bool row_operand = false;
  int32_t npart_t, npart_a;
  int32_t topk = 1;            // 1 = greedy (fused arg-max partials); > 1 = ua2_sample_topk
  float temperature = 1.f;
  float top_p = 0.f;           // 0 < top_p < 1 with topk > 1: the samplers run the nucleus tail (ua2_sample_topp); 0 / 1 = off
  // repetition penalty of the samplers (ua2_stage3_set_rep_penalty; rep_window == 0 = off): caller-owned device rings [max_batch][1 + n_cb][rep_window]
  float rep_penalty = 1.f;
  int32_t rep_window = 0;
  int32_t *rep_hist = nullptr, *rep_len = nullptr;
  hipStream_t cap_stream = nullptr;                 // capture-only stream (the caller's may be the null stream, which cannot capture)
  float cfg_scale = 1.f;       // > 1: classifier-free guidance over a (conditional, unconditional) row pair
  int32_t order_free_rows = 0; // > 0 (bf16 plans): GPT launches (trunk and depth decoder) of at least this many rows take UA2_SUM_ORDER_FREE (ua2_stage3_set_order_free_rows)
  // row groups of the next ua2_stage3_trunk call (prefill): the trunk's attention then runs the MFMA flash kernel
  const int32_t *group_rows = nullptr, *group_seq = nullptr, *group_nkeys = nullptr;
  int32_t n_groups = 0, group_q_tiles = 0;
  // n-gram repeat filter of the text-feedback frames (ua2_stage3_set_ngram; ngram_n <= 1 = off): caller-owned device history
  int32_t ngram_n = 0, ngram_fallback = 0, ngram_cap = 0;
  int32_t *ngram_hist = nullptr, *ngram_hist_len = nullptr;
  // per-row sampler streams (ua2_stage3_set_row_streams; row_streams false = off): caller-owned device arrays, [max_batch][2] and [max_batch]
  bool row_streams = false;
  int32_t *row_key = nullptr, *row_draw = nullptr;
  // beam search of the text loop (ua2_stage3_set_beam[_groups]; beam_W == 0 = off): caller-owned device state of beam_G groups of
  // beam_W slots, the K / V pools of the fork
  int32_t beam_W = 0, beam_G = 1, beam_eos = -1, beam_n_pools = 0;
  ua2_beam_state beam{};
  const ua2_beam_pool* beam_pools = nullptr;
  ua2_beam_ngram beam_ng{};                       // the no-repeat-n-gram ban of the attached beam (ua2_stage3_set_beam_ngram; n == 0 = off)
  // a weight's image and its side array (fp8: exponents; 13-bit: base bytes), keyed by the packed bf16 pointer in the two maps below
  struct WImage { const void *q, *side; };
  // fp8 twins of the plan's weights (ua2_stage3_set_w8): packed bf16 pointer -> (fp8 image, exponents); empty = a plain bf16 / fp32 plan
  std::map<const void*, WImage> w8;
  // Lossless 13-bit images (include/ua2hip.h ua2_pack_linear_l13) of the Linear weights a decode frame streams, packed when a bf16 plan is
  // created: packed bf16 pointer -> (image, base bytes), escape-free matrices only.  One allocation, owned by the handle.  The few-row
  // launches the decode kernel serves stream the image instead of the bf16 form — the same bits, 13/16 of the bytes; fp8 twins, when
  // attached, take precedence.  ua2_stage3_set_lossless / UA2_NO_LOSSLESS=1 (read at creation: no images are packed)
  std::map<const void*, WImage> l13;
  void* l13_mem = nullptr;
  bool lossless = false;
  ua2_lossless_info l13_info{};
  std::map<FrameKey, hipGraphExec_t> graphs;
  int env_gen = 0;             // g_ua2_env_gen the graphs were captured under: the launch-time knobs are baked into them (ua2_stage3_frame)
};

namespace {

size_t align4(size_t n) { return (n + 3) & ~(size_t)3; }
void drop_graphs(ua2_stage3* h) {   // the only code that destroys recorded frames: they bake the kernel choice, the weight pointers and every launch argument
  for (auto& kv : h->graphs) (void)hipGraphExecDestroy(kv.second);
  h->graphs.clear();
}
// Launch-time knobs (A/B hooks): read once and again after ua2_debug_refresh_env, which also makes ua2_stage3_frame re-capture.
Ua2EnvInt g_l13_all{"UA2_L13_ALL", 0}, g_of_scaled{"UA2_OF_SCALED", 0}, g_no_scaled{"UA2_NO_SCALED", 0}, g_no_local_fuse{"UA2_NO_LOCAL_FUSE", 0} /* profiles/r1_notes.md */,
    g_no_packed_handover{"UA2_NO_PACKED_HANDOVER", 0}, g_defer_rows{"UA2_DEFER_ROWS", UA2_DEFER_CAP_ROWS}, g_no_defer{"UA2_NO_DEFER_TEXT_HEAD", 0};
// Creation-time knobs: read from the environment when a plan is sized and created, so one process can hold plans of both forms.
struct PlanKnobs { bool range_split, proj_table, qkv_table, scaled, argmax_fold, lossless, row_operand; };
PlanKnobs read_plan_knobs() {
  auto on = [](const char* name) { return getenv(name) != nullptr; };
  return {on("UA2_RANGE_SPLIT"), !on("UA2_NO_PROJ_TABLE"), !on("UA2_NO_QKV_TABLE"), !on("UA2_NO_SCALED"), !on("UA2_NO_ARGMAX_FOLD"), !on("UA2_NO_LOSSLESS"), !on("UA2_NO_ROW_OPERAND")};
}

struct Carve {
  size_t xa, text, xb, hbuf, xg, hfin, q, act, yattn, xd, curr_h, text_logits, audio_logits, pmax_t, pidx_t,
      pmax_a, pidx_a, gemm_ws, gemm_ws_floats, act_ws, xh, xpk, ssq, split, split_floats, ptab_y, ptab_h, ptab_ssq, ptab_rows, ptab_q, ptab_k, ptab_v, ptab_qkv, range, range_floats,
      defer_stash, defer_logits, defer_pmax, defer_pidx, defer_ws, defer_ws_floats, total;
};

Carve carve(const ua2_stage3_desc& d) {
  Carve c;
  const PlanKnobs knobs = read_plan_knobs();
  const size_t R = d.max_rows;
  const ua2_gpt_desc* gs[4] = {&d.und, &d.backbone, &d.gen, &d.decoder};
  size_t C = d.backbone.n_embd, Cd = d.decoder.n_embd, qmax = 0, actmax = 0;
  for (auto g : gs) {
    qmax = std::max(qmax, (size_t)g->n_head * g->head_size);
    actmax = std::max(actmax, (size_t)g->inter);
  }
  size_t off = 0;
  auto take = [&](size_t n) { size_t o = off; off += align4(n); return o; };
  c.xa = take(R * C); c.text = take(R * C); c.xb = take(R * C); c.hbuf = take(R * C); c.xg = take(R * C);
  c.hfin = take(R * C); c.q = take(R * qmax); c.act = take(R * actmax); c.yattn = take(R * qmax);
  c.xd = take(d.max_batch * Cd); c.curr_h = take(d.max_batch * C);
  const size_t npt = (d.vt + 15) / 16, npa = (d.va + 15) / 16, Bm = d.max_batch;
  c.text_logits = take(Bm * d.vt); c.audio_logits = take(Bm * d.n_cb * d.va);
  c.pmax_t = take(Bm * npt); c.pidx_t = take(Bm * npt); c.pmax_a = take(Bm * npa); c.pidx_a = take(Bm * npa);
  c.gemm_ws_floats = ua2_linear_workspace_bytes(d.dtype, (int64_t)R, (int64_t)std::max(std::max(C, Cd), std::max(qmax, actmax))) / sizeof(float);
  c.gemm_ws = take(c.gemm_ws_floats);
  c.act_ws = take(ua2_linear_workspace_bytes(d.dtype, (int64_t)R, (int64_t)actmax) / sizeof(float));
  const size_t Cw = std::max(C, Cd);
  c.xh = take(R * Cw / 2);                                       // bf16 rows
  c.xpk = take(ua2_linear_workspace_bytes(UA2_BF16, (int64_t)R, (int64_t)Cw) / sizeof(float));
  c.ssq = take(R * (Cw / 16 + 1));
  // K-slab scratch for order-free launches of a few hundred to a few thousand rows (tail tiles of a 300-tile grid; whole-grid slabs of
  // the narrow projections at ~1000 rows): plans that can hold such launches only
  c.split_floats = (d.dtype == UA2_BF16 && R >= 256) ? (size_t)16 << 20 : 0;
  c.split = take(c.split_floats);
  // range-split scratch: 16 ranges x 64 rows x the widest down-projection output, plans that can hold 33-64-row decode batches
  c.range_floats = (d.dtype == UA2_BF16 && d.max_batch >= 33 && knobs.range_split) ? (size_t)16 * 64 * std::max(C, Cd) : 0;   // opt-in: measured slower in the frame (ua2_skinny.hip rsplit_*)
  c.range = take(c.range_floats);
  // projected-embedding table: (n_cb - 1) * va rows of [Cd fp32 | Cd bf16 | Cd / 16 fp32] (the last codebook's sample is never projected);
  // UA2_NO_PROJ_TABLE=1 keeps the per-step projection launch (A/B, and plans that cannot spare ~1.1 GB at the released sizes)
  c.ptab_rows = (d.n_cb > 1 && d.va > 0 && d.projection && d.audio_emb && Cd % 32 == 0 && knobs.proj_table) ? (size_t)(d.n_cb - 1) * d.va : 0;
  c.ptab_y = take(c.ptab_rows * Cd);
  c.ptab_h = take(c.ptab_rows * Cd / 2);
  c.ptab_ssq = take(c.ptab_rows * (Cd / 16));
  {   // q | k | v rows of the decoder's layer 0 (UA2_NO_QKV_TABLE=1: the projection table alone)
    const ua2_gpt_desc& g = d.decoder;
    const size_t esz = d.dtype == UA2_BF16 ? 2 : 4, kvw = (size_t)g.n_kv * g.head_size;
    c.ptab_qkv = (c.ptab_rows && g.n_layer > 0 && d.n_cb <= UA2_PAGE && (g.n_head * g.head_size) % 4 == 0 && (g.head_size * esz) % 16 == 0 &&
                  knobs.qkv_table) ? 1 : 0;
    const size_t rows = c.ptab_qkv ? c.ptab_rows : 0;
    c.ptab_q = take(rows * g.n_head * g.head_size);
    c.ptab_k = take((rows * kvw * esz + 3) / 4);
    c.ptab_v = take((rows * kvw * esz + 3) / 4);
  }
  // deferred text head: UA2_DEFER_CAP_ROWS rows of h_final, of lm_head's logits and partials, and the many-row kernels' packed operand
  c.defer_stash = take((size_t)UA2_DEFER_CAP_ROWS * C); c.defer_logits = take((size_t)UA2_DEFER_CAP_ROWS * d.vt);
  c.defer_pmax = take((size_t)UA2_DEFER_CAP_ROWS * npt); c.defer_pidx = take((size_t)UA2_DEFER_CAP_ROWS * npt);
  c.defer_ws_floats = ua2_linear_workspace_bytes(d.dtype, UA2_DEFER_CAP_ROWS, (int64_t)C) / sizeof(float);
  c.defer_ws = take(c.defer_ws_floats);
  c.total = off;
  return c;
}

// every ua2_linear of the executor may use the large-M kernel (same results, weights read once per 128 rows)
ua2_linear_args fresh_args(const ua2_stage3* h) {
  ua2_linear_args a;
  memset(&a, 0, sizeof(a));
  a.workspace = h->gemm_ws; a.workspace_bytes = h->gemm_ws_bytes;
  return a;
}
ua2_kv_geom kv_geom(const ua2_stage3* h, int gi, const ua2_gpt_desc& g, int l) {   // of layer l of GPT gi
  ua2_kv_geom kv{};                      // ring_pages = 0: the LM's caches are linear
  kv.k_pool = h->pools[gi][0][l]; kv.v_pool = h->pools[gi][1][l]; kv.page_table = g.page_table;
  kv.max_pages = g.max_pages; kv.n_kv = g.n_kv; kv.n_head = g.n_head; kv.head_size = g.head_size;
  return kv;
}

// Every Linear of the frame goes through here: with fp8 twins attached, a launch whose weight(s) all have one hands them to the launcher,
// which streams them where the decode kernel serves the launch (up to 5 rows) or the weights-stationary kernel does (6 ..
// UA2_SKINNY_W8_MAX_ROWS rows of a released Linear shape: decode frames, and prefill chunks that small) and reads a.w0 / a.w1 — the bf16
// forms of W' — everywhere else.  Same bits either way.
// The one launch form of the frame that the image makes clearly LONGER (kernel trace, profiles/lossless_weights.md): a single 16-chunk burst
// per wave on a grid well under the CU count — the depth decoder's down-projection, 8192 -> 2048 on 128 workgroups, 9.6 -> 10.4 us, 32
// times per frame.  Its time is one workgroup's latency chain, which the decode lengthens, not the stream.  It keeps bf16 (the same bits);
// the trunk's down-projection (192 workgroups) gains and keeps its image.  UA2_L13_ALL=1: every served launch (A/B).
bool l13_pays(const ua2_linear_args& a) {
  if (g_l13_all.get()) return true;
  const ua2_gemv_geometry g = ua2_pick_gemv_geometry(a.dtype, a.N, a.K, a.epilogue == UA2_EPI_SWIGLU ? 2 : 1);
  return !(g.cpw == 16 && ua2_ceil_div(a.N, 16) < 160);
}

// The images the plan offers a launch: fp8 twins when attached (they take precedence), otherwise the 13-bit images where the decode kernel
// serves the launch on them and they pay.  false: none, or not of every weight the launch reads.
bool offered(const ua2_stage3* h, const ua2_linear_args& a, Ua2Weights& w) {
  const bool fp8 = !h->w8.empty();
  if (!fp8 && !(h->lossless && !a.x_packed && !a.fold.part_max && a.M <= ua2_gemv_rows_preferred(a.dtype, a.K) && ua2_gemv_l13_ok(a) && l13_pays(a)))
    return false;
  const auto& images = fp8 ? h->w8 : h->l13;
  w.form = fp8 ? UA2_W_FP8 : UA2_W_L13;
  const auto i0 = images.find(a.w0);
  if (i0 == images.end()) return false;
  w.img.q0 = i0->second.q; w.img.e0 = i0->second.side;
  if (a.epilogue == UA2_EPI_SWIGLU) {
    const auto i1 = images.find(a.w1);
    if (i1 == images.end()) return false;
    w.img.q1 = i1->second.q; w.img.e1 = i1->second.side;
  }
  return true;
}

int lin(const ua2_stage3* h, const ua2_linear_args& a, hipStream_t s) {
  Ua2Weights w;
  return ua2_linear_launch(a, s, offered(h, a, w) ? &w : nullptr);
}

// local = the depth decoder: positions < kLocalCtx, short-context attention (fused into the O-projection when R == 1)
// hand-over helpers: which form the consumer of a C-wide row reads (row-major: its launch is one row tile of the decode kernel)
struct Handover {
  ua2_stage3* h; int R, C; bool rows_h;
  Handover(ua2_stage3* h_, int R_, int C_) : h(h_), R(R_), C(C_), rows_h(R_ <= ua2_gemv_rows_preferred(h_->d.dtype, C_)) {}
  void consume(ua2_linear_args& a) const {
    a.prologue = UA2_PRO_SCALED; a.x_ssq = h->ssq; a.x = nullptr; a.norm_w = nullptr;
    if (rows_h) { a.x_h = h->xh; a.ldh = C; } else { a.x_packed = h->xpk; }
  }
  void produce(ua2_linear_args& a, const float* norm_w_next) const {
    if (!norm_w_next) return;
    a.y_norm_w = norm_w_next; a.y_ssq = h->ssq;
    if (rows_h) { a.y_h = h->xh; a.ldh = C; } else { a.y_packed = h->xpk; }
  }
  ua2_handover rowwise(const float* norm_w_next) const {
    ua2_handover ho{};
    ho.norm_w = norm_w_next; ho.ssq = h->ssq;
    if (rows_h) { ho.h = h->xh; ho.ldh = C; } else { ho.packed = h->xpk; }
    return ho;
  }
};

// The three head Linears are built here and nowhere else: the decode frame, the deferred flush and teacher-forced scoring share them, so
// a row carries the same bits whichever of them computed it.
// text_logits = lm_head(x) with the arg-max partials (model_new.py:617); ws: the launch's operand scratch (the flush has its own)
ua2_linear_args lm_head_args(const ua2_stage3* h, int M, const float* x, float* y, float* part_max, int32_t* part_idx, int sum_order, void* ws, size_t ws_bytes) {
  const ua2_stage3_desc& d = h->d;
  ua2_linear_args a = fresh_args(h);
  a.workspace = ws; a.workspace_bytes = ws_bytes;
  a.dtype = d.dtype; a.prologue = UA2_PRO_CAST; a.epilogue = UA2_EPI_STORE; a.sum_order = sum_order;
  a.M = M; a.N = d.vt; a.K = d.backbone.n_embd; a.x = x; a.ldx = a.K; a.w0 = d.lm_head; a.y = y; a.ldy = d.vt;
  a.part_max = part_max; a.part_idx = part_idx;
  return a;
}
// xd = projection(curr), handed over to the decoder's layer-0 norm under `scaled` (model_new.py:631)
ua2_linear_args projection_args(ua2_stage3* h, int R, const float* curr, int order, bool scaled) {
  const int C = h->d.backbone.n_embd, Cd = h->d.decoder.n_embd;
  ua2_linear_args a = fresh_args(h);
  a.dtype = h->d.dtype; a.prologue = UA2_PRO_CAST; a.epilogue = UA2_EPI_STORE; a.sum_order = order;
  a.M = R; a.N = Cd; a.K = C; a.x = curr; a.ldx = C; a.w0 = h->d.projection; a.y = h->xd; a.ldy = Cd;
  if (scaled) Handover(h, R, Cd).produce(a, h->norms[3][0][0]);
  return a;
}
// audio_logits[:, i] = audio_head[i](ln_f(xd)), arg-max partials over the columns >= forbid[m] (NULL: all) (model_new.py:630-641)
ua2_linear_args audio_head_args(ua2_stage3* h, int R, int i, int order, bool scaled, const int32_t* forbid) {
  const ua2_stage3_desc& d = h->d;
  const int Cd = d.decoder.n_embd;
  ua2_linear_args a = fresh_args(h);
  a.dtype = d.dtype; a.prologue = UA2_PRO_NORM; a.epilogue = UA2_EPI_STORE; a.sum_order = order;
  a.M = R; a.N = d.va; a.K = Cd; a.x = h->xd; a.ldx = Cd; a.norm_w = d.decoder.ln_f; a.eps = d.decoder.eps;
  a.w0 = h->audio_head[i]; a.y = h->audio_logits + (size_t)i * d.va; a.ldy = d.n_cb * d.va;
  a.part_max = h->pmax_a; a.part_idx = h->pidx_a; a.forbid = forbid;
  if (scaled) Handover(h, R, Cd).consume(a);
  return a;
}
// launches of R rows under the plan's order-free opt-in (ua2_stage3_set_order_free_rows; bf16 plans)
bool order_free(const ua2_stage3* h, int R) { return h->d.dtype == UA2_BF16 && h->order_free_rows > 0 && R >= h->order_free_rows; }
// ... run the scaled hand-over whatever the plan's decode form (the order-free GEMM's epilogues carry it at any row count, and the
// two prep launches per layer go: profiles/r6_notes.md); the widths must be whole bf16 chunks as for h->scaled
bool order_free_scaled(const ua2_stage3* h, int R, bool prefill = false) {
  // Measured (profiles/r6_notes.md §3): the hand-over through ua2_gemm2.hip's epilogues does not pay in the frame — config-3 prefill
  // 46.43 (prep launches) vs 46.45 ms, B = 1024 decode 22.99 vs 24.55 ms per frame — and in prefill it doubles the distance to the
  // pinned plan (two different bf16 forms of the norm).  Default 0 = never; UA2_OF_SCALED = 1 decode frames, 2 prefill chunks too.
  if (g_of_scaled.get() < (prefill ? 2 : 1)) return false;
  return order_free(h, R) && h->d.backbone.n_embd % 32 == 0 && h->d.decoder.n_embd % 32 == 0 && !g_no_scaled.set();
}

// A one-row-tile GEMV (lm_head) whose column tiles travel on the idle CUs of a GPT's small launches (ua2_gemv.hip gemv_rider_kernel).
// Host kinds: 0 = q|k|v, 1 = o-projection, 2 = down-projection.  Tiles are dealt in launch order in proportion to a weight per
// kind, the last carrying launch takes whatever is left: every tile is computed exactly once per frame whatever the weights.
struct RiderPlan {
  ua2_linear_args r;
  int ntiles = 0, next = 0;
  double w[3] = {0, 0, 0}, wleft = 0;
  bool ok[3] = {false, false, false};
  void take(int kind, int& t0, int& t1) {
    const int left = ntiles - next;
    int n = (wleft <= w[kind] * 1.0001) ? left : (int)(left * (w[kind] / wleft) + 0.5);
    n = std::max(0, std::min(n, left));
    t0 = next; t1 = next + n; next = t1; wleft -= w[kind];
  }
};

// final_norm_w: weight of the RMSNorm + Linear that consumes this GPT's OUTPUT through UA2_PRO_SCALED (the depth decoder's
// ln_f in front of audio_head), or NULL (the trunk GPTs end in ua2_rmsnorm_blend, which reads the fp32 stream).
// With h->scaled the caller has already handed over x for layer 0 (embed_frame / rmsnorm_blend / the projection's epilogue).
// rider: the launches of this GPT that can (RiderPlan::ok) carry their share of the rider's column tiles.  qkv0_given / fold0: explained where layer 0 reads them.
struct GptRun { bool local, grouped, scaled, qkv0_given; const float* final_norm_w; RiderPlan* rider; const ua2_argmax_fold* fold0; };
int run_gpt(ua2_stage3* h, int gi, const ua2_gpt_desc& g, float* x, int R, const int32_t* row_pos, const int32_t* row_seq, hipStream_t s,
            const GptRun& o) {
  auto launch = [&](const ua2_linear_args& a, int kind) -> int {
    if (RiderPlan* rp = o.rider; rp && rp->ok[kind]) {
      int t0, t1;
      rp->take(kind, t0, t1);
      const int rc = ua2_gemv_launch_with_rider(a, rp->r, t0, t1, s);
      UA2_CHECK(rc <= 0, "ua2_stage3: launch kind %d cannot carry its rider (plan / launch mismatch)", kind);
      return rc;
    }
    return lin(h, a, s);
  };
  const int dt = h->d.dtype;
  const int C = g.n_embd, qn = g.n_head * g.head_size, nqkv = (g.n_head + 2 * g.n_kv) * g.head_size;
  const Handover ho(h, R, C);
  // ua2_stage3_set_order_free_rows: many-row launches of the trunk on the 256-row-tile kernel (one chain over K); the launcher falls
  // back to the invariant kernels for anything outside that kernel's forms (scaled hand-over, small grids)
  const int order = order_free(h, R) ? UA2_SUM_ORDER_FREE : UA2_SUM_ORDER_INVARIANT;
  auto free_scratch = [&](ua2_linear_args& a) {           // K slabs are an order-free option: the invariant launches never see the scratch
    if (order == UA2_SUM_ORDER_FREE) { a.split_ws = h->split_ws; a.split_ws_bytes = h->split_ws_bytes; }
  };
  for (int l = 0; l < g.n_layer; ++l) {
    const ua2_kv_geom kv = kv_geom(h, gi, g, l);
    ua2_linear_args a = fresh_args(h);
    a.dtype = dt; a.prologue = UA2_PRO_NORM; a.epilogue = UA2_EPI_QKV_ROPE;
    a.M = R; a.N = nqkv; a.K = C; a.x = x; a.ldx = C; a.norm_w = h->norms[gi][0][l]; a.eps = g.eps;
    a.w0 = h->ptrs[gi][0][l]; a.row_pos = row_pos; a.row_seq = row_seq; a.rope_cos = g.rope_cos;
    a.rope_sin = g.rope_sin; a.q_out = h->q; a.kv = kv;
    if (o.scaled) ho.consume(a);
    a.sum_order = order;
    if (!(o.qkv0_given && l == 0))        // depth decoder, steps >= 1: the previous step's arg-max wrote layer 0's q / k / v from the table
      if (int rc = launch(a, 0)) return rc;

    const bool fuse_attn = o.local && R == 1 && !g_no_local_fuse.set();
    // more than one row tile: the consumer runs a many-row kernel, so its producer writes the packed operand
    // directly and the consumer's prep launch disappears (same bits: the same RNE cast either way)
    const bool no_handover = g_no_packed_handover.set();   // A/B hook
    const int kc = dt == UA2_BF16 ? 32 : 16;
    const bool pack_o = !no_handover && R > ua2_gemv_rows_preferred(dt, qn) && qn % kc == 0;
    const bool pack_act = !no_handover && R > ua2_gemv_rows_preferred(dt, g.inter) && g.inter % kc == 0;
    // one row tile of the decode kernel: the producer writes the bf16 rows its consumer stages (h->row_operand); never an order-free launch
    const bool rows_ok = h->row_operand && order == UA2_SUM_ORDER_INVARIANT;
    const bool rows_o = rows_ok && !o.local && !(o.grouped && h->n_groups > 0) && R <= ua2_gemv_rows_preferred(dt, qn) && qn % 32 == 0;   // the trunk's row-by-row attention
    const bool rows_act = rows_ok && R <= ua2_gemv_rows_preferred(dt, g.inter) && g.inter % 32 == 0;
    if (!fuse_attn) {
      ua2_attn_args at;
      memset(&at, 0, sizeof(at));
      at.dtype = dt; at.R = R; at.q = h->q; at.row_pos = row_pos; at.row_seq = row_seq; at.kv = kv;
      if (pack_o) at.y_packed = h->gemm_ws;
      else if (rows_o) { at.y_h = h->gemm_ws; at.ldh = qn; }
      else at.y = h->yattn;
      if (o.grouped && !o.local && h->n_groups > 0) {
        at.group_rows = h->group_rows; at.group_seq = h->group_seq; at.group_nkeys = h->group_nkeys;
        at.n_groups = h->n_groups; at.group_q_tiles = h->group_q_tiles;
      }
      if (int rc = o.local ? ua2_attn_local_launch(at, s) : ua2_attn_launch(at, s)) return rc;
    }
    a = fresh_args(h);
    a.dtype = dt; a.prologue = fuse_attn ? UA2_PRO_LOCAL_ATTN : UA2_PRO_CAST; a.epilogue = UA2_EPI_RESIDUAL;
    a.M = R; a.N = C; a.K = qn; a.x = fuse_attn ? h->q : h->yattn; a.ldx = qn;
    a.w0 = h->ptrs[gi][1][l]; a.y = x; a.ldy = C; a.resid = x; a.ldr = C;
    if (fuse_attn) { a.row_pos = row_pos; a.row_seq = row_seq; a.kv = kv; }
    if (o.fold0 && l == 0) {            // the previous step's arg-max and table gathers happen inside this launch (ua2_argmax_fold)
      UA2_CHECK(fuse_attn && o.qkv0_given, "ua2_stage3: the arg-max fold needs the fused local attention and the q | k | v table");
      a.fold = *o.fold0;
    }
    if (pack_o && !fuse_attn) a.x_packed = h->gemm_ws;
    if (rows_o) { a.x = nullptr; a.x_h = h->gemm_ws; }
    if (o.scaled) ho.produce(a, h->norms[gi][1][l]);              // x after attention -> norm_2 + fc_1 / fc_2
    a.sum_order = order; free_scratch(a);
    if (int rc = launch(a, 1)) return rc;

    a = fresh_args(h);
    a.dtype = dt; a.prologue = UA2_PRO_NORM; a.epilogue = UA2_EPI_SWIGLU;
    a.M = R; a.N = g.inter; a.K = C; a.x = x; a.ldx = C; a.norm_w = h->norms[gi][1][l]; a.eps = g.eps;
    a.w0 = h->ptrs[gi][2][l]; a.w1 = h->ptrs[gi][3][l]; a.ldy = g.inter;
    if (pack_act) a.y_packed = h->act_ws;
    else if (rows_act) a.y_h = h->act_ws;
    else a.y = h->act;
    if (o.scaled) ho.consume(a);
    a.sum_order = order;
    if (int rc = lin(h, a, s)) return rc;

    a = fresh_args(h);
    a.dtype = dt; a.prologue = UA2_PRO_CAST; a.epilogue = UA2_EPI_RESIDUAL;
    a.M = R; a.N = C; a.K = g.inter; a.x = h->act; a.ldx = g.inter; a.w0 = h->ptrs[gi][4][l];
    a.y = x; a.ldy = C; a.resid = x; a.ldr = C;
    if (pack_act) a.x_packed = h->act_ws;
    if (rows_act) { a.x = nullptr; a.x_h = h->act_ws; }
    if (o.scaled) ho.produce(a, l + 1 < g.n_layer ? h->norms[gi][0][l + 1] : o.final_norm_w);   // x after the MLP -> the next layer's norm_1 + qkv
    a.sum_order = order; free_scratch(a);
    a.range_ws = h->range_ws; a.range_ws_bytes = h->range_ws_bytes;      // 33-64 rows, K = 8192: one K range per workgroup + an in-order combine (same bits)
    if (int rc = launch(a, 2)) return rc;
  }
  return 0;
}

__global__ void bump_kernel(int32_t* c) { c[0] += 1; }

__global__ void feedback_kernel(int R, int ncb, int mode, int reason_eos, int reason_card, int log_frames,
                                int max_rows, int32_t* __restrict__ tokens, uint8_t* __restrict__ mask,
                                int32_t* __restrict__ row_pos, int32_t* __restrict__ forbid,
                                int32_t* out, int32_t* __restrict__ log, int32_t* counters, int no_text,
                                const float* __restrict__ hfin, float* __restrict__ stash, int C, int cap_frames,
                                int am_npart, int am_limit, const float* __restrict__ am_pmax, const int32_t* __restrict__ am_pidx) {
  const int w = ncb + 1;
  // am_npart > 0 (R == 1, greedy, heads_impl left the launch out): the last codebook step's arg-max over audio_head's partials, as
  // argmax_embed_kernel takes it — the same 256 threads, candidates, order and tie / all-NaN rules (ua2_row_token) — into out[ncb]
  if (am_npart > 0) {
    __shared__ float sv[4];
    __shared__ int si[4];
    __shared__ int tok_s;
    float bv = -INFINITY;
    int bi = UA2_TOK_NONE;
    for (int p = threadIdx.x; p < am_npart; p += blockDim.x) {
      const float v = am_pmax[p];
      const int i = am_pidx[p];
      if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
    }
    const int tok = ua2_row_token(bv, bi, am_limit, sv, si, &tok_s, [&] {
      int lo = UA2_TOK_NONE;
      for (int p = threadIdx.x; p < am_npart; p += blockDim.x) lo = min(lo, am_pidx[p]);
      return lo;
    });
    if (threadIdx.x == 0) out[ncb] = tok;
    __syncthreads();                  // the row loop below reads it
  }
  const int frame = counters[0];
  // UA2_FRAME_DEFER_TEXT_HEAD, frames of a few rows: this frame's h_final rows go into slot frame % cap_frames of the stash ring (the
  // slot is a device value — the frame is a replayed graph).  cap_frames * R rows fit the ring (checked by the launcher); C % 4 == 0.
  if (stash && frame >= 0) {
    const size_t n4 = (size_t)R * C / 4;
    float4* dst = reinterpret_cast<float4*>(stash + (size_t)(frame % cap_frames) * R * C);
    for (size_t i = threadIdx.x; i < n4; i += blockDim.x) dst[i] = reinterpret_cast<const float4*>(hfin)[i];
  }
  const bool audio_fb = (mode == 0 || mode == 2);
  for (int m = threadIdx.x; m < R; m += blockDim.x) {
    const int32_t* own = out + (size_t)m * w;
    if (frame < log_frames)
      for (int j = 0; j < w; ++j)   // text loop: no audio ids exist; UA2_FRAME_SKIP_TEXT_HEAD: no text id exists (logged as -1)
        log[((size_t)frame * max_rows + m) * w + j] = (j == 0 && no_text) ? -1 : ((audio_fb || j == 0) ? own[j] : 0);
    // mode 2 (classifier-free-guidance pairs, tts_task.py:256-258,278-280): every row continues from the sample of
    // its pair's conditional row (rows 2p, 2p + 1; the reference has the one pair)
    const int32_t* o = (mode == 2) ? out + (size_t)(m & ~1) * w : own;
    bool all_reason_eos = true;
    for (int i = 0; i < ncb; ++i) {
      all_reason_eos = all_reason_eos && (o[1 + i] == reason_eos);
      tokens[(size_t)m * w + i] = audio_fb ? o[1 + i] : 0;
      mask[(size_t)m * w + i] = audio_fb ? 1 : 0;
    }
    tokens[(size_t)m * w + ncb] = no_text ? 0 : o[0];           // fed back under a zero mask in the audio loop: any valid id
    mask[(size_t)m * w + ncb] = audio_fb ? 0 : 1;
    row_pos[m] += 1;
    if (audio_fb && all_reason_eos) forbid[m] = reason_card;  // tts_task.py:263-266
  }
  __syncthreads();
  if (threadIdx.x == 0) counters[0] = frame + 1;
}

// the same stash for frames of more rows, as a launch of its own in front of the feedback (which advances counters[0]): one block per row
__global__ void stash_rows_kernel(const float* __restrict__ hfin, float* __restrict__ stash, int R, int C, int cap_frames, const int32_t* __restrict__ counters) {
  const int frame = counters[0], m = blockIdx.x;
  if (frame < 0 || m >= R) return;
  const float4* src = reinterpret_cast<const float4*>(hfin + (size_t)m * C);
  float4* dst = reinterpret_cast<float4*>(stash + ((size_t)(frame % cap_frames) * R + m) * C);
  for (int i = threadIdx.x; i < C / 4; i += blockDim.x) dst[i] = src[i];
}

// ua2_stage3_text_flush: row r = j * R + m of the flush launch is sequence m of frame frame0 + j.  The arg-max over lm_head's
// per-16-column partials, as argmax_embed_kernel takes it (same candidates, same order, same tie and all-NaN rules: ua2_row_token),
// written into the text column of that frame's log row.
__global__ __launch_bounds__(256) void text_flush_kernel(int R, int n_part, int limit, const float* __restrict__ pmax, const int32_t* __restrict__ pidx,
                                                         int32_t* __restrict__ log, int frame0, int log_frames, int max_rows, int w) {
  __shared__ float sv[4];
  __shared__ int si[4];
  __shared__ int tok_s;
  const int r = blockIdx.x, j = r / R, m = r - j * R;
  float bv = -INFINITY;
  int bi = UA2_TOK_NONE;
  for (int p = threadIdx.x; p < n_part; p += blockDim.x) {
    const float v = pmax[(size_t)r * n_part + p];
    const int i = pidx[(size_t)r * n_part + p];
    if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
  }
  const int tok = ua2_row_token(bv, bi, limit, sv, si, &tok_s, [&] {
    int lo = UA2_TOK_NONE;
    for (int p = threadIdx.x; p < n_part; p += blockDim.x) lo = min(lo, pidx[(size_t)r * n_part + p]);
    return lo;
  });
  if (threadIdx.x == 0 && frame0 + j < log_frames) log[((size_t)(frame0 + j) * max_rows + m) * w] = tok;
}

// rows of the stash ring in use: UA2_DEFER_ROWS=n (1 .. UA2_DEFER_CAP_ROWS, the default) for tests and sweeps; UA2_NO_DEFER_TEXT_HEAD=1: none (A/B)
int defer_rows() {
  if (g_no_defer.get() == 1) return 0;
  return std::min(std::max(g_defer_rows.get(), 1), (int)UA2_DEFER_CAP_ROWS);
}

// table rows row0 .. row0 + n - 1: position of the step that consumes row g = i * va + id is i + 1; page table of the scratch cache: row r -> page r
__global__ void ptab_pos_kernel(int32_t* __restrict__ out, int n, long long row0, int va) {
  const int r = threadIdx.x;
  if (r < 64) { out[r] = r < n ? (int)((row0 + r) / va) + 1 : 0; out[64 + r] = r; }
}

// rows [row0, row0 + n) of the embedding table (plan dtype) as fp32 rows: the operand of the table-building projection launches
template <int DT>
__global__ void emb_rows_f32_kernel(const void* __restrict__ emb, long long row0, int n, int C, float* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)n * C; i += (size_t)gridDim.x * blockDim.x)
    out[i] = load_elem<DT>(emb, (size_t)row0 * C + i);
}

// Images of every Linear weight a decode frame streams (the three trunk GPTs, the depth decoder, projection, the audio heads; not lm_head:
// the flush's many-row kernel reads it).  Null stream, once per plan; the escape counts come back in one copy.  A plan that cannot get the
// memory runs without images (the stats say so): the same bits either way.
int build_l13(ua2_stage3* h) {
  const ua2_stage3_desc& d = h->d;
  struct Mat { const void* w; int64_t N, K; int64_t per_frame; size_t img_off, base_off; };
  std::vector<Mat> mats;
  std::map<const void*, int> seen;
  auto add = [&](const void* w, int64_t N, int64_t K, int64_t per_frame) {
    if (!w || N <= 0 || K <= 0) return;
    const auto it = seen.find(w);
    if (it != seen.end()) { mats[it->second].per_frame += per_frame; return; }
    seen[w] = (int)mats.size();
    mats.push_back(Mat{w, N, K, per_frame, 0, 0});
  };
  const ua2_gpt_desc* gs[4] = {&d.und, &d.backbone, &d.gen, &d.decoder};
  for (int gi = 0; gi < 4; ++gi) {
    const ua2_gpt_desc& g = *gs[gi];
    const int64_t C = g.n_embd, qn = (int64_t)g.n_head * g.head_size, nqkv = (int64_t)(g.n_head + 2 * g.n_kv) * g.head_size;
    const int64_t pf = gi == 3 ? std::max(d.n_cb, 1) : 1;          // the depth decoder runs once per codebook
    for (int l = 0; l < g.n_layer; ++l) {
      add(h->ptrs[gi][0][l], nqkv, C, pf); add(h->ptrs[gi][1][l], C, qn, pf);
      add(h->ptrs[gi][2][l], g.inter, C, pf); add(h->ptrs[gi][3][l], g.inter, C, pf); add(h->ptrs[gi][4][l], C, g.inter, pf);
    }
  }
  add(d.projection, d.decoder.n_embd, d.backbone.n_embd, 1);
  for (const void* p : h->audio_head) add(p, d.va, d.decoder.n_embd, 1);
  ua2_lossless_info& info = h->l13_info;
  info = ua2_lossless_info{};
  size_t off = 0;
  auto take = [&](size_t n) { const size_t o = off; off += (n + 255) & ~(size_t)255; return o; };
  for (Mat& m : mats) {
    const size_t ib = ua2_packed_bytes_l13(m.N, m.K);
    if (!ib) continue;
    m.img_off = take(ib); m.base_off = take((size_t)((m.N + 15) / 16));
  }
  const size_t esc_off = take(mats.size() * sizeof(int32_t));
  const auto t0 = std::chrono::steady_clock::now();
  bool have = !mats.empty() && hipMalloc(&h->l13_mem, off) == hipSuccess;
  if (!have) { (void)hipGetLastError(); h->l13_mem = nullptr; }
  std::vector<int32_t> esc(mats.size(), 0);
  if (have) {
    char* base = static_cast<char*>(h->l13_mem);
    for (size_t i = 0; i < mats.size(); ++i) {
      const Mat& m = mats[i];
      if (!ua2_packed_bytes_l13(m.N, m.K)) continue;
      if (int rc = ua2_pack_linear_l13(m.w, m.N, m.K, base + m.img_off, reinterpret_cast<uint8_t*>(base + m.base_off),
                                       reinterpret_cast<int32_t*>(base + esc_off) + i, nullptr)) return rc;
    }
    UA2_HIP(hipMemcpy(esc.data(), base + esc_off, esc.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    info.extra_device_bytes = (int64_t)off;
  }
  for (size_t i = 0; i < mats.size(); ++i) {
    const Mat& m = mats[i];
    const int64_t bf = (int64_t)ua2_packed_elems(UA2_BF16, m.N, m.K) * 2, ib = (int64_t)ua2_packed_bytes_l13(m.N, m.K);
    const bool ok = have && ib && esc[i] == 0;
    info.bf16_bytes_per_frame += bf * m.per_frame;
    info.image_bytes_per_frame += (ok ? ib + (m.N + 15) / 16 : bf) * m.per_frame;
    if (ok) {
      ++info.with_image;
      h->l13[m.w] = ua2_stage3::WImage{static_cast<char*>(h->l13_mem) + m.img_off, static_cast<char*>(h->l13_mem) + m.base_off};
    } else {
      ++info.without_image;
      if (have && ib) ++info.with_escapes;
    }
  }
  info.build_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  h->lossless = !h->l13.empty();
  return 0;
}

}  // namespace

extern "C" size_t ua2_stage3_scratch_floats(const ua2_stage3_desc* d) { return d ? carve(*d).total : 0; }

extern "C" int ua2_stage3_create(const ua2_stage3_desc* d, ua2_stage3** out) {
  UA2_CHECK(d && out, "ua2_stage3_create: NULL argument");
  const Carve c = carve(*d);
  const PlanKnobs knobs = read_plan_knobs();
  UA2_CHECK(d->scratch && d->scratch_floats >= c.total, "ua2_stage3_create: scratch too small (%zu < %zu floats)",
            d->scratch_floats, c.total);
  UA2_CHECK(d->max_batch > 0 && d->max_batch <= d->max_rows, "ua2_stage3_create: need 0 < max_batch <= max_rows");
  UA2_CHECK(d->und.n_embd == d->backbone.n_embd && d->gen.n_embd == d->backbone.n_embd,
            "ua2_stage3_create: expert width must equal backbone width (model_new.py:607,613)");
  ua2_stage3* h = new ua2_stage3();
  h->d = *d;
  const ua2_gpt_desc* gs[4] = {&d->und, &d->backbone, &d->gen, &d->decoder};
  ua2_gpt_desc* hs[4] = {&h->d.und, &h->d.backbone, &h->d.gen, &h->d.decoder};
  for (int gi = 0; gi < 4; ++gi) {
    const ua2_gpt_desc& g = *gs[gi];
    const void* const* src[5] = {g.qkv, g.proj, g.fc1, g.fc2, g.mlp_proj};
    for (int k = 0; k < 5; ++k) h->ptrs[gi][k].assign(src[k], src[k] + g.n_layer);
    h->norms[gi][0].assign(g.norm1, g.norm1 + g.n_layer);
    h->norms[gi][1].assign(g.norm2, g.norm2 + g.n_layer);
    h->pools[gi][0].assign(g.k_pool, g.k_pool + g.n_layer);
    h->pools[gi][1].assign(g.v_pool, g.v_pool + g.n_layer);
    hs[gi]->qkv = hs[gi]->proj = hs[gi]->fc1 = hs[gi]->fc2 = hs[gi]->mlp_proj = nullptr;  // use the copies
  }
  h->audio_head.assign(d->audio_head, d->audio_head + d->n_cb);
  float* b = d->scratch;
  h->xa = b + c.xa; h->text = b + c.text; h->xb = b + c.xb; h->hbuf = b + c.hbuf; h->xg = b + c.xg;
  h->hfin = b + c.hfin; h->q = b + c.q; h->act = b + c.act; h->yattn = b + c.yattn;
  h->xd = b + c.xd; h->curr_h = b + c.curr_h; h->text_logits = b + c.text_logits;
  h->audio_logits = b + c.audio_logits; h->pmax_t = b + c.pmax_t; h->pidx_t = (int32_t*)(b + c.pidx_t);
  h->pmax_a = b + c.pmax_a; h->pidx_a = (int32_t*)(b + c.pidx_a);
  h->gemm_ws = b + c.gemm_ws; h->gemm_ws_bytes = c.gemm_ws_floats * sizeof(float);
  h->act_ws = b + c.act_ws;
  h->xh = b + c.xh; h->xpk = b + c.xpk; h->ssq = b + c.ssq;
  h->split_ws = c.split_floats ? b + c.split : nullptr; h->split_ws_bytes = c.split_floats * sizeof(float);
  h->defer_stash = b + c.defer_stash; h->defer_logits = b + c.defer_logits; h->defer_pmax = b + c.defer_pmax;
  h->defer_pidx = (int32_t*)(b + c.defer_pidx); h->defer_ws = b + c.defer_ws; h->defer_ws_bytes = c.defer_ws_floats * sizeof(float);
  h->range_ws = c.range_floats ? b + c.range : nullptr; h->range_ws_bytes = c.range_floats * sizeof(float);
  // the scaled contract is the bf16 executor's (fp32 keeps the reference's operation order); A/B hook: UA2_NO_SCALED=1
  // Plans for more than 64 live sequences keep the prep form as well: at 256 rows the consumers' per-pass row-scale work and
  // the producers' fragment-order stores cost more than the 140 prep launches they replace (12.6 vs 13.7 ms per frame).  The
  // choice is made once per plan, so every row count served by one plan computes the same function (rows of a 64-sequence
  // batch are bit-identical to their B = 1 runs under the same plan).
  h->scaled = d->dtype == UA2_BF16 && knobs.scaled && d->backbone.n_embd % 32 == 0 && d->decoder.n_embd % 32 == 0 &&
              d->max_batch <= 64;
  h->npart_t = (d->vt + 15) / 16; h->npart_a = (d->va + 15) / 16;
  h->argmax_fold = knobs.argmax_fold;
  h->row_operand = d->dtype == UA2_BF16 && knobs.row_operand;
  if (c.ptab_rows) {
    // The table is what the frame's own projection launches would write: same entry point, same arguments, rows in groups of up to 64
    // (decode kernel / weights-stationary kernel: a row's bits do not depend on its group).  Null stream, once per plan.
    h->ptab_y = b + c.ptab_y; h->ptab_h = b + c.ptab_h; h->ptab_ssq = b + c.ptab_ssq;
    h->ptab_ho = h->scaled;
    const int C = d->backbone.n_embd, Cd = d->decoder.n_embd;
    const int chunk = std::min(64, d->max_rows);          // operand rows staged in the trunk's first row buffer (max_rows x C): a B = 1 plan still builds 64 rows per launch
    void *tmp_k = nullptr, *tmp_v = nullptr;
    int32_t* tmp_i = nullptr;          // [64] positions, [64] page table (row r -> page r)
    if (c.ptab_qkv) {
      h->ptab_q = b + c.ptab_q; h->ptab_k = b + c.ptab_k; h->ptab_v = b + c.ptab_v;
      const size_t pool = (size_t)64 * d->decoder.n_kv * UA2_PAGE * d->decoder.head_size * (d->dtype == UA2_BF16 ? 2 : 4);
      if (hipMalloc(&tmp_k, pool) != hipSuccess || hipMalloc(&tmp_v, pool) != hipSuccess || hipMalloc((void**)&tmp_i, 128 * sizeof(int32_t)) != hipSuccess) {
        ua2_set_error("ua2_stage3_create: scratch cache of the q|k|v table"); delete h; return -1;
      }
    }
    for (size_t row0 = 0; row0 < c.ptab_rows; row0 += chunk) {
      const int n = (int)std::min<size_t>(chunk, c.ptab_rows - row0);
      if (d->dtype == UA2_BF16) hipLaunchKernelGGL(emb_rows_f32_kernel<UA2_BF16>, dim3(std::min(1024, n * 4)), dim3(256), 0, nullptr, d->audio_emb, (long long)row0, n, C, h->xa);
      else hipLaunchKernelGGL(emb_rows_f32_kernel<UA2_F32>, dim3(std::min(1024, n * 4)), dim3(256), 0, nullptr, d->audio_emb, (long long)row0, n, C, h->xa);
      ua2_linear_args a = fresh_args(h);
      a.dtype = d->dtype; a.prologue = UA2_PRO_CAST; a.epilogue = UA2_EPI_STORE;
      a.M = n; a.N = Cd; a.K = C; a.x = h->xa; a.ldx = C; a.w0 = d->projection; a.y = h->ptab_y + row0 * Cd; a.ldy = Cd;
      if (h->ptab_ho) {
        a.y_norm_w = h->norms[3][0][0]; a.y_ssq = h->ptab_ssq + row0 * (Cd / 16);
        a.y_h = reinterpret_cast<unsigned short*>(h->ptab_h) + row0 * Cd; a.ldh = Cd;
      }
      const Handover hod(h, n, Cd);
      const bool scaled_q = h->ptab_ho && c.ptab_qkv;
      if (scaled_q && !hod.rows_h) a.y_packed = h->xpk;        // the q|k|v launch below reads the fragment-order form, as in the frame
      if (int rc = ua2_linear_launch(a, nullptr)) { delete h; return rc; }
      if (!c.ptab_qkv) continue;
      // layer 0's q|k|v of these rows, exactly as run_gpt launches it: row r of the group = its own one-page sequence of a scratch cache
      const ua2_gpt_desc& g = d->decoder;
      const int qn = g.n_head * g.head_size, nqkv = (g.n_head + 2 * g.n_kv) * g.head_size, esz = d->dtype == UA2_BF16 ? 2 : 4;
      hipLaunchKernelGGL(ptab_pos_kernel, dim3(1), dim3(64), 0, nullptr, tmp_i, n, (long long)row0, d->va);
      ua2_kv_geom kv{};
      kv.k_pool = tmp_k; kv.v_pool = tmp_v; kv.page_table = tmp_i + 64; kv.max_pages = 1; kv.n_kv = g.n_kv; kv.n_head = g.n_head; kv.head_size = g.head_size;
      a = fresh_args(h);
      a.dtype = d->dtype; a.prologue = UA2_PRO_NORM; a.epilogue = UA2_EPI_QKV_ROPE;
      a.M = n; a.N = nqkv; a.K = Cd; a.x = h->ptab_y + row0 * Cd; a.ldx = Cd; a.norm_w = h->norms[3][0][0]; a.eps = g.eps;
      a.w0 = h->ptrs[3][0][0]; a.row_pos = tmp_i; a.row_seq = nullptr; a.rope_cos = g.rope_cos; a.rope_sin = g.rope_sin;
      a.q_out = h->ptab_q + row0 * qn; a.kv = kv;
      if (scaled_q) {
        a.prologue = UA2_PRO_SCALED; a.x_ssq = h->ptab_ssq + row0 * (Cd / 16); a.x = nullptr; a.norm_w = nullptr;
        if (hod.rows_h) { a.x_h = reinterpret_cast<unsigned short*>(h->ptab_h) + row0 * Cd; a.ldh = Cd; } else { a.x_packed = h->xpk; }
      }
      if (int rc = ua2_linear_launch(a, nullptr)) { delete h; return rc; }
      const size_t kvw = (size_t)g.n_kv * g.head_size * esz;
      if (int rc = ua2_kv_rows_extract(tmp_k, tmp_v, tmp_i, n, g.n_kv, g.head_size, esz, (char*)h->ptab_k + row0 * kvw, (char*)h->ptab_v + row0 * kvw, nullptr)) { delete h; return rc; }
    }
    const hipError_t e = hipStreamSynchronize(nullptr);
    if (tmp_k) { (void)hipFree(tmp_k); (void)hipFree(tmp_v); (void)hipFree(tmp_i); }
    if (e != hipSuccess) { ua2_set_error("ua2_stage3_create: building the projected-embedding table failed: %s", hipGetErrorString(e)); delete h; return -1; }
  }
  if (d->dtype == UA2_BF16 && knobs.lossless)
    if (int rc = build_l13(h)) { ua2_stage3_destroy(h); return rc; }
  *out = h;
  return 0;
}

extern "C" void ua2_stage3_destroy(ua2_stage3* h) {
  if (!h) return;
  drop_graphs(h);
  if (h->cap_stream) (void)hipStreamDestroy(h->cap_stream);
  if (h->l13_mem) (void)hipFree(h->l13_mem);
  delete h;
}

// identity: rows are sequences 0..R-1 (decode frames) -> no row_seq indirection in the kernels
// skip_experts (UA2_FRAME_SKIP_AUDIO_EXPERTS): every row of the frame is a TEXT step of a text-only continuation — the understanding and
// generation experts' outputs are multiplied by audio_step_mask = 0 (model_new.py:607, :613) and their caches are never read again, so
// the two GPTs are not run; the blends see zeros in their place and select the text / backbone operand exactly as before.
static int trunk_impl(ua2_stage3* h, int32_t R, bool identity, hipStream_t s, bool skip_experts = false) {
  UA2_CHECK(h && R > 0 && R <= h->d.max_rows, "ua2_stage3_trunk: R=%d out of range", R);
  ua2_stage3_desc d = h->d;
  if (identity) d.row_seq = nullptr;
  const int C = d.backbone.n_embd, w = d.n_cb + 1;
  // Decode frames run the scaled hand-over; PREFILL chunks (row groups set: the MFMA flash attention path) keep the
  // prep + RMSNorm-prologue form: prefill rows already differ from decode rows by bf16-level summation order,
  // and there the hand-over's epilogue costs more than the prep launches it saves (the tiled kernel's RESIDUAL epilogue
  // with the emission spills its accumulators: 8192-row prefill 82 -> 131 ms, profiles/r3_notes.md)
  const bool grouped = !identity;   // prefill chunks (ua2_stage3_trunk) may carry row groups; decode frames never do
  // (under the order-free opt-in the hand-over rides in ua2_gemm2.hip's epilogues at any row count: prefill chunks and plans for more
  // than 64 sequences take it too)
  const bool prefill = grouped && (h->n_groups > 0 || R > h->d.max_batch);   // ua2_stage3_trunk with row groups, or with more rows than sequences: a prefill chunk
  const bool scaled = (h->scaled && !prefill) || order_free_scaled(h, R, prefill);
  const Handover ho(h, R, C);
  ua2_handover e0{}, e1{}, e2{};
  if (scaled) { e0 = ho.rowwise(h->norms[0][0][0]); e1 = ho.rowwise(h->norms[1][0][0]); e2 = ho.rowwise(h->norms[2][0][0]); }
  GptRun run{}; run.grouped = grouped; run.scaled = scaled;
  if (int rc = ua2_embed_frame(d.dtype, R, C, d.n_cb, d.va, d.tokens, d.mask, d.audio_emb, d.wte, h->xa, h->text, &e0, s)) return rc;
  if (!skip_experts)
    if (int rc = run_gpt(h, 0, d.und, h->xa, R, d.row_pos, d.row_seq, s, run)) return rc;
  // backbone_input = h_audio*audio_step + text_embeds*text_step   (model_new.py:607)
  if (int rc = ua2_rmsnorm_blend(R, C, h->xa, d.und.ln_f, d.und.eps, h->text, d.mask, w, 0, d.n_cb, h->xb, nullptr, &e1, s)) return rc;
  if (int rc = run_gpt(h, 1, d.backbone, h->xb, R, d.row_pos, d.row_seq, s, run)) return rc;
  // h = ln_f(x); generation_input = h*audio_step                   (model_new.py:609-610)
  if (int rc = ua2_rmsnorm_blend(R, C, h->xb, d.backbone.ln_f, d.backbone.eps, nullptr, d.mask, w, 0, -1, h->xg, h->hbuf, &e2, s)) return rc;
  if (!skip_experts)
    if (int rc = run_gpt(h, 2, d.gen, h->xg, R, d.row_pos, d.row_seq, s, run)) return rc;
  // h_final = h_audio*audio_step + h*text_step                     (model_new.py:613)
  if (int rc = ua2_rmsnorm_blend(R, C, h->xg, d.gen.ln_f, d.gen.eps, h->hbuf, d.mask, w, 0, d.n_cb, h->hfin, nullptr, nullptr, s)) return rc;
  return 0;
}

// (re-)seeding also rewinds the draw index (counters[1]): an utterance's samples are then a function of its own key and its
// own frame count, whatever was generated before it on this rank (per-utterance keys alone did not make the
// samples independent of the sharding — the index kept counting across utterances)
__global__ void set_seed_kernel(int32_t* c, uint32_t lo, uint32_t hi) { c[1] = 0; c[2] = (int32_t)lo; c[3] = (int32_t)hi; }

// The seed lives in device memory (counters[2..3]) and the samplers read it there, so a captured frame graph
// serves every seed: re-seeding between utterances is one 8-byte store on the caller's stream, never a re-capture.
extern "C" int ua2_stage3_set_sampling(ua2_stage3* h, int32_t topk, float temperature, uint64_t seed, void* stream) {
  UA2_CHECK(h != nullptr, "ua2_stage3_set_sampling: NULL handle");
  UA2_CHECK(temperature > 0.f, "temperature must be > 0");
  UA2_CHECK(topk >= 1 && topk <= h->d.va, "topk must be in 1..%d", h->d.va);
  h->topk = topk; h->temperature = temperature;
  hipLaunchKernelGGL(set_seed_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, h->d.counters, (uint32_t)seed, (uint32_t)(seed >> 32));
  UA2_LAUNCH_CHECK();
  return 0;
}

extern "C" int ua2_stage3_set_top_p(ua2_stage3* h, float top_p) {
  UA2_CHECK(h != nullptr, "ua2_stage3_set_top_p: NULL handle");
  UA2_CHECK(top_p >= 0.f && top_p <= 1.f, "ua2_stage3_set_top_p: top_p must be in [0, 1] (0 and 1 = off), got %g", (double)top_p);
  h->top_p = top_p;            // selects among the recorded frames (FrameKey.topp_bits): nothing to drop
  return 0;
}

extern "C" int ua2_stage3_set_rep_penalty(ua2_stage3* h, float penalty, int32_t window, int32_t* hist, int32_t* len) {
  UA2_CHECK(h != nullptr, "ua2_stage3_set_rep_penalty: NULL handle");
  UA2_CHECK(penalty > 0.f && penalty < INFINITY, "ua2_stage3_set_rep_penalty: penalty must be finite and > 0 (1 = off), got %g", (double)penalty);
  if (penalty == 1.f || (!hist && !len)) {   // off: the frame graphs key on (penalty, window), so the penalised ones stay valid for the same buffers
    h->rep_penalty = 1.f; h->rep_window = 0;
    return 0;
  }
  UA2_CHECK(window >= 1 && window <= 512, "ua2_stage3_set_rep_penalty: window must be in 1..512, got %d", window);
  UA2_CHECK(hist && len, "ua2_stage3_set_rep_penalty: hist and len go together");
  UA2_CHECK(h->d.va <= (1 << 17) && h->d.vt <= (1 << 17), "ua2_stage3_set_rep_penalty: the penalised samplers serve vocabularies up to 131072 columns");
  if (hist != h->rep_hist || len != h->rep_len) drop_graphs(h);   // recorded top-k frames bake the samplers' arguments
  h->rep_penalty = penalty; h->rep_window = window; h->rep_hist = hist; h->rep_len = len;
  return 0;
}

extern "C" int ua2_stage3_set_prefill_groups(ua2_stage3* h, const int32_t* group_rows, const int32_t* group_seq, const int32_t* group_nkeys,
                                             int32_t n_groups, int32_t group_q_tiles) {
  UA2_CHECK(h != nullptr, "ua2_stage3_set_prefill_groups: NULL handle");
  UA2_CHECK(n_groups == 0 || (group_rows && group_seq && group_nkeys && group_q_tiles > 0), "ua2_stage3_set_prefill_groups: missing tables");
  h->group_rows = group_rows; h->group_seq = group_seq; h->group_nkeys = group_nkeys;
  h->n_groups = n_groups; h->group_q_tiles = group_q_tiles;
  return 0;
}

extern "C" int ua2_stage3_set_order_free_rows(ua2_stage3* h, int32_t rows) {
  UA2_CHECK(h != nullptr && rows >= 0, "ua2_stage3_set_order_free_rows: NULL handle or rows < 0");
  if (h->order_free_rows != rows) drop_graphs(h);    // recorded frames bake the kernel choice
  h->order_free_rows = rows;
  return 0;
}

extern "C" int ua2_stage3_set_w8(ua2_stage3* h, const ua2_w8_entry* table, int32_t n) {
  UA2_CHECK(h != nullptr && n >= 0 && (n == 0 || table), "ua2_stage3_set_w8: NULL handle / table or n < 0");
  UA2_CHECK(n == 0 || h->d.dtype == UA2_BF16, "ua2_stage3_set_w8: fp8 weights are an option of UA2_BF16 plans");
  std::map<const void*, ua2_stage3::WImage> m;
  for (int i = 0; i < n; ++i) {
    const ua2_w8_entry& e = table[i];
    UA2_CHECK(e.w && e.q && e.exp, "ua2_stage3_set_w8: entry %d has a NULL pointer", i);
    bool mine = e.w == h->d.lm_head || e.w == h->d.projection;
    for (const void* p : h->audio_head) mine = mine || p == e.w;
    for (int gi = 0; gi < 4 && !mine; ++gi)
      for (int k = 0; k < 5 && !mine; ++k)
        for (const void* p : h->ptrs[gi][k]) mine = mine || p == e.w;
    UA2_CHECK(mine, "ua2_stage3_set_w8: entry %d is not a weight of this plan", i);
    m[e.w] = ua2_stage3::WImage{e.q, e.exp};
  }
  drop_graphs(h);                                    // recorded frames bake the kernels and the weight pointers
  h->w8.swap(m);
  return 0;
}

extern "C" int ua2_stage3_set_lossless(ua2_stage3* h, int32_t on) {
  UA2_CHECK(h != nullptr, "ua2_stage3_set_lossless: NULL handle");
  const bool want = on != 0 && !h->l13.empty();
  if (want != h->lossless) drop_graphs(h);           // recorded frames bake the kernels and the weight pointers
  h->lossless = want;
  return 0;
}

extern "C" int ua2_stage3_lossless_stats(const ua2_stage3* h, ua2_lossless_info* out) {
  UA2_CHECK(h != nullptr && out != nullptr, "ua2_stage3_lossless_stats: NULL argument");
  *out = h->l13_info;
  out->on = h->lossless ? 1 : 0;
  return 0;
}

extern "C" int ua2_stage3_set_ngram(ua2_stage3* h, int32_t n, int32_t fallback, int32_t* hist, int32_t* hist_len, int32_t cap) {
  UA2_CHECK(h != nullptr, "ua2_stage3_set_ngram: NULL handle");
  if (n <= 1) {                    // off: the frame graphs key on n, so the filtered ones stay valid for the same buffers
    h->ngram_n = 0;
    return 0;
  }
  UA2_CHECK(n <= 16, "ua2_stage3_set_ngram: n must be <= 16, got %d", n);
  UA2_CHECK(hist && hist_len && cap >= 1, "ua2_stage3_set_ngram: missing history buffers");
  if (fallback != h->ngram_fallback || hist != h->ngram_hist || hist_len != h->ngram_hist_len || cap != h->ngram_cap) drop_graphs(h);   // recorded text frames bake the filter's arguments
  h->ngram_n = n; h->ngram_fallback = fallback; h->ngram_hist = hist; h->ngram_hist_len = hist_len; h->ngram_cap = cap;
  return 0;
}

extern "C" int ua2_stage3_set_row_streams(ua2_stage3* h, int32_t* row_key, int32_t* row_draw) {
  UA2_CHECK(h != nullptr, "ua2_stage3_set_row_streams: NULL handle");
  if (!row_key && !row_draw) {     // off: the frame graphs key on the mode, so the row-stream ones stay valid for the same arrays
    h->row_streams = false;
    return 0;
  }
  UA2_CHECK(row_key && row_draw, "ua2_stage3_set_row_streams: row_key and row_draw go together");
  if (row_key != h->row_key || row_draw != h->row_draw) drop_graphs(h);   // recorded top-k frames bake the samplers' arguments
  h->row_streams = true; h->row_key = row_key; h->row_draw = row_draw;
  return 0;
}

extern "C" int ua2_stage3_set_beam_groups(ua2_stage3* h, int32_t W, int32_t G, int32_t eos, const ua2_beam_state* st, const ua2_beam_pool* pools,
                                          int32_t n_pools) {
  UA2_CHECK(h != nullptr, "ua2_stage3_set_beam: NULL handle");
  if (h->beam_ng.n != 0) { drop_graphs(h); h->beam_ng = ua2_beam_ngram{}; }   // the ban belongs to one attachment: set again behind this call
  if (W == 0) {
    if (h->beam_W != 0) drop_graphs(h);
    h->beam_W = 0; h->beam_G = 1;
    return 0;
  }
  const ua2_stage3_desc& d = h->d;
  UA2_CHECK(W >= 1 && W <= 8, "ua2_stage3_set_beam: beam width must be in 1..8, got %d", W);
  UA2_CHECK(G >= 1 && G * W <= 64, "ua2_stage3_set_beam: %d groups of %d slots: need 1 <= G and G * W <= 64 rows", G, W);
  UA2_CHECK(2 * G * W <= d.max_batch, "ua2_stage3_set_beam: %d beam(s) of %d need a plan of %d sequences (max_batch), got %d", G, W, 2 * G * W, d.max_batch);
  UA2_CHECK(st && st->score && st->fin && st->len && st->parent && st->ctrl && st->cand_logp && st->cand_id && st->log && st->lp_inv,
            "ua2_stage3_set_beam: NULL state buffer");
  UA2_CHECK(st->log_cap >= 1 && st->lp_n >= 2, "ua2_stage3_set_beam: log capacity %d / %d length-penalty entries", st->log_cap, st->lp_n);
  UA2_CHECK(n_pools >= 0 && (n_pools == 0 || pools), "ua2_stage3_set_beam: missing pool descriptors");
  UA2_CHECK(d.und.max_pages == d.backbone.max_pages && d.gen.max_pages == d.backbone.max_pages && d.backbone.max_pages >= 1 &&
            (size_t)W * d.backbone.max_pages * sizeof(int32_t) <= 48 * 1024, "ua2_stage3_set_beam: the three trunk page tables must have one width");
  UA2_CHECK(d.vt >= W, "ua2_stage3_set_beam: vocabulary smaller than the beam");
  if (W != h->beam_W || G != h->beam_G || eos != h->beam_eos || memcmp(st, &h->beam, sizeof(*st)) != 0 || pools != h->beam_pools || n_pools != h->beam_n_pools) drop_graphs(h);   // recorded beam frames bake the state's pointers
  h->beam_W = W; h->beam_G = G; h->beam_eos = eos; h->beam = *st; h->beam_pools = pools; h->beam_n_pools = n_pools;
  return 0;
}

extern "C" int ua2_stage3_set_beam_ngram(ua2_stage3* h, const ua2_beam_ngram* ng) {
  UA2_CHECK(h != nullptr, "ua2_stage3_set_beam_ngram: NULL handle");
  ua2_beam_ngram v{};
  if (ng && ng->n != 0) {
    UA2_CHECK(h->beam_W >= 1, "ua2_stage3_set_beam_ngram: no beam is attached (ua2_stage3_set_beam)");
    UA2_CHECK(ng->n >= 2 && ng->n <= 16, "ua2_stage3_set_beam_ngram: no_repeat_ngram_size must be 0 (off) or in 2..16, got %d", ng->n);
    UA2_CHECK(ng->cap >= 1, "ua2_stage3_set_beam_ngram: history capacity %d", ng->cap);
    UA2_CHECK(ng->hist != nullptr, "ua2_stage3_set_beam_ngram: NULL history buffer");
    UA2_CHECK((size_t)((h->d.vt + 31) / 32) * sizeof(uint32_t) <= 48 * 1024, "ua2_stage3_set_beam_ngram: a vocabulary of %d does not fit the ban bitmap (48 KB)", h->d.vt);
    v = *ng;
  }
  if (v.n != h->beam_ng.n || v.cap != h->beam_ng.cap || v.hist != h->beam_ng.hist) drop_graphs(h);   // recorded beam frames bake the step's launches
  h->beam_ng = v;
  return 0;
}

extern "C" int ua2_stage3_set_beam(ua2_stage3* h, int32_t W, int32_t eos, const ua2_beam_state* st, const ua2_beam_pool* pools, int32_t n_pools) {
  return ua2_stage3_set_beam_groups(h, W, 1, eos, st, pools, n_pools);
}

extern "C" int ua2_stage3_set_cfg(ua2_stage3* h, float cfg_scale) {
  UA2_CHECK(h != nullptr && cfg_scale >= 1.f, "ua2_stage3_set_cfg: NULL handle or cfg_scale < 1");
  h->cfg_scale = cfg_scale;
  return 0;
}

extern "C" int ua2_stage3_trunk(ua2_stage3* h, int32_t R, void* stream) {
  UA2_CHECK(h != nullptr, "ua2_stage3_trunk: NULL handle");
  const int rc = trunk_impl(h, R, false, (hipStream_t)stream);
  h->n_groups = 0;                 // row groups describe ONE chunk: they never outlive the call they were set for
  return rc;
}

// text_only: the text head and its sample only.  The on-device text loop (feedback mode 1, asr_task.py:668-682) feeds
// back zeros for the audio streams, so what the depth decoder would sample is never read: skipping its 8 passes leaves
// the text ids unchanged ("waste removal with identical outputs") and removes ~45 % of the frame.
// skip_text: the depth decoder only.  In the audio-feedback loops (feedback modes 0 and 2 of the TTS / TTA / TTM / LTS / S2S
// generators) the sampled text id is fed back under a ZERO mask (evaluation/tts_task.py:274-277: text_mask = False) and appended
// to a list nobody reads (:259), so the frame's audio ids do not depend on it: skipping lm_head + its arg-max (788 MB of weights
// at 3072 x 128256 bf16 = 117 us of the 3.1 ms B = 1 frame, 220 us at 64 rows) leaves (reason, semantic) bit-identical
// (model_new.py:617 computes it every frame).  generate_frame's (B, 9) API never sets it.
// fold_last != NULL: the caller runs feedback_kernel next and can take the last step's arg-max (set to true when it must)
static int heads_impl(ua2_stage3* h, int32_t R, bool text_only, void* stream, bool skip_text = false, bool beam = false, bool* fold_last = nullptr) {
  UA2_CHECK(h && R > 0 && R <= h->d.max_batch, "ua2_stage3_heads: R=%d out of range", R);
  hipStream_t s = (hipStream_t)stream;
  const ua2_stage3_desc& d = h->d;
  const int C = d.backbone.n_embd, Cd = d.decoder.n_embd, w = d.n_cb + 1;
  // the plan's order-free opt-in covers the heads and the projection as well (arg-max partials and the hand-over are forms of
  // ua2_gemm2.hip since round 6); `scaled` as in trunk_impl
  const int order = order_free(h, R) ? UA2_SUM_ORDER_FREE : UA2_SUM_ORDER_INVARIANT;
  const bool scaled = h->scaled || order_free_scaled(h, R);
  UA2_CHECK(!(skip_text && text_only), "ua2_stage3_heads: nothing left to compute");
  // text_logits = lm_head(last_h); greedy text sample             (model_new.py:617,623)
  const ua2_linear_args lm = lm_head_args(h, R, h->hfin, h->text_logits, h->pmax_t, h->pidx_t, order, h->gemm_ws, h->gemm_ws_bytes);
  // lm_head does not feed the depth decoder (model_new.py:617 vs :629-640).  A forked graph branch for it replays 0.4 ms per frame
  // SLOWER than the linear chain on ROCm 7.2 (3.49 vs 3.09 ms, re-measured in round 6), so it stays in the chain — but not as a
  // launch of its own when the depth decoder's down-projections can carry it: each of their n_cb x n_layer launches fills half the
  // device (128 workgroups: the per-CU ingest cap, ua2_gemv.hip) and takes one slice of lm_head's column tiles on the other half.
  // Same bits as lm_head's own launch; the text sample moves behind the depth decoder (nothing in between reads it).
  RiderPlan rp;
  bool ride = false;
  // fp8 twins attached: the rider kernel has no fp8 form, so lm_head runs as a launch of its own (on its fp8 image when it has one)
  if (!skip_text && !text_only && d.n_cb > 0 && d.decoder.n_layer > 0 && h->w8.empty()) {
    const ua2_gpt_desc& g = d.decoder;
    const int qn = g.n_head * g.head_size, nqkv = (g.n_head + 2 * g.n_kv) * g.head_size;
    ua2_linear_args hs[3];
    for (auto& v : hs) { v = fresh_args(h); v.dtype = d.dtype; v.M = R; v.x = h->act; }
    hs[0].prologue = scaled ? UA2_PRO_SCALED : UA2_PRO_NORM; hs[0].epilogue = UA2_EPI_QKV_ROPE; hs[0].N = nqkv; hs[0].K = Cd;
    hs[1].prologue = (R == 1 && d.n_cb <= 8 && !g_no_local_fuse.set()) ? UA2_PRO_LOCAL_ATTN : UA2_PRO_CAST; hs[1].epilogue = UA2_EPI_RESIDUAL; hs[1].N = Cd; hs[1].K = qn;
    hs[2].prologue = UA2_PRO_CAST; hs[2].epilogue = UA2_EPI_RESIDUAL; hs[2].N = Cd; hs[2].K = g.inter;
    const double wk[3] = {0.0, 0.0, 1.0};    // the down-projections only: riders on the 6-us q|k|v / o launches made the frame slower (profiles/r6_notes.md)
    rp.r = lm; rp.ntiles = (lm.N + 15) / 16;
#ifdef UA2_RIDER_EXPERIMENTS
    static Ua2EnvInt frac{"UA2_RIDER_TIMING_PCT", 100};   // timing only (wrong text ids): only this share of lm_head's tiles is computed at all
    rp.ntiles = (int)((long)rp.ntiles * frac.get() / 100);
#endif
    for (int k = 0; k < 3; ++k) {
      rp.ok[k] = wk[k] > 0 && ua2_gemv_rider_ok(hs[k], lm);
      rp.w[k] = rp.ok[k] ? wk[k] : 0.0;
      rp.wleft += rp.w[k] * d.n_cb * g.n_layer;
      ride = ride || rp.ok[k];
    }
  }
  if (!skip_text && !ride)
    if (int rc = lin(h, lm, s)) return rc;
  // model_new.py:618-622: with guidance the sampler sees l[1] + (l[0] - l[1]) * cfg_scale and both rows take its sample
  const bool cfg = h->cfg_scale > 1.f && R > 1;
  UA2_CHECK(!cfg || R % 2 == 0, "ua2_stage3_heads: classifier-free guidance needs (conditional, unconditional) row pairs, R=%d", R);
  const int key_shift = cfg ? 1 : 0;                       // the two rows of a pair hold the same guided logits and draw the same numbers
  // the frame's samplers: per-row streams when set (the caller gives both rows of a pair one key: no key shift), else the executor's one
  // seed and draw index with the row index in the key
  const bool nucleus = h->top_p > 0.f && h->top_p < 1.f;
  auto sample = [&](const float* logits, int ld, int V, int topk, const int32_t* forbid, int stream_id, const void* emb, int emb_off, float* next_h) -> int {
    if (h->rep_window > 0) {             // penalised: every form behind the one entry, against the ring of (row, stream_id)
      UA2_CHECK(R <= d.max_batch, "ua2_stage3_heads: the repetition histories hold %d rows, R=%d", d.max_batch, R);
      ua2_sample_args a{};
      a.dtype = d.dtype; a.M = R; a.logits = logits; a.ld = ld; a.V = V; a.topk = topk; a.temperature = h->temperature; a.forbid = forbid;
      a.stream_id = stream_id; a.out_tokens = d.out_tokens; a.out_ld = w; a.out_col = stream_id; a.emb = emb; a.emb_row_offset = emb_off; a.C = C;
      a.next_h = next_h; a.top_p = nucleus ? h->top_p : 0.f;
      if (h->row_streams) { a.row_key = h->row_key; a.row_draw = h->row_draw; }
      else { a.counter = d.counters + 1; a.row_key_shift = key_shift; }
      a.rep_penalty = h->rep_penalty; a.rep_window = a.rep_cap = h->rep_window; a.rep_hist_ld = w * h->rep_window; a.rep_len_ld = w;
      a.rep_hist = h->rep_hist + (size_t)stream_id * h->rep_window; a.rep_len = h->rep_len + stream_id;
      return ua2_sample_penalized(&a, s);
    }
    if (nucleus && h->row_streams)
      return ua2_sample_topp_rows(d.dtype, R, logits, ld, V, topk, h->temperature, forbid, h->row_key, h->row_draw, stream_id, d.out_tokens, w,
                                  stream_id, emb, emb_off, C, next_h, h->top_p, nullptr, s);
    if (nucleus)
      return ua2_sample_topp(d.dtype, R, logits, ld, V, topk, h->temperature, forbid, 0, d.counters + 1, stream_id, d.out_tokens, w, stream_id, emb,
                             emb_off, C, next_h, key_shift, h->top_p, nullptr, s);
    if (h->row_streams)
      return ua2_sample_topk_rows(d.dtype, R, logits, ld, V, topk, h->temperature, forbid, h->row_key, h->row_draw, stream_id, d.out_tokens, w,
                                  stream_id, emb, emb_off, C, next_h, s);
    return ua2_sample_topk(d.dtype, R, logits, ld, V, topk, h->temperature, forbid, 0, d.counters + 1, stream_id, d.out_tokens, w, stream_id, emb,
                           emb_off, C, next_h, key_shift, s);
  };
  auto text_tail = [&]() -> int {
    if (skip_text || beam) return 0;   // (beam frames: ua2_beam_step reads the fp32 logits and chooses the ids)  the sampler streams are keyed by (seed, draw index, row, stream id), so the audio streams' draws do not move
    if (cfg)
      if (int rc = ua2_cfg_mix(h->text_logits, d.vt, d.vt, h->cfg_scale, nullptr, h->pmax_t, h->pidx_t, R / 2, s)) return rc;
    if (h->topk == 1)
      return ua2_argmax_embed_launch(d.dtype, R, h->npart_t, d.vt, h->pmax_t, h->pidx_t, d.out_tokens, w, 0, nullptr, 0, C, nullptr, s);
    // model_new.py:623 sample_topk(text_logits, topk, temperature)
    return sample(h->text_logits, d.vt, d.vt, std::min(h->topk, d.vt), nullptr, 0, nullptr, 0, nullptr);
  };
  if (!ride)
    if (int rc = text_tail()) return rc;
  const float* curr = h->hfin;
  // steps 1 .. n_cb - 1 take their projected input (and its hand-over) from the table, gathered by the previous step's arg-max
  // (under the order-free opt-in as well: the table rows are the row-invariant kernels' sums, one of the orders that contract allows)
  const bool tab = h->ptab_y && h->topk == 1 && (!scaled || h->ptab_ho || h->ptab_q);
  ua2_argmax_fold fg{};
  bool fold_next = false;             // step i left its arg-max + table gather to layer 0's O-projection of step i + 1
  for (int i = 0; i < (text_only ? 0 : d.n_cb); ++i) {             // model_new.py:630-641
    const Handover hod(h, R, Cd);
    if (!(tab && i > 0))
      if (int rc = lin(h, projection_args(h, R, curr, order, scaled), s)) return rc;
    GptRun run{}; run.local = d.n_cb <= 8; run.scaled = scaled; run.final_norm_w = scaled ? d.decoder.ln_f : nullptr;
    run.rider = ride ? &rp : nullptr; run.qkv0_given = tab && i > 0 && h->ptab_q; run.fold0 = fold_next ? &fg : nullptr;
    if (int rc = run_gpt(h, 3, d.decoder, h->xd, R, d.dec_pos + (size_t)i * d.max_rows, nullptr, s, run)) return rc;
    fold_next = false;
    if (int rc = lin(h, audio_head_args(h, R, i, order, scaled, d.forbid), s)) return rc;
    if (cfg)   // model_new.py:634-637
      if (int rc = ua2_cfg_mix(h->audio_logits + (size_t)i * d.va, d.n_cb * d.va, d.va, h->cfg_scale, d.forbid, h->pmax_a,
                               h->pidx_a, R / 2, s)) return rc;
    // R == 1 with layer 0's q | k | v in the table and the attention fused into the O-projection: that launch of step i + 1 takes the tail
    const ua2_gpt_desc& gdec = d.decoder;
    if (tab && i + 1 < d.n_cb && h->argmax_fold && h->ptab_q && R == 1 && !cfg && d.n_cb <= 8 && !g_no_local_fuse.set() && gdec.n_layer > 0 && h->w8.empty() &&
        ua2_gemv_fold_ok(d.dtype, gdec.n_embd, gdec.n_head * gdec.head_size)) {          // (fp8 plans keep the arg-max launches: the fold has no fp8 form)
      fg = ua2_argmax_fold{};
      fg.part_max = h->pmax_a; fg.part_idx = h->pidx_a; fg.n_part = h->npart_a; fg.limit = d.va;
      fg.out_token = d.out_tokens + 1 + i; fg.row_off = (int64_t)i * d.va; fg.pos = i + 1;
      fg.tab_y = h->ptab_y; fg.tab_q = h->ptab_q; fg.tab_k = h->ptab_k; fg.tab_v = h->ptab_v;
      fold_next = true;
    } else if (tab && i + 1 < d.n_cb) {
      const ua2_handover g = hod.rowwise(nullptr);
      ua2_qkv_gather qg{};
      if (h->ptab_q) {
        qg.tab_q = h->ptab_q; qg.tab_k = h->ptab_k; qg.tab_v = h->ptab_v; qg.q_out = h->q; qg.qn = gdec.n_head * gdec.head_size;
        qg.esz = d.dtype == UA2_BF16 ? 2 : 4; qg.pos = i + 1; qg.kv = kv_geom(h, 3, gdec, 0);
      }
      // with layer 0's q | k | v in hand nothing reads the hand-over of the projected row (its only consumer was that launch)
      if (int rc = ua2_argmax_gather(R, h->npart_a, d.va, h->pmax_a, h->pidx_a, d.out_tokens, w, 1 + i, h->ptab_y, h->ptab_h, h->ptab_ssq,
                                     (int64_t)i * d.va, Cd, h->xd, (scaled && !h->ptab_q) ? &g : nullptr, h->ptab_q ? &qg : nullptr, s)) return rc;
    } else if (h->topk == 1 && fold_last && h->argmax_fold && tab && R == 1 && i + 1 == d.n_cb) {
      *fold_last = true;              // nothing reads this step's embedding (tab: steps >= 1 read the table), and the id is feedback_kernel's
    } else if (h->topk == 1) {
      if (int rc = ua2_argmax_embed_launch(d.dtype, R, h->npart_a, d.va, h->pmax_a, h->pidx_a, d.out_tokens, w, 1 + i, d.audio_emb,
                                    i * d.va, C, h->curr_h, s)) return rc;
    } else {   // model_new.py:639 audio_sample_topk(ci_logits, topk, temperature, forbid_prefix)
      if (int rc = sample(h->audio_logits + (size_t)i * d.va, d.n_cb * d.va, d.va, h->topk, d.forbid, 1 + i, d.audio_emb, i * d.va, h->curr_h)) return rc;
    }
    curr = h->curr_h;
  }
  if (ride) {
    UA2_CHECK(rp.next == rp.ntiles, "ua2_stage3_heads: %d of %d lm_head tiles rode", rp.next, rp.ntiles);
    if (int rc = text_tail()) return rc;
  }
  if (h->topk != 1) {   // one draw index per frame, advanced after every sampler of the frame has read it
    if (h->row_streams) {
      if (int rc = ua2_row_draw_bump(h->row_draw, R, s)) return rc;
    } else {
      hipLaunchKernelGGL(bump_kernel, dim3(1), dim3(1), 0, s, d.counters + 1);
      UA2_LAUNCH_CHECK();
    }
  }
  return 0;
}

extern "C" int ua2_stage3_heads(ua2_stage3* h, int32_t R, void* stream) { return heads_impl(h, R, false, stream); }

// defer_frames > 0 (UA2_FRAME_DEFER_TEXT_HEAD): the frame's h_final rows go into the stash ring of that many frame slots.  Up to 4 rows the
// copy (48 KB at C = 3072) is part of feedback_kernel's one block — no launch is added to the B = 1 frame; more rows take a launch of
// one block per row in front of it (one block would copy 390 KB at 32 rows: longer than the 3.5 us of a launch).
static int feedback_impl(ua2_stage3* h, int32_t R, int32_t mode, int32_t reason_eos, int32_t reason_card, void* stream, int no_text, int defer_frames = 0,
                         bool fold_argmax = false) {
  UA2_CHECK(h && R > 0 && R <= h->d.max_rows && mode >= 0 && mode <= 2, "ua2_stage3_feedback: bad arguments");
  const ua2_stage3_desc& d = h->d;
  if (mode == 1 && h->ngram_n > 1) {   // asr_task.py:371-375: the filtered id is what the log records and the next frame consumes
    UA2_CHECK(R <= d.max_batch, "ua2_stage3_feedback: n-gram history holds %d rows, R=%d", d.max_batch, R);
    if (int rc = ua2_ngram_filter(d.out_tokens, d.n_cb + 1, R, h->ngram_n, h->ngram_fallback, h->ngram_hist, h->ngram_hist_len,
                                  h->ngram_cap, stream)) return rc;
  }
  const int C = d.backbone.n_embd;
  bool fold = false;
  if (defer_frames > 0) {
    UA2_CHECK(mode == 0 && R <= d.max_batch && (int64_t)defer_frames * R <= UA2_DEFER_CAP_ROWS && C % 4 == 0,
              "ua2_stage3_feedback: stash of %d frames x %d rows (mode %d) does not fit the ring of %d rows", defer_frames, R, mode, UA2_DEFER_CAP_ROWS);
    fold = R <= 4;
    if (!fold) {
      hipLaunchKernelGGL(stash_rows_kernel, dim3(R), dim3(256), 0, (hipStream_t)stream, h->hfin, h->defer_stash, R, C, defer_frames, d.counters);
      UA2_LAUNCH_CHECK();
    }
  }
  hipLaunchKernelGGL(feedback_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, R, d.n_cb, mode, reason_eos,
                     reason_card, d.log_frames, d.max_rows, d.tokens, d.mask, d.row_pos, d.forbid, d.out_tokens,
                     d.frame_log, d.counters, no_text, h->hfin, fold ? h->defer_stash : nullptr, C, fold ? defer_frames : 1,
                     fold_argmax ? h->npart_a : 0, d.va, h->pmax_a, h->pidx_a);
  UA2_LAUNCH_CHECK();
  return 0;
}

extern "C" int ua2_stage3_feedback(ua2_stage3* h, int32_t R, int32_t mode, int32_t reason_eos, int32_t reason_card,
                                   void* stream) {
  return feedback_impl(h, R, mode, reason_eos, reason_card, stream, 0);
}

extern "C" int ua2_stage3_frame(ua2_stage3* h, int32_t R, int32_t mode, int32_t reason_eos, int32_t reason_card,
                                int32_t use_graph, void* stream) {
  UA2_CHECK(h != nullptr, "ua2_stage3_frame: NULL handle");
  hipStream_t s = (hipStream_t)stream;
  const bool defer = mode >= 0 && (mode & UA2_FRAME_DEFER_TEXT_HEAD) != 0;
  UA2_CHECK(!defer || (mode & UA2_FRAME_SKIP_TEXT_HEAD) == 0, "ua2_stage3_frame: UA2_FRAME_DEFER_TEXT_HEAD and UA2_FRAME_SKIP_TEXT_HEAD exclude each other");
  const bool skip_text = defer || (mode >= 0 && (mode & UA2_FRAME_SKIP_TEXT_HEAD) != 0);     // a deferring frame is a skipping frame that keeps h_final
  const bool skip_experts = mode >= 0 && (mode & UA2_FRAME_SKIP_AUDIO_EXPERTS) != 0;
  if (mode >= 0) mode &= ~(UA2_FRAME_SKIP_TEXT_HEAD | UA2_FRAME_SKIP_AUDIO_EXPERTS | UA2_FRAME_DEFER_TEXT_HEAD);
  int defer_frames = 0;                            // frame slots of the stash ring: baked into the recorded frame, so part of its key
  if (defer) {
    UA2_CHECK(mode == 0, "ua2_stage3_frame: UA2_FRAME_DEFER_TEXT_HEAD goes with feedback mode 0");
    UA2_CHECK(R > 0 && R <= h->d.max_batch, "ua2_stage3_frame: R=%d out of range", R);
    defer_frames = defer_rows() / R;
    UA2_CHECK(defer_frames >= 1, "ua2_stage3_frame: the stash ring (%d rows: UA2_DEFER_ROWS / UA2_NO_DEFER_TEXT_HEAD) holds no frame of %d rows", defer_rows(), R);
  }
  UA2_CHECK(!skip_text || mode == 0 || mode == 2, "ua2_stage3_frame: UA2_FRAME_SKIP_TEXT_HEAD goes with the audio-feedback modes (0, 2)");
  UA2_CHECK(!skip_experts || mode == 1 || mode == 3, "ua2_stage3_frame: UA2_FRAME_SKIP_AUDIO_EXPERTS goes with the text-feedback modes (1, 3)");
  const bool beam = mode == 3;
  if (beam) {                                     // every argument of the beam launches is checked here, before the first launch
    UA2_CHECK(h->beam_W >= 1, "ua2_stage3_frame: mode 3 needs a beam (ua2_stage3_set_beam)");
    UA2_CHECK(R == h->beam_G * h->beam_W, "ua2_stage3_frame: a beam frame has one row per slot (W=%d, groups=%d), got R=%d", h->beam_W, h->beam_G, R);
    UA2_CHECK(2 * R <= h->d.max_batch, "ua2_stage3_frame: beams of %d rows need a plan of %d sequences", R, 2 * R);
    UA2_CHECK(!(h->cfg_scale > 1.f), "ua2_stage3_frame: beam search does not combine with classifier-free guidance");
    UA2_CHECK(h->ngram_n <= 1, "ua2_stage3_frame: beam search does not combine with the n-gram filter");
    UA2_CHECK(h->topk == 1, "ua2_stage3_frame: beam search needs top-k = 1 (it ranks the logits itself)");
  }
  auto body = [&](hipStream_t st) -> int {
    if (int rc = trunk_impl(h, R, true, st, skip_experts)) return rc;
    bool fold_last = false;
    if (int rc = heads_impl(h, R, mode == 1 || beam, st, skip_text, beam, (mode == 0 && R == 1) ? &fold_last : nullptr)) return rc;
    if (mode < 0) return 0;
    if (beam) {
      const ua2_stage3_desc& d = h->d;
      if (h->beam_ng.n != 0) {
        if (int rc = ua2_beam_step_groups_ngram(h->text_logits, d.vt, d.vt, h->beam_W, h->beam_G, h->beam_eos, &h->beam, &h->beam_ng, d.out_tokens, d.n_cb + 1, st)) return rc;
      } else if (int rc = ua2_beam_step_groups(h->text_logits, d.vt, d.vt, h->beam_W, h->beam_G, h->beam_eos, &h->beam, d.out_tokens, d.n_cb + 1, st)) return rc;
      int32_t* const tables[3] = {const_cast<int32_t*>(d.und.page_table), const_cast<int32_t*>(d.backbone.page_table), const_cast<int32_t*>(d.gen.page_table)};
      if (int rc = ua2_beam_reorder_groups(h->beam_W, h->beam_G, h->beam.parent, d.row_pos, 1, h->beam_pools, h->beam_n_pools, tables, 3, d.max_batch, d.backbone.max_pages, st)) return rc;
      return feedback_impl(h, R, 1, reason_eos, reason_card, st, 0);   // out_tokens' text column holds the step's ids: the text feedback as it is
    }
    return feedback_impl(h, R, mode, reason_eos, reason_card, st, skip_text ? 1 : 0, defer_frames, fold_last);
  };
  if (!use_graph) return body(s);
  // the launch-time knobs are baked into the recorded frames: after ua2_debug_refresh_env every frame is captured anew
  if (const int gen = g_ua2_env_gen.load(std::memory_order_acquire); gen != h->env_gen) { drop_graphs(h); h->env_gen = gen; }
  // the n-gram filter is part of a text-feedback frame: its n selects the graph (its buffers and fallback drop them, set_ngram; mode 3: R is
  // groups x beam width, and set_beam drops the graphs with the state, W or G)
  FrameKey key{};
  key.rows = R; key.mode = mode; key.skip_text = skip_text; key.skip_experts = skip_experts; key.defer_slots = defer_frames;
  key.ngram_n = mode == 1 ? h->ngram_n : 0; key.eos = reason_eos; key.card = reason_card; key.topk = h->topk;
  memcpy(&key.temp_bits, &h->temperature, sizeof(int)); memcpy(&key.cfg_bits, &h->cfg_scale, sizeof(int));
  key.row_streams = (h->row_streams && h->topk != 1) ? 1 : 0;     // greedy frames neither read nor advance the streams
  if (h->topk != 1 && h->top_p > 0.f && h->top_p < 1.f) memcpy(&key.topp_bits, &h->top_p, sizeof(int));   // (0 < top_p < 1: never the bits of 0)
  if (h->topk != 1 && h->rep_window > 0) { memcpy(&key.rep_bits, &h->rep_penalty, sizeof(int)); key.rep_window = h->rep_window; }
  auto it = h->graphs.find(key);
  if (it == h->graphs.end()) {
    hipGraph_t graph = nullptr;
    if (!h->cap_stream) UA2_HIP(hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking));
    UA2_HIP(hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeThreadLocal));
    const int rc = body(h->cap_stream);
    const hipError_t e = hipStreamEndCapture(h->cap_stream, &graph);
    if (rc) return rc;
    if (e != hipSuccess) {
      ua2_set_error("hipStreamEndCapture failed: %s", hipGetErrorString(e));
      return -2;
    }
    hipGraphExec_t exec = nullptr;
    UA2_HIP(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    (void)hipGraphDestroy(graph);
    it = h->graphs.emplace(key, exec).first;
  }
  UA2_HIP(hipGraphLaunch(it->second, s));
  return 0;
}

extern "C" int32_t ua2_stage3_defer_rows(void) { return defer_rows(); }

extern "C" int ua2_stage3_text_flush(ua2_stage3* h, int32_t R, int32_t frame0, int32_t n, void* stream) {
  UA2_CHECK(h != nullptr, "ua2_stage3_text_flush: NULL handle");
  const ua2_stage3_desc& d = h->d;
  UA2_CHECK(R > 0 && R <= d.max_batch, "ua2_stage3_text_flush: R=%d out of range", R);
  const int cap_frames = defer_rows() / R;
  UA2_CHECK(cap_frames >= 1, "ua2_stage3_text_flush: the stash ring (%d rows) holds no frame of %d rows", defer_rows(), R);
  UA2_CHECK(frame0 >= 0 && n >= 1 && n <= cap_frames && frame0 % cap_frames + n <= cap_frames && (int64_t)frame0 + n <= 0x7fffffff,
            "ua2_stage3_text_flush: window [%d, %d + %d) wraps the ring of %d frames", frame0, frame0, n, cap_frames);
  UA2_CHECK(h->topk == 1 && !(h->cfg_scale > 1.f && R > 1), "ua2_stage3_text_flush: the deferred text head is the greedy, unguided one");
  const int C = d.backbone.n_embd, M = n * R;      // M <= cap_frames * R <= UA2_DEFER_CAP_ROWS: the rows every defer_* buffer holds
  hipStream_t s = (hipStream_t)stream;
  // the frame's own lm_head launch (lm_head_args) over the stashed rows, with the flush's buffers: the launcher picks the kernel by M as
  // it does for a batch, and a row's bits depend on neither (row invariance), so ids and logits are those of the per-frame launch
  const ua2_linear_args a = lm_head_args(h, M, h->defer_stash + (size_t)(frame0 % cap_frames) * R * C, h->defer_logits, h->defer_pmax, h->defer_pidx,
                                         UA2_SUM_ORDER_INVARIANT, h->defer_ws, h->defer_ws_bytes);
  if (int rc = lin(h, a, s)) return rc;
  hipLaunchKernelGGL(text_flush_kernel, dim3(M), dim3(256), 0, s, R, h->npart_t, d.vt, h->defer_pmax, h->defer_pidx, d.frame_log, frame0,
                     d.log_frames, d.max_rows, d.n_cb + 1);
  UA2_LAUNCH_CHECK();
  ua2_count_launch(UA2_CNT_TEXT_FLUSH);
  return 0;
}

// Teacher-forced scoring of the R rows ua2_stage3_trunk has just run (model_new.py:445-453 of forward, with the cross-entropy of
// :59-109 taken on the device): heads_impl's plain path — no riders, no per-id tables, no arg-max fold, no graph, no guidance, no
// sampler, forbid_prefix ignored — with ua2_xent_embed as the tail of every head: it scores the label and gathers the LABEL's
// embedding for the next codebook step.  The head launches come from the builders the frame uses (lm_head_args, projection_args,
// audio_head_args) and the depth decoder from run_gpt, so on the row-invariant plans a teacher-forced row carries the bits of the decode
// frame that saw the same ids.
// labels / nll / pred: [R, n_cb + 1] in the token layout (a0 .. a(n_cb-1), text).  Writes none of out_tokens, frame_log, counters, the
// n-gram history or the beam state.
extern "C" int ua2_stage3_score(ua2_stage3* h, int32_t R, const int32_t* labels, float* nll, int32_t* pred, void* stream) {
  UA2_CHECK(h != nullptr, "ua2_stage3_score: NULL handle");
  UA2_CHECK(R > 0 && R <= h->d.max_batch, "ua2_stage3_score: R=%d out of range (1..max_batch=%d)", R, h->d.max_batch);
  UA2_CHECK(labels && nll && pred, "ua2_stage3_score: NULL labels / nll / pred");
  UA2_CHECK(h->beam_W == 0, "ua2_stage3_score: a beam search is attached (ua2_stage3_set_beam); end it first");
  hipStream_t s = (hipStream_t)stream;
  const ua2_stage3_desc& d = h->d;
  const int C = d.backbone.n_embd, w = d.n_cb + 1;
  const int order = order_free(h, R) ? UA2_SUM_ORDER_FREE : UA2_SUM_ORDER_INVARIANT;
  const bool scaled = h->scaled || order_free_scaled(h, R);
  // text_logits = lm_head(h_final)                                (model_new.py:445)
  if (int rc = lin(h, lm_head_args(h, R, h->hfin, h->text_logits, h->pmax_t, h->pidx_t, order, h->gemm_ws, h->gemm_ws_bytes), s)) return rc;
  if (int rc = ua2_xent_embed(d.dtype, R, h->text_logits, d.vt, d.vt, labels, w, d.n_cb, nll, pred, w, d.n_cb, nullptr, 0, C, nullptr, s)) return rc;
  const float* curr = h->hfin;
  GptRun run{}; run.local = d.n_cb <= 8; run.scaled = scaled; run.final_norm_w = scaled ? d.decoder.ln_f : nullptr;
  for (int i = 0; i < d.n_cb; ++i) {                               // model_new.py:447-453, one codebook position at a time
    if (int rc = lin(h, projection_args(h, R, curr, order, scaled), s)) return rc;
    if (int rc = run_gpt(h, 3, d.decoder, h->xd, R, d.dec_pos + (size_t)i * d.max_rows, nullptr, s, run)) return rc;
    if (int rc = lin(h, audio_head_args(h, R, i, order, scaled, nullptr), s)) return rc;
    // the last step's gather has no consumer
    const bool gather = i + 1 < d.n_cb;
    if (int rc = ua2_xent_embed(d.dtype, R, h->audio_logits + (size_t)i * d.va, d.n_cb * d.va, d.va, labels, w, i, nll, pred, w, i,
                                gather ? d.audio_emb : nullptr, (int64_t)i * d.va, C, gather ? h->curr_h : nullptr, s)) return rc;
    curr = h->curr_h;
  }
  ua2_count_launch(UA2_CNT_SCORE);
  return 0;
}

extern "C" float* ua2_stage3_buffer(ua2_stage3* h, const char* name) {
  if (!h || !name) return nullptr;
  if (!strcmp(name, "h_final")) return h->hfin;
  if (!strcmp(name, "text_logits")) return h->text_logits;
  if (!strcmp(name, "audio_logits")) return h->audio_logits;
  if (!strcmp(name, "h")) return h->hbuf;
  return nullptr;
}
