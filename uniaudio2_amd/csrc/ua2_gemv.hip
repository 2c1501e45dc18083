// Decode-regime weight-streaming GEMM (M <= 16 rows per tile, activations small enough for LDS).
//
// Same contract and epilogues as ua2_linear.hip (include/ua2hip.h ua2_linear), restructured after
// the first rocprof pass (profiles/r1_a_*): at B = 1 every kernel of the frame was bound by
// dependent-load latency, not bandwidth.  What changed, and why it maps to CDNA4:
//   * every wave issues ALL of its weight loads (CPW x NT non-temporal 1 KiB bursts) as its first
//     instructions; nothing in the prologue is ordered before them, so up to 16 waves x 16 KiB of
//     HBM traffic per CU is in flight while the activations are prepared;
//   * the activation rows are staged once per workgroup: coalesced float4 loads by all threads,
//     RMSNorm statistics by a workgroup reduction, normalised values written to LDS in the MFMA
//     operand dtype; A fragments are then ds_read_b128 (one per chunk) instead of per-wave
//     global loads that serialised behind the weight stream;
//   * the wave count (8-16) and chunks-per-wave (CPW) are chosen by the launcher so that
//     waves x CPW tiles K exactly for the model's shapes: no tail, no predicated loads.
#include <stdlib.h>

#include <algorithm>

#include "ua2_common.h"
#include "ua2_linear_common.h"
#include "ua2_attn_local.h"

namespace {

constexpr int kMaxWaves = 16;

// gemv_body's form of UA2_PRO_CAST with the operand handed over as bf16 rows (ua2_linear_args.x_h; never an ABI value: a.prologue stays
// UA2_PRO_CAST).  An instantiation of its own, so that the fp32-operand forms keep their registers.
constexpr int kProRowH = 5;

// UA2_PRO_LOCAL_ATTN: this wave's share of the row's short-context attention, written straight into the LDS
// operand row.  `burst` issues the wave's weight loads; it is called after the first pass's small loads are out
// (a wave's loads return in order: q / K / V must not queue behind the weight stream).
template <int DT, int HS, typename Burst>
__device__ __forceinline__ void local_attn_prologue(const ua2_linear_args& a, char* a_lds, int m, int wave, int nw, int lane,
                                                    Burst&& burst) {
  using LA = LocalAttn<DT, HS>;
  constexpr int BYTES = Elem<DT>::BYTES;
  const int pos = a.row_pos[m];
  const int page = a.kv.page_table[(size_t)kv_table_row(a, m) * a.kv.max_pages];
  const float* q_row = a.x + (size_t)m * a.ldx;
  bool streamed = false;
  for (int h0 = wave * LA::HPW; h0 < a.kv.n_head; h0 += nw * LA::HPW) {
    const int h = h0 + lane / LA::LPH, d = (lane % LA::LPH) * 2;
    LA la;
    la.issue(a.kv, q_row, page, h, d);
    if (!streamed) { burst(); streamed = true; }
    const float2 o = la.finish(pos);
    char* dst = a_lds + ((size_t)h * HS + d) * BYTES;
    if constexpr (DT == UA2_BF16) *reinterpret_cast<unsigned*>(dst) = (unsigned)f2bf(o.x) | ((unsigned)f2bf(o.y) << 16);
    else *reinterpret_cast<float2*>(dst) = o;
  }
  if (!streamed) burst();
}

// The same prologue with the previous step's greedy tail folded in (ua2_argmax_fold, include/ua2hip.h): the workgroup reduces the
// arg-max partials itself — the 16 waves share them, one barrier, the candidates, order and tie / all-NaN rules of ua2_row_token — and
// takes q and the K / V row of this step's position from the per-id tables; older positions come from the cache page and do not depend
// on the id, so they are requested first.  on_id(row) runs once the table row is known, in front of the weight burst (the epilogue's
// residual is a table row too).  Workgroup 0 (`writer`) publishes what later launches read: the id, and the K / V row of the cache page
// (stored by the lanes that load it for the attention: every kv head is some query head's).
// `red`: 3 * kMaxWaves words of LDS nobody else uses before the MFMA phase.
template <int DT, int HS, typename Burst, typename OnId>
__device__ __forceinline__ void local_attn_fold_prologue(const ua2_linear_args& a, char* a_lds, float* red, int wave, int nw, int lane, bool writer,
                                                         Burst&& burst, OnId&& on_id) {
  using LA = LocalAttn<DT, HS>;
  constexpr int BYTES = Elem<DT>::BYTES;
  const ua2_argmax_fold& f = a.fold;
  const int pos = f.pos, tid = wave * 64 + lane;
  float bv = -INFINITY;
  int bi = UA2_TOK_NONE, lo = UA2_TOK_NONE;
  for (int p = tid; p < f.n_part; p += nw * 64) {
    const float v = f.part_max[p];
    const int i = f.part_idx[p];
    if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
    lo = min(lo, i);
  }
  const int page = a.kv.page_table[(size_t)kv_table_row(a, 0) * a.kv.max_pages];
  LA la;
  const int hl = lane / LA::LPH, d = (lane % LA::LPH) * 2;
  const bool mine = wave * LA::HPW < a.kv.n_head;             // wave-uniform: this wave has a first pass
  if (mine) la.issue_older(a.kv, page, wave * LA::HPW + hl, d, pos);
  bool streamed = false;
#ifdef UA2_FOLD_BURST_FIRST   // measurement build (profiles/b1_latency_chain.md): the weights go out before the id is known and the id-dependent
  burst();                    // loads land behind them: 9.80 us per launch against 9.01 us in the default order (burst once the id is known)
  streamed = true;
#endif
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float ov = __shfl_xor(bv, o);
    const int oi = __shfl_xor(bi, o);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    lo = min(lo, __shfl_xor(lo, o));
  }
  int* redi = reinterpret_cast<int*>(red);
  if (lane == 0) { red[wave] = bv; redi[kMaxWaves + wave] = bi; redi[2 * kMaxWaves + wave] = lo; }
  __syncthreads();
  bv = red[0]; bi = redi[kMaxWaves]; lo = redi[2 * kMaxWaves];
  for (int w = 1; w < nw; ++w) {
    const float ov = red[w];
    const int oi = redi[kMaxWaves + w];
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    lo = min(lo, redi[2 * kMaxWaves + w]);
  }
  const int tok = min(max(bi == UA2_TOK_NONE ? lo : bi, 0), f.limit - 1);   // nobody won (all NaN): the lowest candidate id
  const size_t row = (size_t)((long long)tok + f.row_off);
  const size_t kvw = (size_t)a.kv.n_kv * HS;                   // elements of a K (V) table row
  const float* q_row = f.tab_q + row * a.K;
  const char* k_row = reinterpret_cast<const char*>(f.tab_k) + row * kvw * BYTES;
  const char* v_row = reinterpret_cast<const char*>(f.tab_v) + row * kvw * BYTES;
  on_id(row);
  for (int h0 = wave * LA::HPW; h0 < a.kv.n_head; h0 += nw * LA::HPW) {
    const int h = h0 + hl;
    if (h0 != wave * LA::HPW) la.issue_older(a.kv, page, h, d, pos);
    la.issue_row(a.kv, q_row, k_row, v_row, h, d, pos, writer, page);     // the writer's lanes also put the K / V row into the cache page
    if (!streamed) { burst(); streamed = true; }
    const float2 o = la.finish(pos);
    char* dst = a_lds + ((size_t)h * HS + d) * BYTES;
    if constexpr (DT == UA2_BF16) *reinterpret_cast<unsigned*>(dst) = (unsigned)f2bf(o.x) | ((unsigned)f2bf(o.y) << 16);
    else *reinterpret_cast<float2*>(dst) = o;
  }
  if (!streamed) burst();
  if (writer && tid == 0) *f.out_token = tok;
}

// fp8 weights (W8 != 0; include/ua2hip.h ua2_pack_linear_w8).  One 16-byte lane load of the fp8 image carries the lane's B fragments of
// TWO chunks (2j: bytes 0-7, 2j + 1: bytes 8-15), so a wave streams half the bytes of the bf16 launch in half as many 1 KiB bursts.
// Eight OCP e4m3fn codes -> the bf16 B fragment of one chunk, exactly (an e4m3 value has 4 significant bits and sits inside the bf16
// exponent range, subnormals included): v_cvt_pk_f32_fp8 x 4, v_cvt_pk_bf16_f32 x 4.  The row's power-of-two scale is NOT applied here
// but once on the reduced tile (a power of two commutes with every fp32 rounding of the chain and of the cross-wave sum).
// (dequant_e4m3x8: ua2_linear_common.h — the weights-stationary kernel of ua2_skinny.hip reads the same image.)

// ---- lossless 13-bit image (W8 = 3 / 4; include/ua2hip.h ua2_pack_linear_l13) ------------------------------------------------------
// Per 16-column tile and group of 4 chunks, 3328 B in dense planes: 2 x 1 KiB of low bytes (E[0] | mantissa; the fp8 image's shape: a lane's
// 16 bytes are its 8 of chunk 2p and its 8 of chunk 2p + 1), 1 KiB of codes (a lane's dword per chunk: byte b = q of element b | q of element
// b + 4 << 4) and 256 B of signs (a lane's dword per group: bit 8 b + 2 c + h = sign of element 4 h + b of chunk c).  Decoding is SWAR on
// four high bytes at a time — s | (q ? base + q : 0) — and one v_perm_b32 per two weights interleaves them with the low bytes: the B
// fragment the bf16 image holds, bit for bit.  Counted in the ISA of gemv_l13_kernel<SCALED, SWIGLU, 4, true, 3>: 23 VALU per chunk
// of 8 weights (2 nibble masks + a shift, 2 x (add, and, shift, sub, add, and) for the exponent bytes, 2 x (shift, and-or) for the signs,
// 4 perms), 2.9 per weight.
constexpr int kL13Group = 208;                                 // u32x4 per group: 64 + 64 low, 64 codes, 16 of signs
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
struct L13Group { u32x4 lo0, lo1, code; unsigned sign; };      // W8 = 3: a lane's share of a whole group, 13 dwords for 4 chunks
struct L13Chunk { u32x2 lo; unsigned code, sign; };            // W8 = 4: of one chunk (the group's sign dword whole)
template <int W8> struct WFrag { using type = u32x4; };
template <> struct WFrag<3> { using type = L13Group; };
template <> struct WFrag<4> { using type = L13Chunk; };

// chunk `cg` of its group: low bytes of elements 0-3 / 4-7, the chunk's code dword, the group's sign dword; base4 = the tile's base in every byte
__device__ __forceinline__ u32x4 l13_decode(unsigned lo_a, unsigned lo_b, unsigned code, unsigned sign, int cg, unsigned base4) {
  auto high = [&](unsigned qb, int bit) {
    const unsigned nz = (qb + 0x7f7f7f7fu) & 0x80808080u;      // bit 7 of a byte: q != 0 (q <= 15: no carry)
    const unsigned keep = nz - (nz >> 7);                      // 0x7f where q != 0: E[7:1] has seven bits (base + q <= 127)
    return ((sign << (7 - bit)) & 0x80808080u) | ((qb + base4) & keep);
  };
  const unsigned h_a = high(code & 0x0f0f0f0fu, 2 * cg), h_b = high((code >> 4) & 0x0f0f0f0fu, 2 * cg + 1);
  return u32x4{__builtin_amdgcn_perm(h_a, lo_a, 0x05010400u), __builtin_amdgcn_perm(h_a, lo_a, 0x07030602u),
               __builtin_amdgcn_perm(h_b, lo_b, 0x05010400u), __builtin_amdgcn_perm(h_b, lo_b, 0x07030602u)};
}

// 1 KiB burst of the weight image that load `u` of the round starting at chunk `cb` fetches (`last` = the wave's last chunk: clamped, never predicated)
template <int W8>
__device__ __forceinline__ int burst_index(int cb, int u, int last) {
  if constexpr (W8 == 1) return min((cb >> 1) + u, last >> 1);
  else if constexpr (W8 == 2) return min(cb + u, last) >> 1;
  else return min(cb + u, last);
}

// load `u` of the round starting at chunk `cb`: a 1 KiB burst (W8 <= 2; wp carries the lane), a group's four planes (3), a chunk's share of them (4)
template <int W8>
__device__ __forceinline__ typename WFrag<W8>::type weight_load(const u32x4* wp, int lane, int cb, int u, int last) {
  if constexpr (W8 == 3) {
    const u32x4* p = wp + (size_t)min((cb >> 2) + u, last >> 2) * kL13Group;
    L13Group f;
    f.sign = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(p + 192) + lane);
    f.code = __builtin_nontemporal_load(p + 128 + lane);
    f.lo0 = __builtin_nontemporal_load(p + lane);
    f.lo1 = __builtin_nontemporal_load(p + 64 + lane);
    return f;
  } else if constexpr (W8 == 4) {
    const int c = min(cb + u, last);
    const u32x4* p = wp + (size_t)(c >> 2) * kL13Group;
    L13Chunk f;
    f.sign = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(p + 192) + lane);
    f.code = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(p + 128 + lane) + (c & 3));
    f.lo = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p + ((c >> 1) & 1) * 64 + lane) + (c & 1));
    return f;
  } else {
    return __builtin_nontemporal_load(wp + (size_t)burst_index<W8>(cb, u, last) * 64);
  }
}

// ---- hot arguments: what a launch reads in front of its weight burst -------------------------------------------------------------------
// ua2_linear_args is 700-odd bytes of kernel arguments, and the fields the path up to the burst reads lie in five or more 64-byte lines of
// them: the kernels fetched them in two or three batches of scalar loads, each a round trip the burst stood behind.  The hot kernels
// (gemv_hot_kernel) take those fields as their FIRST parameters instead, 14 dwords of pointers and packed ints: one line of the segment,
// and what the dispatcher can place in user SGPRs before the wave starts (kernarg preload; uniaudio2_amd/build.py gives the option to this
// file).  Everything else still comes from the ua2_linear_args that follows them, read behind the burst.  GemvHot is the decoded form
// gemv_body works on; the by-value kernels (launches whose values do not fit the packed fields; the riders) fill it from ua2_linear_args.
struct GemvHot {
  const void *w0, *w1, *e0, *e1;   // weight stream(s): a.w0 / a.w1 or the image's q0 / q1; the image's side arrays
  const void *x;                   // the operand rows: a.x_h (bf16 rows) or a.x
  const void *p, *q;               // by form (hot_roles)
  const int32_t* row_seq;          // QKV_ROPE; the hot kernels serve row_seq == NULL only
  int K, N, M, nthreads, ldx, ldp, rt, norm_kind;
};
// the packed form, in kernel-parameter order: 4 pointers, the other three as offsets from w in 16-byte units, 3 dwords of ints
struct GemvHotArgs {
  const void *w, *x, *p, *q;
  int o1, oe0, oe1;
  unsigned kn, mw, ld;             // K | N << 16;  M | waves << 16 | rt << 21 | norm_kind << 26;  ldx | ldp << 16
};

// Which of a's fields a (prologue, epilogue) form reads in front of its burst besides the weights: the operand rows and their stride; p =
// the sum-of-squares partials (SCALED), the norm weight (NORM) or the residual rows with their stride (RESIDUAL: never with those two);
// q = the row positions (QKV_ROPE, LOCAL_ATTN) or the arg-max floor (STORE with partials).
template <int PRO, int EPI>
__host__ __device__ __forceinline__ void hot_roles(const ua2_linear_args& a, const void*& x, int& ldx, const void*& p, int& ldp, const void*& q) {
  constexpr bool ROWH = PRO == UA2_PRO_SCALED || PRO == kProRowH;
  x = ROWH ? static_cast<const void*>(a.x_h) : static_cast<const void*>(a.x);
  ldx = PRO == UA2_PRO_SCALED ? a.ldh : a.ldx;                 // x_h in x's place (kProRowH): x's stride
  p = nullptr; ldp = 0; q = nullptr;
  if constexpr (PRO == UA2_PRO_SCALED) p = a.x_ssq;
  else if constexpr (PRO == UA2_PRO_NORM) p = a.norm_w;
  else if constexpr (EPI == UA2_EPI_RESIDUAL) { p = a.resid; ldp = a.ldr; }
  if constexpr (EPI == UA2_EPI_QKV_ROPE || PRO == UA2_PRO_LOCAL_ATTN) q = a.row_pos;
  else if constexpr (EPI == UA2_EPI_STORE) q = a.part_max ? static_cast<const void*>(a.forbid) : nullptr;
}

template <int PRO, int EPI>
__device__ __forceinline__ GemvHot hot_from_args(const ua2_linear_args& a, const Ua2WImage* w8, int rt) {
  GemvHot h;
  h.w0 = w8 ? w8->q0 : a.w0; h.w1 = w8 ? w8->q1 : a.w1;
  h.e0 = w8 ? w8->e0 : nullptr; h.e1 = w8 ? w8->e1 : nullptr;
  hot_roles<PRO, EPI>(a, h.x, h.ldx, h.p, h.ldp, h.q);
  h.row_seq = a.row_seq;
  h.K = a.K; h.N = a.N; h.M = a.M; h.nthreads = blockDim.x; h.rt = rt; h.norm_kind = a.norm_kind;
  return h;
}

template <int EPI, int W8>
__device__ __forceinline__ GemvHot hot_unpack(const void* w, const void* x, const void* p, const void* q, int o1, int oe0, int oe1,
                                              unsigned kn, unsigned mw, unsigned ld) {
  auto at = [&](int o) { return static_cast<const void*>(static_cast<const char*>(w) + (ptrdiff_t)o * 16); };
  GemvHot h;
  h.w0 = w; h.w1 = EPI == UA2_EPI_SWIGLU ? at(o1) : nullptr;
  h.e0 = W8 != 0 ? at(oe0) : nullptr; h.e1 = (W8 != 0 && EPI == UA2_EPI_SWIGLU) ? at(oe1) : nullptr;
  h.x = x; h.p = p; h.q = q; h.row_seq = nullptr;
  h.K = (int)(kn & 0xffffu); h.N = (int)(kn >> 16);
  h.M = (int)(mw & 0xffffu); h.nthreads = (int)((mw >> 16) & 31u) * 64; h.rt = (int)((mw >> 21) & 31u); h.norm_kind = (int)(mw >> 26);
  h.ldx = (int)(ld & 0xffffu); h.ldp = (int)(ld >> 16);
  return h;
}

// Size of the hot block in the kernel arguments (4 pointers, 6 dwords): where gemv_hot_kernel's ua2_linear_args starts.
constexpr int kHotBytes = 4 * 8 + 6 * 4;
static_assert(kHotBytes == 14 * 4 && kHotBytes % alignof(ua2_linear_args) == 0, "the hot block is 14 dwords and ua2_linear_args follows it without padding");
// The launch's ua2_linear_args for the code behind the burst.  Left to itself the compiler issues some of their scalar loads at the kernel's
// entry, and a register one of them is still to land in is soon wanted for the hot block's address arithmetic: a wait on ALL of them in
// front of the burst, which is what the hot block is there to remove (seen in the ISA of the q|k|v form; tools/kernel_entry.py).  So a HOT
// instantiation reads them through the kernel-argument pointer taken HERE: the empty asm is opaque to the scheduler, no load through it
// moves above this point.  (LOCAL_ATTN forms: their prologue reads the attention's geometry in front of the burst anyway; a0 as it is.)
template <bool HOT>
__device__ __forceinline__ const ua2_linear_args& cold_args(const ua2_linear_args& a0) {
  if constexpr (HOT) {
    const __attribute__((address_space(4))) char* kp = (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kp) : : "memory");
    return *reinterpret_cast<const ua2_linear_args*>((const char*)(kp + kHotBytes));
  } else {
    return a0;
  }
}

// LDS carve of a launch, one definition for the launcher and the hot kernels (the by-value kernels get both numbers as arguments): the
// operand rows' stride in elements (+16 B per row: breaks the power-of-two row stride, LDS bank conflicts across rows) and the offset of the
// reduction buffers behind the rows actually present.
__host__ __device__ __forceinline__ int carve_a_stride(int nchunks, int kc, int bytes) { return nchunks * kc + 16 / bytes; }
__host__ __device__ __forceinline__ int carve_red_off(int M, int rt, int a_stride, int bytes) {
  return (int)(((size_t)(M < rt ? M : rt) * a_stride * bytes + 255) & ~(size_t)255);
}

// epilogue_prefetch_a (ua2_linear_common.h) on the hot block: the same loads into the same fields, no address from a cold argument
template <int EPI>
__device__ __forceinline__ void hot_prefetch_a(const GemvHot& h, int tile0, int row, int col, EpiPre& p, int m0) {
  const int mr = m0 + row;
  if (mr >= h.M) return;
  const int n = tile0 * 16 + col;
  if constexpr (EPI == UA2_EPI_STORE) {
    if (h.q) p.forbid = static_cast<const int32_t*>(h.q)[mr];
  } else if constexpr (EPI == UA2_EPI_RESIDUAL) {
    if (n < h.N) p.resid = static_cast<const float*>(h.p)[(size_t)mr * h.ldp + n];
  } else if constexpr (EPI == UA2_EPI_QKV_ROPE) {
    p.pos = static_cast<const int32_t*>(h.q)[mr];
    p.page = h.row_seq ? h.row_seq[mr] : mr;   // table row for now; resolved to a page id in stage B
  }
}

// MR = multi-round: <= 8 waves per workgroup, several rounds of CPW chunks per wave, next round's
// weights prefetched (double buffer); !MR = single burst: up to 16 waves, everything up front.
// W8: 0 = the weights of a.w0 / a.w1 in the launch dtype; 1 = fp8 image, the wave's chunk range is a whole number of rounds of CPW
// chunks (every shape of the released model): CPW / 2 loads per round; 2 = fp8 image, any range of up to CPW chunks (odd starts,
// single-chunk ranges: small K): one load per chunk, the half picked by the chunk's parity.  The geometry, the chunk order inside a
// wave's chain and the order of the cross-wave sum are those of W8 = 0, whatever the form.
// 3 / 4 = the lossless 13-bit image of the same bf16 weights (l13_decode above), shaped like 1 / 2: 3 = whole rounds, one load set per group of 4
// chunks (a wave's range starts on a group: CPW >= 4), decoded chunk by chunk as the planes land (the round in flight behind it in the
// multi-round forms); 4 = any range of up to CPW chunks, a load set per chunk.  No scale: the decoded fragment IS the bf16 one.
// FOLD (UA2_PRO_LOCAL_ATTN, W8 = 0): the launch carries a ua2_argmax_fold; an instantiation of its own, so that the plain launches keep
// their registers (the CPW = 16 forms sit at the 128-register limit of a 16-wave workgroup).
// HOT: the instantiation of gemv_hot_kernel.  a0 = the launch's ua2_linear_args as the path up to the burst may see them — in a HOT
// instantiation only where a prologue cannot do without (the attention's geometry, LayerNorm's bias); behind the burst the body reads `a`.
template <int DT, int PRO, int EPI, int CPW, bool MR, int W8 = 0, bool FOLD = false, bool HOT = false>
__device__ __forceinline__ void gemv_body(const ua2_linear_args& a0, const GemvHot& h, char* smem, const int a_stride, const int red_off,
                                          const int bx, const int by) {
  constexpr int KC = Elem<DT>::KC, EPL = Elem<DT>::EPL, BYTES = Elem<DT>::BYTES;
  constexpr int NT = (EPI == UA2_EPI_SWIGLU) ? 2 : 1;
  static_assert(W8 == 0 || DT == UA2_BF16, "fp8 weights and 13-bit images are bf16-plan options");
  constexpr bool FP8 = W8 == 1 || W8 == 2, L13 = W8 == 3 || W8 == 4;
  constexpr int NL = (W8 == 1) ? CPW / 2 : (W8 == 3) ? CPW / 4 : CPW;     // weight loads (load sets) per matrix per round
  using WF = typename WFrag<W8>::type;
  char* a_lds = smem;                                        // [rows][a_stride] of T
  float* red = reinterpret_cast<float*>(smem + red_off);     // [nw][NT][256]
  float* ssq = red + kMaxWaves * NT * 256;                   // [nw][16]
  float* ssum = ssq + kMaxWaves * 16;                        // [nw][16]
  float* rstd_s = ssum + kMaxWaves * 16;                     // [16]
  float* mean_s = rstd_s + 16;                               // [16]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nthreads = h.nthreads, nw = nthreads >> 6;   // not blockDim.x: that is a load from the hidden arguments, far behind the hot block
  const int i = lane & 15, g = lane >> 4;
  const int rt = h.rt;
  const int m0 = by * rt;                    // rt rows per workgroup: a function of K and dtype only
  const int rows = min(rt, h.M - m0);

  // Up to the burst every argument comes from h (the hot block); a's other fields are read behind it.
  const int nchunks = (h.K + KC - 1) / KC;
  int tile[NT];
  const u32x4* wp[NT];
  if constexpr (L13) {                                         // [N/16][K/128] groups of kL13Group x 16 B (K % 128 == 0); the lane goes on in weight_load
    tile[0] = bx;
    wp[0] = reinterpret_cast<const u32x4*>(h.w0) + (size_t)bx * (nchunks >> 2) * kL13Group;
    if constexpr (NT == 2) { tile[1] = bx; wp[1] = reinterpret_cast<const u32x4*>(h.w1) + (size_t)bx * (nchunks >> 2) * kL13Group; }
  } else if constexpr (W8 != 0) {                              // [N/16][K/64][64 lanes][16 B]: nchunks / 2 bursts per tile (K % 64 == 0)
    tile[0] = bx;
    wp[0] = reinterpret_cast<const u32x4*>(h.w0) + (size_t)bx * (nchunks >> 1) * 64 + lane;
    if constexpr (NT == 2) { tile[1] = bx; wp[1] = reinterpret_cast<const u32x4*>(h.w1) + (size_t)bx * (nchunks >> 1) * 64 + lane; }
  } else if constexpr (EPI == UA2_EPI_SWIGLU) {
    tile[0] = tile[1] = bx;
    wp[0] = reinterpret_cast<const u32x4*>(h.w0) + (size_t)tile[0] * nchunks * 64 + lane;
    wp[1] = reinterpret_cast<const u32x4*>(h.w1) + (size_t)tile[0] * nchunks * 64 + lane;
  } else {
    tile[0] = bx;
    wp[0] = reinterpret_cast<const u32x4*>(h.w0) + (size_t)tile[0] * nchunks * 64 + lane;
  }
  // chunk range of this wave; rounds of CPW chunks (exactly one round for the model's shapes)
  const int c0 = (wave * nchunks) / nw, c1 = ((wave + 1) * nchunks) / nw;
  const int last = max(c1 - 1, 0);

  // Issue order matters: a wave's loads return in order, so everything small that the prologue or
  // the epilogue needs goes out BEFORE the weight burst (it then completes in one L2 round trip
  // while the weights are still streaming), never behind it.
  constexpr int XPT = 2;  // float4 per thread kept in registers on the single-row fast path
  constexpr bool ROWH = PRO == UA2_PRO_SCALED || PRO == kProRowH;     // the operand arrives as bf16 rows (a.x_h)
  const bool one = (PRO != UA2_PRO_LOCAL_ATTN) && !ROWH && (rows == 1) && (h.K <= XPT * 4 * nthreads);
  // UA2_PRO_SCALED: the operand row(s) arrive already rounded (RNE_bf16(x (.) w), written by the producer of x): a 16-byte
  // copy into the LDS tile — no statistics, no conversion, one barrier.  The first row's piece goes out before the weights.
  // kProRowH (UA2_PRO_CAST with x_h): the same copy of RNE_bf16(x), rounded once by x's producer instead of in every workgroup —
  // half the operand bytes in front of the burst; no statistics and no row scale.
  u32x4 xh0 = u32x4{0u, 0u, 0u, 0u};
  const int ldxh = h.ldx;                                          // kProRowH (x_h in x's place): x's stride; SCALED: ldh (hot_roles)
  if constexpr (ROWH) {
    if (tid * 8 < h.K) xh0 = *reinterpret_cast<const u32x4*>(reinterpret_cast<const unsigned short*>(h.x) + (size_t)m0 * ldxh + tid * 8);
  }
  float4 xv[XPT], nv[XPT], nb[XPT];
  const bool ln = (PRO == UA2_PRO_NORM) && h.norm_kind == UA2_NORM_LAYERNORM;
  const float* x_f = static_cast<const float*>(h.x);               // !ROWH: a.x
  const float* norm_w = static_cast<const float*>(h.p);            // UA2_PRO_NORM: a.norm_w
  if (one) {
    const float* xr = x_f + (size_t)m0 * h.ldx;
#pragma unroll
    for (int it = 0; it < XPT; ++it) {
      const int k = (tid + it * nthreads) * 4;
      xv[it] = make_float4(0.f, 0.f, 0.f, 0.f);
      nv[it] = make_float4(1.f, 1.f, 1.f, 1.f);
      nb[it] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (k < h.K) {
        xv[it] = *reinterpret_cast<const float4*>(xr + k);
        if constexpr (PRO == UA2_PRO_NORM) {
          nv[it] = *reinterpret_cast<const float4*>(norm_w + k);
          if (ln) nb[it] = *reinterpret_cast<const float4*>(a0.norm_b + k);
        }
      }
    }
  }
  EpiPre pre;
  static_assert(!FOLD || (PRO == UA2_PRO_LOCAL_ATTN && EPI == UA2_EPI_RESIDUAL && W8 == 0), "ua2_argmax_fold: the O-projection of the local attention");
  // (FOLD: the residual is a table row, known once the prologue has the id)
  if (tid < 256 && !FOLD) hot_prefetch_a<EPI>(h, tile[0], tid >> 4, tid & 15, pre, m0);
  float ssqv[16];                                        // UA2_PRO_SCALED: the row's sum-of-squares partials, requested before the burst
  if constexpr (PRO == UA2_PRO_SCALED) {
    if (tid < 256) scaled_ssq_request(static_cast<const float*>(h.p), h.K, h.M, m0 + min(tid >> 4, rows - 1), tid & 15, ssqv);
  }
  // fp8 weights: exponent of this thread's epilogue column (16 bytes per tile, padded to 16 columns: in bounds for every thread).  Every
  // thread loads it, not just the 256 epilogue threads: a load under a lane predicate ends in a wait in front of the weight burst
  int wexp[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) wexp[t] = 0;
  if constexpr (FP8) {
    wexp[0] = static_cast<const int8_t*>(h.e0)[bx * 16 + (tid & 15)];
    if constexpr (NT == 2) wexp[1] = static_cast<const int8_t*>(h.e1)[bx * 16 + (tid & 15)];
  }
  // 13-bit image: the tile's base byte (workgroup-uniform, needed at decode time only), spread to the four bytes of a dword
  unsigned base4[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) base4[t] = 0u;
  if constexpr (L13) {
    base4[0] = (unsigned)static_cast<const uint8_t*>(h.e0)[bx] * 0x01010101u;
    if constexpr (NT == 2) base4[1] = (unsigned)static_cast<const uint8_t*>(h.e1)[bx] * 0x01010101u;
  }

  // Every other argument, for the code behind the burst.  Single-round forms: requested HERE and not before (cold_args) — the scalar loads
  // go out with the weights and land under them; nothing up to the end of the burst reads one, so nothing in front of it waits for them.
  // Multi-round forms: left to the compiler, which issues some at the kernel's entry.  Pinned, their round trip stood between the first
  // burst and the barrier, i.e. in front of the SECOND round's loads, and the frame measured slower (profiles/hot_args.md: the trunk
  // q|k|v 8.33 -> 8.71 us per launch); the price is one wait in front of the burst in the q|k|v forms (four before the hot block).
  const ua2_linear_args a = cold_args < HOT && !MR && PRO != UA2_PRO_LOCAL_ATTN > (a0);
  WF wf[NT][NL];
  auto burst = [&]() {
#pragma unroll
    for (int u = 0; u < NL; ++u)
#pragma unroll
      for (int t = 0; t < NT; ++t) wf[t][u] = weight_load<W8>(wp[t], lane, c0, u, last);
  };
  if constexpr (PRO == UA2_PRO_LOCAL_ATTN) {
    if constexpr (FOLD) {
      auto on_id = [&](size_t row) {
        const int n = tile[0] * 16 + (tid & 15);
        if (tid < 16 && n < h.N) pre.resid = a0.fold.tab_y[row * h.N + n];       // epilogue row 0 (M == 1)
      };
      const bool writer = bx == 0 && by == 0;
      switch (a0.kv.head_size) {
        case 32: local_attn_fold_prologue<DT, 32>(a0, a_lds, ssq, wave, nw, lane, writer, burst, on_id); break;
        case 64: local_attn_fold_prologue<DT, 64>(a0, a_lds, ssq, wave, nw, lane, writer, burst, on_id); break;
        default: local_attn_fold_prologue<DT, 128>(a0, a_lds, ssq, wave, nw, lane, writer, burst, on_id); break;
      }
    } else
    switch (a0.kv.head_size) {
      case 32: local_attn_prologue<DT, 32>(a0, a_lds, m0, wave, nw, lane, burst); break;
      case 64: local_attn_prologue<DT, 64>(a0, a_lds, m0, wave, nw, lane, burst); break;
      default: local_attn_prologue<DT, 128>(a0, a_lds, m0, wave, nw, lane, burst); break;
    }
  } else {
    burst();
  }
  if (tid < 256) epilogue_prefetch_b<DT, EPI>(a, tile[0], tid >> 4, tid & 15, pre, m0);

  // ---- stage the activation rows into LDS (operand dtype) ----
  auto put = [&](int r0, int k, float4 t) {
    char* dst = a_lds + ((size_t)r0 * a_stride + k) * BYTES;
    if constexpr (DT == UA2_BF16) {
      uint2 p;
      p.x = (unsigned)f2bf(t.x) | ((unsigned)f2bf(t.y) << 16);
      p.y = (unsigned)f2bf(t.z) | ((unsigned)f2bf(t.w) << 16);
      *reinterpret_cast<uint2*>(dst) = p;
    } else {
      *reinterpret_cast<float4*>(dst) = t;
    }
  };
  if constexpr (PRO == UA2_PRO_LOCAL_ATTN) {
    // operand row already in LDS
  } else if constexpr (ROWH) {
    static_assert(DT == UA2_BF16 || !ROWH, "bf16 operand rows are a bf16 contract");
    const int kpad = nchunks * KC;                               // K % 32 == 0 (checked by the launcher): kpad == K
    // The piece requested before the burst is written in straight-line code: its wait then counts the loads issued behind it and lets
    // the burst stay in flight.  Inside the loop below it shared one wait with the pieces loaded there, and that wait is for EVERY
    // outstanding load: the LDS write, the barrier and the first MFMA stood behind the last weight fragment (the ISA showed vmcnt(0)).
    if (tid * 8 < kpad) *reinterpret_cast<u32x4*>(a_lds + (size_t)tid * 8 * BYTES) = xh0;
    for (int r0 = 0; r0 < rows; ++r0) {        // what is left: further pieces of a long row, further rows (they queue behind the burst)
      const unsigned short* xr = reinterpret_cast<const unsigned short*>(h.x) + (size_t)(m0 + r0) * ldxh;
      for (int k = (r0 == 0 ? nthreads : 0) * 8 + tid * 8; k < kpad; k += nthreads * 8)
        *reinterpret_cast<u32x4*>(a_lds + ((size_t)r0 * a_stride + k) * BYTES) = *reinterpret_cast<const u32x4*>(xr + k);
    }
  } else if (one) {
    NormStat st{0.f, 1.f, 0.f};
    if constexpr (PRO == UA2_PRO_NORM) {
      float ss = 0.f, sm = 0.f;
#pragma unroll
      for (int it = 0; it < XPT; ++it) {
        ss = sumsq4(ss, xv[it]);
        sm = sum4(sm, xv[it]);
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) { ss += __shfl_xor(ss, o); sm += __shfl_xor(sm, o); }
      if (lane == 0) { ssq[wave * 16] = ss; ssum[wave * 16] = sm; }
      __syncthreads();
      float t = 0.f, u = 0.f;
      for (int w = 0; w < nw; ++w) { t += ssq[w * 16]; u += ssum[w * 16]; }   // every thread, same order: no second barrier
      st = norm_stat(a, u, t);
      if (ln) {                                // second pass (norm_stat_centred), the first pass's order
        float cs = 0.f, sd = 0.f;
#pragma unroll
        for (int it = 0; it < XPT; ++it)
          if ((tid + it * nthreads) * 4 < h.K) centred4(cs, sd, xv[it], st.mean);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { cs += __shfl_xor(cs, o); sd += __shfl_xor(sd, o); }
        __syncthreads();                       // every thread has read the first pass's partials
        if (lane == 0) { ssq[wave * 16] = cs; ssum[wave * 16] = sd; }
        __syncthreads();
        float c = 0.f, d = 0.f;
        for (int w = 0; w < nw; ++w) { c += ssq[w * 16]; d += ssum[w * 16]; }
        norm_stat_centred(a, st, c, d);
      }
    }
#pragma unroll
    for (int it = 0; it < XPT; ++it) {
      const int k = (tid + it * nthreads) * 4;
      if (k < nchunks * KC) {                             // also zero-fills the K padding of the last chunk
        float4 t = xv[it];
        if constexpr (PRO == UA2_PRO_NORM) {
          if (k < h.K) {
            t.x = norm_apply(a, t.x, nv[it].x, nb[it].x, st);
            t.y = norm_apply(a, t.y, nv[it].y, nb[it].y, st);
            t.z = norm_apply(a, t.z, nv[it].z, nb[it].z, st);
            t.w = norm_apply(a, t.w, nv[it].w, nb[it].w, st);
          }
        }
        put(0, k, t);
      }
    }
  } else {
    if constexpr (PRO == UA2_PRO_NORM) {
      for (int r0 = 0; r0 < rows; ++r0) {  // pass 1: sum and sum of squares per row
        const float* xr = x_f + (size_t)(m0 + r0) * h.ldx;
        float ss = 0.f, sm = 0.f;
        for (int k = tid * 4; k < h.K; k += nthreads * 4) {
          const float4 t = *reinterpret_cast<const float4*>(xr + k);
          ss = sumsq4(ss, t);
          sm = sum4(sm, t);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { ss += __shfl_xor(ss, o); sm += __shfl_xor(sm, o); }
        if (lane == 0) { ssq[wave * 16 + r0] = ss; ssum[wave * 16 + r0] = sm; }
      }
      __syncthreads();
      if (tid < rows) {
        float t = 0.f, u = 0.f;
        for (int w = 0; w < nw; ++w) { t += ssq[w * 16 + tid]; u += ssum[w * 16 + tid]; }
        const NormStat st = norm_stat(a, u, t);
        rstd_s[tid] = st.rstd; mean_s[tid] = st.mean;
      }
      __syncthreads();
      if (ln) {                                // second pass per row (norm_stat_centred), the first pass's order
        for (int r0 = 0; r0 < rows; ++r0) {
          const float* xr = x_f + (size_t)(m0 + r0) * h.ldx;
          const float mean = mean_s[r0];
          float cs = 0.f, sd = 0.f;
          for (int k = tid * 4; k < h.K; k += nthreads * 4) centred4(cs, sd, *reinterpret_cast<const float4*>(xr + k), mean);
#pragma unroll
          for (int o = 32; o >= 1; o >>= 1) { cs += __shfl_xor(cs, o); sd += __shfl_xor(sd, o); }
          if (lane == 0) { ssq[wave * 16 + r0] = cs; ssum[wave * 16 + r0] = sd; }
        }
        __syncthreads();
        if (tid < rows) {
          float c = 0.f, d = 0.f;
          for (int w = 0; w < nw; ++w) { c += ssq[w * 16 + tid]; d += ssum[w * 16 + tid]; }
          NormStat st{mean_s[tid], 1.f, 0.f};
          norm_stat_centred(a, st, c, d);
          rstd_s[tid] = st.rstd;
          ssum[tid] = st.mean_lo;              // row tid's own column of partials: nobody else reads it
        }
        __syncthreads();
      }
    }
    for (int r0 = 0; r0 < rows; ++r0) {
      const float* xr = x_f + (size_t)(m0 + r0) * h.ldx;
      NormStat st{0.f, 1.f, 0.f};
      if constexpr (PRO == UA2_PRO_NORM) { st.rstd = rstd_s[r0]; st.mean = mean_s[r0]; if (ln) st.mean_lo = ssum[r0]; }
      for (int k = tid * 4; k < nchunks * KC; k += nthreads * 4) {
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k < h.K) {
          t = *reinterpret_cast<const float4*>(xr + k);
          if constexpr (PRO == UA2_PRO_NORM) {
            const float4 w = *reinterpret_cast<const float4*>(norm_w + k);
            float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ln) b = *reinterpret_cast<const float4*>(a.norm_b + k);
            t.x = norm_apply(a, t.x, w.x, b.x, st);
            t.y = norm_apply(a, t.y, w.y, b.y, st);
            t.z = norm_apply(a, t.z, w.z, b.z, st);
            t.w = norm_apply(a, t.w, w.w, b.w, st);
          }
        }
        put(r0, k, t);
      }
    }
  }
  if constexpr (PRO == UA2_PRO_SCALED) {
    if (tid < 256) pre.rstd = scaled_rstd_reduce(a, tid & 15, ssqv);     // requested before the burst: landed long ago
  }
  __syncthreads();

  // ---- MFMA over this wave's chunks ----
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool arow = i < rows;
  const char* abase = a_lds + ((size_t)i * a_stride + g * EPL) * BYTES;
  for (int cb = c0; cb < c1; cb += CPW) {
    // multi-round geometries: the next round's weights go out before this round's MFMAs
    WF wn[NT][MR ? NL : 1];
    const bool more = MR && (cb + CPW < c1);
    if constexpr (MR) if (more) {
#pragma unroll
      for (int u = 0; u < NL; ++u)
#pragma unroll
        for (int t = 0; t < NT; ++t) wn[t][u] = weight_load<W8>(wp[t], lane, cb + CPW, u, last);
    }
#pragma unroll
    for (int u = 0; u < CPW; ++u) {
      const int c = cb + u;
      AFrag<DT> af;
      u32x4 raw = u32x4{0u, 0u, 0u, 0u};
      if (arow && c < c1) raw = *reinterpret_cast<const u32x4*>(abase + (size_t)c * KC * BYTES);
      af.v = __builtin_bit_cast(decltype(af.v), raw);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        if constexpr (W8 == 1) {                           // chunk cb + u: half (u & 1) of load u / 2 (cb is even)
          const u32x4 w = wf[t][u >> 1];
          af.mma(dequant_e4m3x8(w[(u & 1) * 2], w[(u & 1) * 2 + 1]), acc[t]);
        } else if constexpr (W8 == 2) {                    // chunk c: half (c & 1) of its own load (a clamped chunk meets a zero A fragment)
          const u32x4 w = wf[t][u];
          const bool odd = (min(c, last) & 1) != 0;
          af.mma(dequant_e4m3x8(odd ? w[2] : w[0], odd ? w[3] : w[1]), acc[t]);
        } else if constexpr (W8 == 3) {                    // chunk cb + u: chunk u % 4 of load set u / 4 (cb is a multiple of 4)
          const L13Group& w = wf[t][u >> 2];
          const u32x4& lo = (u & 2) ? w.lo1 : w.lo0;
          af.mma(l13_decode(lo[(u & 1) * 2], lo[(u & 1) * 2 + 1], w.code[u & 3], w.sign, u & 3, base4[t]), acc[t]);
        } else if constexpr (W8 == 4) {                    // chunk c: its own load set (a clamped chunk meets a zero A fragment)
          const L13Chunk& w = wf[t][u];
          af.mma(l13_decode(w.lo[0], w.lo[1], w.code, w.sign, min(c, last) & 3, base4[t]), acc[t]);
        } else {
          af.mma(wf[t][u], acc[t]);
        }
      }
    }
    if constexpr (MR) {
      if (more) {
#pragma unroll
        for (int u = 0; u < NL; ++u)
#pragma unroll
          for (int t = 0; t < NT; ++t) wf[t][u] = wn[t][u];
      }
    } else if (cb + CPW < c1) {  // rare: single-burst geometry that does not tile K exactly
#pragma unroll
      for (int u = 0; u < NL; ++u)
#pragma unroll
        for (int t = 0; t < NT; ++t) wf[t][u] = weight_load<W8>(wp[t], lane, cb + CPW, u, last);
    }
  }

  // ---- fixed-order cross-wave reduction, epilogue ----
#pragma unroll
  for (int t = 0; t < NT; ++t) *reinterpret_cast<f32x4*>(&red[(wave * NT + t) * 256 + lane * 4]) = acc[t];
  __syncthreads();
  if (tid >= 256) return;
  const int row = tid >> 4, col = tid & 15;
  const int src = (((row >> 2) << 4) + col) * 4 + (row & 3);
  float v[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    float s = 0.f;
    for (int w = 0; w < nw; ++w) s += red[(w * NT + t) * 256 + src];
    v[t] = s;
    // fp8 weights: the column's scale 2^e, once, on the reduced sum (exact: e in [-117, 120] keeps 2^e a normal float)
    if constexpr (FP8) v[t] = __fmul_rn(s, __uint_as_float((unsigned)(wexp[t] + 127) << 23));
  }
  linear_epilogue<DT, EPI, NT, true, true>(a, v, tile, row, col, pre, m0, rows);
}

template <int DT, int PRO, int EPI, int CPW, bool MR, bool FOLD = false>
__global__ __launch_bounds__(MR ? 512 : kMaxWaves * 64) void gemv_kernel(const ua2_linear_args a, const int a_stride,
                                                              const int red_off, const int rt) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemv_body<DT, PRO, EPI, CPW, MR, 0, FOLD>(a, hot_from_args<PRO, EPI>(a, nullptr, rt), smem, a_stride, red_off, blockIdx.x, blockIdx.y);
}

// The hot form of the three kernels below and above (W8 as gemv_body's): the hot block first — pointers and ints only, a by-value struct in
// front of them would keep the dispatcher from preloading any — then ua2_linear_args for everything read behind the burst.  The image's
// pointers travel in the hot block, so there is no Ua2WImage parameter.
template <int DT, int PRO, int EPI, int CPW, bool MR, int W8, bool FOLD = false>
__global__ __launch_bounds__(MR ? 512 : kMaxWaves * 64) void gemv_hot_kernel(const void* hw, const void* hx, const void* hp, const void* hq,
                                                                  const int o1, const int oe0, const int oe1, const unsigned kn,
                                                                  const unsigned mw, const unsigned ld, const ua2_linear_args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const GemvHot h = hot_unpack<EPI, W8>(hw, hx, hp, hq, o1, oe0, oe1, kn, mw, ld);
  const int a_stride = carve_a_stride((h.K + Elem<DT>::KC - 1) / Elem<DT>::KC, Elem<DT>::KC, Elem<DT>::BYTES);
  gemv_body<DT, PRO, EPI, CPW, MR, W8, FOLD, true>(a, h, smem, a_stride, carve_red_off(h.M, h.rt, a_stride, Elem<DT>::BYTES), blockIdx.x, blockIdx.y);
}

// the same launch on the fp8 image of its weight(s): bf16 activations in LDS, bf16 MFMA, half the weight bytes
template <int PRO, int EPI, int CPW, bool MR, int W8>
__global__ __launch_bounds__(MR ? 512 : kMaxWaves * 64) void gemv_w8_kernel(const ua2_linear_args a, const int a_stride,
                                                                 const int red_off, const int rt, const Ua2WImage w8) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemv_body<UA2_BF16, PRO, EPI, CPW, MR, W8>(a, hot_from_args<PRO, EPI>(a, &w8, rt), smem, a_stride, red_off, blockIdx.x, blockIdx.y);
}

// ... and on the lossless 13-bit image of the bf16 weights themselves (W8 = 3 / 4): 13/16 of the bytes, the same bits
template <int PRO, int EPI, int CPW, bool MR, int W8>
__global__ __launch_bounds__(MR ? 512 : kMaxWaves * 64) void gemv_l13_kernel(const ua2_linear_args a, const int a_stride,
                                                                  const int red_off, const int rt, const Ua2WImage w8) {
  static_assert(W8 == 3 || W8 == 4, "the 13-bit forms");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  gemv_body<UA2_BF16, PRO, EPI, CPW, MR, W8>(a, hot_from_args<PRO, EPI>(a, &w8, rt), smem, a_stride, red_off, blockIdx.x, blockIdx.y);
}

// ---- riders: a second, independent one-row-tile GEMV carried by the idle CUs of a launch that cannot fill the device -----------
// Why.  A CU takes in at most ~31 GB/s of an HBM stream (~64 KB in flight per CU: profiles/r6_notes.md), so a launch with fewer
// workgroups than CUs is capped below the HBM rate by the CUs it does not use: the depth decoder's down-projection (K = 8192 ->
// N = 2048: 128 workgroups of 262 KB) streams 33.5 MB in 10.6 us = 3.2 TB/s with half the device idle, 32 times per frame.
// lm_head (model_new.py:617: 788 MB, 114 us on its own) depends only on the trunk's output, not on the depth decoder
// (:629-640), and a forked graph branch replays 0.4 ms per frame SLOWER on ROCm 7.2 (measured in rounds 1 and 6).  So its column
// tiles ride along: workgroups past the host's grid each take TWO rider tiles (waves 0-7 and 8-15: the rider's eight K ranges
// each, the operand row staged once), and one slice of lm_head goes with every down-projection launch of the frame.
// Same bits as the rider's own launch (gemv_kernel<bf16, CAST, STORE, 4, MR>): the bf16 operand row, per range one MFMA chain
// over its CPWR chunks in order, the eight partial sums added in range order from zero, linear_epilogue.
template <int CPWR>
__device__ __forceinline__ void rider_body(const ua2_linear_args& a, char* smem, const int tile0, const int tile1, const int rid) {
  constexpr int DT = UA2_BF16, KC = 32, NWR = 8;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = wave >> 3, wv = wave & 7;
  const int i = lane & 15, g = lane >> 4;
  const int rows = a.M;                                      // one row tile (the launcher checks)
  constexpr int nchunks = NWR * CPWR;                        // == K / 32 (the launcher checks)
  constexpr int a_stride = nchunks * KC + 8;
  char* a_lds = smem;
  float* red = reinterpret_cast<float*>(smem + (((size_t)rows * a_stride * 2 + 255) & ~(size_t)255));     // [2][NWR][256]
  const int tile = tile0 + 2 * rid + half;
  const bool live = tile < tile1;                            // wave-uniform
  const int tl = min(tile, tile1 - 1);
  const u32x4* wp = reinterpret_cast<const u32x4*>(a.w0) + ((size_t)tl * nchunks + wv * CPWR) * 64 + lane;
  const int et = tid & 511;                                  // epilogue thread of this half: (row, col) = (et >> 4, et & 15)
  // small loads first (a wave's loads return in order): the single-row operand piece, the epilogue's row data
  const bool one = rows == 1 && a.K <= 4 * kMaxWaves * 64;
  float4 xv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (one && tid * 4 < a.K) xv = *reinterpret_cast<const float4*>(a.x + tid * 4);
  EpiPre pre;
  if (et < 256) epilogue_prefetch_a<DT, UA2_EPI_STORE>(a, tl, et >> 4, et & 15, pre, 0);
  u32x4 wf[CPWR];
#pragma unroll
  for (int u = 0; u < CPWR; ++u) wf[u] = __builtin_nontemporal_load(wp + (size_t)u * 64);
  if (et < 256) epilogue_prefetch_b<DT, UA2_EPI_STORE>(a, tl, et >> 4, et & 15, pre, 0);
  auto put = [&](int r0, int k, const float4& t) {
    uint2 p;
    p.x = (unsigned)f2bf(t.x) | ((unsigned)f2bf(t.y) << 16);
    p.y = (unsigned)f2bf(t.z) | ((unsigned)f2bf(t.w) << 16);
    *reinterpret_cast<uint2*>(a_lds + ((size_t)r0 * a_stride + k) * 2) = p;
  };
  if (one) {
    if (tid * 4 < a.K) put(0, tid * 4, xv);
  } else {
    for (int r0 = 0; r0 < rows; ++r0)
      for (int k = tid * 4; k < a.K; k += kMaxWaves * 64 * 4) put(r0, k, *reinterpret_cast<const float4*>(a.x + (size_t)r0 * a.ldx + k));
  }
  __syncthreads();
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool arow = i < rows;
  const char* abase = a_lds + ((size_t)i * a_stride + g * 8) * 2 + (size_t)(wv * CPWR) * KC * 2;
#pragma unroll
  for (int u = 0; u < CPWR; ++u) {
    AFrag<DT> af;
    u32x4 raw = u32x4{0u, 0u, 0u, 0u};
    if (arow) raw = *reinterpret_cast<const u32x4*>(abase + (size_t)u * KC * 2);
    af.v = raw;
    af.mma(wf[u], acc);
  }
  *reinterpret_cast<f32x4*>(&red[((half * NWR + wv) * 256) + lane * 4]) = acc;
  __syncthreads();
  if (et >= 256 || !live) return;
  const int row = et >> 4, col = et & 15;
  const int src = (((row >> 2) << 4) + col) * 4 + (row & 3);
  float v[1];
  {
    float sacc = 0.f;
    for (int w = 0; w < NWR; ++w) sacc += red[(half * NWR + w) * 256 + src];
    v[0] = sacc;
  }
  const int tl1[1] = {tile};
  linear_epilogue<DT, UA2_EPI_STORE, 1>(a, v, tl1, row, col, pre, 0, rows);
}

// host = a single-burst 16-wave bf16 instantiation of gemv_body (one row tile); workgroups >= host_gx are riders
template <int PRO, int EPI, int CPW, int CPWR>
__global__ __launch_bounds__(kMaxWaves * 64) void gemv_rider_kernel(const ua2_linear_args a, const int a_stride, const int red_off, const int rt,
                                                                    const ua2_linear_args ra, const int tile0, const int tile1, const int host_gx) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  if ((int)blockIdx.x < host_gx) gemv_body<UA2_BF16, PRO, EPI, CPW, false>(a, hot_from_args<PRO, EPI>(a, nullptr, rt), smem, a_stride, red_off, blockIdx.x, 0);
  else rider_body<CPWR>(ra, smem, tile0, tile1, (int)blockIdx.x - host_gx);
}

constexpr size_t kLdsABudget = 112 * 1024;   // activation tile budget (of 160 KiB; the rest holds the reduction buffers)

}  // namespace
int ua2_gemv_rows_per_tile(int dtype, int K) {
  const int kc = dtype == UA2_BF16 ? 32 : 16, bytes = dtype == UA2_BF16 ? 2 : 4;
  const size_t row_bytes = ((size_t)ua2_ceil_div(K, kc) * kc + 16 / bytes) * bytes;
  const int r = (int)(kLdsABudget / row_bytes);
  return r > 16 ? 16 : r;
}
// Rows up to which the launchers PREFER this kernel over the many-row ones (bf16; both give the same bits, so a pure cost choice).  The
// decode kernel stages every row of its tile in LDS in every workgroup: its frame grows ~0.14 ms per row (2.89 ms at 1 row, 3.58 at 5,
// 5.04 at 16), while the weights-stationary kernel runs 6 ... 16 rows in a flat 3.58-3.60 ms (tools/ubench/frame_vs_batch.py,
// profiles/r6_frame_vs_batch.txt) — until round 6 a 16-sequence batch decoded slower than a 64-sequence one.  UA2_GEMV_MAX_ROWS=n: sweeps.
int ua2_gemv_rows_preferred(int dtype, int K) {
  static const int pref = getenv("UA2_GEMV_MAX_ROWS") ? atoi(getenv("UA2_GEMV_MAX_ROWS")) : 5;       // read once
  const int r = ua2_gemv_rows_per_tile(dtype, K);
  return dtype == UA2_BF16 ? std::min(r, std::max(pref, 1)) : r;
}
namespace {
int rows_per_tile(int dtype, int K) { return ua2_gemv_rows_per_tile(dtype, K); }

struct Geometry {
  int waves, cpw;
};

// waves x cpw == nchunks when possible (no tail); prefer many waves for small grids (latency),
// fewer + deeper for large grids (two workgroups per CU overlap each other's prologue/epilogue).
Geometry pick_geometry(int nchunks, int blocks, int nt) {
  if (const char* e = getenv("UA2_GEMV_GEOM")) {  // experiment hook: "waves,cpw"
    int w = 0, c = 0;
    if (sscanf(e, "%d,%d", &w, &c) == 2 && w >= 1 && w <= kMaxWaves && (c == 4 || c == 8 || (c == 16 && nt == 1)) && w <= nchunks &&
        nchunks % w == 0 && (nchunks / w) % c == 0)
      return Geometry{w, c};
  }
  // measured (tools/ubench/gemv_shapes.py, profiles/r1_gemv_geometry.txt): grids larger than the CU
  // count stream best as 8-wave workgroups walking K in double-buffered rounds of 4 chunks (two
  // workgroups per CU overlap each other's reduce/epilogue); smaller grids as one wide burst.
  // (K = 2048 -> 64 chunks included: the local decoder's SwiGLU runs 13.1 us this way vs 16.0 us as one burst)
  if (blocks > 256 && nchunks >= 64 && nchunks % 32 == 0) return Geometry{8, 4};
  const int cap = (nt == 2) ? 8 : 16;
  const int cpws[3] = {4, 8, 16};
  Geometry best{0, 0};
  int best_score = -1;
  for (int w = 4; w <= kMaxWaves; ++w) {
    for (int ci = 0; ci < 3; ++ci) {
      const int c = cpws[ci];
      if (c > cap || w * c != nchunks) continue;
      int score = (blocks <= 320) ? w * 4 + c : (w >= 8 && w <= 12 ? 100 : 0) + c;
      if (score > best_score) { best_score = score; best = Geometry{w, c}; }
    }
  }
  if (best.waves) return best;
  // no exact tiling: 16 waves (or fewer if K is tiny), rounds of `cap` chunks with clamped loads
  int w = kMaxWaves;
  while (w > 4 && nchunks < w) w >>= 1;
  int per = (nchunks + w - 1) / w;
  int c = per <= 4 ? 4 : (per <= 8 ? 8 : cap);
  return Geometry{w, c};
}

// grid, workgroup and LDS carve of a launch: a function of (N, K, M, dtype), the same whatever the weight stream
struct Launch {
  dim3 grid;
  int waves, a_stride, red_off, rt;
  size_t smem;
  hipStream_t s;
};

// One launch of a decode-kernel instantiation.  extra: the weight image of gemv_w8_kernel / gemv_l13_kernel; counters: the families it counts in.
template <auto Kern, class... Extra>
void launch_one(std::initializer_list<int> counters, const ua2_linear_args& a, const Launch& l, const Extra&... extra) {
  ua2_allow_big_lds<Kern>();
  hipLaunchKernelGGL(Kern, l.grid, dim3(l.waves * 64), l.smem, l.s, a, l.a_stride, l.red_off, l.rt, extra...);
  for (const int c : counters) ua2_count_launch(c);
}

// The hot block of a launch (GemvHotArgs), or false where a value does not fit its packed field — 16 bits for K, N, M and the strides, a
// 16-byte-aligned distance of less than 2^31 x 16 B from the first weight pointer for the second one and the side arrays (the plan's images
// lie in one allocation), row_seq == NULL — and the launch takes the by-value kernel.  UA2_GEMV_NO_HOT=1: every launch does (A/B, tests).
template <int PRO, int EPI>
bool pack_hot(const ua2_linear_args& a, const Launch& l, bool mr, const Ua2WImage* img, GemvHotArgs& h) {
  static Ua2EnvInt off{"UA2_GEMV_NO_HOT", 0};
  if ((off.get() & 1) || (mr && (off.get() & 2))) return false;
  int ldx = 0, ldp = 0;
  hot_roles<PRO, EPI>(a, h.x, ldx, h.p, ldp, h.q);
  if (EPI == UA2_EPI_QKV_ROPE && a.row_seq) return false;
  h.w = img ? img->q0 : a.w0;
  auto rel = [&](const void* p, int& o) {
    o = 0;
    if (!p) return true;
    const long long d = static_cast<const char*>(p) - static_cast<const char*>(h.w);
    if (d % 16 != 0 || d / 16 > INT32_MAX || d / 16 < INT32_MIN) return false;
    o = (int)(d / 16);
    return true;
  };
  const bool two = EPI == UA2_EPI_SWIGLU;
  if (!rel(two ? (img ? img->q1 : a.w1) : nullptr, h.o1) || !rel(img ? img->e0 : nullptr, h.oe0) || !rel(img && two ? img->e1 : nullptr, h.oe1)) return false;
  auto u16 = [](int v) { return v >= 0 && v <= 0xffff; };
  if (!u16(a.K) || !u16(a.N) || !u16(a.M) || !u16(ldx) || !u16(ldp) || a.norm_kind < 0 || a.norm_kind > 3 || l.waves > 31 || l.rt > 31) return false;
  h.kn = (unsigned)a.K | (unsigned)a.N << 16;
  h.mw = (unsigned)a.M | (unsigned)l.waves << 16 | (unsigned)l.rt << 21 | (unsigned)a.norm_kind << 26;
  h.ld = (unsigned)ldx | (unsigned)ldp << 16;
  return true;
}
template <auto Kern>
void launch_hot(std::initializer_list<int> counters, const ua2_linear_args& a, const Launch& l, const GemvHotArgs& h) {
  ua2_allow_big_lds<Kern>();
  hipLaunchKernelGGL(Kern, l.grid, dim3(l.waves * 64), l.smem, l.s, h.w, h.x, h.p, h.q, h.o1, h.oe0, h.oe1, h.kn, h.mw, h.ld, a);
  for (const int c : counters) ua2_count_launch(c);
  ua2_count_launch(UA2_CNT_GEMV_HOT);     // besides the families the launch counts in: which form served it
}

// chunks one load (set) of an image form carries: a K that is no whole number of them has no image
constexpr int image_group(Ua2WForm form) { return form == UA2_W_L13 ? 4 : 2; }

// Which form of the image serves a geometry: 1 = every wave's range is whole rounds of cpw chunks (it then starts on a group: cpw >= 4);
// 2 = ranges of up to 4 chunks in one single-burst round of 4 (the small-K fall-back geometries), a load (set) per chunk; 0 = none (an
// offered image then stays unused: the launch reads a.w0 / a.w1).
int image_form(Ua2WForm form, int nchunks, const Geometry& geo) {
  if (nchunks % image_group(form)) return 0;
  if (nchunks % geo.waves == 0 && (nchunks / geo.waves) % geo.cpw == 0) return 1;
  const bool mr = geo.waves <= 8 && geo.waves * geo.cpw < nchunks;
  if (!mr && geo.cpw == 4 && ua2_ceil_div(nchunks, geo.waves) <= 4) return 2;
  return 0;
}

// the (prologue, epilogue) pairs of the bf16 decode frame: the ones with image instantiations
constexpr bool w8_pair(int pro, int epi) {
  switch (pro) {
    case UA2_PRO_NORM: case UA2_PRO_SCALED: return epi == UA2_EPI_QKV_ROPE || epi == UA2_EPI_SWIGLU || epi == UA2_EPI_STORE;
    case UA2_PRO_CAST: case kProRowH: return epi == UA2_EPI_RESIDUAL || epi == UA2_EPI_STORE;
    case UA2_PRO_LOCAL_ATTN: return epi == UA2_EPI_RESIDUAL;
    default: return false;
  }
}

// The one place a geometry becomes the compile-time (CPW, multi-round) pair of an instantiation: f(integral_constant<int, CPW>,
// bool_constant<MR>).  Rounds of 16 chunks exist as a single burst of one matrix (NT == 1); every other geometry above 4 runs rounds of 8.
template <int NT, class F>
void with_rounds(const Geometry& geo, bool mr, F&& f) {
  using std::integral_constant;
  if (geo.cpw == 4) return mr ? f(integral_constant<int, 4>{}, std::true_type{}) : f(integral_constant<int, 4>{}, std::false_type{});
  if (mr) return f(integral_constant<int, 8>{}, std::true_type{});
  if constexpr (NT == 1)
    if (geo.cpw != 8) return f(integral_constant<int, 16>{}, std::false_type{});
  return f(integral_constant<int, 8>{}, std::false_type{});
}

template <int DT, int PRO, int EPI>
int launch_cpw(const ua2_linear_args& a, hipStream_t s, const Ua2Weights* w = nullptr) {
  constexpr int KC = Elem<DT>::KC, BYTES = Elem<DT>::BYTES;
  constexpr int NT = (EPI == UA2_EPI_SWIGLU) ? 2 : 1;
  const int nchunks = ua2_ceil_div(a.K, KC);
  const int ntiles = ua2_ceil_div(a.N, 16);
  const int gx = ntiles;
  // rows per workgroup and launch geometry depend on (N, K, dtype) only — never on M — so that a row
  // sees the same instruction stream and summation order whatever the batch around it
  const Geometry geo = pick_geometry(nchunks, gx, NT);
  Launch l;
  l.waves = geo.waves; l.s = s;
  l.a_stride = carve_a_stride(nchunks, KC, BYTES);
  l.rt = rows_per_tile(a.dtype, a.K);
  // LDS is sized for the rows actually present (occupancy: two single-row workgroups share a CU);
  // the size changes nothing a row computes
  l.red_off = carve_red_off(a.M, l.rt, l.a_stride, BYTES);
  l.smem = (size_t)l.red_off + (size_t)(kMaxWaves * NT * 256 + 2 * kMaxWaves * 16 + 32) * sizeof(float);
  l.grid = dim3(gx, ua2_ceil_div(a.M, l.rt));
  const bool mr = geo.waves <= 8 && geo.waves * geo.cpw < nchunks;
  // What is instantiated beyond the plain kernels: image forms for the bf16 pairs of w8_pair, the arg-max fold for the O-projection of the
  // local attention in rounds of 4 or 8 chunks (attention-wide K).  A new weight form adds its rows here.
  constexpr bool IMAGE = DT == UA2_BF16 && w8_pair(PRO, EPI), FOLD = PRO == UA2_PRO_LOCAL_ATTN && EPI == UA2_EPI_RESIDUAL;
  int w8 = 0;     // gemv_body's W8: the same grid, waves, LDS carve and chunk ranges whatever it is, only the weight stream differs
  if (w) {
    const int form = IMAGE ? image_form(w->form, nchunks, geo) : 0;
    if (!form) return 1;
    w8 = (w->form == UA2_W_L13 ? 2 : 0) + form;
  }
  const bool fold = FOLD && a.fold.part_max;     // ua2_argmax_fold (never with an image: launch_dt)
  if (fold && (a.M != 1 || geo.cpw > 8)) return 1;
  // the hot form (gemv_hot_kernel): the bf16 pairs of the decode frame, the same set as the images'; the by-value kernels serve the rest
  GemvHotArgs hot;
  // (LOCAL_ATTN on an image stays by-value: its prologue reads the attention's geometry from ua2_linear_args in front of the burst in
  // either form, and the hot form measured 0.15 us per launch SLOWER inside the frame, twice: profiles/hot_args.md §3)
  const bool is_hot = IMAGE && !(PRO == UA2_PRO_LOCAL_ATTN && w8 != 0) && pack_hot<PRO, EPI>(a, l, mr, w8 ? &w->img : nullptr, hot);
  int rc = 1;
  with_rounds<NT>(geo, mr, [&](auto cpw, auto multi) {
    constexpr int CPW = decltype(cpw)::value;
    constexpr bool MR = decltype(multi)::value;
    rc = 0;
    if constexpr (IMAGE) {
      constexpr bool FALLBACK = CPW == 4 && !MR;     // the only geometry of forms 2 / 4 (image_form)
      if (is_hot && w8 == 0) {
        if constexpr (FOLD && CPW <= 8)
          if (fold) return launch_hot<gemv_hot_kernel<DT, PRO, EPI, CPW, MR, 0, true>>({UA2_CNT_GEMV}, a, l, hot);
        return launch_hot<gemv_hot_kernel<DT, PRO, EPI, CPW, MR, 0>>({UA2_CNT_GEMV}, a, l, hot);
      }
      if constexpr (PRO != UA2_PRO_LOCAL_ATTN) if (is_hot) switch (w8) {
        case 1: return launch_hot<gemv_hot_kernel<DT, PRO, EPI, CPW, MR, 1>>({UA2_CNT_GEMV_W8}, a, l, hot);
        case 3: return launch_hot<gemv_hot_kernel<DT, PRO, EPI, CPW, MR, 3>>({UA2_CNT_GEMV, UA2_CNT_GEMV_L13}, a, l, hot);
        case 2:
          if constexpr (FALLBACK) return launch_hot<gemv_hot_kernel<DT, PRO, EPI, 4, false, 2>>({UA2_CNT_GEMV_W8}, a, l, hot);
          rc = 1; return;
        case 4:
          if constexpr (FALLBACK) return launch_hot<gemv_hot_kernel<DT, PRO, EPI, 4, false, 4>>({UA2_CNT_GEMV, UA2_CNT_GEMV_L13}, a, l, hot);
          rc = 1; return;
      }
      switch (w8) {
        case 1: return launch_one<gemv_w8_kernel<PRO, EPI, CPW, MR, 1>>({UA2_CNT_GEMV_W8}, a, l, w->img);
        // bf16 weights through the decode kernel: a "gemv" launch as well (the counter's readers count launches of the frame)
        case 3: return launch_one<gemv_l13_kernel<PRO, EPI, CPW, MR, 3>>({UA2_CNT_GEMV, UA2_CNT_GEMV_L13}, a, l, w->img);
        case 2:
          if constexpr (FALLBACK) return launch_one<gemv_w8_kernel<PRO, EPI, 4, false, 2>>({UA2_CNT_GEMV_W8}, a, l, w->img);
          rc = 1; return;
        case 4:
          if constexpr (FALLBACK) return launch_one<gemv_l13_kernel<PRO, EPI, 4, false, 4>>({UA2_CNT_GEMV, UA2_CNT_GEMV_L13}, a, l, w->img);
          rc = 1; return;
      }
    }
    if constexpr (FOLD && CPW <= 8)
      if (fold) return launch_one<gemv_kernel<DT, PRO, EPI, CPW, MR, true>>({UA2_CNT_GEMV}, a, l);
    launch_one<gemv_kernel<DT, PRO, EPI, CPW, MR>>({UA2_CNT_GEMV}, a, l);
  });
  if (rc) return rc;
  UA2_LAUNCH_CHECK();
  return 0;
}

template <int DT>
int launch_dt(const ua2_linear_args& a, hipStream_t s, const Ua2Weights* w = nullptr) {
  // a weight image: a bf16 launch of the pairs of w8_pair without an arg-max fold (launch_cpw instantiates the image kernels for exactly those)
  if (w && (DT != UA2_BF16 || !w8_pair(a.prologue, a.epilogue) || a.fold.part_max)) return 1;
  if (a.prologue == UA2_PRO_NORM) {
    if (a.epilogue == UA2_EPI_QKV_ROPE) return launch_cpw<DT, UA2_PRO_NORM, UA2_EPI_QKV_ROPE>(a, s, w);
    if (a.epilogue == UA2_EPI_SWIGLU) return launch_cpw<DT, UA2_PRO_NORM, UA2_EPI_SWIGLU>(a, s, w);
    if (a.epilogue == UA2_EPI_STORE) return launch_cpw<DT, UA2_PRO_NORM, UA2_EPI_STORE>(a, s, w);
    if (a.epilogue == UA2_EPI_GELU) return launch_cpw<DT, UA2_PRO_NORM, UA2_EPI_GELU>(a, s, w);
  } else if (a.prologue == UA2_PRO_CAST && a.x_h) {      // bf16 operand rows (the launcher has checked: UA2_BF16, K % 32 == 0, ldx % 8 == 0)
    if constexpr (DT == UA2_BF16) {
      if (a.epilogue == UA2_EPI_RESIDUAL) return launch_cpw<DT, kProRowH, UA2_EPI_RESIDUAL>(a, s, w);
      if (a.epilogue == UA2_EPI_STORE) return launch_cpw<DT, kProRowH, UA2_EPI_STORE>(a, s, w);
    }
  } else if (a.prologue == UA2_PRO_CAST) {
    if (a.epilogue == UA2_EPI_RESIDUAL) return launch_cpw<DT, UA2_PRO_CAST, UA2_EPI_RESIDUAL>(a, s, w);
    if (a.epilogue == UA2_EPI_STORE) return launch_cpw<DT, UA2_PRO_CAST, UA2_EPI_STORE>(a, s, w);
    if (a.epilogue == UA2_EPI_SWIGLU) return launch_cpw<DT, UA2_PRO_CAST, UA2_EPI_SWIGLU>(a, s, w);     // codec GLU (no norm in front)
    if (a.epilogue == UA2_EPI_GELU) return launch_cpw<DT, UA2_PRO_CAST, UA2_EPI_GELU>(a, s, w);
    if (a.epilogue == UA2_EPI_QKV_ROPE) return launch_cpw<DT, UA2_PRO_CAST, UA2_EPI_QKV_ROPE>(a, s, w);
  } else if (a.prologue == UA2_PRO_LOCAL_ATTN) {
    if (a.epilogue == UA2_EPI_RESIDUAL) return launch_cpw<DT, UA2_PRO_LOCAL_ATTN, UA2_EPI_RESIDUAL>(a, s, w);
  } else if (a.prologue == UA2_PRO_SCALED) {
    if constexpr (DT == UA2_BF16) {
      if (a.epilogue == UA2_EPI_QKV_ROPE) return launch_cpw<DT, UA2_PRO_SCALED, UA2_EPI_QKV_ROPE>(a, s, w);
      if (a.epilogue == UA2_EPI_SWIGLU) return launch_cpw<DT, UA2_PRO_SCALED, UA2_EPI_SWIGLU>(a, s, w);
      if (a.epilogue == UA2_EPI_STORE) return launch_cpw<DT, UA2_PRO_SCALED, UA2_EPI_STORE>(a, s, w);
    }
  }
  return 1;  // combination not specialised here: the caller falls back to the general kernel
}

}  // namespace

// ---- riders (see gemv_rider_kernel) ------------------------------------------------------------------------------------------
namespace {
// host forms with a rider instantiation: (prologue, epilogue, chunks per wave) of a 16-wave single-burst launch.  Only the
// down-projection (K = 8192, 10.6 us: longer than a rider workgroup's own ~8 us) carries riders: on the 6-us launches (q|k|v and
// o-projection of the depth decoder: forms measured in round 6, profiles/r6_notes.md) a rider workgroup outlasts its host and the
// frame got SLOWER (3.18 against 3.11 ms).
int rider_host_form(const ua2_linear_args& a, const Geometry& geo) {
  if (geo.waves != 16) return -1;
  if (a.prologue == UA2_PRO_CAST && a.epilogue == UA2_EPI_RESIDUAL && geo.cpw == 16) return 0;
  return -1;
}
}  // namespace

// Can launches of `a`'s shape (the host) carry column tiles of `r` (the rider)?  A function of the two problems only, so a plan
// decides once.  Host: a bf16 launch of one row tile in a single-burst 16-wave geometry (rider_host_form) whose grid leaves CUs
// idle.  Rider: bf16 CAST / STORE (+ arg-max partials), no bias / hand-over, the 8-range x 12-chunk geometry its own launch would
// take (K = 3072), the same rows.
bool ua2_gemv_rider_ok(const ua2_linear_args& a, const ua2_linear_args& r) {
  static Ua2EnvInt off{"UA2_NO_RIDER", 0};
  if (off.set()) return false;
  if (a.dtype != UA2_BF16 || a.K % 32 || a.x_packed) return false;
  if (a.x_h ? (a.ldx % 8 != 0 || a.ldx < a.K || (reinterpret_cast<uintptr_t>(a.x_h) & 15)) : !a.x) return false;     // the host's operand: bf16 rows (16-byte pieces) or fp32 x
  const int nch = a.K / 32, gx = ua2_ceil_div(a.N, 16);
  const Geometry geo = pick_geometry(nch, gx, 1);
  if (geo.waves * geo.cpw != nch || gx >= 256 || rider_host_form(a, geo) < 0) return false;
  if (a.M > ua2_gemv_rows_preferred(a.dtype, a.K) || r.M != a.M) return false;      // the host launch must be one the launchers give this kernel
  if (r.dtype != UA2_BF16 || r.prologue != UA2_PRO_CAST || r.epilogue != UA2_EPI_STORE || r.K != 3072 || !r.x || r.ldx % 4) return false;
  if (r.bias || r.y_norm_w || r.x_packed || r.M > rows_per_tile(r.dtype, r.K)) return false;
  const Geometry rg = pick_geometry(r.K / 32, ua2_ceil_div(r.N, 16), 1);
  return rg.waves == 8 && rg.waves * 12 == r.K / 32;       // what the rider's own launch sums like (8 ranges of 12 chunks)
}

// The host launch with rider tiles [tile0, tile1) of `r` on workgroups past its grid.  0 = launched, 1 = not applicable.
int ua2_gemv_launch_with_rider(const ua2_linear_args& a, const ua2_linear_args& r, int tile0, int tile1, hipStream_t s) {
  if (!ua2_gemv_rider_ok(a, r)) return 1;
  const int nchunks = a.K / 32, gx = ua2_ceil_div(a.N, 16);
  const int form = rider_host_form(a, pick_geometry(nchunks, gx, 1));
  const int a_stride = nchunks * 32 + 8;
  const int red_off = (int)(((size_t)a.M * a_stride * 2 + 255) & ~(size_t)255);
  const size_t host_smem = (size_t)red_off + (size_t)(kMaxWaves * 256 + 2 * kMaxWaves * 16 + 32) * sizeof(float);
  const size_t rider_smem = (((size_t)r.M * (r.K + 8) * 2 + 255) & ~(size_t)255) + (size_t)2 * 8 * 256 * sizeof(float);
  const size_t smem = std::max(host_smem, rider_smem);
  const int riders = tile1 > tile0 ? ua2_ceil_div(tile1 - tile0, 2) : 0;
  const int rt = rows_per_tile(a.dtype, a.K);
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(gx + riders, 1), dim3(kMaxWaves * 64), smem, s, a, a_stride, red_off, rt, r, tile0, tile1, gx);
  };
#define UA2_RIDER(PRO_, EPI_, CPW_) { constexpr auto kern = gemv_rider_kernel<PRO_, EPI_, CPW_, 12>; ua2_allow_big_lds<kern>(); go(kern); }
  if (form != 0) return 1;
  if (a.x_h) UA2_RIDER(kProRowH, UA2_EPI_RESIDUAL, 16)       // the host's operand as bf16 rows (ua2_gemv_rider_ok has checked them)
  else UA2_RIDER(UA2_PRO_CAST, UA2_EPI_RESIDUAL, 16)
#undef UA2_RIDER
  ua2_count_launch(UA2_CNT_GEMV);
  UA2_LAUNCH_CHECK();
  return 0;
}

int ua2_gemv_fold_ok(int dtype, int N, int K) {
  const int kc = dtype == UA2_BF16 ? 32 : 16;
  return pick_geometry(ua2_ceil_div(K, kc), ua2_ceil_div(N, 16), 1).cpw <= 8 ? 1 : 0;
}

ua2_gemv_geometry ua2_pick_gemv_geometry(int dtype, int N, int K, int nt) {
  const int kc = dtype == UA2_BF16 ? 32 : 16;
  const Geometry g = pick_geometry(ua2_ceil_div(K, kc), ua2_ceil_div(N, 16), nt);
  return ua2_gemv_geometry{g.waves, g.cpw};
}

extern "C" int ua2_debug_gemv_geometry(int dtype, int32_t N, int32_t K, int32_t nt, int32_t* waves, int32_t* cpw, int32_t* multi_round) {
  UA2_CHECK(waves && cpw && multi_round && N > 0 && K > 0 && (nt == 1 || nt == 2), "ua2_debug_gemv_geometry: bad arguments");
  const int nchunks = ua2_ceil_div(K, dtype == UA2_BF16 ? 32 : 16);
  const Geometry g = pick_geometry(nchunks, ua2_ceil_div(N, 16), nt);
  *waves = g.waves; *cpw = g.cpw; *multi_round = (g.waves <= 8 && g.waves * g.cpw < nchunks) ? 1 : 0;
  return 0;
}

// does the decode kernel have a form on an image of this kind for the launch (ua2_common.h: ua2_gemv_w8_ok / ua2_gemv_l13_ok)?
static bool image_ok(Ua2WForm form, const ua2_linear_args& a) {
  if (a.dtype != UA2_BF16 || a.K % (32 * image_group(form)) || a.N <= 0 || !w8_pair(a.prologue, a.epilogue) || rows_per_tile(a.dtype, a.K) < 1) return false;
  const int nt = a.epilogue == UA2_EPI_SWIGLU ? 2 : 1;
  return image_form(form, a.K / 32, pick_geometry(a.K / 32, ua2_ceil_div(a.N, 16), nt)) != 0;
}
bool ua2_gemv_w8_ok(const ua2_linear_args& a) { return image_ok(UA2_W_FP8, a); }
bool ua2_gemv_l13_ok(const ua2_linear_args& a) { return !a.fold.part_max && image_ok(UA2_W_L13, a); }

// Returns 0 if launched, 1 if this problem is outside the decode regime (caller uses the general
// kernel), negative on error.
int ua2_gemv_try_launch(const ua2_linear_args& a, hipStream_t s, const Ua2Weights* w) {
  if (rows_per_tile(a.dtype, a.K) < 1) return 1;   // a single row does not fit the LDS budget
  if (w) {
    const bool ok = w->form == UA2_W_L13 ? ua2_gemv_l13_ok(a) : ua2_gemv_w8_ok(a);
    if (w->complete(a.epilogue) && ok) return launch_dt<UA2_BF16>(a, s, w);
    if (w->by_name()) return 1;                    // asked for by name: never a.w0 / a.w1 in its place
  }                                                // an offered image the decode kernel has no form for: the launch reads a.w0 / a.w1 (the same bits)
  if (a.dtype == UA2_BF16) return launch_dt<UA2_BF16>(a, s);
  if (a.dtype == UA2_F32) return launch_dt<UA2_F32>(a, s);
  return 1;
}
