// Multi-head attention core, exact fp32 on the f32 matrix cores (gfx950 v_mfma_f32_32x32x2_f32),
// flash style (no score matrix in memory), head_dim 64.
//
//   out[b, q, h*64 + d] = sum_k softmax_k(scale * Q[b,q,h,:] . K[b,k,h,:]) V[b,k,h,d]
//
// This is the arithmetic torch.nn.MultiheadAttention performs between its in- and out-projections,
// which is what every attention operator of the reference's decoder bottoms out in
// (/root/reference/projects/mmdet3d_plugin/models/simpb_head.py:298-321 -> mmcv MultiheadAttention,
// models/group_attn.py:25-133, models/aggregation.py:96-99). Optionally camera-grouped: query slot q
// attends only key slots of its own camera group (query_cam / group_start device tables). That is
// the reference's N2 x N2 additive mask with -inf across groups (group_attn.py:104-113) without the
// mask tensor and without the cross-group score work; slots with query_cam < 0 (capacity padding)
// produce zeros, which is what nan_to_num gives the reference's fully-masked rows (:131).
//
// Mapping: one workgroup = 32 queries of one (batch, head); its 4 waves split the key tiles (32 keys
// each) and merge their (max, sum, O) partials through LDS at the end. Orientation follows the
// "key on the register, query on the lane" form: S^T = K.Q^T puts each query's scores of a tile in
// ONE lane pair, so the row max/sum are in-register plus one xor-32 shuffle, and the accumulator
// tile is directly the B operand of O^T += V^T.P^T (k-order of the second product follows the
// accumulator's row map), leaving O^T with the query on the lane again for the rescale.
#include <hip/hip_runtime.h>
#include "../../include/simpb_hip.h"

#include "launch.h"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
constexpr int kHD = 64;
constexpr int kWaves = 4;  // (8 waves per workgroup, 2 per SIMD, measured no faster: 406 vs 391 us per frame)

// A second key / value set for some streams of the batch (the ungrouped forms; simpb_attention_select): the workgroups of
// stream b read the kernel's own (k, v, Nk, ldk, ldv) where select[b] == 0 and this set otherwise -- a workgroup-uniform
// choice of five scalars taken once, in front of everything that reads them, so a stream's rows are the bits the kernel
// gives on the set it selected alone and no address of the other set is ever formed (it may hold anything, NaN included).
// A batch of streams in which one restarts cold: its temporal attention runs over its own current instances while its
// neighbours attend their cached ones (simpb_amd/runner.py `restart`). The kernels take it as a trailing parameter PACK:
// empty for the entry points that have one set, whose kernels are then the functions they were, instruction for instruction.
struct AltKeys {
  const unsigned char* select;
  const float* k;
  const float* v;
  int Nk, ldk, ldv;
};
#define SIMPB_PICK_KEYS()                                                \
  if constexpr (sizeof...(Alt) != 0) {                                   \
    const AltKeys a[] = {alt...};                                        \
    if (a[0].select[blockIdx.z] != 0) {                                  \
      k = a[0].k; v = a[0].v; Nk = a[0].Nk; ldk = a[0].ldk; ldv = a[0].ldv; \
    }                                                                    \
  }

// ---------------------------------------------------------------------------------------------------------------------
// Parts that the three kernels of this file share, each written once:
//   Tile, KeyRange, group_range<GROUPED>   who a lane is, and the key range of its query tile and of its own query
//   load_q_row                  a query's 32 head dims of this lane, zeros for a dead query; the caller's per-quad operation
//                               scales (f32), scales and splits (f16s) or unpacks (halfs)
//   load_k_tile, load_v_tile    a key tile's operand rows with the clamp rule (and the unclamped form of a full tile)
//   key_ok<GROUPED>             which (query, key) pairs are scored
//   split4, unpack4, pv_split_step<PACKED_V>   one k group of O^T += V^T.P^T on split operands: six matrix instructions
//   meet_four_and_store<Exp>    four waves' (max, sum, O) partials meet in LDS, are normalised and stored
// NOT merged, on purpose. The three tile loops stay three bodies; their differences are measured decisions, recorded in
// the comments of each:
//   * attention_f32_kernel double-buffers K (the next tile's rows requested ahead of the matrix work and held there by a
//     sched_barrier) and multiplies exact fp32 operands;
//   * attention_f16s_kernel keeps that pipeline on operands split in the kernel and sums four split terms of S;
//   * attention_halfs_kernel reloads K into the registers just consumed, sums three terms, works in base 2, skips masks
//     and clamps on full tiles, zeroes dead queries' probabilities and rescales under a ballot. Its eight-wave hand-over
//     stays in front of the shared meeting, in that kernel.
// What was measured about sharing them: profiles/attention_shared_parts.md.

__device__ __forceinline__ int acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// Lane (qi, half) of wave `wave` serves query qg = 32 * blockIdx.x + qi of (batch b, head); q_ok: that query exists.
struct Tile {
  int lane, wave, qi, half, head, b, qg;
  bool q_ok;
};
__device__ __forceinline__ Tile this_tile(int wave, int Nq) {
  Tile t;
  t.lane = threadIdx.x & 63;
  t.wave = wave;
  t.qi = t.lane & 31;
  t.half = t.lane >> 5;
  t.head = blockIdx.y;
  t.b = blockIdx.z;
  t.qg = blockIdx.x * 32 + t.qi;
  t.q_ok = t.qg < Nq;
  return t;
}

// The workgroup's keys are [kb, ke); this lane's query attends keys [my_lo, my_hi): its own camera group (groups are
// contiguous slot ranges), or every key.
struct KeyRange {
  int kb, ke, my_lo, my_hi;
};

// UNIFORM: kb / ke through readfirstlane (every lane holds the same two values; the eight-wave kernel wants them in scalar
// registers for its loop bounds and its full-tile test).
template <bool GROUPED, bool UNIFORM = false>
__device__ __forceinline__ KeyRange group_range(const int* __restrict__ query_cam, const int* __restrict__ group_start,
                                                const Tile& t, int Nk) {
  KeyRange r{0, Nk, 0, Nk};
  if (GROUPED) {
    const int cam_q = t.q_ok ? query_cam[t.qg] : -1;
    int lo = cam_q >= 0 ? group_start[cam_q] : 0x7fffffff;
    int hi = cam_q >= 0 ? group_start[cam_q + 1] : 0;
    r.my_lo = lo;
    r.my_hi = hi;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      lo = min(lo, __shfl_xor(lo, m));
      hi = max(hi, __shfl_xor(hi, m));
    }
    // a tile made only of capacity slots (cam -1) has no group at all: empty key range. (lo stays
    // INT_MAX there; adding the wave offset to it would wrap around.)
    const bool any = hi > lo;
    r.kb = any ? lo : 0;
    r.ke = any ? min(hi, Nk) : 0;
    if (UNIFORM) {
      r.kb = __builtin_amdgcn_readfirstlane(r.kb);
      r.ke = __builtin_amdgcn_readfirstlane(r.ke);
    }
  }
  return r;
}

// Q^T operand: lane (query qi, half) reads Q[query][32*half + 4c + i], c = 0..7, and hands each quad to op(c, x). A dead
// query reads nothing and hands over zeros.
template <class Op>
__device__ __forceinline__ void load_q_row(const float* __restrict__ q, const Tile& t, int Nq, int ldq, Op op) {
  const float* qp = q + ((size_t)t.b * Nq + (t.q_ok ? t.qg : 0)) * ldq + t.head * kHD + 32 * t.half;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float4 w = t.q_ok ? *reinterpret_cast<const float4*>(qp + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float x[4] = {w.x, w.y, w.z, w.w};
    op(c, x);
  }
}

// K rows of the tile at kt: lane (key qi, half) holds K[kt + qi][32*half + s], s = 0..31. kbase: the first key of this
// (batch, head) at column 32*half. Rows past the range read the first key of the range instead (finite values): their
// scores are masked to -inf (their probability is 0), so no select touches the loaded registers before the product needs
// them. full (wave-uniform: the whole tile lies inside the range): the unclamped address.
__device__ __forceinline__ void load_k_tile(float (&kreg)[32], const float* kbase, int kt, const Tile& t, const KeyRange& r,
                                            int ldk, bool full = false) {
  const int kk = kt + t.qi;
  const float* kp = kbase + (size_t)(full || kk < r.ke ? kk : r.kb) * ldk;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float4 w = *reinterpret_cast<const float4*>(kp + 4 * j);
    kreg[4 * j + 0] = w.x; kreg[4 * j + 1] = w.y; kreg[4 * j + 2] = w.z; kreg[4 * j + 3] = w.w;
  }
}

// V values of the tile at kt: lane (d, half) holds V[kt + acc_row(s, half)][d] in a0[s] and [d + 32] in a1[s], s = 0..15.
// vbase: the first key at column d = qi. Past the range: the first key of the range (weight 0). full: unclamped, with the
// row base kt + 4 * half taken once.
__device__ __forceinline__ void load_v_tile(float (&a0)[16], float (&a1)[16], const float* vbase, int kt, const Tile& t,
                                            const KeyRange& r, int ldv, bool full = false) {
  if (full) {
    const float* vt = vbase + (size_t)(kt + 4 * t.half) * ldv;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const float* vp = vt + (size_t)acc_row(s, 0) * ldv;
      a0[s] = vp[0];
      a1[s] = vp[32];
    }
  } else {
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const int kidx = kt + acc_row(s, t.half);
      const float* vp = vbase + (size_t)(kidx < r.ke ? kidx : r.kb) * ldv;
      a0[s] = vp[0];
      a1[s] = vp[32];
    }
  }
}

// Is key kidx scored for this lane's query: inside the tile's range, a live query, and (grouped) the query's own group
// (= query_cam[kidx] == cam_q, without 16 loads per tile in front of the softmax).
template <bool GROUPED>
__device__ __forceinline__ bool key_ok(int kidx, const KeyRange& r, bool q_ok) {
  bool ok = kidx < r.ke && q_ok;
  if (GROUPED) ok = ok && kidx >= r.my_lo && kidx < r.my_hi;
  return ok;
}

// x = hi + lo / 2^11 in two halfs (22 bits); see attention_f16s_kernel.
__device__ __forceinline__ void split4(const float* x, h16x4& hi, h16x4& lo) {
  hi = h16x4{(_Float16)x[0], (_Float16)x[1], (_Float16)x[2], (_Float16)x[3]};
  lo = h16x4{(_Float16)((x[0] - (float)hi[0]) * 2048.f), (_Float16)((x[1] - (float)hi[1]) * 2048.f),
             (_Float16)((x[2] - (float)hi[2]) * 2048.f), (_Float16)((x[3] - (float)hi[3]) * 2048.f)};
}

// Packed operands (attention_halfs_kernel, behind simpb_attention_split_halfs): the producer (csrc/gemm.hip, out_fmt =
// SIMPB_GEMM_OUT_SPLIT_HALFS) already left every element as its two halfs in the element's own 32-bit word (hi in the low
// 16 bits, lo * 2^11 in the high 16 bits): same strides, same loads, and four consecutive words become one (hi, lo) operand
// pair with four byte permutes -- instead of ~5 conversions per value repeated by each of the 29 query-tile workgroups that
// read the same keys.
__device__ __forceinline__ void unpack4(const float* w, h16x4& hi, h16x4& lo) {
  const unsigned w0 = __float_as_uint(w[0]), w1 = __float_as_uint(w[1]), w2 = __float_as_uint(w[2]), w3 = __float_as_uint(w[3]);
  typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
  const u32x2 h = {__builtin_amdgcn_perm(w1, w0, 0x05040100u), __builtin_amdgcn_perm(w3, w2, 0x05040100u)};
  const u32x2 l = {__builtin_amdgcn_perm(w1, w0, 0x07060302u), __builtin_amdgcn_perm(w3, w2, 0x07060302u)};
  hi = __builtin_bit_cast(h16x4, h);
  lo = __builtin_bit_cast(h16x4, l);
}

// O^T += V^T . P^T on split operands, instruction group c of a tile: it covers keys 8c + 4*half + i = accumulator rows
// 4c + i of this lane. o0 / o1: leading terms of the two d-tiles; x0 / x1: cross terms (scaled by 2^11). The trailing term
// Vl.Pl, 2^-22 of sum p |v|, is dropped. PACKED_V: V arrives as half pairs (unpack4), else as fp32 (split4).
template <bool PACKED_V>
__device__ __forceinline__ void pv_split_step(int c, const float (&st)[16], const float (&va0)[16], const float (&va1)[16],
                                              f32x16& o0, f32x16& x0, f32x16& o1, f32x16& x1) {
  h16x4 ph, pl, vh, vl;
  split4(&st[4 * c], ph, pl);
  if (PACKED_V) unpack4(&va0[4 * c], vh, vl); else split4(&va0[4 * c], vh, vl);
  o0 = __builtin_amdgcn_mfma_f32_32x32x8f16(vh, ph, o0, 0, 0, 0);
  x0 = __builtin_amdgcn_mfma_f32_32x32x8f16(vh, pl, x0, 0, 0, 0);
  x0 = __builtin_amdgcn_mfma_f32_32x32x8f16(vl, ph, x0, 0, 0, 0);
  if (PACKED_V) unpack4(&va1[4 * c], vh, vl); else split4(&va1[4 * c], vh, vl);
  o1 = __builtin_amdgcn_mfma_f32_32x32x8f16(vh, ph, o1, 0, 0, 0);
  x1 = __builtin_amdgcn_mfma_f32_32x32x8f16(vh, pl, x1, 0, 0, 0);
  x1 = __builtin_amdgcn_mfma_f32_32x32x8f16(vl, ph, x1, 0, 0, 0);
}

struct ExpE {   // running maxima are natural exponents (f32, f16s)
  __device__ __forceinline__ float operator()(float x) const { return expf(x); }
};
struct Exp2 {   // ... base-2 exponents (halfs)
  __device__ __forceinline__ float operator()(float x) const { return __builtin_amdgcn_exp2f(x); }
};

// The LDS in which partial results meet: 34 KB.
struct MeetLds {
  float m[4][64];
  float l[4][64];
  float o[4][2][16][64];
};

// Merge of four waves: wave w < 4 holds (m_run, l_run, o0 | o1) of its share of the keys. They meet in LDS; wave w then
// finishes d-tile w / 2, a share of 8 accumulator registers, and stores it (orow: this lane's output row at its head).
// WAVES == 8: waves 4..7 have handed their partials over and only keep the barrier company.
template <class Exp, int WAVES>
__device__ __forceinline__ void meet_four_and_store(MeetLds& s, const Tile& t, float m_run, float l_run, const f32x16& o0,
                                                    const f32x16& o1, float* __restrict__ orow) {
  static_assert(kWaves == 4, "the meeting is four-way");
  const Exp ex;
  const int wave = t.wave, lane = t.lane;
  if (WAVES == 4 || wave < 4) {
    s.m[wave][lane] = m_run;
    s.l[wave][lane] = l_run;
#pragma unroll
    for (int r = 0; r < 16; ++r) { s.o[wave][0][r][lane] = o0[r]; s.o[wave][1][r][lane] = o1[r]; }
  }
  __syncthreads();
  if (WAVES != 4 && wave >= 4) return;
  float mx = -INFINITY;
#pragma unroll
  for (int w = 0; w < 4; ++w) mx = fmaxf(mx, s.m[w][lane]);
  float f[4];
  float lsum = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    f[w] = mx == -INFINITY ? 0.f : ex(s.m[w][lane] - mx);
    lsum += f[w] * (s.l[w][lane] + s.l[w][lane ^ 32]);
  }
  const float inv = lsum > 0.f ? 1.f / lsum : 0.f;  // no admissible key: zeros (group_attn.py:131)
  const int dt = wave / 2, r0 = 8 * (wave % 2);
  if (t.q_ok) {
    float* op = orow + 32 * dt;
#pragma unroll
    for (int r = r0; r < r0 + 8; ++r) {
      float acc = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) acc += f[w] * s.o[w][dt][r][lane];
      op[acc_row(r, t.half)] = acc * inv;
    }
  }
}

template <bool GROUPED, class... Alt>
__global__ __launch_bounds__(kWaves * 64) void attention_f32_kernel(
    float* __restrict__ out, const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
    const int* __restrict__ query_cam, const int* __restrict__ group_start, int Nq, int Nk, int ldq, int ldk, int ldv,
    int ldo, float scale, Alt... alt) {
  SIMPB_PICK_KEYS()
  __shared__ MeetLds lds;
  const Tile t = this_tile(threadIdx.x >> 6, Nq);
  const KeyRange range = group_range<GROUPED>(query_cam, group_start, t, Nk);
  const int kb = range.kb, ke = range.ke;

  // Q^T operand: lane (query qi, half) holds Q[query][32*half + s], s = 0..31, pre-scaled
  float qreg[32];
  load_q_row(q, t, Nq, ldq, [&](int c, const float (&x)[4]) {
    qreg[4 * c + 0] = x[0] * scale; qreg[4 * c + 1] = x[1] * scale;
    qreg[4 * c + 2] = x[2] * scale; qreg[4 * c + 3] = x[3] * scale;
  });

  float m_run = -INFINITY, l_run = 0.f;
  f32x16 o0, o1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }

  const float* kbase = k + (size_t)t.b * Nk * ldk + t.head * kHD + 32 * t.half;
  const float* vbase = v + (size_t)t.b * Nk * ldv + t.head * kHD + t.qi;

  // K tile of this wave's first key tile; inside the loop the NEXT tile's K rows and the CURRENT tile's
  // V values are requested before the matrix work that does not need them, so their latency hides
  // behind the S^T product and the softmax (nothing else overlaps it at 2 waves per SIMD).
  float kcur[32], knext[32];
  const int kt0 = kb + 32 * t.wave;
  if (kt0 < ke) load_k_tile(kcur, kbase, kt0, t, range, ldk);
  for (int kt = kt0; kt < ke; kt += 32 * kWaves) {
    float va0[16], va1[16];
    load_v_tile(va0, va1, vbase, kt, t, range, ldv);
    // requested UNCONDITIONALLY (past the last tile load_k_tile clamps every row to the first key of the
    // range and the values are never used): a load behind `if (ktn < ke)` made the compiler wait for
    // every outstanding load -- these and the V values above -- in front of the S^T product.
    // (V of the NEXT tile requested a whole tile ahead was measured slower in both forms -- with K at the top: 35 vs 30 us
    // at 900 x 900, 80 loads in flight against a counter of 63; behind the S^T product with two alternating register sets:
    // 31.3 us, and 31-37 vs 25-31 us for the grouped form at 314 VGPRs. What is exposed per tile is not the V round trip but
    // the ~300 vector instructions of the softmax, which one wave per SIMD cannot overlap with its own matrix work.)
    const int ktn = kt + 32 * kWaves;
    load_k_tile(knext, kbase, ktn, t, range, ldk);
    __builtin_amdgcn_sched_barrier(0);  // the requests stay here, ahead of the matrix work (the scheduler sank them)
    // ---- S^T tile = K_tile . Q^T  (A: lane (key, half) holds K[key][32*half + s])
    f32x16 st;
#pragma unroll
    for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
    for (int s = 0; s < 32; ++s) st = __builtin_amdgcn_mfma_f32_32x32x2f32(kcur[s], qreg[s], st, 0, 0, 0);
    // ---- mask + online softmax; this lane: query qi, keys kt + acc_row(r, half)
    float mt = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      st[r] = key_ok<GROUPED>(kt + acc_row(r, t.half), range, t.q_ok) ? st[r] : -INFINITY;
      mt = fmaxf(mt, st[r]);
    }
    mt = fmaxf(mt, __shfl_xor(mt, 32));
    const float m_new = fmaxf(m_run, mt);
    const float m_safe = m_new == -INFINITY ? 0.f : m_new;
    const float alpha = expf(m_run - m_safe);  // m_run = -inf -> 0
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      st[r] = expf(st[r] - m_safe);
      psum += st[r];
    }
    l_run = l_run * alpha + psum;
    m_run = m_new;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }
    // ---- O^T += V^T . P^T  (A: va0/va1; B: st[s])
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(va0[s], st[s], o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(va1[s], st[s], o1, 0, 0, 0);
    }
#pragma unroll
    for (int s = 0; s < 32; ++s) kcur[s] = knext[s];
  }

  meet_four_and_store<ExpE, kWaves>(lds, t, m_run, l_run, o0, o1, out + ((size_t)t.b * Nq + t.qg) * ldo + t.head * kHD);
}


// ---------------------------------------------------------------------------------------------------------------------
// The same attention on the FP16 matrix cores with SPLIT operands (round 4), fp32-grade like csrc/gemm.hip's
// gemm_f16x3_kernel: every fp32 operand x is carried as xh + xl / 2^11 (two halfs, 22 bits), products of halfs are exact
// in the fp32 accumulators, and the partial products are summed in separate accumulators per scale:
//     S = Kh.Qh + (Kh.Ql + Kl.Qh) / 2^11 + Kl.Ql / 2^22           (all four terms: the softmax sits behind it)
//     O = Vh.Ph + (Vh.Pl + Vl.Ph) / 2^11                           (the dropped term is 2^-22 of sum p |v|)
// Why: the exact-fp32 kernel above is matrix-bound per SIMD at one stream -- 900 x 900 x 8 heads is 29 x 8 workgroups,
// one wave per SIMD, 64 v_mfma_f32_32x32x2_f32 of 64 cycles each per key tile = 4 096 cycles of the ~5 300 a tile
// takes. v_mfma_f32_32x32x8_f16 moves 4x the k-depth in half the cycles: 56 instructions of 32 cycles = 1 792.
// Same mapping, same operand registers: a lane's 32 contiguous head dims pair up as k = 4c + i of instruction c on BOTH
// operands (a dot product does not care in which order its terms meet), and the accumulator row map of S^T is again
// the B-operand k map of the second product (rows 8c + 4g + i of lane half g = k index 4g + i of instruction c).
template <bool GROUPED, class... Alt>
__global__ __launch_bounds__(kWaves * 64) void attention_f16s_kernel(
    float* __restrict__ out, const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
    const int* __restrict__ query_cam, const int* __restrict__ group_start, int Nq, int Nk, int ldq, int ldk, int ldv,
    int ldo, float scale, Alt... alt) {
  SIMPB_PICK_KEYS()
  __shared__ MeetLds lds;
  const Tile t = this_tile(threadIdx.x >> 6, Nq);
  const KeyRange range = group_range<GROUPED>(query_cam, group_start, t, Nk);
  const int kb = range.kb, ke = range.ke;

  // Q^T operand, split once: lane (query qi, half) holds Q[query][32*half + 4c + i] * scale as (hi, lo) of instruction c
  h16x4 qh[8], ql[8];
  load_q_row(q, t, Nq, ldq, [&](int c, const float (&x)[4]) {
    const float y[4] = {x[0] * scale, x[1] * scale, x[2] * scale, x[3] * scale};
    split4(y, qh[c], ql[c]);
  });

  float m_run = -INFINITY, l_run = 0.f;
  f32x16 o0, o1, x0, x1;   // O^T d-tiles: leading terms / cross terms (scaled by 2^11)
#pragma unroll
  for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; x0[r] = 0.f; x1[r] = 0.f; }

  const float* kbase = k + (size_t)t.b * Nk * ldk + t.head * kHD + 32 * t.half;
  const float* vbase = v + (size_t)t.b * Nk * ldv + t.head * kHD + t.qi;
  constexpr float kInv = 1.f / 2048.f;
  float kcur[32], knext[32];
  const int kt0 = kb + 32 * t.wave;
  if (kt0 < ke) load_k_tile(kcur, kbase, kt0, t, range, ldk);
  for (int kt = kt0; kt < ke; kt += 32 * kWaves) {
    float va0[16], va1[16];
    load_v_tile(va0, va1, vbase, kt, t, range, ldv);
    const int ktn = kt + 32 * kWaves;
    load_k_tile(knext, kbase, ktn, t, range, ldk);   // unconditional (clamped): see the exact kernel
    __builtin_amdgcn_sched_barrier(0);
    // ---- S^T tile = K_tile . Q^T in four split terms
    f32x16 shh, sx, sll;
#pragma unroll
    for (int r = 0; r < 16; ++r) { shh[r] = 0.f; sx[r] = 0.f; sll[r] = 0.f; }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      h16x4 kh, kl;
      split4(&kcur[4 * c], kh, kl);
      shh = __builtin_amdgcn_mfma_f32_32x32x8f16(kh, qh[c], shh, 0, 0, 0);
      sx = __builtin_amdgcn_mfma_f32_32x32x8f16(kh, ql[c], sx, 0, 0, 0);
      sx = __builtin_amdgcn_mfma_f32_32x32x8f16(kl, qh[c], sx, 0, 0, 0);
      sll = __builtin_amdgcn_mfma_f32_32x32x8f16(kl, ql[c], sll, 0, 0, 0);
    }
    // ---- mask + online softmax (fp32 vector arithmetic, as the exact kernel)
    float st[16];
    float mt = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float sv = shh[r] + (sx[r] + sll[r] * kInv) * kInv;
      st[r] = key_ok<GROUPED>(kt + acc_row(r, t.half), range, t.q_ok) ? sv : -INFINITY;
      mt = fmaxf(mt, st[r]);
    }
    mt = fmaxf(mt, __shfl_xor(mt, 32));
    const float m_new = fmaxf(m_run, mt);
    const float m_safe = m_new == -INFINITY ? 0.f : m_new;
    const float alpha = expf(m_run - m_safe);
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      st[r] = expf(st[r] - m_safe);
      psum += st[r];
    }
    l_run = l_run * alpha + psum;
    m_run = m_new;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; x0[r] *= alpha; x1[r] *= alpha; }
    // ---- O^T += V^T . P^T
#pragma unroll
    for (int c = 0; c < 4; ++c) pv_split_step<false>(c, st, va0, va1, o0, x0, o1, x1);
#pragma unroll
    for (int s = 0; s < 32; ++s) kcur[s] = knext[s];
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) { o0[r] += x0[r] * kInv; o1[r] += x1[r] * kInv; }

  meet_four_and_store<ExpE, kWaves>(lds, t, m_run, l_run, o0, o1, out + ((size_t)t.b * Nq + t.qg) * ldo + t.head * kHD);
}


// ---------------------------------------------------------------------------------------------------------------------
// Packed-operand attention, second form (what simpb_attention_split_halfs launches): with the matrix work down to 56
// half-rate-free instructions per key tile (1 792 cycles) the ~600 vector instructions of a tile (mask, softmax, the
// split of P, address arithmetic: ~2 600 cycles) are the larger half, and one wave per SIMD runs the two strictly one
// after the other (S -> softmax -> O is a dependent chain inside a tile). So: EIGHT waves per workgroup = two per SIMD,
// whose matrix and vector phases interleave in hardware, under a 256-register budget (K in one register set, re-loaded
// right behind the S^T product that consumed it; no Kl.Ql accumulator: that term, 2^-22 of sum |q||k|, is added into the
// cross-term accumulator pre-scaled instead -- see below); and fewer vector instructions: exp2 on pre-multiplied
// arguments, no masks / clamps on full tiles (workgroup-uniform branch), accumulators rescaled only when some lane's
// running maximum moved. The eight partial results meet in two steps (waves 4-7 hand theirs to waves 0-3 through LDS,
// then the four-way meeting of the kernels above), so LDS stays at 35 KB.
// (launch bounds: at least 8 waves per CU in either form, i.e. at most 256 registers per wave. The four-wave form -- used for the
// camera-grouped launches, whose ~190-key groups are 6 key tiles: nothing for eight waves to split -- then fits two workgroups
// per CU, and the 280 live workgroups of a 1 130-slot 2D set run as ONE round of the chip instead of 256 + 24.)
template <bool GROUPED, int WAVES, class... Alt>
__global__ __launch_bounds__(WAVES * 64, 8 / WAVES) void attention_halfs_kernel(
    float* __restrict__ out, const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
    const int* __restrict__ query_cam, const int* __restrict__ group_start, int Nq, int Nk, int ldq, int ldk, int ldv,
    int ldo, Alt... alt) {
  SIMPB_PICK_KEYS()
  static_assert(WAVES == 4 || WAVES == 8, "four waves, or eight meeting in two steps");
  __shared__ MeetLds lds;
  const Tile t = this_tile(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6), Nq);
  const int lane = t.lane, wave = t.wave;
  const bool q_ok = t.q_ok;
  const KeyRange range = group_range<GROUPED, true>(query_cam, group_start, t, Nk);
  const int kb = range.kb, ke = range.ke;

  // (the producer folded the softmax scale into the query rows of its weights: a power of two, exact)
  h16x4 qh[8], ql[8];
  load_q_row(q, t, Nq, ldq, [&](int c, const float (&x)[4]) { unpack4(x, qh[c], ql[c]); });

  float m_run = -INFINITY, l_run = 0.f;
  f32x16 o0, o1, x0, x1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; x0[r] = 0.f; x1[r] = 0.f; }

  const float* kbase = k + (size_t)t.b * Nk * ldk + t.head * kHD + 32 * t.half;
  const float* vbase = v + (size_t)t.b * Nk * ldv + t.head * kHD + t.qi;
  constexpr float kInv = 1.f / 2048.f, kLog2e = 1.4426950408889634f;
  // clamped loads (load_k_tile, load_v_tile) on the last, partial tile only
  float kcur[32];
  const int kt0 = kb + 32 * wave;
  if (kt0 < ke) load_k_tile(kcur, kbase, kt0, t, range, ldk, kt0 + 32 <= ke);
  for (int kt = kt0; kt < ke; kt += 32 * WAVES) {
    const bool full = kt + 32 <= ke;   // wave-uniform
    float va0[16], va1[16];
    load_v_tile(va0, va1, vbase, kt, t, range, ldv, full);
    // ---- S^T = K_tile . Q^T: leading term / cross terms and the trailing term pre-scaled into one accumulator
    f32x16 shh, sx;
#pragma unroll
    for (int r = 0; r < 16; ++r) { shh[r] = 0.f; sx[r] = 0.f; }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      h16x4 kh, kl;
      unpack4(&kcur[4 * c], kh, kl);
      shh = __builtin_amdgcn_mfma_f32_32x32x8f16(kh, qh[c], shh, 0, 0, 0);
      sx = __builtin_amdgcn_mfma_f32_32x32x8f16(kh, ql[c], sx, 0, 0, 0);
      sx = __builtin_amdgcn_mfma_f32_32x32x8f16(kl, qh[c], sx, 0, 0, 0);
    }
    // (Kl.Ql: 2^-22 of sum |q||k| -- dropped like the trailing term of the second product; the S^T of this kernel is the
    // three-term form csrc/linear_split.hip uses for value_proj, bounded by tests/test_gpu_ops.py against float64)
    const int ktn = kt + 32 * WAVES;
    load_k_tile(kcur, kbase, ktn, t, range, ldk, ktn + 32 <= ke);   // this wave's next K tile into the registers the product above has read
    // ---- mask + online softmax in base 2
    float st[16];
    float mt = -INFINITY;
    if (full && !GROUPED) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        st[r] = (shh[r] + sx[r] * kInv) * kLog2e;
        mt = fmaxf(mt, st[r]);
      }
      if (!q_ok) mt = -INFINITY;
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        st[r] = key_ok<GROUPED>(kt + acc_row(r, t.half), range, q_ok) ? (shh[r] + sx[r] * kInv) * kLog2e : -INFINITY;
        mt = fmaxf(mt, st[r]);
      }
    }
    mt = fmaxf(mt, __shfl_xor(mt, 32));
    const float m_new = fmaxf(m_run, mt);
    const float m_safe = m_new == -INFINITY ? 0.f : m_new;
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_safe);  // m_run = -inf -> 0
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      st[r] = q_ok ? __builtin_amdgcn_exp2f(st[r] - m_safe) : 0.f;
      psum += st[r];
    }
    l_run = l_run * alpha + psum;
    m_run = m_new;
    if (__builtin_amdgcn_ballot_w64(alpha != 1.f)) {   // some lane's maximum moved: rescale (wave-uniform branch)
#pragma unroll
      for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; x0[r] *= alpha; x1[r] *= alpha; }
    }
    // ---- O^T += V^T . P^T
#pragma unroll
    for (int c = 0; c < 4; ++c) pv_split_step<true>(c, st, va0, va1, o0, x0, o1, x1);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) { o0[r] += x0[r] * kInv; o1[r] += x1[r] * kInv; }

  // ---- eight waves: waves 4..7 hand their partials to waves 0..3 (running maxima are base-2 exponents here)
  if (WAVES == 8) {
    if (wave >= 4) {
      lds.m[wave - 4][lane] = m_run;
      lds.l[wave - 4][lane] = l_run;
#pragma unroll
      for (int r = 0; r < 16; ++r) { lds.o[wave - 4][0][r][lane] = o0[r]; lds.o[wave - 4][1][r][lane] = o1[r]; }
    }
    __syncthreads();
    if (wave < 4) {
      const float m_b = lds.m[wave][lane], l_b = lds.l[wave][lane];
      const float m_new = fmaxf(m_run, m_b);
      const float m_safe = m_new == -INFINITY ? 0.f : m_new;
      const float fa = __builtin_amdgcn_exp2f(m_run - m_safe), fb = __builtin_amdgcn_exp2f(m_b - m_safe);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        o0[r] = o0[r] * fa + lds.o[wave][0][r][lane] * fb;
        o1[r] = o1[r] * fa + lds.o[wave][1][r][lane] * fb;
      }
      l_run = l_run * fa + l_b * fb;
      m_run = m_new;
    }
    __syncthreads();
  }
  // ---- the four-way meeting
  meet_four_and_store<Exp2, WAVES>(lds, t, m_run, l_run, o0, o1, out + ((size_t)t.b * Nq + t.qg) * ldo + t.head * kHD);
}

// ---------------------------------------------------------------------------------------------------------------------
// Host side: one set of argument rules, one launch ladder.
struct Args {
  float* out;
  const float *q, *k, *v;
  const int *query_cam, *group_start;
  int batch_size, num_heads, head_dim, num_query, num_key, ldq, ldk, ldv, ldo;
  float scale;
};

// A key / value set obeys: present, at least one key, rows at least E wide, K rows float4-readable.
bool key_set_ok(const void* k, const void* v, int num_key, int ldk, int ldv, int e) {
  return k && v && num_key > 0 && ldk >= e && ldv >= e && (ldk & 3) == 0 && (reinterpret_cast<size_t>(k) & 15) == 0;
}

// Shape, stride, alignment and grid-limit rules of every entry point; alt: the second set of the selector form.
bool check_args(const Args& a, const AltKeys* alt) {
  if (a.batch_size <= 0 || a.num_heads <= 0 || a.batch_size > 65535 || a.num_heads > 65535) return false;   // grid y, z
  const int e = a.num_heads * kHD;
  if (!a.out || !a.q || a.num_query <= 0 || a.head_dim != kHD || a.ldq < e || a.ldo < e) return false;
  if ((a.ldq & 3) || (reinterpret_cast<size_t>(a.q) & 15)) return false;
  if (!key_set_ok(a.k, a.v, a.num_key, a.ldk, a.ldv, e)) return false;
  if (alt && !key_set_ok(alt->k, alt->v, alt->Nk, alt->ldk, alt->ldv, e)) return false;
  if ((a.query_cam == nullptr) != (a.group_start == nullptr)) return false;
  if (a.query_cam && a.num_key != a.num_query) return false;  // grouped form is self-attention over one slot set
  return true;
}

template <auto KERNEL, class... Tail>
void launch_one(int waves, const Args& a, hipStream_t s, Tail... tail) {
  const dim3 grid((a.num_query + 31) / 32, a.num_heads, a.batch_size);
  hipLaunchKernelGGL(KERNEL, grid, dim3(waves * 64), 0, s, a.out, a.q, a.k, a.v, a.query_cam, a.group_start, a.num_query,
                     a.num_key, a.ldq, a.ldk, a.ldv, a.ldo, tail...);
}

// split: 0 exact fp32, 1 operands split in the kernel, 2 packed half pairs. alt (ungrouped only): the AltKeys instantiations.
int attention_launch(int split, const Args& a, const AltKeys* alt, void* stream) {
  if (split < 0 || split > 2 || !check_args(a, alt)) return SIMPB_EINVAL;
  (void)hipGetLastError();
  const bool grouped = a.query_cam != nullptr;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (alt) {
    if (split == 2) launch_one<attention_halfs_kernel<false, 8, AltKeys>>(8, a, s, *alt);
    else if (split) launch_one<attention_f16s_kernel<false, AltKeys>>(kWaves, a, s, a.scale, *alt);
    else launch_one<attention_f32_kernel<false, AltKeys>>(kWaves, a, s, a.scale, *alt);
  } else if (split == 2) {
    if (grouped) launch_one<attention_halfs_kernel<true, 4>>(4, a, s);
    else launch_one<attention_halfs_kernel<false, 8>>(8, a, s);
  } else if (split) {
    if (grouped) launch_one<attention_f16s_kernel<true>>(kWaves, a, s, a.scale);
    else launch_one<attention_f16s_kernel<false>>(kWaves, a, s, a.scale);
  } else {
    if (grouped) launch_one<attention_f32_kernel<true>>(kWaves, a, s, a.scale);
    else launch_one<attention_f32_kernel<false>>(kWaves, a, s, a.scale);
  }
  return simpb_check_launch();
}

}  // namespace

extern "C" int simpb_attention_select(int split, float* out, const void* q, const void* k, const void* v, const void* k2,
                                      const void* v2, const unsigned char* select, int batch_size, int num_heads, int head_dim,
                                      int num_query, int num_key, int num_key2, int ldq, int ldk, int ldv, int ldk2, int ldv2,
                                      int ldo, float scale, void* stream) {
  const Args a{out, static_cast<const float*>(q), static_cast<const float*>(k), static_cast<const float*>(v), nullptr, nullptr,
               batch_size, num_heads, head_dim, num_query, num_key, ldq, ldk, ldv, ldo, scale};
  // no selector: every stream reads set 1 -- the kernels (and the bits) of the entry points below
  const AltKeys alt{select, static_cast<const float*>(k2), static_cast<const float*>(v2), num_key2, ldk2, ldv2};
  return attention_launch(split, a, select ? &alt : nullptr, stream);
}

extern "C" int simpb_attention_f32(float* out, const float* q, const float* k, const float* v, const int* query_cam,
                                   const int* group_start, int batch_size, int num_heads, int head_dim, int num_query,
                                   int num_key, int ldq, int ldk, int ldv, int ldo, float scale, void* stream) {
  return attention_launch(0, {out, q, k, v, query_cam, group_start, batch_size, num_heads, head_dim, num_query, num_key, ldq,
                              ldk, ldv, ldo, scale}, nullptr, stream);
}

extern "C" int simpb_attention_f32_split(float* out, const float* q, const float* k, const float* v, const int* query_cam,
                                         const int* group_start, int batch_size, int num_heads, int head_dim, int num_query,
                                         int num_key, int ldq, int ldk, int ldv, int ldo, float scale, void* stream) {
  return attention_launch(1, {out, q, k, v, query_cam, group_start, batch_size, num_heads, head_dim, num_query, num_key, ldq,
                              ldk, ldv, ldo, scale}, nullptr, stream);
}

extern "C" int simpb_attention_split_halfs(float* out, const void* q, const void* k, const void* v, const int* query_cam,
                                           const int* group_start, int batch_size, int num_heads, int head_dim, int num_query,
                                           int num_key, int ldq, int ldk, int ldv, int ldo, void* stream) {
  return attention_launch(2, {out, static_cast<const float*>(q), static_cast<const float*>(k), static_cast<const float*>(v),
                              query_cam, group_start, batch_size, num_heads, head_dim, num_query, num_key, ldq, ldk, ldv, ldo,
                              1.f}, nullptr, stream);
}
