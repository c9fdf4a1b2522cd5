// Grouped small-GEMM kernel of the decoder (gfx950, exact fp32 on v_mfma_f32_32x32x2_f32) and the
// segmented LayerNorm that goes with it.
//
// What it replaces: every `nn.Linear` of the decoder whose M is the query count (900 anchors, 600
// cached instances, <= 1 536 2D slots) -- the in/out projections of the four attention operators
// (/root/reference/projects/mmdet3d_plugin/models/simpb_head.py:298-321, group_attn.py:60-133), the
// AsymmetricFFN (blocks.py:384-393), output_proj / weights_fc / learnable_fc of the deformable
// operators (blocks.py:110-196, group_attn.py:176-243) -- together with the `torch.cat` / `+` that
// feed them. In the reference each is one vendor GEMM of 0.1-0.9 GFLOP (8-15 us on MI355X through
// the vendor heuristic, 3-5 % of the fp32 matrix rate) plus 1-3 elementwise kernels.
//
// Shape of the problem: M ~ 1 k, N and K in 256..1 536. A 64x256 tile (csrc/linear.hip, built for
// the 90 k-row value projection) would give 15-60 workgroups on a 256-CU chip, so the tile here is
// 32 x 32 (or 32 x 64) and the EIGHT WAVES OF A WORKGROUP SPLIT K: each wave owns a whole 32 x 32
// output tile over an eighth (quarter) of every 64-wide K chunk, so no operand is read from LDS
// twice, and the partial tiles meet once in LDS at the end. M = 900, N = 256 is 232 workgroups; two
// waves per SIMD let one wave's staging instructions run under the other's matrix instructions
// (measured with one wave per SIMD: the matrix pipe was 30-47 % busy, the waves 30 % in issue).
//
//  * X is given as up to four COLUMN SEGMENTS (pointer, row stride, width): y = [x0 | x1 | ...] W^T.
//    That is how cat([feature, pos_embed]) (simpb_head.py:299-301), the `identity +` branches and the
//    FFN's identity_fc are folded into one product without materialising the concatenation.
//  * Up to four independent problems share a launch (q / kv projections of the temporal attention).
//  * `m_live` (device int, optional): rows >= *m_live are capacity slots of the static 2D query set;
//    they are written as zeros without touching X or W.
//  * Four K chunks are kept in flight in registers ahead of the one being multiplied (all loads
//    unconditional, so the waits are counted); LDS is double buffered, one barrier per chunk.
//  * Workgroups are numbered so that each XCD (blockIdx % 8) walks a contiguous range of tiles:
//    neighbouring tiles share their X rows in that XCD's L2.
//
// The three kernels below differ in their wave-to-tile map and in how partial tiles meet. What they
// have in common -- segment select, K loop, epilogue element -- stands once, ahead of them;
// the split of x and its range window stand in csrc/mfma_f16.h, shared with csrc/linear_split.hip.
#include <hip/hip_runtime.h>
#include <type_traits>
#include "../../include/simpb_hip.h"
#include "mfma_f16.h"

#include "launch.h"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;  // native vector: plain loads/stores, no struct memcpy
using h16x8 = __attribute__((ext_vector_type(8))) _Float16;
using h16x4 = __attribute__((ext_vector_type(4))) _Float16;
using simpb::acc_row;

constexpr int BM = 32, BK = 64;  // BK: granularity the host checks; kernels use BKT = 64 or 128
constexpr int kWaves = 8;
constexpr int kThreads = kWaves * 64;

// compile-time loop: the register-set index must be a constant in the front end already, or the
// prefetch arrays are not promoted to registers (they were placed in scratch with a plain
// `#pragma unroll` loop over lambdas)
template <int D, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (D < N) {
    f(std::integral_constant<int, D>{});
    static_for<D + 1, N>(f);
  }
}

// out_fmt = SIMPB_GEMM_OUT_SPLIT_HALFS: the element as the two halfs the split-operand attention kernel multiplies
// (csrc/attention.hip unpack4), in the element's own 32-bit word
__device__ __forceinline__ float out_word(float v, int fmt) {
  if (fmt != SIMPB_GEMM_OUT_SPLIT_HALFS) return v;
  _Float16 h, l;
  simpb::split_halfs(v, h, l);
  const unsigned bits = (unsigned)__builtin_bit_cast(unsigned short, h) | ((unsigned)__builtin_bit_cast(unsigned short, l) << 16);
  return __uint_as_float(bits);
}

struct GemmLaunch {
  simpb_gemm_args a;
  int tile_start[SIMPB_GEMM_MAX_JOBS + 1];
  int per_xcd;  // tiles per XCD range
};

// ---- the column segments of x: where the chunk that starts at column k0 of [x0 | x1 | x2 | x3] lives (scalar
// selects; segment widths are multiples of the chunk)
struct XSegments {
  const float *x0, *x1, *x2, *x3;
  int e1, e2, e3;  // first column past segments 0, 1, 2
  unsigned l0, l1, l2, l3;
  __device__ __forceinline__ explicit XSegments(const simpb_gemm_job& job)
      : x0(job.x[0]), x1(job.x[1]), x2(job.x[2]), x3(job.x[3]),
        e1(job.kseg[0]), e2(e1 + (job.num_seg > 1 ? job.kseg[1] : 0)), e3(e2 + (job.num_seg > 2 ? job.kseg[2] : 0)),
        l0(job.ldx[0]), l1(job.ldx[1]), l2(job.ldx[2]), l3(job.ldx[3]) {}
  __device__ __forceinline__ const float* at(int k0, unsigned& ldx) const {
    const float* xs = x0 + k0;
    ldx = l0;
    if (k0 >= e1) { xs = x1 + (k0 - e1); ldx = l1; }
    if (k0 >= e2) { xs = x2 + (k0 - e2); ldx = l2; }
    if (k0 >= e3) { xs = x3 + (k0 - e3); ldx = l3; }
    return xs;
  }
};

// ---- the K loop. DEPTH register sets = DEPTH chunks in flight ahead of the one being multiplied: the operands
// come from the Infinity Cache / HBM (activations were just written by another XCD, and every workgroup walks K in
// step, so a chunk is a first touch for all of them at once). Chunk c lives in register set c % DEPTH and LDS buffer
// c & 1: stashed one barrier ahead of its product. fetch(set, chunk) / stash(set) / multiply(buffer) are the kernel's.
// Loads are UNCONDITIONAL (a fetch past the end asks for the last chunk again, never used; row / column indices are
// clamped, and the surplus rows and columns of an edge tile are computed on repeated data and never stored): a load
// behind a branch makes the compiler wait for every outstanding load (vmcnt(0)) instead of the oldest register set only.
template <int DEPTH, class Fetch, class Stash, class Multiply>
__device__ __forceinline__ void k_loop(int nchunks, Fetch&& fetch, Stash&& stash, Multiply&& multiply) {
  static_assert(DEPTH % 2 == 0, "LDS buffer index = register set index & 1");
  static_for<0, DEPTH>([&](auto d) __attribute__((always_inline)) { fetch(d, decltype(d)::value); });
  const int groups = nchunks / DEPTH;
  for (int g = 0; g < groups; ++g) {
    static_for<0, DEPTH>([&](auto d) __attribute__((always_inline)) {
      stash(d);
      __syncthreads();
      fetch(d, (g + 1) * DEPTH + decltype(d)::value);
      multiply(decltype(d)::value & 1);
    });
  }
  const int rem = nchunks - groups * DEPTH;
  static_for<0, DEPTH - 1>([&](auto d) __attribute__((always_inline)) {
    if (decltype(d)::value < rem) {
      stash(d);
      __syncthreads();
      multiply(decltype(d)::value & 1);
    }
  });
}

// ---- epilogue of element (gr, gc): v is its finished sum, bcol / b2 its column's entries of bias / bias2 (0.f where
// the job has none: the sum of accumulators that started at +0 is never -0, so adding 0.f changes no bit)
__device__ __forceinline__ void finish_element(const simpb_gemm_job& job, float* __restrict__ y, float v, float bcol,
                                               float b2, int gr, int gc, int live) {
  v += bcol;
  if (job.row_flag && job.row_flag[gr]) v += b2;
  if (job.relu) v = fmaxf(v, 0.f);
  y[(size_t)gr * job.ldy + gc] = gr < live ? out_word(v, job.out_fmt) : 0.f;
}

template <int BN, int DEPTH, int BKT>
__global__ __launch_bounds__(kThreads) void gemm_f32_kernel(GemmLaunch L) {
  constexpr int LDK = BKT + 4;            // LDS row stride: 16-lane groups of ds_read_b128 hit 16 distinct 4-bank slots
  constexpr int C4 = BKT / 4;             // 16-byte columns of a chunk row
  constexpr int WN = BN / 32;             // waves across N
  constexpr int WK = kWaves / WN;         // waves across K
  constexpr int KW = BKT / WK;            // k values of a chunk per wave
  constexpr int KH = KW / 2;              // ... per lane half
  constexpr int NX4 = BM * C4 / kThreads; // 16-byte X loads per thread per chunk
  constexpr int NW4 = BN * C4 / kThreads; // 16-byte W loads per thread per chunk
  constexpr int RS = kThreads / C4;       // rows covered by one pass of the staging threads
  constexpr int LDP = BN + 1;
  constexpr int kStage = 2 * (BM + BN) * LDK;
  constexpr int kPart = WK * BM * LDP;
  static_assert(KH % 4 == 0 && NX4 >= 1 && NW4 >= 1, "tile / wave split");
  __shared__ float smem[kStage > kPart ? kStage : kPart];
  float* s_x = smem;                     // [2][BM][LDK]
  float* s_w = smem + 2 * BM * LDK;      // [2][BN][LDK]

  // ---- which tile (spelled out in each of the three kernels: as one shared function, with zero scratch and equal registers, it cost
  // every 32-row launch ~0.35 us, profiles/gemm_shared_parts.md)
  const int tile = simpb::xcd_tile(L.per_xcd, L.tile_start[L.a.num_jobs]);
  if (tile < 0) return;
  int j = 0;
#pragma unroll
  for (int t = 1; t < SIMPB_GEMM_MAX_JOBS; ++t)
    if (t < L.a.num_jobs && tile >= L.tile_start[t]) j = t;
  const simpb_gemm_job& job = L.a.job[j];
  const int local = tile - L.tile_start[j];
  const int tiles_n = (job.N + BN - 1) / BN;
  const int row0 = (local / tiles_n) * BM;
  const int col0 = (local % tiles_n) * BN;
  const int M = job.M, N = job.N, K = job.K;
  const int live = job.m_live ? min(M, *job.m_live) : M;

  const int tid = threadIdx.x;
  float* __restrict__ y = job.y;
  if (row0 >= live) {  // capacity rows: zeros
    for (int idx = tid; idx < BM * BN; idx += kThreads) {
      const int r = idx / BN, c = idx - r * BN;
      if (row0 + r < M && col0 + c < N) y[(size_t)(row0 + r) * job.ldy + col0 + c] = 0.f;
    }
    return;
  }
  const int lane = tid & 63, wave = tid >> 6;
  const int r32 = lane & 31, half = lane >> 5;
  const int wn = wave % WN, wk = wave / WN;

  // ---- staging: thread f -> (row f >> 4, 16-byte column f & 15) of a [rows][64] chunk. Addresses are a
  // wave-uniform base (segment pointer + k offset, scalar registers) plus a per-thread 32-bit offset
  // that does not change along K.
  const int sr = tid / C4, sc4 = tid % C4;
  f32x4 px[DEPTH][NX4], pw[DEPTH][NW4];
  const float* __restrict__ w = job.w;
  unsigned xrow[NX4], wofs[NW4];
#pragma unroll
  for (int i = 0; i < NX4; ++i) xrow[i] = (unsigned)min(row0 + sr + RS * i, live - 1);
#pragma unroll
  for (int i = 0; i < NW4; ++i) wofs[i] = (unsigned)min(col0 + sr + RS * i, N - 1) * (unsigned)job.ldw + sc4 * 4;
  const int nchunks = K / BKT;
  const XSegments seg(job);

  auto fetch = [&](auto set_c, int chunk) __attribute__((always_inline)) {
    constexpr int set = decltype(set_c)::value;
    const int k0 = min(chunk, nchunks - 1) * BKT;
    unsigned ldx;
    const float* xs = seg.at(k0, ldx);
    const float* wk0 = w + k0;
    static_for<0, NX4>([&](auto i) __attribute__((always_inline)) {
      px[set][decltype(i)::value] = *reinterpret_cast<const f32x4*>(xs + (xrow[decltype(i)::value] * ldx + sc4 * 4));
    });
    static_for<0, NW4>([&](auto i) __attribute__((always_inline)) {
      pw[set][decltype(i)::value] = *reinterpret_cast<const f32x4*>(wk0 + wofs[decltype(i)::value]);
    });
  };
  auto stash = [&](auto set_c) __attribute__((always_inline)) {
    constexpr int set = decltype(set_c)::value;
    constexpr int buf = set & 1;
    static_for<0, NX4>([&](auto i) __attribute__((always_inline)) {
      constexpr int ii = decltype(i)::value;
      *reinterpret_cast<f32x4*>(&s_x[(buf * BM + sr + RS * ii) * LDK + sc4 * 4]) = px[set][ii];
    });
    static_for<0, NW4>([&](auto i) __attribute__((always_inline)) {
      constexpr int ii = decltype(i)::value;
      *reinterpret_cast<f32x4*>(&s_w[(buf * BN + sr + RS * ii) * LDK + sc4 * 4]) = pw[set][ii];
    });
  };

  // one accumulator per wave (two, for even / odd k steps, measured no faster and cost 16 registers:
  // at <= 80 VGPRs three 8-wave workgroups fit a CU instead of two)
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  auto multiply = [&](int buf) __attribute__((always_inline)) {
    // lane (r32, half) holds k = wk*KW + half*KH + 0..KH-1 of its x row and of its W row: the same
    // permutation of k on both operands, so the product is unchanged and both arrive as b128 reads
    const float* ax = &s_x[(buf * BM + r32) * LDK + wk * KW + half * KH];
    const float* bx = &s_w[(buf * BN + wn * 32 + r32) * LDK + wk * KW + half * KH];
    float a[KH], b[KH];
#pragma unroll
    for (int q = 0; q < KH / 4; ++q) {
      const float4 va = *reinterpret_cast<const float4*>(ax + 4 * q);
      const float4 vb = *reinterpret_cast<const float4*>(bx + 4 * q);
      a[4 * q] = va.x; a[4 * q + 1] = va.y; a[4 * q + 2] = va.z; a[4 * q + 3] = va.w;
      b[4 * q] = vb.x; b[4 * q + 1] = vb.y; b[4 * q + 2] = vb.z; b[4 * q + 3] = vb.w;
    }
#pragma unroll
    for (int s = 0; s < KH; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s], acc, 0, 0, 0);
  };

  k_loop<DEPTH>(nchunks, fetch, stash, multiply);

  // ---- the WK partial tiles meet in LDS
  __syncthreads();
  float* part = smem;  // [WK][BM][LDP]
#pragma unroll
  for (int r = 0; r < 16; ++r) part[(wk * BM + acc_row(r, half)) * LDP + wn * 32 + r32] = acc[r];
  __syncthreads();
  const float* __restrict__ bias = job.bias;
  for (int idx = tid; idx < BM * BN; idx += kThreads) {
    const int r = idx / BN, c = idx - r * BN;
    const int gr = row0 + r, gc = col0 + c;
    if (gr < M && gc < N) {
      float v = part[r * LDP + c];
#pragma unroll
      for (int p = 1; p < WK; ++p) v += part[(p * BM + r) * LDP + c];  // fixed order: deterministic
      finish_element(job, y, v, bias ? bias[gc] : 0.f, job.row_flag ? job.bias2[gc] : 0.f, gr, gc, live);
    }
  }
}

// ---- the same grouped GEMM on the FP16 matrix cores at fp32-grade accuracy (see csrc/linear_split.hip):
// x = xh + xl / 2048 is split while it is staged, W = Wh + Wl / 2048 arrives pre-split (f16 [N, K] each),
// y = xh.Wh^T + (xh.Wl^T + xl.Wh^T) / 2^11 + xl.Wl^T / 2^22 in three fp32 accumulators. A wave's share of a K chunk
// is exactly one 16-deep matrix instruction per term (four per chunk instead of eight fp32 ones at 1/16 the
// rate), so what remains is the staging, the LDS round trip and the barrier.
//
// ---- range of the split operands. x = xh + xl / 2^11 carries 22 bits only while half(x) is a normal half: |x| >= 65520
// makes xh infinite, and a row whose largest |x| is far below 2^-14 loses its trailing bits to half subnormals. The split
// kernels therefore stage each row as x * 2^-e with e = 0 while the row's largest |x| lies in [2^-10, 2^15) (or the row
// is all zeros), and otherwise e = the exponent of that largest |x|; the epilogue multiplies the sum by 2^e before the
// bias. Scaling by powers of two is exact, so rows inside the window compute exactly what they did without it.
// The row maxima are collected while the first pass stages x (which splits unscaled, as before); only a workgroup that
// met a row outside the window makes a second pass with the exponents. (simpb::split_staged / split_needs_second_pass:
// csrc/mfma_f16.h; the window's host-side twin for weights: plugin/dense.py SPLIT_WINDOW.)

// one 16-byte load of x as it goes to LDS in two parts
template <bool kScaled>
__device__ __forceinline__ void stash_x_split(const f32x4& v, int e, float& xmax, _Float16* dst_h, _Float16* dst_l) {
  h16x4 hi, lo;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    _Float16 h, l;
    simpb::split_staged<kScaled>(v[q], e, xmax, h, l);
    hi[q] = h;
    lo[q] = l;
  }
  *reinterpret_cast<h16x4*>(dst_h) = hi;
  *reinterpret_cast<h16x4*>(dst_l) = lo;
}

// leading term / cross terms scaled by 2^11 / trailing term scaled by 2^22. The last one (~2^-22 relative) is
// kept here although csrc/linear_split.hip drops it: the matrix pipe has cycles to spare, and without it one 2D
// query of the golden R50 stream changed sides of the image border (an N2 of 1129 instead of 1130): the decoder's
// discrete decisions sit downstream of these products.
struct SplitAcc {
  f32x16 acc, acs, act;
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[r] = 0.f; acs[r] = 0.f; act[r] = 0.f; }
  }
  __device__ __forceinline__ void step(const h16x8& ah, const h16x8& al, const h16x8& bh, const h16x8& bl) {
    act = simpb::mfma_32x32x16_f16(al, bl, act);
    acs = simpb::mfma_32x32x16_f16(al, bh, acs);
    acs = simpb::mfma_32x32x16_f16(ah, bl, acs);
    acc = simpb::mfma_32x32x16_f16(ah, bh, acc);
  }
  __device__ __forceinline__ float sum(int r) const { return acc[r] + (acs[r] + act[r] * (1.f / 2048.f)) * (1.f / 2048.f); }
};

// (four waves per SIMD = two workgroups per CU, as the LDS allows: at most 128 registers, which the row-range bookkeeping
// below would otherwise push the 32 x 32 form past)
template <int BN, int DEPTH, int BKT>
__global__ __launch_bounds__(kThreads, 4) void gemm_f16x3_kernel(GemmLaunch L) {
  constexpr int LDH = BKT + 8;            // LDS row stride in halfs: conflict-free 16-lane groups for ds_read_b128
  constexpr int WN = BN / 32, WK = kWaves / WN, KW = BKT / WK;
  static_assert(KW == 16, "one 32x32x16 step per wave per chunk");
  constexpr int C4 = BKT / 4, NX4 = BM * C4 / kThreads, RSX = kThreads / C4;   // x: fp32, 16-byte loads
  constexpr int C8 = BKT / 8, NW8 = BN * C8 / kThreads, RSW = kThreads / C8;   // w: f16, 16-byte loads
  static_assert(NX4 >= 1 && NW8 >= 1, "tile / thread split");
  constexpr int LDP = BN + 1;
  constexpr int kStageBytes = 2 * 2 * (BM + BN) * LDH * 2;
  constexpr int kPartBytes = WK * BM * LDP * 4;
  __shared__ __attribute__((aligned(16))) unsigned char smem_raw[kStageBytes > kPartBytes ? kStageBytes : kPartBytes];
  __shared__ int s_rowexp[BM];                              // row exponents of the second pass (split_row_exp)
  __shared__ int s_any;                                     // some row of the tile lies outside the window
  _Float16* s_xh = reinterpret_cast<_Float16*>(smem_raw);  // [2][BM][LDH]
  _Float16* s_xl = s_xh + 2 * BM * LDH;
  _Float16* s_wh = s_xl + 2 * BM * LDH;                    // [2][BN][LDH]
  _Float16* s_wl = s_wh + 2 * BN * LDH;

  // ---- which tile (as gemm_f32_kernel)
  const int tile = simpb::xcd_tile(L.per_xcd, L.tile_start[L.a.num_jobs]);
  if (tile < 0) return;
  int j = 0;
#pragma unroll
  for (int t = 1; t < SIMPB_GEMM_MAX_JOBS; ++t)
    if (t < L.a.num_jobs && tile >= L.tile_start[t]) j = t;
  const simpb_gemm_job& job = L.a.job[j];
  const int local = tile - L.tile_start[j];
  const int tiles_n = (job.N + BN - 1) / BN;
  const int row0 = (local / tiles_n) * BM;
  const int col0 = (local % tiles_n) * BN;
  const int M = job.M, N = job.N, K = job.K;
  const int live = job.m_live ? min(M, *job.m_live) : M;

  const int tid = threadIdx.x;
  float* __restrict__ y = job.y;
  if (row0 >= live) {  // capacity rows: zeros
    for (int idx = tid; idx < BM * BN; idx += kThreads) {
      const int r = idx / BN, c = idx - r * BN;
      if (row0 + r < M && col0 + c < N) y[(size_t)(row0 + r) * job.ldy + col0 + c] = 0.f;
    }
    return;
  }
  const int lane = tid & 63, wave = tid >> 6;
  const int r32 = lane & 31, kb = lane >> 5;
  const int wn = wave % WN, wk = wave / WN;

  const int srx = tid / C4, scx = tid % C4;   // x staging: (row, float4 column)
  const int srw = tid / C8, scw = tid % C8;   // w staging: (row, 8-half column)
  f32x4 px[DEPTH][NX4];
  h16x8 pwh[DEPTH][NW8], pwl[DEPTH][NW8];
  const _Float16* __restrict__ wh = static_cast<const _Float16*>(job.w_hi);
  const _Float16* __restrict__ wl = static_cast<const _Float16*>(job.w_lo);
  unsigned xrow[NX4], wofs[NW8];
#pragma unroll
  for (int i = 0; i < NX4; ++i) xrow[i] = (unsigned)min(row0 + srx + RSX * i, live - 1);
#pragma unroll
  for (int i = 0; i < NW8; ++i) wofs[i] = (unsigned)min(col0 + srw + RSW * i, N - 1) * (unsigned)K + scw * 8;
  const int nchunks = K / BKT;
  const XSegments seg(job);

  auto fetch = [&](auto set_c, int chunk) __attribute__((always_inline)) {
    constexpr int set = decltype(set_c)::value;
    const int k0 = min(chunk, nchunks - 1) * BKT;
    unsigned ldx;
    const float* xs = seg.at(k0, ldx);
    static_for<0, NX4>([&](auto i) __attribute__((always_inline)) {
      px[set][decltype(i)::value] = *reinterpret_cast<const f32x4*>(xs + (xrow[decltype(i)::value] * ldx + scx * 4));
    });
    static_for<0, NW8>([&](auto i) __attribute__((always_inline)) {
      pwh[set][decltype(i)::value] = *reinterpret_cast<const h16x8*>(wh + k0 + wofs[decltype(i)::value]);
      pwl[set][decltype(i)::value] = *reinterpret_cast<const h16x8*>(wl + k0 + wofs[decltype(i)::value]);
    });
  };
  float xmax[NX4];   // largest |x| this thread staged per row (first pass), then the row's
  int xe[NX4];       // exponent of the row (second pass)
#pragma unroll
  for (int i = 0; i < NX4; ++i) { xmax[i] = 0.f; xe[i] = 0; }
  auto stash = [&](auto set_c, auto scaled_c) __attribute__((always_inline)) {
    constexpr int set = decltype(set_c)::value;
    constexpr int buf = set & 1;
    static_for<0, NX4>([&](auto i) __attribute__((always_inline)) {
      constexpr int ii = decltype(i)::value;
      const int at = (buf * BM + srx + RSX * ii) * LDH + scx * 4;
      stash_x_split<decltype(scaled_c)::value>(px[set][ii], xe[ii], xmax[ii], &s_xh[at], &s_xl[at]);
    });
    static_for<0, NW8>([&](auto i) __attribute__((always_inline)) {
      constexpr int ii = decltype(i)::value;
      *reinterpret_cast<h16x8*>(&s_wh[(buf * BN + srw + RSW * ii) * LDH + scw * 8]) = pwh[set][ii];
      *reinterpret_cast<h16x8*>(&s_wl[(buf * BN + srw + RSW * ii) * LDH + scw * 8]) = pwl[set][ii];
    });
  };

  SplitAcc a;
  auto multiply = [&](int buf) __attribute__((always_inline)) {
    const int off = wk * KW + 8 * kb;  // lane (r32, kb) holds k = wk*16 + 8*kb .. +7 of its x row / W row
    a.step(*reinterpret_cast<const h16x8*>(&s_xh[(buf * BM + r32) * LDH + off]),
           *reinterpret_cast<const h16x8*>(&s_xl[(buf * BM + r32) * LDH + off]),
           *reinterpret_cast<const h16x8*>(&s_wh[(buf * BN + wn * 32 + r32) * LDH + off]),
           *reinterpret_cast<const h16x8*>(&s_wl[(buf * BN + wn * 32 + r32) * LDH + off]));
  };
  auto pass = [&](auto scaled_c) __attribute__((always_inline)) {
    a.zero();
    k_loop<DEPTH>(nchunks, fetch, [&](auto d) __attribute__((always_inline)) { stash(d, scaled_c); }, multiply);
  };
  if (tid == 0) s_any = 0;   // (ordered before any write below by the loop's barriers)
  pass(std::false_type{});
  const bool scaled = simpb::split_needs_second_pass<C4>(xmax, xe, s_any, s_rowexp, srx, RSX, scx == 0);
  if (scaled) {
    pass(std::true_type{});
    __syncthreads();
  }
  // ---- the WK partial tiles meet in LDS
  float* part = reinterpret_cast<float*>(smem_raw);  // [WK][BM][LDP]
#pragma unroll
  for (int r = 0; r < 16; ++r) part[(wk * BM + acc_row(r, kb)) * LDP + wn * 32 + r32] = a.sum(r);
  __syncthreads();
  const float* __restrict__ bias = job.bias;
  for (int idx = tid; idx < BM * BN; idx += kThreads) {
    const int r = idx / BN, c = idx - r * BN;
    const int gr = row0 + r, gc = col0 + c;
    if (gr < M && gc < N) {
      float v = part[r * LDP + c];
#pragma unroll
      for (int p = 1; p < WK; ++p) v += part[(p * BM + r) * LDP + c];  // fixed order: deterministic
      if (scaled) v = __builtin_amdgcn_ldexpf(v, s_rowexp[r]);
      finish_element(job, y, v, bias ? bias[gc] : 0.f, job.row_flag ? job.bias2[gc] : 0.f, gr, gc, live);
    }
  }
}

// ---- the split-operand GEMM for launches with MANY output tiles (every product of a batch of streams): 64 x 128 output tiles, one 32 x 32 tile per wave over the WHOLE K. Why a second form: with
// the matrix work down to four half-rate-free passes the 32 x 64 tiles above are bound by what they pull through L2 -- a
// 900 x 512 -> 1 536 projection re-reads x 24 times and W 29 times, 134 MB per launch, ~13 us at the ~10 TB/s the L2 gives
// 696 small workgroups -- and by one barrier + one cross-wave reduction per 16-deep step. Here x is re-read 12 times and W 15
// times (67 MB), a wave issues 32 matrix instructions per barrier instead of 8, and nothing is reduced across waves: the
// accumulators go straight to memory. Operands staged exactly as above (x split while staged, W pre-split, 144-byte LDS pitch).
constexpr int kWM = 64, kWN = 128;

template <int DEPTH>
__global__ __launch_bounds__(kThreads) void gemm_f16x3_wide_kernel(GemmLaunch L) {
  static_assert(DEPTH == 2, "two register sets, two LDS buffers");
  constexpr int BKT = 64;   // (the split route needs 128-aligned segments, so the chunk count is even: the K loop's tail never runs)
  constexpr int LDH = BKT + 8;
  constexpr int C4 = BKT / 4, NX4 = kWM * C4 / kThreads, RSX = kThreads / C4;   // x: 64 x 64 fp32 = 1024 float4, 2 per thread
  constexpr int C8 = BKT / 8, NW8 = kWN * C8 / kThreads, RSW = kThreads / C8;   // w: 128 x 64 halfs = 1024 x 16 B, 2 per thread (hi and lo each)
  static_assert(NX4 == 2 && NW8 == 2, "tile / thread split");
  __shared__ __attribute__((aligned(16))) _Float16 s_xh[2 * kWM * LDH];
  __shared__ __attribute__((aligned(16))) _Float16 s_xl[2 * kWM * LDH];
  __shared__ __attribute__((aligned(16))) _Float16 s_wh[2 * kWN * LDH];
  __shared__ __attribute__((aligned(16))) _Float16 s_wl[2 * kWN * LDH];
  __shared__ int s_rowexp[kWM];   // row exponents of the second pass (split_row_exp)
  __shared__ int s_any;

  // ---- which tile (as gemm_f32_kernel)
  const int tile = simpb::xcd_tile(L.per_xcd, L.tile_start[L.a.num_jobs]);
  if (tile < 0) return;
  int j = 0;
#pragma unroll
  for (int t = 1; t < SIMPB_GEMM_MAX_JOBS; ++t)
    if (t < L.a.num_jobs && tile >= L.tile_start[t]) j = t;
  const simpb_gemm_job& job = L.a.job[j];
  const int local = tile - L.tile_start[j];
  const int tiles_n = (job.N + kWN - 1) / kWN;
  const int row0 = (local / tiles_n) * kWM;
  const int col0 = (local % tiles_n) * kWN;
  const int M = job.M, N = job.N, K = job.K;
  const int live = job.m_live ? min(M, *job.m_live) : M;

  const int tid = threadIdx.x;
  float* __restrict__ y = job.y;
  if (row0 >= live) {  // capacity rows: zeros
    for (int idx = tid; idx < kWM * kWN; idx += kThreads) {
      const int r = idx / kWN, c = idx - r * kWN;
      if (row0 + r < M && col0 + c < N) y[(size_t)(row0 + r) * job.ldy + col0 + c] = 0.f;
    }
    return;
  }
  const int lane = tid & 63, wave = tid >> 6;
  const int r32 = lane & 31, kb = lane >> 5;
  const int wm = wave >> 2, wn = wave & 3;   // this wave's 32 x 32 tile: rows 32 wm.., columns 32 wn..

  const int srx = tid / C4, scx = tid % C4;
  const int srw = tid / C8, scw = tid % C8;
  f32x4 px[DEPTH][NX4];
  h16x8 pwh[DEPTH][NW8], pwl[DEPTH][NW8];
  const _Float16* __restrict__ wh = static_cast<const _Float16*>(job.w_hi);
  const _Float16* __restrict__ wl = static_cast<const _Float16*>(job.w_lo);
  unsigned xrow[NX4], wofs[NW8];
#pragma unroll
  for (int i = 0; i < NX4; ++i) xrow[i] = (unsigned)min(row0 + srx + RSX * i, live - 1);
#pragma unroll
  for (int i = 0; i < NW8; ++i) wofs[i] = (unsigned)min(col0 + srw + RSW * i, N - 1) * (unsigned)K + scw * 8;
  const int nchunks = K / BKT;
  const XSegments seg(job);

  auto fetch = [&](auto set_c, int chunk) __attribute__((always_inline)) {
    constexpr int set = decltype(set_c)::value;
    const int k0 = min(chunk, nchunks - 1) * BKT;
    unsigned ldx;
    const float* xs = seg.at(k0, ldx);
    static_for<0, NX4>([&](auto i) __attribute__((always_inline)) {
      px[set][decltype(i)::value] = *reinterpret_cast<const f32x4*>(xs + (xrow[decltype(i)::value] * ldx + scx * 4));
    });
    static_for<0, NW8>([&](auto i) __attribute__((always_inline)) {
      pwh[set][decltype(i)::value] = *reinterpret_cast<const h16x8*>(wh + k0 + wofs[decltype(i)::value]);
      pwl[set][decltype(i)::value] = *reinterpret_cast<const h16x8*>(wl + k0 + wofs[decltype(i)::value]);
    });
  };
  float xmax[NX4];   // largest |x| this thread staged per row, then the row's (as gemm_f16x3_kernel)
  int xe[NX4];
#pragma unroll
  for (int i = 0; i < NX4; ++i) { xmax[i] = 0.f; xe[i] = 0; }
  auto stash = [&](auto set_c, auto scaled_c) __attribute__((always_inline)) {
    constexpr int set = decltype(set_c)::value;
    constexpr int buf = set & 1;
    static_for<0, NX4>([&](auto i) __attribute__((always_inline)) {
      constexpr int ii = decltype(i)::value;
      const int at = (buf * kWM + srx + RSX * ii) * LDH + scx * 4;
      stash_x_split<decltype(scaled_c)::value>(px[set][ii], xe[ii], xmax[ii], &s_xh[at], &s_xl[at]);
    });
    static_for<0, NW8>([&](auto i) __attribute__((always_inline)) {
      constexpr int ii = decltype(i)::value;
      *reinterpret_cast<h16x8*>(&s_wh[(buf * kWN + srw + RSW * ii) * LDH + scw * 8]) = pwh[set][ii];
      *reinterpret_cast<h16x8*>(&s_wl[(buf * kWN + srw + RSW * ii) * LDH + scw * 8]) = pwl[set][ii];
    });
  };

  SplitAcc a;
  auto multiply = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int st = 0; st < BKT / 16; ++st) {
      const int off = 16 * st + 8 * kb;  // lane (r32, kb) holds k = 16 st + 8 kb .. +7 of its x row / W row
      a.step(*reinterpret_cast<const h16x8*>(&s_xh[(buf * kWM + wm * 32 + r32) * LDH + off]),
             *reinterpret_cast<const h16x8*>(&s_xl[(buf * kWM + wm * 32 + r32) * LDH + off]),
             *reinterpret_cast<const h16x8*>(&s_wh[(buf * kWN + wn * 32 + r32) * LDH + off]),
             *reinterpret_cast<const h16x8*>(&s_wl[(buf * kWN + wn * 32 + r32) * LDH + off]));
    }
  };
  auto pass = [&](auto scaled_c) __attribute__((always_inline)) {
    a.zero();
    k_loop<DEPTH>(nchunks, fetch, [&](auto d) __attribute__((always_inline)) { stash(d, scaled_c); }, multiply);
  };
  if (tid == 0) s_any = 0;   // (ordered before any write below by the loop's barriers)
  pass(std::false_type{});
  const bool scaled = simpb::split_needs_second_pass<C4>(xmax, xe, s_any, s_rowexp, srx, RSX, scx == 0);
  if (scaled) pass(std::true_type{});

  // ---- epilogue straight from the accumulators: lane (column r32, row group kb)
  const float* __restrict__ bias = job.bias;
  const int gc = col0 + wn * 32 + r32;
  if (gc < N) {
    const float bcol = bias ? bias[gc] : 0.f;
    const float b2 = job.row_flag ? job.bias2[gc] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int lr = wm * 32 + acc_row(r, kb), gr = row0 + lr;
      if (gr < M) {
        float v = a.sum(r);
        if (scaled) v = __builtin_amdgcn_ldexpf(v, s_rowexp[lr]);
        finish_element(job, y, v, bcol, b2, gr, gc, live);
      }
    }
  }
}

// ---- LayerNorm over the concatenation of up to two column segments, one wave per row, eps 1e-5,
// biased variance (torch.nn.LayerNorm); width <= 512, multiple of 64 per segment.
__global__ __launch_bounds__(256) void layernorm_seg_kernel(float* __restrict__ out, int ldo,
                                                            const float* __restrict__ x0, int ld0, int k0,
                                                            const float* __restrict__ x1, int ld1, int k1,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, int M,
                                                            const int* __restrict__ m_live) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int D = k0 + k1;
  const int live = m_live ? min(M, *m_live) : M;
  float v[8];
  float s = 0.f;
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) {
    const int e = lane + 64 * jj;
    float t = 0.f;
    if (e < D && row < live) t = e < k0 ? x0[(size_t)row * ld0 + e] : x1[(size_t)row * ld1 + (e - k0)];
    v[jj] = t;
    s += t;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
  const float mean = s / (float)D;
  float q = 0.f;
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) {
    const float d = (lane + 64 * jj) < D ? v[jj] - mean : 0.f;
    q += d * d;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) q += __shfl_xor(q, m);
  const float inv = 1.f / sqrtf(q / (float)D + 1e-5f);
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) {
    const int e = lane + 64 * jj;
    if (e < D) out[(size_t)row * ldo + e] = row < live ? (v[jj] - mean) * inv * gamma[e] + beta[e] : 0.f;
  }
}

// tiles of tm x tn over every job of a launch; with `start`, the first tile of each job as well
long long count_tiles(const simpb_gemm_args* args, int tm, int tn, int* start = nullptr) {
  long long total = 0;
  for (int j = 0; j < args->num_jobs; ++j) {
    if (start) start[j] = (int)total;
    total += (long long)((args->job[j].M + tm - 1) / tm) * ((args->job[j].N + tn - 1) / tn);
  }
  return total;
}

}  // namespace

extern "C" int simpb_gemm_f32(const simpb_gemm_args* args, void* stream) {
  if (!args || args->num_jobs <= 0 || args->num_jobs > SIMPB_GEMM_MAX_JOBS) return SIMPB_EINVAL;
  GemmLaunch L;
  L.a = *args;
  bool wide_k = true;  // every segment a multiple of 128 and K >= 512
  bool split = true;   // every job brings pre-split f16 weights (dense rows: ldw == K) and 128-aligned segments
  for (int j = 0; j < args->num_jobs; ++j) {
    const simpb_gemm_job& job = args->job[j];
    if (!job.y || !job.w || job.M <= 0 || job.N <= 0 || job.K <= 0 || job.K % BK) return SIMPB_EINVAL;
    if (job.num_seg <= 0 || job.num_seg > SIMPB_GEMM_MAX_SEGS || job.ldy < job.N || job.ldw < job.K) return SIMPB_EINVAL;
    if ((reinterpret_cast<size_t>(job.w) & 15) || (job.ldw & 3)) return SIMPB_EINVAL;
    if ((job.row_flag != nullptr) != (job.bias2 != nullptr)) return SIMPB_EINVAL;
    int ksum = 0;
    for (int s = 0; s < job.num_seg; ++s) {
      if (!job.x[s] || job.kseg[s] <= 0 || job.kseg[s] % BK || job.ldx[s] < job.kseg[s] || (job.ldx[s] & 3) ||
          (reinterpret_cast<size_t>(job.x[s]) & 15))
        return SIMPB_EINVAL;
      ksum += job.kseg[s];
      if (job.kseg[s] % 128) { wide_k = false; split = false; }
    }
    if (job.K < 512) wide_k = false;
    if (!job.w_hi || !job.w_lo || ((reinterpret_cast<size_t>(job.w_hi) | reinterpret_cast<size_t>(job.w_lo)) & 15)) split = false;
    if (ksum != job.K) return SIMPB_EINVAL;
  }
  // tile width: 64 columns once that still fills the chip, 32 otherwise
  const int bn = count_tiles(args, BM, 64) >= 200 ? 64 : 32;
  // the 64 x 128-tile form for launches with thousands of rows (a batch of streams: 10-20 % faster there, profiles/
  // r04_gemm_wide_tiles.txt); at one stream's ~1 k rows it has at most 288 tiles and measured no faster (q|k|v 19.0 vs 18.9 us)
  // or slower (fc1 17.3 vs 12.6 us: 120 tiles leave half the chip idle), so the switch-over sits above those
  constexpr long long kWideMinTiles = 400;
  const bool wide_tiles = split && count_tiles(args, kWM, kWN) >= kWideMinTiles;
  const long long total = wide_tiles ? count_tiles(args, kWM, kWN, L.tile_start) : count_tiles(args, BM, bn, L.tile_start);
  if (total > (1 << 24)) return SIMPB_EINVAL;
  for (int j = args->num_jobs; j <= SIMPB_GEMM_MAX_JOBS; ++j) L.tile_start[j] = (int)total;
  L.per_xcd = (int)((total + 7) / 8);
  (void)hipGetLastError();
  dim3 grid(L.per_xcd * 8);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (wide_tiles)
    hipLaunchKernelGGL((gemm_f16x3_wide_kernel<2>), grid, dim3(kThreads), 0, s, L);
  else if (split && bn == 64)
    hipLaunchKernelGGL((gemm_f16x3_kernel<64, 2, 64>), grid, dim3(kThreads), 0, s, L);
  else if (split)
    hipLaunchKernelGGL((gemm_f16x3_kernel<32, 2, 128>), grid, dim3(kThreads), 0, s, L);
  else if (bn == 64)
    hipLaunchKernelGGL((gemm_f32_kernel<64, 2, 64>), grid, dim3(kThreads), 0, s, L);
  else if (wide_k)  // 32-wide tiles: 128-deep chunks halve the barriers per matrix instruction (LDS 66 KB, 2 workgroups per CU)
    hipLaunchKernelGGL((gemm_f32_kernel<32, 2, 128>), grid, dim3(kThreads), 0, s, L);
  else
    hipLaunchKernelGGL((gemm_f32_kernel<32, 4, 64>), grid, dim3(kThreads), 0, s, L);
  return simpb_check_launch();
}

extern "C" int simpb_layernorm_f32(float* out, int ldo, const float* x0, int ld0, int k0, const float* x1, int ld1,
                                   int k1, const float* gamma, const float* beta, int num_rows, const int* m_live,
                                   void* stream) {
  if (!out || !x0 || !gamma || !beta || num_rows <= 0 || k0 <= 0 || k1 < 0 || (k1 > 0 && !x1)) return SIMPB_EINVAL;
  if (k0 + k1 > 512 || ldo < k0 + k1 || ld0 < k0 || (k1 > 0 && ld1 < k1)) return SIMPB_EINVAL;
  (void)hipGetLastError();
  hipLaunchKernelGGL(layernorm_seg_kernel, dim3((num_rows + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream),
                     out, ldo, x0, ld0, k0, x1, ld1, k1, gamma, beta, num_rows, m_live);
  return simpb_check_launch();
}
