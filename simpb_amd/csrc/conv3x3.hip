// 3x3 convolution (padding 1, stride 1 or 2) of the fp16 channels_last backbone as an implicit GEMM with its epilogue in
// the launch:   y[n, ho, wo, :] = relu?( sum_{dy,dx} x[n, ho*s + dy - 1, wo*s + dx - 1, :] . W[:, dy, dx, :]^T + bias )
// These are conv2 of every ResNet bottleneck and the four output convolutions of the FPN (mmdet ResNet style="pytorch" + FPN)
// after conv-BN folding (tools/fuse_conv_bn.py). The FPN's output convolutions write the decoder's token buffer themselves
// (`tok`, `tok16` below): no separate format pass.
//
// GEMM view: M = output pixels, N = output channels, K = 9 taps x Cin walked tap by tap in chunks of 64 input channels.
// Weights as PyTorch keeps a channels_last convolution weight: [Cout][3][3][Cin], i.e. row-major [Cout][K] in this chunk order.
//
//  variant  kernel                                       tile px x ch   waves    variant 0 runs it                  its bits are those of
//  1        conv3x3_f16_kernel<1, false>                 128 x 64       4 (M)    choose_variant                     1, 2, 9
//  2        conv3x3_f16_kernel<2, false>                 256 x 64       4 (M)    never (tests, tuning tools)        1, 2, 9
//  3        conv3x3_f16_kernel<1, true>                  32 x 64        4 (K)    choose_variant, the smallest maps  3, 4, 11
//  4        conv3x3_f16_kernel<2, true>                  64 x 64        4 (K)    choose_variant                     3, 4, 11
//  5        conv_staged_kernel<128, 64, 4, 1>            128 x 64       4 x 1    never                              5-8, 12, 13
//  6        conv_staged_kernel<128, 128, 2, 2>           128 x 128      2 x 2    choose_variant, >= 2048 tiles      5-8, 12, 13
//  7        conv_staged_kernel<96, 64, 3, 1>             96 x 64        3 x 1    choose_variant                     5-8, 12, 13
//  8        conv_staged_kernel<96, 128, 1, 4>            96 x 128       1 x 4    choose_variant; the group launch   5-8, 12, 13
//  9        conv_staged_ksplit_kernel<64, 64, 2, 2, 1>   64 x 64        2 x 2    choose_variant, Cin, Cout >= 256   1, 2, 9
//  10       conv_staged_ksplit_kernel<64, 64, 2, 2, 2>   64 x 64        2 x 2 x 2  never                            its own
//  11       conv_staged_ksplit_kernel<64, 64, 2, 2, 4>   64 x 64        2 x 2 x 4  choose_variant, Cin, Cout >= 512 3, 4, 11
//  12       conv_resident_kernel<Cin, 4, 64, 2, 2, 2>    4 x 16 x 64    2 x 2    choose_resident                    5-8, 12, 13
//  13       conv_resident_kernel<Cin, 8, 128, 4, 2, 3>   8 x 16 x 128   4 x 2    choose_resident; the group launch  5-8, 12, 13
// (the forms are stated once, as V1 .. V13 below; 1x1 convolutions run conv_staged_kernel with one tap: P0 .. P2.) Forms whose
// bits agree add the same products in the same order with the same eight k-values in every matrix instruction, so variant 0's
// choice between them changes no output.
// Every form has a LIVE sibling for the *_live entry points (a launch over the live images of the batch only: conv_parts.h,
// "the live-image table"): the same tile code with one more template argument, in kernels of their own, so that the code of
// the forms above is what it was. A live form gives a live image's pixels the bits of its sibling on the full batch.
//
// The direct forms (1-4): the MFMA contraction does not care WHICH eight k-values a lane brings as long as both operands agree,
// so lane (row r32, half kb) of a wave takes channels [32*kb, 32*kb + 32) of the chunk: its four 16-byte loads are 64 contiguous
// bytes of ITS pixel's row, and the A operand goes global -> registers directly; a tap outside the image is read from the
// pixel's own centre (always in bounds) and zeroed when it is consumed. The 4 waves of a workgroup share the work two ways:
//  * M split: waves tile M (32*AF pixels x 64 channels each); the 64 x 64 weight chunk is shared through a double-buffered
//    LDS stage (one barrier per chunk), three register sets of A in flight;
//  * K split: all four waves own the SAME 32*AF x 64 tile and take every fourth chunk; both operands straight from global
//    memory, no LDS and no barrier in the loop, one LDS meeting at the end.
// Both are bound by their load instructions (a wave-instruction touches 32 different lines); the staged and resident forms
// further below load whole lines.
//
// No double-K MFMA: the FP16 matrix step is two v_mfma_f32_32x32x8f16 (csrc/mfma_f16.h). The gfx950 double-K FP16 instruction
// makes other kernels' vector arithmetic go wrong while it runs, which is also why these convolutions
// are not left to the vendor library, whose fastest kernels for these shapes are built on it.
// Loads are pinned where they are written (sched_barrier): left to itself the scheduler sinks them to the end of the matrix
// work in front of their use, and the wait for them then drains the queue.
// LDS pitches: a staged chunk row is LDH = 72 halfs (144 B, an odd number of 16-byte slots: conflict-free 16-lane groups for
// ds_read_b128); a wave's fp32 epilogue tile has an odd pitch in floats (LDC, 32 * NF + 1); the resident halo: see there.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include "../../include/simpb_hip.h"
#include "conv_parts.h"

#include "launch.h"

namespace {

using namespace simpb::conv;   // vector types, BN / BK / LDH / LDC / kThreads, pixel split, epilogue parts

constexpr int kStageBytes = 2 * BN * LDH * 2;        // two weight chunks
constexpr int kTileBytes = 4 * 32 * LDC * 4;         // one 32 x 64 fp32 tile per wave
constexpr int kSmemBytes = kStageBytes > kTileBytes ? kStageBytes : kTileBytes;

struct ConvArgs {
  _Float16* y;            // f16 [P_out, Cout] or NULL
  float* tok;             // f32 token buffer or NULL (ops/__init__.py:63-92 layout: [bs, cams * tokens_per_cam, Cout])
  _Float16* tok16;        // the same rows in f16 (for value_proj's two-pass product) or NULL
  const _Float16 *x, *w, *bias;
  const _Float16* residual;   // f16 like y (or half-size with res_up: read with nearest 2x upsampling), or NULL
  int res_up;
  int P_out, Cin, Cout, relu, stride, Ho, Wo, H, W;
  int tokens_per_cam, level_start;
  int gx, gy, per_xcd;    // tile grid and tiles per XCD range
  int tiles_w, tiles_h;   // resident form: 2-D tiles across and down one image (gx = images x tiles_h x tiles_w)
};

// Several convolutions of one form in ONE launch (the FPN's four output convolutions: 240 us as four launches, of which
// the three small levels -- 352, 88 and 22 tiles -- leave most of the chip idle for 97 us; in one launch their tiles fill
// the last round of the large level's 1 408). Problem j owns the tiles [start[j], start[j + 1]) of one XCD-contiguous walk.
constexpr int kMaxConvGroup = 4;
struct ConvGroup {
  ConvArgs a[kMaxConvGroup];
  int start[kMaxConvGroup + 1];
  int n, per_xcd;
};
__device__ __forceinline__ int group_problem(const ConvGroup& g, int gt) {
  int j = 0;
#pragma unroll
  for (int t = 1; t < kMaxConvGroup; ++t)
    if (t < g.n && gt >= g.start[t]) j = t;
  return j;
}

// one 16-byte piece of an output row (channels c0 + c8 .. + 7 of pixel p; Cout is a multiple of 8, so a piece lies inside
// the channels or outside them, never across): the epilogue element, then to the f16 map or, widened, to the token buffer.
// TOK16 (a kernel's template argument): the launch writes the f16 token rows alone (tok == NULL, tok16 set) -- the fp32
// conversions and stores are not in that kernel at all
template <bool TOK16>
__device__ __forceinline__ void emit_piece(const ConvArgs& a, int c0, int p, int c8, const float (&v)[8]) {
  const int c = c0 + c8;
  if (p >= a.P_out || c >= a.Cout) return;
  const bool to_tokens = TOK16 || a.tok;   // the FPN's output convolution writes the decoder's token row itself
  size_t row = p;                         // the piece's row in the map, or in the token buffer
  if (to_tokens) {
    const int hw = a.Ho * a.Wo;
    const int n = p / hw, pix = p - n * hw;
    row = (size_t)n * a.tokens_per_cam + a.level_start + pix;
  }
  const size_t at = row * a.Cout + c;
  const h16x8 bv = *reinterpret_cast<const h16x8*>(a.bias + c);
  h16x8 rv = {0, 0, 0, 0, 0, 0, 0, 0};
  if (a.residual) rv = *reinterpret_cast<const h16x8*>(a.residual + (size_t)(a.res_up ? up2_row(p, a.Ho, a.Wo) : p) * a.Cout + c);
  const h16x8 o = finish_piece(v, bv, rv, a.relu);
  if (!to_tokens) {
    *reinterpret_cast<h16x8*>(a.y + at) = o;
  } else {   // the fp16 result, widened to fp32 or (TOK16) as it is
    if constexpr (!TOK16) {
      *reinterpret_cast<float4*>(a.tok + at) = make_float4((float)o[0], (float)o[1], (float)o[2], (float)o[3]);
      *reinterpret_cast<float4*>(a.tok + at + 4) = make_float4((float)o[4], (float)o[5], (float)o[6], (float)o[7]);
    }
    if (TOK16 || a.tok16) *reinterpret_cast<h16x8*>(a.tok16 + at) = o;
  }
}

// The live forms' walk over flat tiles of BMt virtual pixels (conv_parts.h): the tile grid of `a` (gx, per_xcd) becomes that
// of the live images, which the ordinary walk then deals out; everything else of `a`, P_out included, goes on describing
// the real arrays. Uniform: one load of L and a few scalar operations.
template <int BMt>
__device__ __forceinline__ void live_flat_walk(ConvArgs& a, const LiveTable& lt) {
  a.gx = (live_count(lt) * a.Ho * a.Wo + BMt - 1) / BMt;
  a.per_xcd = (a.gx * a.gy + 7) >> 3;
}

// Lt: nothing (the launch as ever, the kernel as ever) or the LiveTable of a live launch. (The kernels whose tile is a
// function of its own further below have a second kernel for the live form; here the body is the kernel's, and moving it
// changes the registers of the ordinary form.)
template <int AF, bool KSPLIT, bool TOK16, class... Lt>
__global__ __launch_bounds__(kThreads, 2) void conv3x3_f16_kernel(std::conditional_t<sizeof...(Lt) != 0, ConvArgs, const ConvArgs> a,
                                                                  const Lt... live) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[kSmemBytes];
  _Float16* s_b = reinterpret_cast<_Float16*>(smem);
  float* s_c = reinterpret_cast<float*>(smem);
  constexpr int WROWS = 32 * AF;
  constexpr int BMt = KSPLIT ? WROWS : 4 * WROWS;
  constexpr bool LIVE = sizeof...(Lt) != 0;
  const LiveTable lt = table_of(live...);
  if constexpr (LIVE) live_flat_walk<BMt>(a, lt);

  // channel blocks of one pixel block are next to each other in an XCD's range: neighbouring tiles share their activation rows
  const int tile = simpb::xcd_tile(a.per_xcd, a.gx * a.gy);
  if (tile < 0) return;
  const int tx = tile / a.gy, ty = tile - tx * a.gy;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int r32 = lane & 31, kb = lane >> 5;
  const int p0 = tx * BMt, c0 = ty * BN;
  const int row0 = KSPLIT ? 0 : wave * WROWS;
  const int Cin = a.Cin, W = a.W, H = a.H;
  const int per_tap = Cin / BK, nchunks = 9 * per_tap;
  const size_t K = (size_t)9 * Cin;
  const _Float16* __restrict__ wgt = a.w;
  // LIVE: the tile's rows are virtual pixels of the `walked` live ones; what each is in memory is looked up once, in front of
  // every store of the kernel, and kept for the epilogue (the barriers of the K loop lie between)
  const int walked = LIVE ? live_count(lt) * a.Ho * a.Wo : a.P_out;
  const int* real_row = nullptr;
  if constexpr (LIVE) {
    __shared__ int s_rows[BMt];
    live_tile_rows<BMt>(s_rows, lt, p0, walked, a.Ho * a.Wo, a.P_out);
    real_row = s_rows;
  }

  // A: this lane's pixel per fragment: centre address (+ its half of the chunk) and the 9-bit in-image mask of its taps
  const _Float16* actr[AF];
  unsigned amask[AF];
#pragma unroll
  for (int f = 0; f < AF; ++f) {
    Pixel q = split_pixel(min(p0 + row0 + 32 * f + r32, walked - 1), a.Ho, a.Wo);
    if constexpr (LIVE) q.n = live_image(lt, q.n);
    const int hc = q.ho * a.stride, wc = q.wo * a.stride;
    actr[f] = a.x + ((size_t)(q.n * H + hc) * W + wc) * Cin + 32 * kb;
    unsigned m = 0;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int hi = hc + t / 3 - 1, wi = wc + t % 3 - 1;
      m |= (hi >= 0 && hi < H && wi >= 0 && wi < W) ? (1u << t) : 0u;
    }
    amask[f] = m;
  }
  // B rows: MSPLIT stages 64 rows x 8 pieces with 256 threads (2 pieces each); KSPLIT loads its fragments directly
  const int sr = tid >> 3, sc = (tid & 7) * 8;
  size_t brow[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
    brow[i] = KSPLIT ? (size_t)min(c0 + 32 * i + r32, a.Cout - 1) * K + 32 * kb : (size_t)min(c0 + sr + 32 * i, a.Cout - 1) * K + sc;

  h16x8 ar[3][AF][4];
  h16x8 bp[3][2];        // MSPLIT: staged pieces
  h16x8 bq[3][2][4];     // KSPLIT: fragments
  unsigned alive[3];     // bit f: fragment f of the set is inside the image (and the chunk exists)

  auto load_a = [&](auto set_c, int chunk) __attribute__((always_inline)) {
    constexpr int s = decltype(set_c)::value;
    const bool exists = chunk < nchunks;
    const int c = min(chunk, nchunks - 1);
    const int tap = c / per_tap, k0 = (c - tap * per_tap) * BK;
    const int dy = tap / 3, dx = tap - dy * 3;
    const int toff = ((dy - 1) * W + (dx - 1)) * Cin;
    unsigned m = 0;
#pragma unroll
    for (int f = 0; f < AF; ++f) {
      const bool in = ((amask[f] >> tap) & 1u) != 0 && exists;
      m |= (in ? 1u : 0u) << f;
      const _Float16* src = actr[f] + (in ? toff : 0) + k0;
#pragma unroll
      for (int j = 0; j < 4; ++j) ar[s][f][j] = *reinterpret_cast<const h16x8*>(src + 8 * j);
    }
    alive[s] = m;
  };
  auto load_b = [&](auto set_c, int chunk) __attribute__((always_inline)) {
    constexpr int s = decltype(set_c)::value;
    const int c = min(chunk, nchunks - 1);
    const int tap = c / per_tap, k0 = (c - tap * per_tap) * BK;
    const size_t koff = (size_t)tap * Cin + k0;
    if constexpr (KSPLIT) {
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int j = 0; j < 4; ++j) bq[s][n][j] = *reinterpret_cast<const h16x8*>(wgt + brow[n] + koff + 8 * j);
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i) bp[s][i] = *reinterpret_cast<const h16x8*>(wgt + brow[i] + koff);
    }
  };
  auto stash_b = [&](auto set_c, int buf) __attribute__((always_inline)) {
    constexpr int s = decltype(set_c)::value;
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<h16x8*>(&s_b[(buf * BN + sr + 32 * i) * LDH + sc]) = bp[s][i];
  };

  f32x16 acc[AF][2];
  zero_acc(acc);

  auto multiply = [&](auto set_c, int buf) __attribute__((always_inline)) {
    constexpr int s = decltype(set_c)::value;
    const h16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      h16x8 b[2];
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        if constexpr (KSPLIT) b[n] = bq[s][n][j];
        else b[n] = *reinterpret_cast<const h16x8*>(&s_b[(buf * BN + n * 32 + r32) * LDH + 32 * kb + 8 * j]);
      }
#pragma unroll
      for (int f = 0; f < AF; ++f) {
        const h16x8 av = ((alive[s] >> f) & 1u) ? ar[s][f][j] : zero;
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[f][n] = simpb::mfma_32x32x16_f16(av, b[n], acc[f][n]);
      }
    }
  };

  if constexpr (KSPLIT) {
    // wave w takes chunks w, w + 4, ...; three register sets in flight; chunks past the end are loaded from the last one
    // and contribute zeros (alive = 0)
    const int mine_n = (nchunks + 3) / 4;
    auto step = [&](auto cur, auto nxt, int chunk) __attribute__((always_inline)) {
      load_a(nxt, chunk);
      load_b(nxt, chunk);
      __builtin_amdgcn_sched_barrier(0);
      multiply(cur, 0);
      __builtin_amdgcn_sched_barrier(0);
    };
    load_a(IC<0>{}, wave);
    load_b(IC<0>{}, wave);
    if constexpr (AF == 1) {
      load_a(IC<1>{}, wave + 4);
      load_b(IC<1>{}, wave + 4);
      for (int i = 0; i < (mine_n + 2) / 3 * 3; i += 3) {
        step(IC<0>{}, IC<2>{}, wave + 4 * (i + 2));
        step(IC<1>{}, IC<0>{}, wave + 4 * (i + 3));
        step(IC<2>{}, IC<1>{}, wave + 4 * (i + 4));
      }
    } else {
      // 64 x 64 tile per wave: two register sets (a chunk is 16 matrix steps of cover)
      for (int i = 0; i < (mine_n + 1) / 2 * 2; i += 2) {
        step(IC<0>{}, IC<1>{}, wave + 4 * (i + 1));
        step(IC<1>{}, IC<0>{}, wave + 4 * (i + 2));
      }
    }
  } else {
    // chunk c: A(c) in register set c % 3 (requested two chunks ago); B(c) in LDS buffer c & 1, written during chunk c - 1
    // from register set c % 3 (requested during chunk c - 3)
    load_b(IC<0>{}, 0);
    load_b(IC<1>{}, 1);
    load_b(IC<2>{}, 2);
    load_a(IC<0>{}, 0);
    load_a(IC<1>{}, 1);
    __builtin_amdgcn_sched_barrier(0);
    stash_b(IC<0>{}, 0);
    __syncthreads();
    auto step = [&](auto cur, auto nxt, auto nxt2, int c) __attribute__((always_inline)) {
      load_b(cur, c + 3);    // set `cur` was written to LDS during chunk c - 1
      load_a(nxt2, c + 2);
      __builtin_amdgcn_sched_barrier(0);
      stash_b(nxt, (c + 1) & 1);
      __builtin_amdgcn_sched_barrier(0);
      multiply(cur, c & 1);
      __syncthreads();
    };
    for (int c = 0; c < nchunks; c += 3) {   // nchunks = 9 * per_tap: a multiple of 3
      step(IC<0>{}, IC<1>{}, IC<2>{}, c);
      step(IC<1>{}, IC<2>{}, IC<0>{}, c + 1);
      step(IC<2>{}, IC<0>{}, IC<1>{}, c + 2);
    }
  }

  // epilogue, one A fragment at a time through the waves' fp32 tiles
  float* mine = s_c + wave * 32 * LDC;
#pragma unroll
  for (int f = 0; f < AF; ++f) {
    __syncthreads();   // the weight stage (or the previous fragment's tile) is no longer read
    acc_to_tile<2, LDC>(mine, acc[f], r32, kb);
    __syncthreads();
    if constexpr (KSPLIT) {
      // the meeting of the K split: every thread adds one piece of the four waves' tiles, in a fixed order. (Not
      // tile_pieces: there a WAVE walks all 32 rows; here the four waves share them.)
      const int r = tid >> 3, c8 = (tid & 7) * 8;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float s = 0.f;
#pragma unroll
        for (int w4 = 0; w4 < 4; ++w4) s += s_c[(w4 * 32 + r) * LDC + c8 + e];
        v[e] = s;
      }
      emit_piece<TOK16>(a, c0, LIVE ? real_row[32 * f + r] : p0 + 32 * f + r, c8, v);
    } else {
      tile_pieces<2, LDC>(mine, 0, lane, [&](int, int r, int c8, const float (&v)[8]) __attribute__((always_inline)) {
        emit_piece<TOK16>(a, c0, LIVE ? real_row[row0 + 32 * f + r] : p0 + row0 + 32 * f + r, c8, v);
      });
    }
  }
}

// ---- both operands staged through LDS with coalesced loads (variants 5-11, the 1x1 tilings) ------------------------------------
// Reading A straight into the MFMA layout costs a wave-instruction 32 different 128-byte lines (one per pixel row, two lanes
// each), and the texture path takes them a quad of lanes at a time: the direct kernels above top out near 430 TFLOP/s on the
// 64 x 176 maps with the matrix cores half idle. Here 8 consecutive lanes load the 8 pieces of one pixel row (a
// wave-instruction = 8 whole lines), the chunk goes through a double-buffered LDS stage (one barrier per chunk, three register
// sets: loads run two chunks ahead), and fragments are read back with ds_read_b128 (256 B/clk per CU on gfx950, conflict-free
// at a 144-byte row pitch). BMt x BNt output tile, WGM x WGN waves, each (BMt / WGM) x (BNt / WGN). The tile is chosen per shape so
// that the grid fills whole rounds of the chip: 67 584 pixels are 528 tiles of 128 (two per CU and sixteen left over) but 704 of 96.
//
// KS > 1 (small maps, long K: stages 3-4): the workgroup is KS such pipelines side by side, 64 * WGM * WGN * KS threads. Group g
// of WGM x WGN waves stages and multiplies the chunks g, g + KS, ... in that order through a stage of its own; the groups
// share only the barrier, so one barrier passes KS chunks and a SIMD holds KS waves. At the end group 0 adds the groups'
// partial tiles in ascending g (a fixed order) and writes the output.
//
// DIRECTK: lane (r32, kb) reads channels [32 * kb + 8 * j, + 8) of the chunk at matrix step j, as the direct kernels above
// do, where the pipeline's own map is [16 * j + 8 * kb, + 8). Which eight k-values share a matrix instruction decides how
// their sum is rounded: with the direct map, KS = 1 adds exactly what conv3x3_f16_kernel<., false> adds and KS = 4 what
// conv3x3_f16_kernel<., true> adds, in the same order -- the same bits, so replacing one by the other changes no output.
template <int BMt, int BNt, int WGM, int WGN, int TAPS, bool TOK16, int KS = 1, bool DIRECTK = false, bool LIVE = false>
__device__ __forceinline__ void conv_staged_tile(const ConvArgs& a, const int tile, const LiveTable& lt = {}) {
  constexpr int NT = 64 * WGM * WGN;   // threads of one K group
  constexpr int AF = BMt / WGM / 32, NF = BNt / WGN / 32;
  static_assert(AF * WGM * 32 == BMt && NF * WGN * 32 == BNt && NF <= 2, "tile = waves x 32-row / 32-column fragments");
  constexpr int NA = (BMt * 8 + NT - 1) / NT, NB = (BNt * 8 + NT - 1) / NT;   // staged 16-byte pieces per thread and chunk
  constexpr int kRows = BMt + BNt;
  constexpr int LDW = 32 * NF + 1;                                             // floats per row of a wave's epilogue tile
  constexpr int kStage = KS * 2 * kRows * LDH * 2, kTile = KS * WGM * WGN * 32 * LDW * 4;
  __shared__ __attribute__((aligned(16))) unsigned char smem[kStage > kTile ? kStage : kTile];
  const int grp = KS > 1 ? (int)threadIdx.x / NT : 0;   // wave-uniform
  _Float16* s_ab = reinterpret_cast<_Float16*>(smem) + grp * (2 * kRows * LDH);
  float* s_c = reinterpret_cast<float*>(smem);

  const int tx = tile / a.gy, ty = tile - tx * a.gy;
  const int tid = threadIdx.x - grp * NT;
  const int lane = tid & 63, wave = tid >> 6;
  const int r32 = lane & 31, kb = lane >> 5;
  const int wm = WGM == 1 ? 0 : wave / WGN, wn = wave - wm * WGN;   // (said outright for one row of waves: a register less)
  const int p0 = tx * BMt, c0 = ty * BNt;
  const int Cin = a.Cin, W = a.W, H = a.H;
  const int per_tap = Cin / BK, nchunks = TAPS * per_tap;
  const int nsteps = (nchunks + KS - 1) / KS;   // a group's chunk of a step past the last chunk is staged as zeros
  const size_t K = (size_t)TAPS * Cin;
  const _Float16* __restrict__ wgt = a.w;
  // LIVE: as in conv3x3_f16_kernel, the rows' real pixels are looked up in front of every store and kept for the epilogue
  const int walked = LIVE ? live_count(lt) * a.Ho * a.Wo : a.P_out;
  const int* real_row = nullptr;
  if constexpr (LIVE) {
    __shared__ int s_rows[BMt];
    live_tile_rows<BMt>(s_rows, lt, p0, walked, a.Ho * a.Wo, a.P_out);
    real_row = s_rows;
  }

  // piece i of this thread: index tid + NT * i -> (row, 8-half column) of the A or B part of the stage
  const int sc = (tid & 7) * 8;
  const _Float16* actr[NA];   // centre of this thread's staged pixel rows (+ its piece)
  unsigned amask = 0;         // 6 bits per row: which of the 3 input rows / 3 input columns around it are inside the image
  static_assert(NA <= 5, "6 mask bits per staged row in one register");
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    Pixel q = split_pixel(min(p0 + ((tid + NT * i) >> 3), walked - 1), a.Ho, a.Wo);
    if constexpr (LIVE) q.n = live_image(lt, q.n);
    const int hc = q.ho * a.stride, wc = q.wo * a.stride;
    actr[i] = a.x + ((size_t)(q.n * H + hc) * W + wc) * Cin + sc;
    const unsigned rows = (hc > 0 ? 1u : 0u) | 2u | (hc + 1 < H ? 4u : 0u), cols = (wc > 0 ? 1u : 0u) | 2u | (wc + 1 < W ? 4u : 0u);
    amask |= (rows | (cols << 3)) << (6 * i);
  }
  size_t brow[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) brow[i] = (size_t)min(c0 + ((tid + NT * i) >> 3), a.Cout - 1) * K + sc;

  h16x8 ra[3][NA], rb[3][NB];
  unsigned alive[3];

  auto fetch = [&](auto set_c, int step_i) __attribute__((always_inline)) {
    constexpr int s = decltype(set_c)::value;
    const int chunk = step_i * KS + grp;
    const bool exists = KS == 1 || chunk < nchunks;
    const int c = min(chunk, nchunks - 1);
    if constexpr (TAPS == 1) {   // a 1x1 convolution: the centre pixel only, always inside the image
      const int k0 = c * BK;
#pragma unroll
      for (int i = 0; i < NA; ++i) ra[s][i] = *reinterpret_cast<const h16x8*>(actr[i] + k0);
      alive[s] = exists ? ~0u : 0u;
#pragma unroll
      for (int i = 0; i < NB; ++i) rb[s][i] = *reinterpret_cast<const h16x8*>(wgt + brow[i] + k0);
    } else {
      const int tap = c / per_tap, k0 = (c - tap * per_tap) * BK;
      const int dy = tap / 3, dx = tap - dy * 3;
      const int toff = ((dy - 1) * W + (dx - 1)) * Cin;
      unsigned m = 0;
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const bool in = ((amask >> (6 * i + dy)) & (amask >> (6 * i + 3 + dx)) & 1u) != 0;
        m |= (in ? 1u : 0u) << i;
        ra[s][i] = *reinterpret_cast<const h16x8*>(actr[i] + (in ? toff : 0) + k0);
      }
      alive[s] = exists ? m : 0u;
      const size_t koff = (size_t)tap * Cin + k0;
#pragma unroll
      for (int i = 0; i < NB; ++i) rb[s][i] = *reinterpret_cast<const h16x8*>(wgt + brow[i] + koff);
    }
  };
  auto stash = [&](auto set_c, int buf) __attribute__((always_inline)) {
    constexpr int s = decltype(set_c)::value;
    const h16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    _Float16* base = s_ab + buf * kRows * LDH;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int idx = tid + NT * i;
      if ((BMt * 8) % NT == 0 || idx < BMt * 8)
        *reinterpret_cast<h16x8*>(&base[(idx >> 3) * LDH + sc]) = ((alive[s] >> i) & 1u) ? ra[s][i] : zero;
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int idx = tid + NT * i;
      if ((BNt * 8) % NT == 0 || idx < BNt * 8) *reinterpret_cast<h16x8*>(&base[(BMt + (idx >> 3)) * LDH + sc]) = rb[s][i];
    }
  };

  f32x16 acc[AF][NF];
  zero_acc(acc);

  auto multiply = [&](int buf) __attribute__((always_inline)) {
    constexpr int KLANE = DIRECTK ? 32 : 8, KSTEP = DIRECTK ? 8 : 16;   // halfs between the lane halves / the matrix steps
    const _Float16* sa = s_ab + buf * kRows * LDH + (wm * AF * 32 + r32) * LDH + KLANE * kb;
    const _Float16* sb = s_ab + buf * kRows * LDH + (BMt + wn * NF * 32 + r32) * LDH + KLANE * kb;
#pragma unroll
    for (int ks = 0; ks < BK / 16; ++ks) {
      h16x8 av[AF], bv[NF];
#pragma unroll
      for (int f = 0; f < AF; ++f) av[f] = *reinterpret_cast<const h16x8*>(sa + f * 32 * LDH + KSTEP * ks);
#pragma unroll
      for (int n = 0; n < NF; ++n) bv[n] = *reinterpret_cast<const h16x8*>(sb + n * 32 * LDH + KSTEP * ks);
#pragma unroll
      for (int f = 0; f < AF; ++f)
#pragma unroll
        for (int n = 0; n < NF; ++n) acc[f][n] = simpb::mfma_32x32x16_f16(av[f], bv[n], acc[f][n]);
    }
  };

  // chunk c: LDS buffer c & 1; register set (c + 1) % 3 holds chunk c + 1 (requested during chunk c - 2)
  fetch(IC<0>{}, 0);
  fetch(IC<1>{}, 1);
  fetch(IC<2>{}, 2);
  __builtin_amdgcn_sched_barrier(0);
  stash(IC<0>{}, 0);
  __syncthreads();
  auto step = [&](auto cur, auto nxt, int c) __attribute__((always_inline)) {
    fetch(cur, c + 3);      // set `cur` went to LDS during chunk c - 1
    __builtin_amdgcn_sched_barrier(0);
    stash(nxt, (c + 1) & 1);
    __builtin_amdgcn_sched_barrier(0);
    multiply(c & 1);
    __syncthreads();
  };
  for (int c = 0; c < nsteps; c += 3) {   // 9 * per_tap is a multiple of 3; a 1x1 convolution or a K split has any count
    step(IC<0>{}, IC<1>{}, c);
    if ((TAPS == 9 && KS == 1) || c + 1 < nsteps) step(IC<1>{}, IC<2>{}, c + 1);
    if ((TAPS == 9 && KS == 1) || c + 2 < nsteps) step(IC<2>{}, IC<0>{}, c + 2);
  }

  // epilogue, one A fragment at a time through the wave's own 32 x (32 * NF) fp32 tile
  float* mine = s_c + (grp * WGM * WGN + wave) * 32 * LDW;
  const int cw = c0 + wn * NF * 32;
#pragma unroll
  for (int f = 0; f < AF; ++f) {
    if (f) __syncthreads();
    acc_to_tile<NF, LDW>(mine, acc[f], r32, kb);
    __syncthreads();
    if (KS > 1 && grp) continue;          // K split: group 0 adds the partial tiles of its wave's place in every group
    tile_pieces<NF, LDW, KS>(mine, WGM * WGN * 32 * LDW, lane, [&](int, int r, int c8, const float (&v)[8]) __attribute__((always_inline)) {
      emit_piece<TOK16>(a, cw, LIVE ? real_row[(wm * AF + f) * 32 + r] : p0 + (wm * AF + f) * 32 + r, c8, v);
    });
  }
}

template <int BMt, int BNt, int WGM, int WGN, int TAPS, bool TOK16>
__global__ __launch_bounds__(64 * WGM * WGN, WGM * WGN == 3 ? 3 : 2) void conv_staged_kernel(const ConvArgs a) {
  const int tile = simpb::xcd_tile(a.per_xcd, a.gx * a.gy);
  if (tile < 0) return;
  conv_staged_tile<BMt, BNt, WGM, WGN, TAPS, TOK16>(a, tile);
}

template <int BMt, int BNt, int WGM, int WGN, int TAPS, bool TOK16>
__global__ __launch_bounds__(64 * WGM * WGN, WGM * WGN == 3 ? 3 : 2) void conv_staged_live_kernel(const ConvArgs full, const LiveTable lt) {
  ConvArgs a = full;
  live_flat_walk<BMt>(a, lt);
  const int tile = simpb::xcd_tile(a.per_xcd, a.gx * a.gy);
  if (tile < 0) return;
  conv_staged_tile<BMt, BNt, WGM, WGN, TAPS, TOK16, 1, false, true>(a, tile, lt);
}

// the small maps with long K (3x3 variants 9-11): KS groups of waves, the direct kernels' k map (their sums, bit for bit)
template <int BMt, int BNt, int WGM, int WGN, int TAPS, bool TOK16, int KS>
__global__ __launch_bounds__(64 * WGM * WGN * KS, 2) void conv_staged_ksplit_kernel(const ConvArgs a) {
  const int tile = simpb::xcd_tile(a.per_xcd, a.gx * a.gy);
  if (tile < 0) return;
  conv_staged_tile<BMt, BNt, WGM, WGN, TAPS, TOK16, KS, true>(a, tile);
}

template <int BMt, int BNt, int WGM, int WGN, int TAPS, bool TOK16, int KS>
__global__ __launch_bounds__(64 * WGM * WGN * KS, 2) void conv_staged_ksplit_live_kernel(const ConvArgs full, const LiveTable lt) {
  ConvArgs a = full;
  live_flat_walk<BMt>(a, lt);
  const int tile = simpb::xcd_tile(a.per_xcd, a.gx * a.gy);
  if (tile < 0) return;
  conv_staged_tile<BMt, BNt, WGM, WGN, TAPS, TOK16, KS, true, true>(a, tile, lt);
}

template <int BMt, int BNt, int WGM, int WGN, int TAPS, bool TOK16>
__global__ __launch_bounds__(64 * WGM * WGN, WGM * WGN == 3 ? 3 : 2) void conv_staged_group_kernel(const ConvGroup g) {
  const int gt = simpb::xcd_tile(g.per_xcd, g.start[g.n]);
  if (gt < 0) return;
  const int j = group_problem(g, gt);
  conv_staged_tile<BMt, BNt, WGM, WGN, TAPS, TOK16>(g.a[j], gt - g.start[j]);
}

// The live group walk: the problems' tile ranges start[j] follow from L, so they are made here; `a` becomes this workgroup's
// problem over the live images; -> its tile there or -1. shrink(a): a problem's tile grid (gx) for the live count.
template <class Shrink>
__device__ __forceinline__ int live_group_tile(const ConvGroup& g, ConvArgs& a, Shrink&& shrink) {
  int start[kMaxConvGroup + 1];
  start[0] = 0;
#pragma unroll
  for (int t = 0; t < kMaxConvGroup; ++t) {
    ConvArgs b = g.a[t];
    shrink(b);
    start[t + 1] = start[t] + (t < g.n ? b.gx * b.gy : 0);
  }
  const int total = start[kMaxConvGroup];
  const int gt = simpb::xcd_tile((total + 7) >> 3, total);
  if (gt < 0) return -1;
  int j = 0;
#pragma unroll
  for (int t = 1; t < kMaxConvGroup; ++t)
    if (t < g.n && gt >= start[t]) j = t;
  int first = 0;
#pragma unroll
  for (int t = 0; t < kMaxConvGroup; ++t)
    if (t == j) {
      a = g.a[t];
      first = start[t];
    }
  shrink(a);
  return gt - first;
}

template <int BMt, int BNt, int WGM, int WGN, int TAPS, bool TOK16>
__global__ __launch_bounds__(64 * WGM * WGN, WGM * WGN == 3 ? 3 : 2) void conv_staged_group_live_kernel(const ConvGroup g, const LiveTable lt) {
  const int L = live_count(lt);
  ConvArgs a;
  const int tile = live_group_tile(g, a, [&](ConvArgs& b) { b.gx = (L * b.Ho * b.Wo + BMt - 1) / BMt; });
  if (tile < 0) return;
  conv_staged_tile<BMt, BNt, WGM, WGN, TAPS, TOK16, 1, false, true>(a, tile, lt);
}

// ---- stride 1: the input tile stays in LDS (3x3 variants 12, 13) --------------------------------------------------------------
// The staged pipeline above stages the A tile once per chunk: nine taps x Cin / 64 times the same pixels, shifted by one tap.
// Here a workgroup owns a 2-D tile of TH x 16 output pixels of ONE image (clipped at the image's border) and loads the
// (TH + 2) x 18 input pixels under it, all Cin channels, into LDS once, with the same coalesced 16-byte loads (8 lanes per 128
// bytes of a pixel's row); a pixel outside the image is written as zeros -- that is the padding, there are no per-tap masks.
// A tap is then an address: fragment row r32 of a wave is output pixel (2 * fragment + r32 / 16, r32 % 16) of the tile, and
// tap (dy, dx) reads input pixel (row + dy, column + dx) of the halo. Only the 64-channel weight chunks still go through an
// LDS stage, one barrier per chunk (1 + 9 * Cin / 64 per tile of 128 pixels, the count of the 96-pixel staged tile).
//  * All loads of the halo are issued at once, 64 channels (what one chunk reads) per slice; slice 0 is written to LDS in
//    front of the first barrier, slice s > 0 during chunk s - 1: the first Cin / 64 chunks run while the rest is in flight.
//  * The weight stage is a ring of THREE chunks: chunk c + 2 is written during chunk c, so chunk c + 1 is complete and
//    visible while chunk c runs, and a wave reads its first operands of chunk c + 1 (weights and, resident anyway, pixels)
//    BEFORE the barrier that ends chunk c -- after the barrier the matrix pipe goes on at once instead of waiting for LDS.
// LDS image: a pixel's channels at a pitch of 2 * Cin + 16 bytes (an odd number of 16-byte slots, like the 144 bytes of the
// weight stage) and a halo row at a pitch that is a multiple of 256 bytes. ds_read_b128 serves lanes {0-3, 12-15, 20-27} in
// one cycle and {4-11, 16-19, 28-31} in the next: each group is eight pixels of one tile row and the OTHER eight columns of
// the next row, so with the row pitch a multiple of the 256-byte bank row the sixteen lanes hit sixteen different slots --
// that is how the jump at the end of a tile row is handled (a plain 18-pixel row pitch would put two pairs of them on one
// slot). Taps shift every lane by the same amount and keep that.
// Every output element receives what conv_staged_tile<.., DIRECTK = false> gives it: tap-major, then 64-channel chunk, then
// four 16-deep steps of two v_mfma_f32_32x32x8f16, lane half kb bringing halfs [16 j + 8 kb, + 8) of the chunk, zero operands
// outside the image, one accumulator per 32 x 32 fragment -- the same bits as variants 5-8.
constexpr int RTW = 16, RHW = RTW + 2;   // output pixels across a tile; input pixels across its halo
constexpr int resident_row_bytes(int cin) { return (RHW * (2 * cin + 16) + 255) & ~255; }

template <int CIN, int TH, int BNt, int WGM, int WGN, int RING>
constexpr size_t resident_lds() {
  const size_t run = (size_t)(TH + 2) * resident_row_bytes(CIN) + RING * BNt * LDH * 2;   // halo + the weight ring
  const size_t tile = (size_t)WGM * WGN * 32 * (BNt / WGN + 1) * 4;                    // the waves' fp32 epilogue tiles
  return run > tile ? run : tile;
}

template <int CIN, int TH, int BNt, int WGM, int WGN, int RING, bool TOK16, bool LIVE = false>
__device__ __forceinline__ void conv_resident_tile(const ConvArgs& a, const int tile, unsigned char* smem, const LiveTable& lt = {}) {
  constexpr int NT = 64 * WGM * WGN;
  constexpr int AF = TH * RTW / WGM / 32, NF = BNt / WGN / 32;
  static_assert(AF * WGM * 32 == TH * RTW && NF * WGN * 32 == BNt && NF <= 2, "tile = waves x 32-row / 32-column fragments");
  static_assert(CIN == 64 || CIN == 128 || CIN == 256, "the whole Cin is resident");
  static_assert(RING == 2 || RING == 3, "weight chunks in LDS");
  constexpr int D = RING - 1;                   // chunk c + D is written to the ring during chunk c
  constexpr int PT = CIN / BK, NCH = 9 * PT;    // chunks per tap (= halo slices) and in all
  constexpr int HEAD = PT <= 2 ? 3 : 6;         // chunks in front of the loop: a multiple of 3 that covers the slices
  constexpr int NB = (BNt * 8 + NT - 1) / NT;   // staged 16-byte weight pieces per thread and chunk
  constexpr int LDW = 32 * NF + 1;
  constexpr int HP = (TH + 2) * RHW;            // pixels of the halo tile
  constexpr int NH = (HP * 8 + NT - 1) / NT;    // 16-byte pieces per thread and slice
  constexpr int PIX = 2 * CIN + 16, ROW = resident_row_bytes(CIN);
  constexpr int WBUF = BNt * LDH;               // halfs of one weight chunk
  _Float16* s_b = reinterpret_cast<_Float16*>(smem + (TH + 2) * ROW);
  float* s_c = reinterpret_cast<float*>(smem);
  const int W = a.W, H = a.H;

  const int tx = tile / a.gy, ty = tile - tx * a.gy;
  const int per_img = a.tiles_w * a.tiles_h;
  const int vimg = tx / per_img, t2 = tx - vimg * per_img;
  const int img = LIVE ? live_image(lt, vimg) : vimg;   // a 2-D tile lies in ONE image: the real one, looked up once
  const int trow = t2 / a.tiles_w;
  const int y0 = trow * TH, x0 = (t2 - trow * a.tiles_w) * RTW;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int r32 = lane & 31, kb = lane >> 5;
  const int wm = wave / WGN, wn = wave - wm * WGN;
  const int c0 = ty * BNt;
  constexpr size_t K = (size_t)9 * CIN;
  const _Float16* __restrict__ wgt = a.w;
  const h16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};

  const int sc = (tid & 7) * 8;
  size_t brow[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) brow[i] = (size_t)min(c0 + ((tid + NT * i) >> 3), a.Cout - 1) * K + sc;
  h16x8 rb[3][NB];   // set s: a chunk = s (mod 3) on its way to the ring
  auto fetch = [&](auto set_c, int chunk) __attribute__((always_inline)) {
    constexpr int s = decltype(set_c)::value;
    const size_t koff = (size_t)min(chunk, NCH - 1) * BK;   // [Cout][3][3][Cin]: chunk c is halfs [64 c, 64 c + 64) of a row
#pragma unroll
    for (int i = 0; i < NB; ++i) rb[s][i] = *reinterpret_cast<const h16x8*>(wgt + brow[i] + koff);
  };
  auto stash = [&](auto set_c, int buf) __attribute__((always_inline)) {
    constexpr int s = decltype(set_c)::value;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int idx = tid + NT * i;
      if ((BNt * 8) % NT == 0 || idx < BNt * 8) *reinterpret_cast<h16x8*>(&s_b[buf * WBUF + (idx >> 3) * LDH + sc]) = rb[s][i];
    }
  };

  fetch(IC<0>{}, 0);
  fetch(IC<1>{}, 1);
  fetch(IC<2>{}, 2);
  // the halo tile: piece i of this thread is pixel (tid + NT * i) / 8 of the halo, 16 bytes of each 64-channel slice
  h16x8 hv[PT][NH];
  {
    const _Float16* __restrict__ src = a.x + (size_t)img * H * W * CIN;
#pragma unroll
    for (int i = 0; i < NH; ++i) {
      const int idx = tid + NT * i;
      const int hp = idx >> 3;
      const int hy = hp / RHW, hx = hp - hy * RHW;
      const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
      const bool in = ((HP * 8) % NT == 0 || idx < HP * 8) && iy >= 0 && iy < H && ix >= 0 && ix < W;
      const _Float16* from = src + ((size_t)iy * W + ix) * CIN + sc;
#pragma unroll
      for (int s = 0; s < PT; ++s) {
        hv[s][i] = zero;
        if (in) hv[s][i] = *reinterpret_cast<const h16x8*>(from + s * BK);
      }
    }
  }
  auto halo_to_lds = [&](auto slice_c) __attribute__((always_inline)) {
    constexpr int s = decltype(slice_c)::value;
#pragma unroll
    for (int i = 0; i < NH; ++i) {
      const int idx = tid + NT * i;
      const int hp = idx >> 3;
      const int hy = hp / RHW, hx = hp - hy * RHW;
      if ((HP * 8) % NT == 0 || idx < HP * 8) *reinterpret_cast<h16x8*>(smem + hy * ROW + hx * PIX + s * (2 * BK) + 2 * sc) = hv[s][i];
    }
  };
  __builtin_amdgcn_sched_barrier(0);
  stash(IC<0>{}, 0);
  fetch(IC<0>{}, 3);
  if constexpr (D == 2) {
    stash(IC<1>{}, 1);
    fetch(IC<1>{}, 4);
  }
  halo_to_lds(IC<0>{});
  __syncthreads();

  f32x16 acc[AF][NF];
  zero_acc(acc);

  // this lane's pixel of fragment 0 at tap (0, 0) and its weight row, its half of a 16-deep step
  const unsigned char* a_lane = smem + (wm * AF * 2 + (r32 >> 4)) * ROW + (r32 & 15) * PIX + 16 * kb;
  const _Float16* b_lane = s_b + (wn * NF * 32 + r32) * LDH + 8 * kb;
  h16x8 av[AF], bv[NF];   // the operands of the next 16-deep step
  auto pixels = [&](int c, int ks) __attribute__((always_inline)) {
    const int tap = c / PT, k0 = (c - tap * PT) * BK;
    const int dy = tap / 3, dx = tap - dy * 3;
    const unsigned char* sa = a_lane + dy * ROW + dx * PIX + 2 * k0 + 32 * ks;
#pragma unroll
    for (int f = 0; f < AF; ++f) av[f] = *reinterpret_cast<const h16x8*>(sa + f * 2 * ROW);
  };
  auto weights = [&](int c, int ks) __attribute__((always_inline)) {
    const _Float16* sb = b_lane + (c % RING) * WBUF + 16 * ks;
#pragma unroll
    for (int n = 0; n < NF; ++n) bv[n] = *reinterpret_cast<const h16x8*>(sb + n * 32 * LDH);
  };
  // chunk c: weights in ring buffer c % RING. Register set (c + D) % 3 holds chunk c + D (requested three chunks earlier), goes
  // to the ring and is requested again for chunk c + D + 3. `ahead`: the first operands of chunk c were read before the
  // barrier (with a ring of two only the pixels: the chunk's weights are written while the chunk before it runs)
  auto step = [&](auto set_c, int c, bool ahead, bool read_ahead) __attribute__((always_inline)) {
    stash(set_c, (c + D) % RING);
    fetch(set_c, c + D + 3);
    if constexpr (PT > 1) {
      if (c == 0) halo_to_lds(IC<1>{});
    }
    if constexpr (PT > 2) {
      if (c == 1) halo_to_lds(IC<2>{});
      if (c == 2) halo_to_lds(IC<3>{});
    }
    __builtin_amdgcn_sched_barrier(0);
    if (!ahead) pixels(c, 0);
    if (!ahead || D == 1) weights(c, 0);
#pragma unroll
    for (int ks = 0; ks < BK / 16; ++ks) {
      h16x8 ca[AF], cb[NF];
#pragma unroll
      for (int f = 0; f < AF; ++f) ca[f] = av[f];
#pragma unroll
      for (int n = 0; n < NF; ++n) cb[n] = bv[n];
      if (ks + 1 < BK / 16) {
        pixels(c, ks + 1);
        weights(c, ks + 1);
      } else if (read_ahead) {
        pixels(min(c + 1, NCH - 1), 0);
        if constexpr (D == 2) weights(min(c + 1, NCH - 1), 0);
      }
#pragma unroll
      for (int f = 0; f < AF; ++f)
#pragma unroll
        for (int n = 0; n < NF; ++n) acc[f][n] = simpb::mfma_32x32x16_f16(ca[f], cb[n], acc[f][n]);
    }
    __syncthreads();
  };
  // in front of the loop: chunk c < PT reads a slice written during chunk c - 1, so nothing of it can be read ahead
  using S0 = IC<D % 3>;
  using S1 = IC<(D + 1) % 3>;
  using S2 = IC<(D + 2) % 3>;
  step(S0{}, 0, false, 1 >= PT);
  step(S1{}, 1, 1 >= PT, 2 >= PT);
  step(S2{}, 2, 2 >= PT, 3 >= PT);
  if constexpr (HEAD == 6) {
    step(S0{}, 3, 3 >= PT, true);
    step(S1{}, 4, true, true);
    step(S2{}, 5, true, true);
  }
  for (int c = HEAD; c < NCH; c += 3) {
    step(S0{}, c, true, true);
    step(S1{}, c + 1, true, true);
    step(S2{}, c + 2, true, true);
  }

  // epilogue as in conv_staged_tile, the wave's fp32 tile over the halo (nobody reads it after the last barrier); tile row r
  // is output pixel (2 * fragment + r / 16, r % 16) of the 2-D tile
  float* mine = s_c + wave * 32 * LDW;
  const int cw = c0 + wn * NF * 32;
#pragma unroll
  for (int f = 0; f < AF; ++f) {
    if (f) __syncthreads();
    acc_to_tile<NF, LDW>(mine, acc[f], r32, kb);
    __syncthreads();
    tile_pieces<NF, LDW>(mine, 0, lane, [&](int, int r, int c8, const float (&v)[8]) __attribute__((always_inline)) {
      const int oy = y0 + (wm * AF + f) * 2 + (r >> 4), ox = x0 + (r & 15);
      const int p = oy < H && ox < W ? (img * H + oy) * W + ox : a.P_out;   // a clipped tile: nothing to write
      emit_piece<TOK16>(a, cw, p, c8, v);
    });
  }
}

// the live forms' walk over the resident 2-D tiles: as live_flat_walk
__device__ __forceinline__ void live_resident_walk(ConvArgs& a, int L) {
  a.gx = L * a.tiles_w * a.tiles_h;
  a.per_xcd = (a.gx * a.gy + 7) >> 3;
}

template <int CIN, int TH, int BNt, int WGM, int WGN, int RING, bool TOK16>
__global__ __launch_bounds__(64 * WGM * WGN) void conv_resident_kernel(const ConvArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char resident_smem[];
  // simpb::xcd_tile, written out: through the function the Cin 64 form of variant 12 takes 66 registers for 64 and loses a
  // wave per SIMD (profiles/conv_shared_parts.md, "What went back")
  const int tile = (blockIdx.x & 7) * a.per_xcd + (blockIdx.x >> 3);
  if ((int)(blockIdx.x >> 3) >= a.per_xcd || tile >= a.gx * a.gy) return;
  conv_resident_tile<CIN, TH, BNt, WGM, WGN, RING, TOK16>(a, tile, resident_smem);
}

template <int CIN, int TH, int BNt, int WGM, int WGN, int RING, bool TOK16>
__global__ __launch_bounds__(64 * WGM * WGN) void conv_resident_live_kernel(const ConvArgs full, const LiveTable lt) {
  extern __shared__ __attribute__((aligned(16))) unsigned char resident_smem[];
  ConvArgs a = full;
  live_resident_walk(a, live_count(lt));
  const int tile = simpb::xcd_tile(a.per_xcd, a.gx * a.gy);
  if (tile < 0) return;
  conv_resident_tile<CIN, TH, BNt, WGM, WGN, RING, TOK16, true>(a, tile, resident_smem, lt);
}

template <int CIN, int TH, int BNt, int WGM, int WGN, int RING, bool TOK16>
__global__ __launch_bounds__(64 * WGM * WGN) void conv_resident_group_kernel(const ConvGroup g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char resident_smem[];
  const int gt = simpb::xcd_tile(g.per_xcd, g.start[g.n]);
  if (gt < 0) return;
  const int j = group_problem(g, gt);
  conv_resident_tile<CIN, TH, BNt, WGM, WGN, RING, TOK16>(g.a[j], gt - g.start[j], resident_smem);
}

template <int CIN, int TH, int BNt, int WGM, int WGN, int RING, bool TOK16>
__global__ __launch_bounds__(64 * WGM * WGN) void conv_resident_group_live_kernel(const ConvGroup g, const LiveTable lt) {
  extern __shared__ __attribute__((aligned(16))) unsigned char resident_smem[];
  const int L = live_count(lt);
  ConvArgs a;
  const int tile = live_group_tile(g, a, [&](ConvArgs& b) { live_resident_walk(b, L); });
  if (tile < 0) return;
  conv_resident_tile<CIN, TH, BNt, WGM, WGN, RING, TOK16, true>(a, tile, resident_smem, lt);
}

// ---- host: the forms, each stated once ------------------------------------------------------------------------------------------
// A form knows its tile count on a shape (what the choose_* rules ask), its grid (what the kernel walks), its threads and its
// kernels; the entry points below take all of them from V1 .. V13 / P0 .. P2 and restate none. A launch with a live-image
// table (lt.live set) runs the form's live kernel on the SAME grid: the full batch's, of which the kernel uses what L needs.
inline long long ceil_div(long long a, int b) { return (a + b - 1) / b; }

// workgroups of the XCD walk over the gx x gy tiles of `a`
inline unsigned xcd_blocks(ConvArgs& a) {
  a.per_xcd = (int)(((long long)a.gx * a.gy + 7) / 8);
  return (unsigned)(a.per_xcd * 8);
}

// a tile of BMt consecutive output pixels x BNt output channels (the direct and the staged forms)
template <int BMt, int BNt>
struct FlatTile {
  static long long tiles(long long p_out, int cout) { return ceil_div(p_out, BMt) * ceil_div(cout, BNt); }
  static void grid(ConvArgs& a) {
    a.gx = (int)ceil_div(a.P_out, BMt);
    a.gy = (int)ceil_div(a.Cout, BNt);
  }
};

template <int AF, bool KSPLIT>
struct Direct : FlatTile<(KSPLIT ? 32 : 128) * AF, BN> {
  template <int TAPS, bool TOK16>
  static void launch(ConvArgs& a, const LiveTable& lt, hipStream_t stream) {
    static_assert(TAPS == 9, "the direct forms are 3x3 only");
    Direct::grid(a);
    if (!lt.live) hipLaunchKernelGGL((conv3x3_f16_kernel<AF, KSPLIT, TOK16>), dim3(xcd_blocks(a)), dim3(kThreads), 0, stream, a);
    else hipLaunchKernelGGL((conv3x3_f16_kernel<AF, KSPLIT, TOK16, LiveTable>), dim3(xcd_blocks(a)), dim3(kThreads), 0, stream, a, lt);
  }
};

// KS = 0: conv_staged_kernel (the pipeline's own k map); KS >= 1: conv_staged_ksplit_kernel with KS groups of waves
template <int BMt, int BNt, int WGM, int WGN, int KS = 0>
struct Staged : FlatTile<BMt, BNt> {
  static constexpr int threads = 64 * WGM * WGN * (KS ? KS : 1);
  template <int TAPS, bool TOK16>
  static void launch(ConvArgs& a, const LiveTable& lt, hipStream_t stream) {
    Staged::grid(a);
    const dim3 blocks(xcd_blocks(a));
    if constexpr (KS == 0) {
      if (!lt.live) hipLaunchKernelGGL((conv_staged_kernel<BMt, BNt, WGM, WGN, TAPS, TOK16>), blocks, dim3(threads), 0, stream, a);
      else hipLaunchKernelGGL((conv_staged_live_kernel<BMt, BNt, WGM, WGN, TAPS, TOK16>), blocks, dim3(threads), 0, stream, a, lt);
    } else {
      if (!lt.live) hipLaunchKernelGGL((conv_staged_ksplit_kernel<BMt, BNt, WGM, WGN, TAPS, TOK16, KS>), blocks, dim3(threads), 0, stream, a);
      else hipLaunchKernelGGL((conv_staged_ksplit_live_kernel<BMt, BNt, WGM, WGN, TAPS, TOK16, KS>), blocks, dim3(threads), 0, stream, a, lt);
    }
  }
  template <bool TOK16>
  static void launch_group(const ConvGroup& g, const LiveTable& lt, hipStream_t stream) {
    const dim3 blocks((unsigned)(g.per_xcd * 8));
    if (!lt.live) hipLaunchKernelGGL((conv_staged_group_kernel<BMt, BNt, WGM, WGN, 9, TOK16>), blocks, dim3(threads), 0, stream, g);
    else hipLaunchKernelGGL((conv_staged_group_live_kernel<BMt, BNt, WGM, WGN, 9, TOK16>), blocks, dim3(threads), 0, stream, g, lt);
  }
};

inline bool resident_shape(int cin, int stride) { return stride == 1 && (cin == 64 || cin == 128 || cin == 256); }

// a kernel is allowed its dynamic LDS (more than 64 KB where Cin = 256) once
template <auto kernel, class... Args>
void launch_with_lds(size_t lds, unsigned blocks, int threads, hipStream_t stream, const Args&... args) {
  static const bool allowed =
      hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
  (void)allowed;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), lds, stream, args...);
}

// whole 2-D tiles of TH x RTW output pixels per image x BNt output channels, channel blocks of one tile next to each other
template <int TH, int BNt, int WGM, int WGN, int RING>
struct Resident {
  static constexpr int threads = 64 * WGM * WGN;
  static long long tiles(long long images, int ho, int wo, int cout) {
    return images * ceil_div(ho, TH) * ceil_div(wo, RTW) * ceil_div(cout, BNt);
  }
  static void grid(ConvArgs& a) {
    a.tiles_w = (int)ceil_div(a.Wo, RTW);
    a.tiles_h = (int)ceil_div(a.Ho, TH);
    a.gx = a.P_out / (a.Ho * a.Wo) * a.tiles_w * a.tiles_h;
    a.gy = (int)ceil_div(a.Cout, BNt);
  }
  // Cin is a template argument of the kernels (64, 128 or 256: resident_shape): the one place that makes it one, for the
  // launch of one problem (Arg = ConvArgs) and of a group (Arg = ConvGroup)
  template <bool TOK16, class Arg>
  static void launch_cin(int cin, unsigned blocks, const Arg& arg, const LiveTable& lt, hipStream_t stream) {
    auto go = [&](auto cin_c) {
      constexpr int CIN = decltype(cin_c)::value;
      constexpr size_t lds = resident_lds<CIN, TH, BNt, WGM, WGN, RING>();
      if constexpr (std::is_same_v<Arg, ConvGroup>) {
        if (!lt.live) launch_with_lds<conv_resident_group_kernel<CIN, TH, BNt, WGM, WGN, RING, TOK16>>(lds, blocks, threads, stream, arg);
        else launch_with_lds<conv_resident_group_live_kernel<CIN, TH, BNt, WGM, WGN, RING, TOK16>>(lds, blocks, threads, stream, arg, lt);
      } else {
        if (!lt.live) launch_with_lds<conv_resident_kernel<CIN, TH, BNt, WGM, WGN, RING, TOK16>>(lds, blocks, threads, stream, arg);
        else launch_with_lds<conv_resident_live_kernel<CIN, TH, BNt, WGM, WGN, RING, TOK16>>(lds, blocks, threads, stream, arg, lt);
      }
    };
    if (cin == 64) go(IC<64>{});
    else if (cin == 128) go(IC<128>{});
    else go(IC<256>{});
  }
  template <int TAPS, bool TOK16>
  static void launch(ConvArgs& a, const LiveTable& lt, hipStream_t stream) {
    static_assert(TAPS == 9, "the resident form is 3x3 only");
    grid(a);
    launch_cin<TOK16>(a.Cin, xcd_blocks(a), a, lt, stream);
  }
  template <bool TOK16>
  static void launch_group(const ConvGroup& g, const LiveTable& lt, hipStream_t stream) {
    launch_cin<TOK16>(g.a[0].Cin, (unsigned)(g.per_xcd * 8), g, lt, stream);
  }
};

// THE statement of every form's shape: 3x3 variants 1-13 (the table at the head of the file) ...
using V1 = Direct<1, false>;                 // 128 pixels x 64 channels, weights through LDS
using V2 = Direct<2, false>;                 // 256 x 64
using V3 = Direct<1, true>;                  // 32 x 64, K split over the waves
using V4 = Direct<2, true>;                  // 64 x 64, K split over the waves
using V5 = Staged<128, 64, 4, 1>;            // 128 x 64, operands staged through LDS
using V6 = Staged<128, 128, 2, 2>;           // 128 x 128
using V7 = Staged<96, 64, 3, 1>;             // 96 x 64, three waves: 704 workgroups for 67 584 pixels
using V8 = Staged<96, 128, 1, 4>;            // 96 x 128, waves side by side along the channels
using V9 = Staged<64, 64, 2, 2, 1>;          // 64 x 64, four waves of 32 x 32: the sums of 1
using V10 = Staged<64, 64, 2, 2, 2>;         // 64 x 64, K split over 2 groups of four waves
using V11 = Staged<64, 64, 2, 2, 4>;         // 64 x 64, K split over 4 groups (16 waves): the sums of 3 / 4
using V12 = Resident<4, 64, 2, 2, 2>;        // resident 4 x 16 pixels x 64 channels, four waves of 32 x 32, weight ring of two
using V13 = Resident<8, 128, 4, 2, 3>;       // resident 8 x 16 x 128, eight waves of 32 x 64, weight ring of three
// ... and the tilings of a 1x1 convolution through the staged pipeline (conv1x1 variants 2-4)
using P0 = V5;                               // 128 x 64
using P1 = V6;                               // 128 x 128
using P2 = Staged<64, 64, 2, 2>;             // 64 x 64 (four waves, 32 x 32 each): the sums of P0 bit for bit

// 3x3 variant v is kVariant[v - 1] (TOK16: the kernels that write the f16 token rows alone)
using Launch = void (*)(ConvArgs&, const LiveTable&, hipStream_t);
template <bool TOK16>
constexpr Launch kVariant[13] = {V1::launch<9, TOK16>,  V2::launch<9, TOK16>,  V3::launch<9, TOK16>, V4::launch<9, TOK16>, V5::launch<9, TOK16>,
                                 V6::launch<9, TOK16>,  V7::launch<9, TOK16>,  V8::launch<9, TOK16>, V9::launch<9, TOK16>, V10::launch<9, TOK16>,
                                 V11::launch<9, TOK16>, V12::launch<9, TOK16>, V13::launch<9, TOK16>};

// The arguments every entry point fills the same way; where the output goes (y / tok / tok16, tokens_per_cam, level_start)
// and the residual are set by name where they exist. The grid is the form's to fill.
ConvArgs conv_args(const void* x, const void* weight, const void* bias, long long p_out, int in_channels, int out_channels, int relu,
                   int stride, int ho, int wo, int in_h, int in_w) {
  ConvArgs a = {};
  a.x = static_cast<const _Float16*>(x);
  a.w = static_cast<const _Float16*>(weight);
  a.bias = static_cast<const _Float16*>(bias);
  a.P_out = (int)p_out;
  a.Cin = in_channels;
  a.Cout = out_channels;
  a.relu = relu;
  a.stride = stride;
  a.Ho = ho;
  a.Wo = wo;
  a.H = in_h;
  a.W = in_w;
  return a;
}

}  // namespace

// The tiling simpb_conv3x3_nhwc_f16 runs for variant 0 on p_out output pixels (no launch: tests restate the rule against it).
extern "C" int simpb_conv3x3_choose_variant(long long p_out, int in_channels, int out_channels) {
  // measured on the ResNet50 / FPN shapes at 6 x 256 x 704 (tools/bench_conv3x3.py): the LDS-staged 96-row tilings while
  // they fill the chip (96 divides the pixel counts of a 6-camera rig and leaves no nearly empty last round of
  // workgroups), then the direct ones, K split inside the workgroup for the smallest maps
  if (out_channels >= 128 && V6::tiles(p_out, out_channels) >= 2048) return 6;   // many rounds: the larger tile wins
  if (out_channels >= 128 && V8::tiles(p_out, out_channels) >= 160) return 8;
  if (V7::tiles(p_out, out_channels) >= 256) return 7;
  // Cin >= 256 on the small maps (tools/bench_conv_small_maps.py, profiles/conv3x3_small_maps.md): the direct forms are
  // bound by their 16-byte loads of 32 different rows per wave-instruction, not by latency (8 or 16 waves on the same loads
  // were no faster); the staged 64 x 64 tile wins, with K split over 16 waves where 64 x 64 tiles leave half the chip empty.
  // 9 gives the bits of 1 and 11 the bits of 4 (DIRECTK above), so neither choice changes an output
  if (V1::tiles(p_out, out_channels) >= 128) return in_channels >= 256 && out_channels >= 256 ? 9 : 1;
  if (V4::tiles(p_out, out_channels) >= 128) return in_channels >= 512 && out_channels >= 512 ? 11 : 4;
  return 3;
}

// Whether variant 0 runs the resident form on a shape where simpb_conv3x3_choose_variant answered 7 or 8: the resident
// variant's number, or 0 for "keep the staged form". Yes only in the region where it measured faster on the device
// (profiles/conv3x3_large_maps.md: 64 -> 64 and 256 -> 256 on 6 x 64 x 176, 128 -> 128 and 256 -> 256 on 6 x 32 x 88, the
// highest of five rounds below the staged form's lowest): Cin = Cout of 64, 128 or 256, stride 1, and no fewer tiles than
// the smallest measured launch had of its kind. It gives the same bits, so the answer changes no output.
extern "C" int simpb_conv3x3_choose_resident(long long p_out, int in_h, int in_w, int in_channels, int out_channels, int stride) {
  if (p_out <= 0 || in_h <= 0 || in_w <= 0 || p_out % ((long long)in_h * in_w) != 0 || !resident_shape(in_channels, stride) ||
      out_channels != in_channels)
    return 0;
  const int staged = simpb_conv3x3_choose_variant(p_out, in_channels, out_channels);
  if (staged != 7 && staged != 8) return 0;
  const long long images = p_out / ((long long)in_h * in_w);
  if (in_channels == 256 && V13::tiles(images, in_h, in_w, out_channels) >= 1024) return 13;   // four rounds of one eight-wave workgroup per CU
  if (V12::tiles(images, in_h, in_w, out_channels) >= 512) return 12;
  return 0;
}

// The same question for the whole group launch of simpb_conv3x3_group_tokens_f16: 13 = every level in the resident
// 8 x 16 x 128 form (measured on the FPN's four levels at 6 x 64 x 176: faster than the staged launch, than any split into
// two launches and than the 4 x 16 x 64 form), 0 = the staged launch.
extern "C" int simpb_conv3x3_group_choose_resident(int num_levels, int num_images, const int* in_h, const int* in_w, int in_channels,
                                                   int out_channels) {
  if (num_levels < 1 || num_levels > kMaxConvGroup || num_images <= 0 || !in_h || !in_w || in_channels != 256 || out_channels != 256) return 0;
  long long tiles = 0;
  for (int j = 0; j < num_levels; ++j) {
    if (in_h[j] <= 0 || in_w[j] <= 0) return 0;
    tiles += V13::tiles(num_images, in_h[j], in_w[j], out_channels);
  }
  return tiles >= 1024 ? 13 : 0;
}

// live: NULL (today's launch, the same kernels as ever) or the live-image table of conv_parts.h
extern "C" int simpb_conv3x3_nhwc_f16_live(void* y, float* tokens, void* tokens_f16, int tokens_per_cam, int level_start,
                                           const void* x, const void* weight, const void* bias, int num_images, int in_h, int in_w,
                                           int in_channels, int out_channels, int stride, int relu, int variant, void* stream,
                                           const int* live) {
  const bool to_tokens = tokens || tokens_f16;   // tokens == NULL with tokens_f16 set: the f16 rows alone
  if ((!y && !to_tokens) || (y && to_tokens) || (reinterpret_cast<size_t>(tokens_f16) & 15) || !x || !weight || !bias || num_images <= 0 || in_h <= 0 || in_w <= 0 ||
      in_channels <= 0 || out_channels <= 0 || (stride != 1 && stride != 2) || in_channels % BK != 0 || out_channels % 8 != 0 ||
      variant < 0 || variant > 13)
    return SIMPB_EINVAL;
  if (variant >= 12 && !resident_shape(in_channels, stride)) return SIMPB_EINVAL;   // the resident form: stride 1, Cin 64 / 128 / 256
  if ((reinterpret_cast<size_t>(y) | reinterpret_cast<size_t>(tokens) | reinterpret_cast<size_t>(x) |
       reinterpret_cast<size_t>(weight) | reinterpret_cast<size_t>(bias)) & 15)
    return SIMPB_EINVAL;
  const int ho = (in_h - 1) / stride + 1, wo = (in_w - 1) / stride + 1;   // padding 1, kernel 3
  const long long p_out = (long long)num_images * ho * wo;
  const long long in_elems = (long long)num_images * in_h * in_w * in_channels;
  if (p_out > (1ll << 30) || in_elems > (1ll << 31) - 1) return SIMPB_EINVAL;   // tap offsets are 32-bit
  if (to_tokens && (tokens_per_cam < ho * wo || level_start < 0 || level_start + ho * wo > tokens_per_cam)) return SIMPB_EINVAL;
  (void)hipGetLastError();
  ConvArgs a = conv_args(x, weight, bias, p_out, in_channels, out_channels, relu, stride, ho, wo, in_h, in_w);
  a.y = static_cast<_Float16*>(y);
  a.tok = tokens;
  a.tok16 = static_cast<_Float16*>(tokens_f16);
  a.tokens_per_cam = tokens_per_cam;
  a.level_start = level_start;
  if (variant == 0) {
    variant = simpb_conv3x3_choose_variant(p_out, in_channels, out_channels);
    if (variant == 7 || variant == 8) {   // the same bits either way: the resident form where it measured faster
      const int resident = simpb_conv3x3_choose_resident(p_out, in_h, in_w, in_channels, out_channels, stride);
      if (resident) variant = resident;
    }
  }
  const bool tok16_alone = !tokens && tokens_f16;   // the f16 token rows alone: kernels without the fp32 stores
  (tok16_alone ? kVariant<true> : kVariant<false>)[variant - 1](a, LiveTable{live, num_images}, static_cast<hipStream_t>(stream));
  return simpb_check_launch();
}

extern "C" int simpb_conv3x3_nhwc_f16(void* y, float* tokens, void* tokens_f16, int tokens_per_cam, int level_start,
                                      const void* x, const void* weight, const void* bias, int num_images, int in_h, int in_w,
                                      int in_channels, int out_channels, int stride, int relu, int variant, void* stream) {
  return simpb_conv3x3_nhwc_f16_live(y, tokens, tokens_f16, tokens_per_cam, level_start, x, weight, bias, num_images, in_h, in_w,
                                     in_channels, out_channels, stride, relu, variant, stream, nullptr);
}

// The FPN's output convolutions (3x3, stride 1, Cin -> Cout, bias, no ReLU; mmdet FPN `fpn_convs[i].conv` after
// tools/fuse_conv_bn.py:10-48) of up to four levels in ONE launch, each writing its level's token rows (f32 and, optionally,
// f16; or, with tokens == NULL, f16 alone) as simpb_conv3x3_nhwc_f16 does with `tokens`: x[j] f16 NHWC [num_images, in_h[j], in_w[j], Cin], weight[j] f16
// [Cout, 3, 3, Cin], bias[j] f16 [Cout], level_start[j] the level's first row inside a camera's tokens_per_cam rows.
// live: NULL or the live-image table, as simpb_conv3x3_nhwc_f16_live; the forms are still chosen on the full batch.
extern "C" int simpb_conv3x3_group_tokens_forms_f16_live(int num_levels, float* tokens, void* tokens_f16, int tokens_per_cam,
                                                         const int* level_start, const void* const* x, const void* const* weight,
                                                         const void* const* bias, int num_images, const int* in_h, const int* in_w,
                                                         int in_channels, int out_channels, int relu, const int* variant,
                                                         void* stream, const int* live) {
  if (num_levels < 1 || num_levels > kMaxConvGroup || (!tokens && !tokens_f16) || !level_start || !x || !weight || !bias || !in_h || !in_w ||
      num_images <= 0 || in_channels <= 0 || out_channels <= 0 || in_channels % BK != 0 || out_channels % 8 != 0 ||
      ((reinterpret_cast<size_t>(tokens) | reinterpret_cast<size_t>(tokens_f16)) & 15))
    return SIMPB_EINVAL;
  // the levels of one form share a launch: form[0] the staged tiles of variant 8, form[1] the resident tiles of variant 13
  ConvGroup form[2] = {};
  long long total[2] = {0, 0};
  const int rule = variant ? 0 : simpb_conv3x3_group_choose_resident(num_levels, num_images, in_h, in_w, in_channels, out_channels);
  for (int j = 0; j < num_levels; ++j) {
    if (!x[j] || !weight[j] || !bias[j] || in_h[j] <= 0 || in_w[j] <= 0 ||
        ((reinterpret_cast<size_t>(x[j]) | reinterpret_cast<size_t>(weight[j]) | reinterpret_cast<size_t>(bias[j])) & 15))
      return SIMPB_EINVAL;
    const long long p_out = (long long)num_images * in_h[j] * in_w[j];
    if (p_out > (1ll << 30) || p_out * in_channels > (1ll << 31) - 1) return SIMPB_EINVAL;   // tap offsets are 32-bit
    if (tokens_per_cam < in_h[j] * in_w[j] || level_start[j] < 0 || level_start[j] + in_h[j] * in_w[j] > tokens_per_cam)
      return SIMPB_EINVAL;
    const int v = variant ? variant[j] : rule ? rule : 8;
    if (v != 8 && v != 13) return SIMPB_EINVAL;
    if (v == 13 && !resident_shape(in_channels, 1)) return SIMPB_EINVAL;
    const int f = v == 13;
    ConvGroup& g = form[f];
    ConvArgs& a = g.a[g.n];
    a = conv_args(x[j], weight[j], bias[j], p_out, in_channels, out_channels, relu, 1, in_h[j], in_w[j], in_h[j], in_w[j]);
    a.tok = tokens;
    a.tok16 = static_cast<_Float16*>(tokens_f16);
    a.tokens_per_cam = tokens_per_cam;
    a.level_start = level_start[j];
    if (f == 1) V13::grid(a);
    else V8::grid(a);
    g.start[g.n++] = (int)total[f];
    total[f] += (long long)a.gx * a.gy;
  }
  for (int f = 0; f < 2; ++f) {
    if (total[f] > (1 << 24)) return SIMPB_EINVAL;
    for (int j = form[f].n; j <= kMaxConvGroup; ++j) form[f].start[j] = (int)total[f];
    form[f].per_xcd = (int)((total[f] + 7) / 8);
  }
  (void)hipGetLastError();
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the large levels first: the staged launch is the short one; tokens == NULL: the f16 token rows alone
  const LiveTable lt{live, num_images};
  if (form[1].n) (tokens ? V13::launch_group<false> : V13::launch_group<true>)(form[1], lt, s);
  if (form[0].n) (tokens ? V8::launch_group<false> : V8::launch_group<true>)(form[0], lt, s);
  return simpb_check_launch();
}

extern "C" int simpb_conv3x3_group_tokens_forms_f16(int num_levels, float* tokens, void* tokens_f16, int tokens_per_cam,
                                                    const int* level_start, const void* const* x, const void* const* weight,
                                                    const void* const* bias, int num_images, const int* in_h, const int* in_w,
                                                    int in_channels, int out_channels, int relu, const int* variant, void* stream) {
  return simpb_conv3x3_group_tokens_forms_f16_live(num_levels, tokens, tokens_f16, tokens_per_cam, level_start, x, weight, bias,
                                                   num_images, in_h, in_w, in_channels, out_channels, relu, variant, stream, nullptr);
}

// variant 0 for every level: what the detector runs
extern "C" int simpb_conv3x3_group_tokens_f16(int num_levels, float* tokens, void* tokens_f16, int tokens_per_cam,
                                              const int* level_start, const void* const* x, const void* const* weight,
                                              const void* const* bias, int num_images, const int* in_h, const int* in_w,
                                              int in_channels, int out_channels, int relu, void* stream) {
  return simpb_conv3x3_group_tokens_forms_f16(num_levels, tokens, tokens_f16, tokens_per_cam, level_start, x, weight, bias, num_images,
                                              in_h, in_w, in_channels, out_channels, relu, nullptr, stream);
}

// 1x1 convolutions through the same staged pipeline (TAPS = 1): csrc/conv1x1.hip validates and forwards here; `tiling` picks
// P0 .. P2 above.
extern "C" int simpb_conv_pointwise_staged(void* y, const void* x, const void* weight, const void* bias, const void* residual,
                                           int p_out, int in_h, int in_w, int ho, int wo, int in_channels, int out_channels,
                                           int stride, int relu, int residual_upsample2x, int tiling, void* stream,
                                           const int* live) {
  ConvArgs a = conv_args(x, weight, bias, p_out, in_channels, out_channels, relu, stride, ho, wo, in_h, in_w);
  a.y = static_cast<_Float16*>(y);
  a.residual = static_cast<const _Float16*>(residual);
  a.res_up = residual_upsample2x ? 1 : 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const LiveTable lt{live, p_out / (ho * wo)};
  if (tiling == 0) P0::launch<1, false>(a, lt, s);
  else if (tiling == 1) P1::launch<1, false>(a, lt, s);
  else P2::launch<1, false>(a, lt, s);
  return simpb_check_launch();
}
