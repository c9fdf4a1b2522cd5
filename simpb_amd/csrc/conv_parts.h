// Parts that csrc/conv3x3.hip and csrc/conv1x1.hip share, each written once: vector types and staging constants, the split
// of an output pixel index, the nearest-2x residual row, the epilogue element, and the walk of a wave's accumulators through
// its fp32 LDS tile into 16-byte pieces of output rows. What was measured about sharing them: profiles/conv_shared_parts.md.
#pragma once
#include <type_traits>
#include "mfma_f16.h"

namespace simpb {
namespace conv {

using f32x16 = f32x16_t;
using h16x8 = h16x8_t;
template <int S>
using IC = std::integral_constant<int, S>;

constexpr int BN = 64, BK = 64;   // output channels of the narrow tiles; input channels of one K chunk
constexpr int LDH = BK + 8;       // halfs per staged chunk row (144 B): conflict-free 16-lane groups for ds_read_b128
constexpr int LDC = BN + 1;       // floats per row of a 64-channel epilogue tile
constexpr int kThreads = 256;

// output pixel p of [N, Ho, Wo]
struct Pixel {
  int n, ho, wo;
};
__device__ __forceinline__ Pixel split_pixel(int p, int Ho, int Wo) {
  const int hw = Ho * Wo;
  const int n = p / hw, rem = p - n * hw;
  const int ho = rem / Wo;
  return {n, ho, rem - ho * Wo};
}

// the row of output pixel p in a residual map of HALF the size, read with nearest-neighbour 2x upsampling
// (F.interpolate(mode="nearest") of an exact 2x: source = floor(dst / 2)): the FPN top-down path
__device__ __forceinline__ int up2_row(int p, int Ho, int Wo) {
  const Pixel q = split_pixel(p, Ho, Wo);
  return (q.n * (Ho >> 1) + (q.ho >> 1)) * (Wo >> 1) + (q.wo >> 1);
}

// ---- the live-image table (the *_live entry points of include/simpb_hip.h) ------------------------------------------------------
// live: i32 [1 + images] on the device. live[0] = L, the number of live images; live[1 .. L] their indices, ascending; what
// lies behind is not read. A live form walks VIRTUAL pixels: its launch covers L * Ho * Wo of them (the resident forms
// L * tiles_h * tiles_w 2-D tiles, the stem L grid planes), tiled and dealt over the XCDs exactly as the full batch is, with
// the tile count and per_xcd recomputed from L in the kernel -- the host sizes the grid for the full batch and the workgroups
// past the live total, the high blockIdx.x >> 3 of every XCD, return before their first load. Virtual image v is real image
// live[1 + v] wherever an address is formed -- x, residual (the nearest-2x read included), y, the token row -- and nowhere
// else: which tile holds a pixel changes nothing of its sum, so a live image's rows are the full batch's bit for bit, and
// nothing of a dead image is read or written. L and every index are clamped: a wrong table gives wrong pixels, never an
// access outside the arrays.
struct LiveTable {
  const int* live;
  int images;
};
__device__ __forceinline__ int live_count(const LiveTable& t) { return min(max(t.live[0], 0), t.images); }
__device__ __forceinline__ int live_image(const LiveTable& t, int v) {
  return min(max(t.live[1 + min(max(v, 0), t.images - 1)], 0), t.images - 1);
}
// what a kernel with an optional trailing LiveTable (a parameter pack of none or one) was given
__device__ __forceinline__ LiveTable table_of() { return {nullptr, 0}; }
__device__ __forceinline__ LiveTable table_of(const LiveTable& t) { return t; }
// virtual output pixel p of a map of hw pixels per image -> the real one
__device__ __forceinline__ int live_pixel(const LiveTable& t, int p, int hw) {
  const int v = p / hw;
  return live_image(t, v) * hw + (p - v * hw);
}
// A flat tile of BMt virtual pixels from p0 on (BMt <= the workgroup's threads): rows[i] = the real pixel of row i, or `none`
// where the row lies past the `walked` live pixels. Filled at the head of a kernel, read in its epilogue behind a barrier:
// the table is read from memory in front of the kernel's first store only, so no store is ever in flight beside these loads.
template <int BMt>
__device__ __forceinline__ void live_tile_rows(int* rows, const LiveTable& t, int p0, int walked, int hw, int none) {
  const int i = threadIdx.x;
  if (i < BMt) rows[i] = p0 + i < walked ? live_pixel(t, p0 + i, hw) : none;
}

// The epilogue element, eight channels of one output pixel: sum + bias + residual in fp32, ReLU, ONE rounding to fp16.
// A launch without a residual passes zeros: a sum of accumulators that start at +0 is never -0, nor is that sum plus the
// bias, so the added 0.f changes no bit.
__device__ __forceinline__ h16x8 finish_piece(const float (&v)[8], const h16x8& bias, const h16x8& residual, int relu) {
  h16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float t = v[e] + (float)bias[e] + (float)residual[e];
    o[e] = (_Float16)(relu ? fmaxf(t, 0.f) : t);
  }
  return o;
}

template <int NF>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[NF]) {
#pragma unroll
  for (int n = 0; n < NF; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
}
template <int AF, int NF>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[AF][NF]) {
#pragma unroll
  for (int f = 0; f < AF; ++f) zero_acc(acc[f]);
}

// Epilogue of a wave, first half: its NF 32 x 32 accumulators (one A fragment) go to its own fp32 LDS tile of 32 rows at a
// pitch of LDW floats (C/D layout: column = lane & 31, row = acc_row(register, lane >> 5)). The barriers around it are the
// caller's: they depend on what else lives in that memory.
template <int NF, int LDW>
__device__ __forceinline__ void acc_to_tile(float* mine, const f32x16 (&acc)[NF], int r32, int kb) {
#pragma unroll
  for (int n = 0; n < NF; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) mine[acc_row(r, kb) * LDW + n * 32 + r32] = acc[n][r];
}

// Second half: the tile comes back as 16-byte pieces of its rows, 4 * NF to a row; the lane takes pieces lane, lane + 64, ...
// and hands each to emit(pass, row, first channel, the eight sums). PARTS > 1 (a K split over groups of waves): the groups'
// tiles lie `part` floats apart and are added in ascending order, a fixed one.
template <int NF, int LDW, int PARTS = 1, class Emit>
__device__ __forceinline__ void tile_pieces(const float* mine, int part, int lane, Emit&& emit) {
  constexpr int PR = 4 * NF;   // pieces per row
#pragma unroll
  for (int pass = 0; pass < 32 * PR / 64; ++pass) {
    const int idx = lane + 64 * pass;
    const int r = idx / PR, c8 = (idx % PR) * 8;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = mine[r * LDW + c8 + e];
#pragma unroll
    for (int g = 1; g < PARTS; ++g)
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] += mine[g * part + r * LDW + c8 + e];
    emit(pass, r, c8, v);
  }
}

}  // namespace conv
}  // namespace simpb
