// Camera frame ingest (gfx950): raw u8 frames as a decoder, a camera or a loader delivers them -> the stem's operand, f16
// [N, h, w, 4] with channel 3 = 0 (what simpb_stem_conv7x7_pool_f16 reads). It replaces the reference's test pipeline on
// the host, ResizeCropFlipImage (datasets/pipelines/augment.py:86-106: PIL resize + crop + left-right flip + rotate) and
// NormalizeMultiviewImage (transform_3d.py:438-466), and the fp32 cast pass of csrc/stem.hip behind it.
//
// The resize is Pillow's 8-bit resampler restated: integer coefficients with 22 fractional bits (computed by the host in
// float64, simpb_amd/preprocess.py), a horizontal pass whose results are rounded and clamped to u8, then a vertical pass
// over those u8 values with the same rule. All arithmetic is int32, so the result is Pillow's byte for byte. Crop and flip
// are index arithmetic: only the kept columns and the source rows the kept output rows need are ever computed. Channel
// order, mean / std and the f16 rounding sit in a [3][256] table made by the host, so that no floating-point
// instruction (and no contraction rule of the compiler) enters the result.
//
// THE TWO PASSES. Every ingest is two launches with a u8 intermediate `mid` [N, rows, pitch] in HBM (1.2 MB per camera at
// 1600 x 900 -> 704 x 256):
//   1. horizontal: one workgroup per (needed source row, image). The row is staged in LDS as (B, G, R) bytes (stage_row,
//      stage_bgr_row; neighbouring output columns share almost all of their taps), a thread makes whole output pixels, the
//      resampled row goes through LDS again and leaves as 16-byte chunks (filter_row_and_store).
//   2. vertical + table: a thread owns 4 neighbouring output pixels, sums their taps into 12 accumulators and writes them
//      through the table as two 16-byte stores (stage_lut, store_lut_group).
// THE SOURCE FORMATS differ in how a row becomes the (B, G, R) row and in nothing else: stage_bgr_row<F> takes interleaved
// BGR as it lies, RGB / BGRA / RGBA as a byte permutation, and 4:2:0 semi-planar (NV12 / NV21, P010 in u16), planar 4:2:0
// and packed 4:2:2 (YUYV / UYVY) through one integer YCbCr rule per pixel (yuv_to_bgr) with replicated chroma, and planar
// 4:4:4 with the chroma it has. with_format maps the runtime code to the instantiation, for the host's launch and inside the
// rig kernel alike.
// JPEG-DECODER PLANES. A format code | SIMPB_SURFACE_CHROMA_JPEG (the five 8-bit formats with subsampled chroma) is a format of
// its own whose chroma is interpolated as libjpeg's decoder does it at its defaults ("fancy" upsampling: fancy_pair states
// h2v2 for 4:2:0 and h2v1 for 4:2:2 in int32); a 4:2:0 workgroup stages one more chroma row for it, the far one. With
// libjpeg's colour constants (the caller's: colour "jpeg" of simpb_amd/preprocess.py) and the native planes of a JPEG the
// (B, G, R) row is the one libjpeg decodes from that file. Pinned to libjpeg-turbo through Pillow: 4:2:0, 4:4:4 and the
// constants (tests/test_chroma_host.py); stated from libjpeg's published algorithm only: 4:2:2.
// THREE WAYS TO ADDRESS THE IMAGES. A tight contiguous batch of BGR or NV12 / NV21 frames (simpb_preprocess_u8_nhwc4_f16,
// simpb_preprocess_yuv420sp_nhwc4_f16) has a horizontal kernel of its own each, where the host decides once whether rows go
// as 16-byte chunks. A SURFACE (simpb_preprocess_surface_nhwc4_f16, simpb_preprocess_planes_nhwc4_f16) has row pitch, chroma
// pitch and offsets and the image stride as arguments, and its images are one contiguous batch or a device table of one
// address per image; it reads no byte outside a needed row's samples. A RIG of cameras that differ
// (simpb_preprocess_rig_nhwc4_f16) gives image n the descriptor of camera n % cams (format, size, layout, row range, taps,
// tables), passed by value, behind a per-workgroup choice; address 0 in its table skips an image, whose output block is
// written as zeros. The vertical pass has a kernel for the uniform batch and one for the rig, which fill a ColsImage each.
// LEVEL AND ROLLED. A camera's mount roll (the reference's img.rotate: simpb_preprocess_roll_nhwc4_f16,
// simpb_preprocess_rig_roll_nhwc4_f16) is a second accumulation loop of the vertical pass, a gather by six integers per
// camera (resample_cols_lut_roll_row) in front of the same epilogue; the level loop is launched as ever where no camera is
// rolled.
// Every load of a thread is retired before its stores are issued (store_fence.h).
#include <hip/hip_runtime.h>
#include <type_traits>
#include "../../include/simpb_hip.h"
#include "store_fence.h"

#include "launch.h"

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));

constexpr int kThreads = 256;
constexpr int kMaxSrcW = 4096;    // staged source row: 12 KB
constexpr int kMaxOutW = 2048;    // staged resampled row: 6 KB
constexpr int kMaxTaps = SIMPB_PREPROCESS_MAX_TAPS;
constexpr int kPrecision = 22;

// the one clamp to a byte: of a filter sum (>> kPrecision) and of a converted colour (>> its fractional bits)
__device__ __forceinline__ int clamp8(int v) { return min(max(v, 0), 255); }

// ---------------------------------------------------------------------------------------------- the horizontal pass
// The part of the horizontal pass every source shares: the staged [Ws][3] row `s_src` (complete: the caller has
// synchronised) -> row `mid_row` of the intermediate.
//   mid_row[j][c] = clamp8((2^21 + sum_t s_src[xlo[jj] + t][c] * kx[jj][t]) >> 22),  jj = flip ? w - 1 - j : j
__device__ __forceinline__ void filter_row_and_store(unsigned char* __restrict__ mid_row, const unsigned char* s_src, unsigned char* s_out,
                                                     const int* __restrict__ kx, const int* __restrict__ xlo,
                                                     const int* __restrict__ xn, int Ws, int w, int taps, int flip, int pitch) {
  const int tid = threadIdx.x;
  const int wpad = pitch / 3;   // (columns past w are padding the vertical pass may read and never uses)
  for (int j = tid; j < wpad; j += kThreads) {
    int v0 = 0, v1 = 0, v2 = 0;
    if (j < w) {
      const int jj = flip ? w - 1 - j : j;
      // (bounds of a consistent table are inside the row already: the clamps keep a wrong table from leaving LDS)
      const int cnt = min(min(xn[jj], taps), Ws);
      const int lo = min(max(xlo[jj], 0), Ws - cnt);
      const int* k = kx + (size_t)jj * taps;
      int a0 = 1 << (kPrecision - 1), a1 = a0, a2 = a0;
      for (int t = 0; t < cnt; ++t) {
        const int c = k[t];
        const unsigned char* s = s_src + (lo + t) * 3;
        a0 += (int)s[0] * c;
        a1 += (int)s[1] * c;
        a2 += (int)s[2] * c;
      }
      v0 = clamp8(a0 >> kPrecision); v1 = clamp8(a1 >> kPrecision); v2 = clamp8(a2 >> kPrecision);
    }
    s_out[j * 3] = (unsigned char)v0;
    s_out[j * 3 + 1] = (unsigned char)v1;
    s_out[j * 3 + 2] = (unsigned char)v2;
  }
  for (int i = wpad * 3 + tid; i < pitch; i += kThreads) s_out[i] = 0;
  simpb::loads_retired();
  __syncthreads();
  uint4* o16 = reinterpret_cast<uint4*>(mid_row);   // pitch % 16 == 0, mid 16-byte aligned
  const uint4* s16 = reinterpret_cast<const uint4*>(s_out);
  for (int i = tid; i < (pitch >> 4); i += kThreads) o16[i] = s16[i];
}

// Exactly `bytes` of one source row into LDS, as 16-byte chunks where the row allows them and bytewise where not.
// kGiven (the tight batches): the host found every row to start on a 16-byte boundary and to be whole chunks, and says so
// in `vec16`; there is no tail to copy, and none is paid for.
// kByAddress (surfaces and rigs): never a byte past `bytes` (a surface may end at its last sample, and what lies between
// two rows is not the caller's to read). A row that starts on a 16-byte boundary goes as floor(bytes / 16) chunks and a
// bytewise tail; any other row bytewise. The choice is made here, from the row's own address (uniform over the workgroup):
// with a pitch that is no multiple of 16 it alternates from row to row, and under a captured graph the address table
// changes between replays while the kernel arguments do not.
enum Chunks { kGiven, kByAddress };

template <Chunks kChunks>
__device__ __forceinline__ void stage_row(unsigned char* s_dst, const unsigned char* __restrict__ p, int bytes, int vec16 = 0) {
  const int tid = threadIdx.x;
  if constexpr (kChunks == kByAddress) vec16 = (reinterpret_cast<size_t>(p) & 15) == 0;
  if (vec16) {
    const int chunks = bytes >> 4;
    const uint4* p16 = reinterpret_cast<const uint4*>(p);
    uint4* s16 = reinterpret_cast<uint4*>(s_dst);
    for (int i = tid; i < chunks; i += kThreads) s16[i] = p16[i];
    if constexpr (kChunks == kByAddress)
      for (int i = (chunks << 4) + tid; i < bytes; i += kThreads) s_dst[i] = p[i];
  } else {
    for (int i = tid; i < bytes; i += kThreads) s_dst[i] = p[i];
  }
}

// One pixel -> its (B, G, R) bytes at d[0 .. 2]: the integer YCbCr rule of every YCbCr format, with S = kShift fractional bits
// and chroma centre C = kCentre: 16 / 128 for 8-bit samples, 18 / 512 for 10-bit ones (P010), whose luma offset is 4 * yoff as well:
//   c = iy * (Y - yoff) + 2^(S-1),  R = clamp8((c + irv * (Cr - C)) >> S),  G = clamp8((c + igu * (Cb - C) + igv * (Cr - C)) >> S),
//   B = clamp8((c + ibu * (Cb - C)) >> S)     (int32, arithmetic shift, clamp to 0..255)
// Every pixel brings its own Cb / Cr: the same pair for both pixels where chroma is replicated (the products are then computed
// once), an interpolated one each where it is not (fancy_pair).
struct YuvCoeffs { int yoff, iy, irv, igu, igv, ibu; };

template <int kShift = 16, int kCentre = 128>
__device__ __forceinline__ void yuv_to_bgr(unsigned char* d, int y, int cb, int cr, const YuvCoeffs& q) {
  cb -= kCentre; cr -= kCentre;
  const int c = q.iy * (y - (q.yoff << (kShift - 16))) + (1 << (kShift - 1));
  d[0] = (unsigned char)clamp8((c + q.ibu * cb) >> kShift);
  d[1] = (unsigned char)clamp8((c + q.igu * cb + q.igv * cr) >> kShift);
  d[2] = (unsigned char)clamp8((c + q.irv * cr) >> kShift);
}

// INTERPOLATED CHROMA (SIMPB_SURFACE_CHROMA_JPEG): libjpeg's "fancy" upsampling, the triangle filter its decoder applies to
// the subsampled planes of a JPEG at its defaults, in int32. For chroma pair j of a row of Wc pairs, with t(k) the pair's two
// samples after the vertical step and l = max(j - 1, 0), r = min(j + 1, Wc - 1):
//   column 2j:      (3 t(j) + t(l) + kEven) >> kBits         column 2j + 1:  (3 t(j) + t(r) + kOdd) >> kBits
// 4:2:0 (h2v2_fancy_upsample): t(k) = 3 near[k] + far[k], near = chroma row r >> 1, far = the row above it for an even luma
// row r and the row below for an odd one, clamped to the plane; kEven / kOdd / kBits = 8 / 7 / 4.
// 4:2:2 (h2v1_fancy_upsample): t(k) = the row's own sample; 1 / 2 / 2.
// tap(k, cb, cr) gives t(k) of both components; cb / cr take the two columns' samples.
template <int kEven, int kOdd, int kBits, class Tap>
__device__ __forceinline__ void fancy_pair(int j, int Wc, Tap&& tap, int (&cb)[2], int (&cr)[2]) {
  int b, r, bl, rl, br, rr;
  tap(j, b, r);
  tap(max(j - 1, 0), bl, rl);
  tap(min(j + 1, Wc - 1), br, rr);
  cb[0] = (3 * b + bl + kEven) >> kBits;
  cb[1] = (3 * b + br + kOdd) >> kBits;
  cr[0] = (3 * r + rl + kEven) >> kBits;
  cr[1] = (3 * r + rr + kOdd) >> kBits;
}

// A tight batch of BGR frames, u8 [N][Hs][Ws][3]:
// mid[n][r][j][c] = clamp8((2^21 + sum_t src[n][row0 + r][xlo[jj] + t][c] * kx[jj][t]) >> 22),  jj = flip ? w - 1 - j : j
__global__ __launch_bounds__(kThreads) void resample_rows_kernel(unsigned char* __restrict__ mid, const unsigned char* __restrict__ src,
                                                                 const int* __restrict__ kx, const int* __restrict__ xlo,
                                                                 const int* __restrict__ xn, int Hs, int Ws, int row0, int rows,
                                                                 int w, int taps, int flip, int pitch, int vec16) {
  __shared__ __attribute__((aligned(16))) unsigned char s_src[kMaxSrcW * 3];
  __shared__ __attribute__((aligned(16))) unsigned char s_out[kMaxOutW * 3 + 16];
  const int r = blockIdx.x, n = blockIdx.y;
  const size_t row_bytes = (size_t)Ws * 3;
  stage_row<kGiven>(s_src, src + ((size_t)n * Hs + row0 + r) * row_bytes, (int)row_bytes, vec16);
  __syncthreads();
  filter_row_and_store(mid + ((size_t)n * rows + r) * pitch, s_src, s_out, kx, xlo, xn, Ws, w, taps, flip, pitch);
}

// A tight batch of 4:2:0 semi-planar frames (NV12 / NV21): one image is u8 [Hs * 3 / 2][Ws], Hs luma rows, then Hs / 2 rows
// of interleaved chroma pairs, (Cb, Cr) or with `vu` (Cr, Cb); chroma sample (i, j) covers luma rows 2i, 2i + 1 and columns
// 2j, 2j + 1 (replicated). The luma row and its chroma row are staged, converted once into the (B, G, R) row the BGR kernel
// stages (yuv_to_bgr) and filtered by the same code.
__global__ __launch_bounds__(kThreads) void resample_rows_yuv420sp_kernel(unsigned char* __restrict__ mid, const unsigned char* __restrict__ src,
                                                                          const int* __restrict__ kx, const int* __restrict__ xlo,
                                                                          const int* __restrict__ xn, int Hs, int Ws, int row0, int rows,
                                                                          int w, int taps, int flip, int pitch, int vec16, int vu, YuvCoeffs q) {
  __shared__ __attribute__((aligned(16))) unsigned char s_src[kMaxSrcW * 3];
  __shared__ __attribute__((aligned(16))) unsigned char s_out[kMaxOutW * 3 + 16];
  __shared__ __attribute__((aligned(16))) unsigned char s_luma[kMaxSrcW];
  __shared__ __attribute__((aligned(16))) unsigned char s_chroma[kMaxSrcW];
  const int tid = threadIdx.x, r = blockIdx.x, n = blockIdx.y;
  const int row = row0 + r;
  const unsigned char* image = src + (size_t)n * (Hs + (Hs >> 1)) * Ws;
  stage_row<kGiven>(s_luma, image + (size_t)row * Ws, Ws, vec16);
  stage_row<kGiven>(s_chroma, image + (size_t)(Hs + (row >> 1)) * Ws, Ws, vec16);
  __syncthreads();
  for (int x = 2 * tid; x < Ws; x += 2 * kThreads) {   // a chroma pair and its two luma samples (Ws is even)
    const int cb = s_chroma[x + vu], cr = s_chroma[x + 1 - vu];
    yuv_to_bgr(s_src + x * 3, (int)s_luma[x], cb, cr, q);
    yuv_to_bgr(s_src + x * 3 + 3, (int)s_luma[x + 1], cb, cr, q);
  }
  __syncthreads();
  filter_row_and_store(mid + ((size_t)n * rows + r) * pitch, s_src, s_out, kx, xlo, xn, Ws, w, taps, flip, pitch);
}

// One image as a decoder delivers it (include/simpb_hip.h, simpb_preprocess_surface_nhwc4_f16): image n starts at
// src + n * image_stride, or at table[n] when `table` is given; luma (or BGR) row r at + r * pitch, chroma row i at
// + chroma_offset + i * chroma_pitch (planar 4:2:0: the Cb row there, the Cr row at + chroma2_offset + i * chroma_pitch). The
// table is read by the kernel: a captured launch follows the addresses written into it before each replay.
struct Surface {
  const unsigned char* src;
  const unsigned long long* table;
  long long image_stride, chroma_offset, pitch, chroma_pitch, chroma2_offset;
  int chroma_rows;   // rows of a 4:2:0 chroma plane (src_height / 2): where the far row of interpolated chroma is clamped
};

constexpr int kBgr = SIMPB_SURFACE_BGR, kNv12 = SIMPB_SURFACE_NV12, kNv21 = SIMPB_SURFACE_NV21, kP010 = SIMPB_SURFACE_P010;
constexpr int kYuv420p = SIMPB_SURFACE_YUV420P, kYuyv = SIMPB_SURFACE_YUYV, kUyvy = SIMPB_SURFACE_UYVY, kRgb = SIMPB_SURFACE_RGB;
constexpr int kBgra = SIMPB_SURFACE_BGRA, kRgba = SIMPB_SURFACE_RGBA, kYuv444p = SIMPB_SURFACE_YUV444P;
// A format code with this flag is a format of its own: the same samples, chroma interpolated (fancy_pair). The five formats
// with subsampled 8-bit chroma take it, and nothing else does.
constexpr int kJpeg = SIMPB_SURFACE_CHROMA_JPEG;
__host__ __device__ constexpr int base_format(int format) { return format & ~kJpeg; }
__host__ __device__ constexpr bool takes_jpeg_chroma(int base) {
  return base == kNv12 || base == kNv21 || base == kYuv420p || base == kYuyv || base == kUyvy;
}

// The one place where a runtime format code becomes a compile-time constant: fn(std::integral_constant<int, F>) for the
// code's F, and true; false, and nothing called, for a code that is no format (the entry points refuse it before any launch).
// kLastIsElse is for the rig kernel alone: there the last format stands for every other code as well, so that the choice
// has no path that stages nothing (the loads of the camera's layout stay in front of it) and ends in no wrong access.
// Interpolated chroma is a template parameter like the format, not a branch inside the replicated code: the instantiations
// of replicated chroma are the code they were (the same instruction counts and registers in every horizontal kernel but the
// rig's, which gains the new arms), and a rig pays for the interpolated form only in the workgroups of a camera that asks
// for it (profiles/jpeg_chroma.md has the figures).
template <bool kLastIsElse = false, class Fn>
__host__ __device__ __forceinline__ bool with_format(int format, Fn&& fn) {
  switch (format) {
#define SIMPB_FORMAT(F) case F: fn(std::integral_constant<int, F>{}); return true
    SIMPB_FORMAT(kBgr);
    SIMPB_FORMAT(kNv12);
    SIMPB_FORMAT(kNv21);
    SIMPB_FORMAT(kYuv420p);
    SIMPB_FORMAT(kYuyv);
    SIMPB_FORMAT(kUyvy);
    SIMPB_FORMAT(kRgb);
    SIMPB_FORMAT(kBgra);
    SIMPB_FORMAT(kRgba);
    SIMPB_FORMAT(kYuv444p);
    SIMPB_FORMAT(kNv12 | kJpeg);
    SIMPB_FORMAT(kNv21 | kJpeg);
    SIMPB_FORMAT(kYuv420p | kJpeg);
    SIMPB_FORMAT(kYuyv | kJpeg);
    SIMPB_FORMAT(kUyvy | kJpeg);
#undef SIMPB_FORMAT
    default:
      if (!kLastIsElse && format != kP010) return false;
      fn(std::integral_constant<int, kP010>{});
      return true;
  }
}

// LDS bytes of the two staging planes of a source `width` wide, s_luma and s_chroma (one plane each; a multiple of 16). A
// packed row that is converted or compacted on its way into the (B, G, R) row (4:2:2: 2 bytes per pixel, BGRA / RGBA: 4) is
// staged from s_luma on and runs through into s_chroma, which lies right behind it; the two chroma rows of planar 4:2:0 share
// s_chroma, the Cr row in its second half, and so do the two full-width chroma rows of planar 4:4:4. BGR and RGB rows are
// staged where the filter reads them. Interpolated chroma changes nothing here: a 4:2:0 format stages its far chroma row in a
// third plane of the same size, s_far, behind s_chroma (far_plane), and 4:2:2 reads its neighbours in the row it has.
__host__ __device__ constexpr int plane_bytes(int format, int width) {
  const int base = base_format(format);
  return base == kBgr || base == kRgb ? 0
         : base == kP010 || base == kBgra || base == kRgba ? (2 * width + 15) / 16 * 16
         : base == kYuv420p ? 2 * ((width / 2 + 15) / 16 * 16)
         : base == kYuv444p ? 2 * ((width + 15) / 16 * 16)
                            : (width + 15) / 16 * 16;   // (NV12 / NV21: a luma and a chroma row; 4:2:2: the halves of its row)
}
__host__ __device__ constexpr bool far_plane(int format) {
  return (format & kJpeg) && (base_format(format) == kNv12 || base_format(format) == kNv21 || base_format(format) == kYuv420p);
}

// One source row of a surface as the (B, G, R) row the filter reads, for every source format. `image` is the image's first
// byte, luma (or BGR) row r at + r * pitch, chroma row i at + chroma_offset + i * chroma_pitch. Returns with s_src complete
// (synchronised). Chroma rows that lie under no needed luma row are never read.
// kBgr: the surface's own interleaved row, staged where the filter reads it (s_luma / s_chroma are not looked at). kRgb: the
// BGR row with bytes 0 and 2 of every pixel exchanged. kBgra / kRgba: 4 bytes per pixel, byte 3 is dropped whatever it holds.
// The YCbCr formats are arrangements of the samples that yuv_to_bgr takes. 4:2:0 semi-planar (kNv12: (Cb, Cr) pairs,
// kNv21: (Cr, Cb), u8; kP010: (Cb, Cr), u16 little-endian with the 10-bit sample in the high bits): chroma sample (i, j) covers
// luma rows 2i, 2i + 1 and columns 2j, 2j + 1 (replicated); the luma row and the chroma row under it are staged, Ws samples
// each in s_luma / s_chroma. kYuv420p (I420 / YV12): three planes, the Cb row i of Ws / 2 bytes at + chroma_offset +
// i * chroma_pitch and the Cr row at + chroma2_offset + i * chroma_pitch; which plane comes first in memory is the caller's to
// say through the two offsets. kYuyv / kUyvy (packed 4:2:2): one plane, a row is Ws / 2 groups (Y0, Cb, Y1, Cr) /
// (Cb, Y0, Cr, Y1); the pair belongs to columns 2j, 2j + 1 of its own row. kYuv444p: three planes of Ws bytes a row, addressed
// like kYuv420p, a Cb and a Cr sample per pixel: nothing to replicate or interpolate (what a 4:4:4 JPEG decodes to).
// F | kJpeg (the five 8-bit formats with subsampled chroma): the same samples, centre-sited, interpolated by fancy_pair. A
// 4:2:0 row stages a second chroma row, the far one, in s_far (arranged like s_chroma): row (row >> 1) - 1 for an even luma
// row and + 1 for an odd one, clamped to 0 .. chroma_rows - 1. It is read whether or not a needed luma row lies over it, and
// like every row exactly its sample bytes; 4:2:2 reads the neighbouring pairs of the row it has staged.
template <int F>
__device__ __forceinline__ void stage_bgr_row(unsigned char* s_src, unsigned char* s_luma, unsigned char* s_chroma, unsigned char* s_far,
                                              const unsigned char* __restrict__ image, long long pitch, long long chroma_offset,
                                              long long chroma_pitch, long long chroma2_offset, int chroma_rows, int row, int Ws,
                                              const YuvCoeffs& q) {
  const int tid = threadIdx.x;
  [[maybe_unused]] const int far = min(max((row >> 1) + ((row & 1) ? 1 : -1), 0), chroma_rows - 1);
  if constexpr (F == (kYuyv | kJpeg) || F == (kUyvy | kJpeg)) {   // (Ws is even)
    stage_row<kByAddress>(s_luma, image + (size_t)row * pitch, Ws * 2);
    __syncthreads();
    const unsigned int* group = reinterpret_cast<const unsigned int*>(s_luma);
    constexpr int kY = base_format(F) == kYuyv ? 0 : 8, kC = 8 - kY;   // bit of Y0 and of Cb inside the group
    const int Wc = Ws >> 1;
    for (int j = tid; j < Wc; j += kThreads) {
      int cb[2], cr[2];
      fancy_pair<1, 2, 2>(j, Wc, [&](int k, int& b, int& r) {
        const unsigned int v = group[k];
        b = (int)((v >> kC) & 255u);
        r = (int)((v >> (kC + 16)) & 255u);
      }, cb, cr);
      const unsigned int v = group[j];
      yuv_to_bgr(s_src + j * 6, (int)((v >> kY) & 255u), cb[0], cr[0], q);
      yuv_to_bgr(s_src + j * 6 + 3, (int)((v >> (kY + 16)) & 255u), cb[1], cr[1], q);
    }
    __syncthreads();
  } else if constexpr (F == (kYuv420p | kJpeg)) {
    const int Wc = Ws >> 1, half = (Wc + 15) & ~15;   // (plane_bytes: the Cr row in the second half of s_chroma / s_far)
    stage_row<kByAddress>(s_luma, image + (size_t)row * pitch, Ws);
    stage_row<kByAddress>(s_chroma, image + chroma_offset + (size_t)(row >> 1) * chroma_pitch, Wc);
    stage_row<kByAddress>(s_chroma + half, image + chroma2_offset + (size_t)(row >> 1) * chroma_pitch, Wc);
    stage_row<kByAddress>(s_far, image + chroma_offset + (size_t)far * chroma_pitch, Wc);
    stage_row<kByAddress>(s_far + half, image + chroma2_offset + (size_t)far * chroma_pitch, Wc);
    __syncthreads();
    for (int j = tid; j < Wc; j += kThreads) {
      int cb[2], cr[2];
      fancy_pair<8, 7, 4>(j, Wc, [&](int k, int& b, int& r) {
        b = 3 * (int)s_chroma[k] + (int)s_far[k];
        r = 3 * (int)s_chroma[half + k] + (int)s_far[half + k];
      }, cb, cr);
      yuv_to_bgr(s_src + j * 6, (int)s_luma[2 * j], cb[0], cr[0], q);
      yuv_to_bgr(s_src + j * 6 + 3, (int)s_luma[2 * j + 1], cb[1], cr[1], q);
    }
    __syncthreads();
  } else if constexpr (F == (kNv12 | kJpeg) || F == (kNv21 | kJpeg)) {
    constexpr int kB = base_format(F) == kNv21 ? 8 : 0, kR = 8 - kB;   // bit of Cb and of Cr inside a pair
    const int Wc = Ws >> 1;
    stage_row<kByAddress>(s_luma, image + (size_t)row * pitch, Ws);
    stage_row<kByAddress>(s_chroma, image + chroma_offset + (size_t)(row >> 1) * chroma_pitch, Ws);
    stage_row<kByAddress>(s_far, image + chroma_offset + (size_t)far * chroma_pitch, Ws);
    __syncthreads();
    const unsigned short* near2 = reinterpret_cast<const unsigned short*>(s_chroma);   // one chroma pair (LDS is 16-byte aligned)
    const unsigned short* far2 = reinterpret_cast<const unsigned short*>(s_far);
    const unsigned short* luma2 = reinterpret_cast<const unsigned short*>(s_luma);
    for (int j = tid; j < Wc; j += kThreads) {
      int cb[2], cr[2];
      fancy_pair<8, 7, 4>(j, Wc, [&](int k, int& b, int& r) {
        const unsigned int n = near2[k], f = far2[k];
        b = 3 * (int)((n >> kB) & 255u) + (int)((f >> kB) & 255u);
        r = 3 * (int)((n >> kR) & 255u) + (int)((f >> kR) & 255u);
      }, cb, cr);
      const unsigned int y = luma2[j];
      yuv_to_bgr(s_src + j * 6, (int)(y & 255u), cb[0], cr[0], q);
      yuv_to_bgr(s_src + j * 6 + 3, (int)(y >> 8), cb[1], cr[1], q);
    }
    __syncthreads();
  } else if constexpr (F == kYuv444p) {
    unsigned char* s_cr = s_chroma + ((Ws + 15) & ~15);   // (plane_bytes: the second half of s_chroma)
    stage_row<kByAddress>(s_luma, image + (size_t)row * pitch, Ws);
    stage_row<kByAddress>(s_chroma, image + chroma_offset + (size_t)row * chroma_pitch, Ws);
    stage_row<kByAddress>(s_cr, image + chroma2_offset + (size_t)row * chroma_pitch, Ws);
    __syncthreads();
    for (int x = tid; x < Ws; x += kThreads) yuv_to_bgr(s_src + x * 3, (int)s_luma[x], (int)s_chroma[x], (int)s_cr[x], q);
    __syncthreads();
  } else if constexpr (F == kBgr) {
    stage_row<kByAddress>(s_src, image + (size_t)row * pitch, Ws * 3);
    __syncthreads();
  } else if constexpr (F == kRgb) {   // permuted where it lies: a thread exchanges the ends of its own pixels
    stage_row<kByAddress>(s_src, image + (size_t)row * pitch, Ws * 3);
    __syncthreads();
    for (int x = tid; x < Ws; x += kThreads) {
      unsigned char* d = s_src + x * 3;
      const unsigned char r = d[0];
      d[0] = d[2];
      d[2] = r;
    }
    __syncthreads();
  } else if constexpr (F == kBgra || F == kRgba) {   // the row of dwords (LDS is 16-byte aligned), compacted
    stage_row<kByAddress>(s_luma, image + (size_t)row * pitch, Ws * 4);
    __syncthreads();
    const unsigned int* px = reinterpret_cast<const unsigned int*>(s_luma);
    for (int x = tid; x < Ws; x += kThreads) {
      const unsigned int v = px[x];
      unsigned char* d = s_src + x * 3;
      d[F == kRgba ? 2 : 0] = (unsigned char)(v & 255u);
      d[1] = (unsigned char)((v >> 8) & 255u);
      d[F == kRgba ? 0 : 2] = (unsigned char)((v >> 16) & 255u);
    }
    __syncthreads();
  } else if constexpr (F == kYuyv || F == kUyvy) {   // one dword = one chroma pair and its two luma samples (Ws is even)
    stage_row<kByAddress>(s_luma, image + (size_t)row * pitch, Ws * 2);
    __syncthreads();
    const unsigned int* group = reinterpret_cast<const unsigned int*>(s_luma);
    constexpr int kY = F == kYuyv ? 0 : 8, kC = 8 - kY;   // bit of Y0 and of Cb inside the group
    for (int j = tid; 2 * j < Ws; j += kThreads) {
      const unsigned int v = group[j];
      const int cb = (int)((v >> kC) & 255u), cr = (int)((v >> (kC + 16)) & 255u);
      yuv_to_bgr(s_src + j * 6, (int)((v >> kY) & 255u), cb, cr, q);
      yuv_to_bgr(s_src + j * 6 + 3, (int)((v >> (kY + 16)) & 255u), cb, cr, q);
    }
    __syncthreads();
  } else if constexpr (F == kYuv420p) {
    unsigned char* s_cr = s_chroma + (((Ws >> 1) + 15) & ~15);   // (plane_bytes: the second half of s_chroma)
    stage_row<kByAddress>(s_luma, image + (size_t)row * pitch, Ws);
    stage_row<kByAddress>(s_chroma, image + chroma_offset + (size_t)(row >> 1) * chroma_pitch, Ws >> 1);
    stage_row<kByAddress>(s_cr, image + chroma2_offset + (size_t)(row >> 1) * chroma_pitch, Ws >> 1);
    __syncthreads();
    for (int j = tid; 2 * j < Ws; j += kThreads) {
      const int cb = s_chroma[j], cr = s_cr[j];
      yuv_to_bgr(s_src + j * 6, (int)s_luma[2 * j], cb, cr, q);
      yuv_to_bgr(s_src + j * 6 + 3, (int)s_luma[2 * j + 1], cb, cr, q);
    }
    __syncthreads();
  } else {
    static_assert(F == kNv12 || F == kNv21 || F == kP010, "a format without a branch of its own");
    constexpr int kSample = F == kP010 ? 2 : 1;   // bytes per sample
    constexpr int kVu = F == kNv21 ? 1 : 0;
    stage_row<kByAddress>(s_luma, image + (size_t)row * pitch, Ws * kSample);
    stage_row<kByAddress>(s_chroma, image + chroma_offset + (size_t)(row >> 1) * chroma_pitch, Ws * kSample);
    __syncthreads();
    for (int x = 2 * tid; x < Ws; x += 2 * kThreads) {   // a chroma pair and its two luma samples (Ws is even)
      if constexpr (F == kP010) {   // sample = word >> 6: the low six bits are ignored whatever they hold
        const unsigned short* l = reinterpret_cast<const unsigned short*>(s_luma);
        const unsigned short* c = reinterpret_cast<const unsigned short*>(s_chroma);
        const int cb = c[x] >> 6, cr = c[x + 1] >> 6;
        yuv_to_bgr<18, 512>(s_src + x * 3, (int)(l[x] >> 6), cb, cr, q);
        yuv_to_bgr<18, 512>(s_src + x * 3 + 3, (int)(l[x + 1] >> 6), cb, cr, q);
      } else {
        const int cb = s_chroma[x + kVu], cr = s_chroma[x + 1 - kVu];
        yuv_to_bgr(s_src + x * 3, (int)s_luma[x], cb, cr, q);
        yuv_to_bgr(s_src + x * 3 + 3, (int)s_luma[x + 1], cb, cr, q);
      }
    }
    __syncthreads();
  }
}

// The horizontal pass over a surface, one workgroup per (needed source row, image), for every source format (stage_bgr_row):
//   mid[n][r][j][c] = clamp8((2^21 + sum_t bgr[n][row0 + r][xlo[jj] + t][c] * kx[jj][t]) >> 22),  jj = flip ? w - 1 - j : j
template <int F>
__global__ __launch_bounds__(kThreads) void resample_rows_surface_kernel(unsigned char* __restrict__ mid, Surface sf,
                                                                         const int* __restrict__ kx, const int* __restrict__ xlo,
                                                                         const int* __restrict__ xn, int Ws, int row0, int rows, int w,
                                                                         int taps, int flip, int pitch, YuvCoeffs q) {
  __shared__ __attribute__((aligned(16))) unsigned char s_src[kMaxSrcW * 3];
  __shared__ __attribute__((aligned(16))) unsigned char s_out[kMaxOutW * 3 + 16];
  // (a BGR / RGB row is staged where the filter reads it; a packed 4:2:2 or 4-byte row lies in s_luma as a whole)
  constexpr bool kPacked = base_format(F) == kYuyv || base_format(F) == kUyvy || F == kBgra || F == kRgba;
  constexpr int kPlane = plane_bytes(F, kMaxSrcW) == 0 ? 16 : plane_bytes(F, kMaxSrcW);
  __shared__ __attribute__((aligned(16))) unsigned char s_luma[kPacked ? 2 * kPlane : kPlane];
  __shared__ __attribute__((aligned(16))) unsigned char s_chroma[kPacked ? 16 : kPlane];
  __shared__ __attribute__((aligned(16))) unsigned char s_far[far_plane(F) ? kPlane : 16];   // (interpolated 4:2:0 alone)
  const int r = blockIdx.x, n = blockIdx.y;
  const unsigned char* image = sf.table ? reinterpret_cast<const unsigned char*>(sf.table[n]) : sf.src + (size_t)n * sf.image_stride;
  stage_bgr_row<F>(s_src, s_luma, s_chroma, s_far, image, sf.pitch, sf.chroma_offset, sf.chroma_pitch, sf.chroma2_offset,
                   sf.chroma_rows, row0 + r, Ws, q);
  filter_row_and_store(mid + ((size_t)n * rows + r) * pitch, s_src, s_out, kx, xlo, xn, Ws, w, taps, flip, pitch);
}

// A RIG (simpb_preprocess_rig_nhwc4_f16): image n belongs to camera n % num_cams, and every camera has its own size, format,
// layout and tables (simpb_rig_camera, handed over by value: a captured launch keeps its rig and reads nothing but the
// address table at replay). The descriptor is chosen by blockIdx alone, i.e. it is uniform over the workgroup and is read
// through scalar loads.
struct Rig { simpb_rig_camera cam[SIMPB_RIG_MAX_CAMS]; };

// The horizontal pass of a rig: the grid spans the tallest camera's rows, and a workgroup past its own camera's rows -- or
// whose image has address 0 (the image is skipped: the vertical pass writes zeros) -- leaves before any barrier; a camera whose
// format is none (the entry point has refused such a rig) is staged as the last format (with_format<true>). Stream n / num_cams keeps its cameras' rows one
// behind the other in a block of `mid_rows` rows, camera c from row mid_row on.
// LDS is dynamic, sized by the entry point for the rig at hand (RigLds: the widest camera's (B, G, R) row, the resampled row,
// and the widest staging planes of any camera, plane_bytes), not for the widest source the file takes: a rig of 1600-wide NV12
// cameras holds 10 KB per workgroup where the static arrays of the surface kernel hold 26 KB, and a BGR rig has no planes.
// A rig with a camera of interpolated 4:2:0 chroma has a third plane of that size behind the two (1.6 KB more at 1600 wide).
struct RigLds { int src_bytes, out_bytes, plane_bytes; };   // each a multiple of 16

__global__ __launch_bounds__(kThreads) void resample_rows_rig_kernel(unsigned char* __restrict__ mid,
                                                                     const unsigned long long* __restrict__ table, Rig rig,
                                                                     int num_cams, const int* __restrict__ kx,
                                                                     const int* __restrict__ xlo, const int* __restrict__ xn, int w,
                                                                     int pitch, int mid_rows, RigLds lds) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_rig[];
  unsigned char* s_src = s_rig;
  unsigned char* s_out = s_src + lds.src_bytes;
  unsigned char* s_luma = s_out + lds.out_bytes;
  unsigned char* s_chroma = s_luma + lds.plane_bytes;
  unsigned char* s_far = s_chroma + lds.plane_bytes;   // (there where a camera of the rig stages a far chroma row: far_plane)
  const int r = blockIdx.x, n = blockIdx.y;
  const int stream = n / num_cams;
  const simpb_rig_camera& c = rig.cam[n - stream * num_cams];
  if (r >= c.src_rows) return;
  const unsigned char* image = reinterpret_cast<const unsigned char*>(table[n]);
  if (image == nullptr) return;
  const YuvCoeffs q = {c.yoff, c.iy, c.irv, c.igu, c.igv, c.ibu};
  const int row = c.src_row0 + r, Ws = c.src_width;
  with_format<true>(c.format, [&](auto f) {
    stage_bgr_row<decltype(f)::value>(s_src, s_luma, s_chroma, s_far, image, c.pitch, c.chroma_offset, c.chroma_pitch, c.chroma2_offset,
                                      c.src_height >> 1, row, Ws, q);
  });
  filter_row_and_store(mid + ((size_t)stream * mid_rows + c.mid_row + r) * pitch, s_src, s_out, kx + c.kx_offset, xlo + c.x_offset,
                       xn + c.x_offset, Ws, w, c.taps_x, c.flip, pitch);
}

// ------------------------------------------------------------------------------------------------ the vertical pass
// Image n as the vertical pass sees it: `mid` its `rows` intermediate rows (source rows row0 ..), ky / ylo / yn its own
// tables; zero (uniform over the workgroup): nothing of mid is read and the image is written as f16 zeros. The two kernels
// below fill it, each for its way of addressing the images, and that is all they do.
struct ColsImage {
  const unsigned char* mid;
  const int *ky, *ylo, *yn;
  int row0, rows, taps;
  bool zero;
};

// The epilogue of both forms of the vertical pass, in two halves around the accumulation loop. First the [3][256] table
// goes into LDS (the caller's barrier completes it) ...
__device__ __forceinline__ void stage_lut(_Float16* s_lut, const _Float16* __restrict__ lut) {
  for (int i = threadIdx.x; i < 3 * 256; i += kThreads) s_lut[i] = lut[i];
}

// ... then the 12 sums of group g of row y (4 pixels x 3 channels) go through it and out as two 16-byte stores:
//   out[y][4 g + px][c] = lut[c][inside[px] ? clamp8(acc[3 px + (swap ? 2 - c : c)] >> 22) : 0],  out[..][3] = 0
// (all of it f16 zeros where `zero`). The values are pinned and every load of the thread retired before the first store.
__device__ __forceinline__ void store_lut_group(_Float16* __restrict__ out_image, const _Float16* s_lut, const int (&acc)[12],
                                                const bool (&inside)[4], bool zero, int y, int g, int w, int swap_rb) {
  h8 v[2];
#pragma unroll
  for (int px = 0; px < 4; ++px) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int ci = swap_rb ? 2 - c : c;
      v[px >> 1][(px & 1) * 4 + c] = zero ? (_Float16)0.f : s_lut[c * 256 + (inside[px] ? clamp8(acc[px * 3 + ci] >> kPrecision) : 0)];
    }
    v[px >> 1][(px & 1) * 4 + 3] = (_Float16)0.f;
  }
  simpb::pin(v[0]);
  simpb::pin(v[1]);
  simpb::loads_retired();
  _Float16* o = out_image + ((size_t)y * w + 4 * g) * 4;
  if (4 * g + 4 <= w) {
    *reinterpret_cast<h8*>(o) = v[0];
    *reinterpret_cast<h8*>(o + 8) = v[1];
  } else {   // the last, partial group of a width that is no multiple of 4
#pragma unroll
    for (int px = 0; px < 3; ++px)
      if (4 * g + px < w) {
#pragma unroll
        for (int c = 0; c < 4; ++c) o[px * 4 + c] = v[px >> 1][(px & 1) * 4 + c];
      }
  }
}

// One output row of one image, the level vertical pass + table: `out_image` f16 [h][w][4]; y = blockIdx.y, the groups of 4
// pixels along blockIdx.x. A thread reads 12 intermediate bytes per tap row (three aligned dwords).
//   out[y][x][c] = lut[c][clamp8((2^21 + sum_t mid[ylo[y] - row0 + t][x][swap ? 2 - c : c] * ky[y][t]) >> 22)], out[..][3] = 0
__device__ __forceinline__ void resample_cols_lut_row(_Float16* __restrict__ out_image, const ColsImage& im,
                                                      const _Float16* __restrict__ lut, int w, int swap_rb, int pitch) {
  __shared__ _Float16 s_lut[3 * 256];
  __shared__ int s_k[kMaxTaps];
  const int tid = threadIdx.x, y = blockIdx.y;
  stage_lut(s_lut, lut);
  const int cnt = im.zero ? 0 : min(min(im.yn[y], im.taps), im.rows);
  if (tid < cnt) s_k[tid] = im.ky[(size_t)y * im.taps + tid];
  __syncthreads();
  const int g = blockIdx.x * kThreads + tid;   // group of 4 output pixels
  if (4 * g >= w) return;
  const int first = im.zero ? 0 : min(max(im.ylo[y] - im.row0, 0), im.rows - cnt);   // (clamped like the horizontal pass: never outside `mid`)
  const unsigned int* p = reinterpret_cast<const unsigned int*>(im.mid + (size_t)first * pitch) + 3 * g;
  const int pitch4 = pitch >> 2;
  int acc[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) acc[i] = 1 << (kPrecision - 1);
  for (int t = 0; t < cnt; ++t) {
    const int c = s_k[t];
    const unsigned int d0 = p[0], d1 = p[1], d2 = p[2];
    p += pitch4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      acc[i] += (int)((d0 >> (8 * i)) & 255u) * c;
      acc[4 + i] += (int)((d1 >> (8 * i)) & 255u) * c;
      acc[8 + i] += (int)((d2 >> (8 * i)) & 255u) * c;
    }
  }
  const bool inside[4] = {true, true, true, true};
  store_lut_group(out_image, s_lut, acc, inside, im.zero, y, g, w, swap_rb);
}

// A camera's MOUNT ROLL (simpb_preprocess_roll_nhwc4_f16, simpb_preprocess_rig_roll_nhwc4_f16): the reference's fourth step,
// PIL.Image.rotate(r) with its defaults, is a nearest-neighbour inverse affine map in 16.16 fixed point over the image that
// resize, crop and flip give. Output pixel (x, y) is the level pass's pixel (xin, yin),
//   xin = (a2 + y * a1 + x * a0) >> 16,  yin = (a5 + y * a4 + x * a3) >> 16     (64-bit, arithmetic shift)
// where 0 <= xin < w and 0 <= yin < h, and black -- lut[c][0] -- elsewhere. The roll maps rows of the cropped image onto rows
// of the cropped image, so the horizontal pass and `mid` are the level path's own, and the roll is a GATHER in the vertical
// pass: the thread still owns 4 neighbouring output pixels and writes two 16-byte stores, but each pixel brings its own row
// of ky and its own column of mid. The six integers per camera are the host's (simpb_amd/preprocess.py:roll_integers) and
// travel by value; the kernel knows nothing else of the angle. (65536, 0, 32768, 0, 65536, 32768) is the identity.
// Image n of a uniform batch takes row n % cams of the table, an image of a rig its camera's.
struct RollTable {
  static constexpr bool kRolled = true;
  int a[SIMPB_RIG_MAX_CAMS][6];
  int cams;
  __device__ __forceinline__ const int* row(int camera) const { return a[camera]; }
};
struct Level {   // in the table's place where no camera is rolled
  static constexpr bool kRolled = false;
  static constexpr int cams = 1;
  __device__ __forceinline__ const int* row(int) const { return nullptr; }
};

constexpr int kMaxRollSize = SIMPB_PREPROCESS_MAX_ROLL_SIZE;

// One output row of one image, the rolled vertical pass + table (arguments as resample_cols_lut_row; `a`: the image's six
// integers, uniform over the workgroup):
//   out[y][x][c] = lut[c][clamp8((2^21 + sum_t mid[ylo[yin] - row0 + t][xin][swap ? 2 - c : c] * ky[yin][t]) >> 22)], out[..][3] = 0
// The range test on (xin, yin) comes first; behind it the tap count, `first`, the row and the dword index are clamped as the
// level pass clamps them, and a pixel out of range (or a tap past its pixel's count) loads from row / column 0 with a
// coefficient of 0: a wrong table gives wrong pixels, never an access outside mid, ky, ylo or yn. The three bytes of a pixel
// start at byte 3 * xin of a row, at any alignment: they are cut out of the aligned dword that holds the first and the one
// behind it (the row's last dword again where there is none; 3 * xin + 2 < 3 * w <= pitch, so the bytes wanted lie in the two).
__device__ __forceinline__ void resample_cols_lut_roll_row(_Float16* __restrict__ out_image, const ColsImage& im,
                                                           const _Float16* __restrict__ lut, int h, int w, int swap_rb, int pitch,
                                                           const int* a) {
  __shared__ _Float16 s_lut[3 * 256];
  const int tid = threadIdx.x, y = blockIdx.y;
  stage_lut(s_lut, lut);
  __syncthreads();
  const int g = blockIdx.x * kThreads + tid;   // group of 4 output pixels
  if (4 * g >= w) return;
  const int pitch4 = pitch >> 2;
  const long long a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5];
  int cnt[4], first[4], dword[4], shift[4], krow[4];
  bool inside[4];
  int most = 0;
#pragma unroll
  for (int px = 0; px < 4; ++px) {
    const int x = 4 * g + px;
    const long long xs = (a2 + y * a1 + x * a0) >> 16, ys = (a5 + y * a4 + x * a3) >> 16;
    inside[px] = !im.zero && xs >= 0 && xs < w && ys >= 0 && ys < h;
    const int xin = inside[px] ? (int)xs : 0, yin = inside[px] ? (int)ys : 0;
    cnt[px] = inside[px] ? max(min(min(im.yn[yin], im.taps), im.rows), 0) : 0;
    first[px] = min(max(im.ylo[yin] - im.row0, 0), im.rows - cnt[px]);
    dword[px] = (3 * xin) >> 2;
    shift[px] = 8 * ((3 * xin) & 3);
    krow[px] = yin * im.taps;   // (h <= 8192, taps <= 64)
    most = max(most, cnt[px]);
  }
  int acc[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) acc[i] = 1 << (kPrecision - 1);
  for (int t = 0; t < most; ++t) {   // (most <= taps: ky[krow + t] lies in the pixel's own row of ky)
#pragma unroll
    for (int px = 0; px < 4; ++px) {
      const unsigned int* p = reinterpret_cast<const unsigned int*>(im.mid + (size_t)min(first[px] + t, im.rows - 1) * pitch);
      const unsigned int d0 = p[dword[px]], d1 = p[min(dword[px] + 1, pitch4 - 1)];
      const int c = t < cnt[px] ? im.ky[krow[px] + t] : 0;
      const unsigned int v = (unsigned int)((((unsigned long long)d1 << 32) | d0) >> shift[px]);
#pragma unroll
      for (int i = 0; i < 3; ++i) acc[px * 3 + i] += (int)((v >> (8 * i)) & 255u) * c;
    }
  }
  store_lut_group(out_image, s_lut, acc, inside, im.zero, y, g, w, swap_rb);
}

// One output row of one image, level or rolled (`a`: the image's six integers, looked at by the rolled form alone)
template <bool kRolled>
__device__ __forceinline__ void resample_cols_lut_either_row(_Float16* __restrict__ out_image, const ColsImage& im,
                                                             const _Float16* __restrict__ lut, int h, int w, int swap_rb, int pitch,
                                                             const int* a) {
  if constexpr (kRolled) resample_cols_lut_roll_row(out_image, im, lut, h, w, swap_rb, pitch, a);
  else resample_cols_lut_row(out_image, im, lut, w, swap_rb, pitch);
}

// The vertical pass of a uniform batch, level (Roll = Level) or rolled (RollTable): every image has the plan's one set of
// tables and its own block of `rows` intermediate rows.
template <class Roll>
__global__ __launch_bounds__(kThreads) void resample_cols_lut_kernel(_Float16* __restrict__ out, const unsigned char* __restrict__ mid,
                                                                     const int* __restrict__ ky, const int* __restrict__ ylo,
                                                                     const int* __restrict__ yn, const _Float16* __restrict__ lut,
                                                                     int row0, int rows, int h, int w, int taps, int swap_rb, int pitch,
                                                                     Roll roll) {
  const int n = blockIdx.z;
  const ColsImage im = {mid + (size_t)n * rows * pitch, ky, ylo, yn, row0, rows, taps, false};
  resample_cols_lut_either_row<Roll::kRolled>(out + (size_t)n * h * w * 4, im, lut, h, w, swap_rb, pitch, roll.row(n % roll.cams));
}

// The vertical pass of a rig, level or rolled: image n reads its camera's ky / ylo / yn, row range and taps, and its own rows
// of its stream's intermediate block; an image whose address is 0 is written as zeros.
template <class Roll>
__global__ __launch_bounds__(kThreads) void resample_cols_lut_rig_kernel(_Float16* __restrict__ out, const unsigned char* __restrict__ mid,
                                                                         const unsigned long long* __restrict__ table, Rig rig,
                                                                         int num_cams, const int* __restrict__ ky,
                                                                         const int* __restrict__ ylo, const int* __restrict__ yn,
                                                                         const _Float16* __restrict__ lut, int h, int w, int swap_rb,
                                                                         int pitch, int mid_rows, Roll roll) {
  const int n = blockIdx.z;
  const int stream = n / num_cams, cam = n - stream * num_cams;
  const simpb_rig_camera& c = rig.cam[cam];
  const ColsImage im = {mid + ((size_t)stream * mid_rows + c.mid_row) * pitch, ky + c.ky_offset, ylo + c.y_offset, yn + c.y_offset,
                        c.src_row0, c.src_rows, c.taps_y, table[n] == 0ull};
  resample_cols_lut_either_row<Roll::kRolled>(out + (size_t)n * h * w * 4, im, lut, h, w, swap_rb, pitch, roll.row(cam));
}

// ---------------------------------------------------------------------------------------------------- the host side
// What every entry point is given beside its images, filled once from its argument list: the device arrays ...
struct Tables {
  void* mid;
  const int *kx, *xlo, *xn, *ky, *ylo, *yn;
  const void* lut;
};

// ... and the numbers (flip and swap_rb as 0 / 1). A rig has one per camera, for the checks.
struct Shape { int num_images, src_height, src_width, out_height, out_width, taps_x, taps_y, src_row0, src_rows, flip, swap_rb; };

}  // namespace

// bytes of one intermediate row: whole groups of 4 pixels, rounded up to 16 bytes
static int mid_pitch(int out_width) { return ((out_width + 3) / 4 * 12 + 15) / 16 * 16; }

extern "C" int simpb_preprocess_mid_pitch(int out_width) {
  return (out_width <= 0 || out_width > kMaxOutW) ? 0 : mid_pitch(out_width);
}

// what every entry point refuses (before any HIP call); `images` is the batch or the address table
static bool bad_arguments(const void* out, const void* images, const Tables& t, const Shape& sh) {
  if (!out || !images || !t.mid || !t.kx || !t.xlo || !t.xn || !t.ky || !t.ylo || !t.yn || !t.lut) return true;
  if (sh.num_images <= 0 || sh.num_images > 65535 || sh.src_height <= 0 || sh.src_width <= 0 || sh.out_height <= 0 ||
      sh.out_width <= 0 || sh.out_height > 65535 || sh.src_width > kMaxSrcW || sh.out_width > kMaxOutW)
    return true;
  if (sh.taps_x <= 0 || sh.taps_y <= 0 || sh.taps_x > kMaxTaps || sh.taps_y > kMaxTaps) return true;
  if (sh.src_row0 < 0 || sh.src_rows <= 0 || (long long)sh.src_row0 + sh.src_rows > sh.src_height) return true;
  if ((reinterpret_cast<size_t>(out) | reinterpret_cast<size_t>(t.mid)) & 15) return true;
  if ((reinterpret_cast<size_t>(t.kx) | reinterpret_cast<size_t>(t.xlo) | reinterpret_cast<size_t>(t.xn) |
       reinterpret_cast<size_t>(t.ky) | reinterpret_cast<size_t>(t.ylo) | reinterpret_cast<size_t>(t.yn)) & 3)
    return true;
  return (reinterpret_cast<size_t>(t.lut) & 1) != 0;
}

// The vertical launch of every entry point, and the status of both launches: launch(grid, block, Level or RollTable) starts
// the caller's kernel, rolled where `roll` is given.
template <class Launch>
static int launch_vertical(int num_images, int out_height, int out_width, const RollTable* roll, Launch&& launch) {
  const int groups = (out_width + 3) / 4;
  const dim3 grid((groups + kThreads - 1) / kThreads, out_height, num_images), block(kThreads);
  if (roll) launch(grid, block, *roll);
  else launch(grid, block, Level{});
  return simpb_check_launch();
}

// the vertical pass + table of a uniform batch
static int uniform_vertical(void* out, const Tables& t, const Shape& sh, const RollTable* roll, hipStream_t s) {
  return launch_vertical(sh.num_images, sh.out_height, sh.out_width, roll, [&](dim3 grid, dim3 block, auto r) {
    hipLaunchKernelGGL(resample_cols_lut_kernel<decltype(r)>, grid, block, 0, s, static_cast<_Float16*>(out),
                       static_cast<const unsigned char*>(t.mid), t.ky, t.ylo, t.yn, static_cast<const _Float16*>(t.lut), sh.src_row0,
                       sh.src_rows, sh.out_height, sh.out_width, sh.taps_y, sh.swap_rb, mid_pitch(sh.out_width), r);
  });
}

// the horizontal pass of one source format on a checked surface, then the vertical pass
static int launch_surface(int format, void* out, const Surface& sf, const Tables& t, const Shape& sh, const YuvCoeffs& q, void* stream,
                          const RollTable* roll) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  (void)hipGetLastError();
  const bool known = with_format(format, [&](auto f) {
    hipLaunchKernelGGL(resample_rows_surface_kernel<decltype(f)::value>, dim3(sh.src_rows, sh.num_images), dim3(kThreads), 0, s,
                       static_cast<unsigned char*>(t.mid), sf, t.kx, t.xlo, t.xn, sh.src_width, sh.src_row0, sh.src_rows, sh.out_width,
                       sh.taps_x, sh.flip, mid_pitch(sh.out_width), q);
  });
  if (!known) return SIMPB_EINVAL;   // (not reached: every entry point has checked `format`)
  return uniform_vertical(out, t, sh, roll, s);
}

extern "C" int simpb_preprocess_u8_nhwc4_f16(void* out, const void* src, void* mid, const int* kx, const int* xlo, const int* xn,
                                             const int* ky, const int* ylo, const int* yn, const void* lut, int num_images,
                                             int src_height, int src_width, int out_height, int out_width, int taps_x, int taps_y,
                                             int src_row0, int src_rows, int flip, int swap_rb, void* stream) {
  const Tables t = {mid, kx, xlo, xn, ky, ylo, yn, lut};
  const Shape sh = {num_images, src_height, src_width, out_height, out_width, taps_x, taps_y, src_row0, src_rows, flip ? 1 : 0,
                    swap_rb ? 1 : 0};
  if (bad_arguments(out, src, t, sh)) return SIMPB_EINVAL;
  const int vec16 = ((size_t)src_width * 3 % 16 == 0 && (reinterpret_cast<size_t>(src) & 15) == 0) ? 1 : 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  (void)hipGetLastError();
  hipLaunchKernelGGL(resample_rows_kernel, dim3(src_rows, num_images), dim3(kThreads), 0, s, static_cast<unsigned char*>(mid),
                     static_cast<const unsigned char*>(src), kx, xlo, xn, src_height, src_width, src_row0, src_rows, out_width,
                     taps_x, sh.flip, mid_pitch(out_width), vec16);
  return uniform_vertical(out, t, sh, nullptr, s);
}

extern "C" int simpb_preprocess_yuv420sp_nhwc4_f16(void* out, const void* src, void* mid, const int* kx, const int* xlo, const int* xn,
                                                   const int* ky, const int* ylo, const int* yn, const void* lut, int num_images,
                                                   int src_height, int src_width, int out_height, int out_width, int taps_x,
                                                   int taps_y, int src_row0, int src_rows, int flip, int swap_rb, int vu_order, int yoff,
                                                   int iy, int irv, int igu, int igv, int ibu, void* stream) {
  const Tables t = {mid, kx, xlo, xn, ky, ylo, yn, lut};
  const Shape sh = {num_images, src_height, src_width, out_height, out_width, taps_x, taps_y, src_row0, src_rows, flip ? 1 : 0,
                    swap_rb ? 1 : 0};
  if (bad_arguments(out, src, t, sh)) return SIMPB_EINVAL;
  if ((src_height & 1) || (src_width & 1) || (vu_order != 0 && vu_order != 1) || iy <= 0) return SIMPB_EINVAL;
  // every luma and chroma row starts on a 16-byte boundary when the width is a multiple of 16 and the first image does
  const int vec16 = (src_width % 16 == 0 && (reinterpret_cast<size_t>(src) & 15) == 0) ? 1 : 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  (void)hipGetLastError();
  const YuvCoeffs q = {yoff, iy, irv, igu, igv, ibu};
  hipLaunchKernelGGL(resample_rows_yuv420sp_kernel, dim3(src_rows, num_images), dim3(kThreads), 0, s, static_cast<unsigned char*>(mid),
                     static_cast<const unsigned char*>(src), kx, xlo, xn, src_height, src_width, src_row0, src_rows, out_width,
                     taps_x, sh.flip, mid_pitch(out_width), vec16, vu_order, q);
  return uniform_vertical(out, t, sh, nullptr, s);
}

// [lo, lo + len) of two ranges overlap
static bool ranges_overlap(long long a, long long alen, long long b, long long blen) { return a < b + blen && b < a + alen; }

// a format code as the planes, roll and rig entry points take it: a format, or one with subsampled 8-bit chroma | kJpeg
static bool known_format(int format) {
  const int base = base_format(format);
  if (!((base >= kBgr && base <= kP010) || (base >= kYuv420p && base <= kRgba) || base == kYuv444p)) return false;
  return format == base || takes_jpeg_chroma(base);
}

// The layout rules of one surface of a known format, shared by every entry point that takes one: the offset one past the
// image's last sample, or -1 for a layout that is refused. The fields a format does not look at are set to 0.
static long long surface_extent(int format, int src_height, int src_width, long long pitch, long long& chroma_pitch,
                                long long& chroma_offset, long long& chroma2_offset, int iy) {
  constexpr long long kMaxPitch = 1LL << 30, kMaxOffset = 1LL << 40;   // (keeps every offset below far inside 63 bits)
  format = base_format(format);   // (interpolated chroma reads the samples of its format, and no others)
  const bool full = format == kYuv444p;   // three planes like planar 4:2:0, the chroma planes as large as the luma plane
  const bool planar = format == kYuv420p || full, semi = format == kNv12 || format == kNv21 || format == kP010;
  const bool ycbcr = planar || semi || format == kYuyv || format == kUyvy;
  const long long pixel = format == kBgr || format == kRgb ? 3 : format == kBgra || format == kRgba ? 4
                          : format == kP010 || format == kYuyv || format == kUyvy ? 2 : 1;
  const long long row = (long long)src_width * pixel;   // sample bytes of a luma (packed) row
  if (pitch < row || pitch > kMaxPitch) return -1;
  if (ycbcr && ((!full && (src_width & 1)) || iy <= 0)) return -1;
  const long long luma_end = (long long)(src_height - 1) * pitch + row;
  if (!planar) chroma2_offset = 0;
  if (!planar && !semi) {
    chroma_pitch = chroma_offset = 0;
    return luma_end;
  }
  if (!full && (src_height & 1)) return -1;
  const long long chroma_row = full ? row : planar ? src_width / 2 : row;   // sample bytes of a chroma row
  if (chroma_pitch < chroma_row || chroma_pitch > kMaxPitch) return -1;
  const long long span = (long long)((full ? src_height : src_height / 2) - 1) * chroma_pitch + chroma_row;
  if (chroma_offset < luma_end || chroma_offset > kMaxOffset) return -1;   // a chroma plane lies behind the luma plane
  if (format == kP010 && ((pitch | chroma_pitch | chroma_offset) & 1)) return -1;
  if (!planar) return chroma_offset + span;
  if (chroma2_offset < luma_end || chroma2_offset > kMaxOffset) return -1;
  if (ranges_overlap(chroma_offset, span, chroma2_offset, span)) return -1;
  return (chroma_offset > chroma2_offset ? chroma_offset : chroma2_offset) + span;
}

// what the surface entry points do behind their own check of `format`: `sf` as the caller gave it (both forms of the images,
// one of them null), checked and set right here (roll: the rolled one's table, or null)
static int preprocess_surface(void* out, Surface sf, int format, const Tables& t, const Shape& sh, const YuvCoeffs& q, void* stream,
                              const RollTable* roll = nullptr) {
  if ((sf.src != nullptr) == (sf.table != nullptr)) return SIMPB_EINVAL;   // exactly one form of the images
  if (bad_arguments(out, sf.src ? static_cast<const void*>(sf.src) : sf.table, t, sh)) return SIMPB_EINVAL;
  if (reinterpret_cast<size_t>(sf.table) & 7) return SIMPB_EINVAL;
  const long long end = surface_extent(format, sh.src_height, sh.src_width, sf.pitch, sf.chroma_pitch, sf.chroma_offset,
                                       sf.chroma2_offset, q.iy);
  if (end < 0) return SIMPB_EINVAL;
  sf.chroma_rows = sh.src_height >> 1;
  if (sf.src) {
    if (sf.image_stride < end || sf.image_stride > (1LL << 40)) return SIMPB_EINVAL;
    if (format == kP010 && ((sf.image_stride | (long long)reinterpret_cast<size_t>(sf.src)) & 1)) return SIMPB_EINVAL;
  } else {
    sf.image_stride = 0;   // (not looked at)
  }
  return launch_surface(format, out, sf, t, sh, q, stream, roll);
}

extern "C" int simpb_preprocess_surface_nhwc4_f16(void* out, const void* src, const void* image_table, void* mid, const int* kx,
                                                  const int* xlo, const int* xn, const int* ky, const int* ylo, const int* yn,
                                                  const void* lut, int num_images, int src_height, int src_width, int out_height,
                                                  int out_width, int taps_x, int taps_y, int src_row0, int src_rows, int flip, int swap_rb,
                                                  int format, long long pitch, long long chroma_pitch, long long chroma_offset,
                                                  long long image_stride, int yoff, int iy, int irv, int igu, int igv, int ibu,
                                                  void* stream) {
  if (format != kBgr && format != kNv12 && format != kNv21 && format != kP010) return SIMPB_EINVAL;
  const Surface sf = {static_cast<const unsigned char*>(src), static_cast<const unsigned long long*>(image_table), image_stride,
                      chroma_offset, pitch, chroma_pitch, 0, 0};
  const Tables t = {mid, kx, xlo, xn, ky, ylo, yn, lut};
  const Shape sh = {num_images, src_height, src_width, out_height, out_width, taps_x, taps_y, src_row0, src_rows, flip ? 1 : 0,
                    swap_rb ? 1 : 0};
  return preprocess_surface(out, sf, format, t, sh, YuvCoeffs{yoff, iy, irv, igu, igv, ibu}, stream);
}

extern "C" int simpb_preprocess_planes_nhwc4_f16(void* out, const void* src, const void* image_table, void* mid, const int* kx,
                                                 const int* xlo, const int* xn, const int* ky, const int* ylo, const int* yn,
                                                 const void* lut, int num_images, int src_height, int src_width, int out_height,
                                                 int out_width, int taps_x, int taps_y, int src_row0, int src_rows, int flip, int swap_rb,
                                                 int format, long long pitch, long long chroma_pitch, long long chroma_offset,
                                                 long long chroma2_offset, long long image_stride, int yoff, int iy, int irv, int igu,
                                                 int igv, int ibu, void* stream) {
  if (!known_format(format)) return SIMPB_EINVAL;
  const Surface sf = {static_cast<const unsigned char*>(src), static_cast<const unsigned long long*>(image_table), image_stride,
                      chroma_offset, pitch, chroma_pitch, chroma2_offset, 0};
  const Tables t = {mid, kx, xlo, xn, ky, ylo, yn, lut};
  const Shape sh = {num_images, src_height, src_width, out_height, out_width, taps_x, taps_y, src_row0, src_rows, flip ? 1 : 0,
                    swap_rb ? 1 : 0};
  return preprocess_surface(out, sf, format, t, sh, YuvCoeffs{yoff, iy, irv, igu, igv, ibu}, stream);
}

// what both rolled entry points refuse on top of their level forms (before any HIP call); `table` takes the rows otherwise
static bool bad_roll(RollTable& table, const int* roll, int roll_cams, int out_height, int out_width) {
  if (!roll || roll_cams < 1 || roll_cams > SIMPB_RIG_MAX_CAMS || out_height > kMaxRollSize || out_width > kMaxRollSize) return true;
  table = RollTable{};
  table.cams = roll_cams;
  for (int i = 0; i < roll_cams * 6; ++i) table.a[i / 6][i % 6] = roll[i];
  return false;
}

extern "C" int simpb_preprocess_roll_nhwc4_f16(void* out, const void* src, const void* image_table, void* mid, const int* kx,
                                               const int* xlo, const int* xn, const int* ky, const int* ylo, const int* yn,
                                               const void* lut, int num_images, int src_height, int src_width, int out_height,
                                               int out_width, int taps_x, int taps_y, int src_row0, int src_rows, int flip, int swap_rb,
                                               int format, long long pitch, long long chroma_pitch, long long chroma_offset,
                                               long long chroma2_offset, long long image_stride, int yoff, int iy, int irv, int igu,
                                               int igv, int ibu, const int* roll, int roll_cams, void* stream) {
  RollTable table;
  if (bad_roll(table, roll, roll_cams, out_height, out_width) || !known_format(format)) return SIMPB_EINVAL;
  const Surface sf = {static_cast<const unsigned char*>(src), static_cast<const unsigned long long*>(image_table), image_stride,
                      chroma_offset, pitch, chroma_pitch, chroma2_offset, 0};
  const Tables t = {mid, kx, xlo, xn, ky, ylo, yn, lut};
  const Shape sh = {num_images, src_height, src_width, out_height, out_width, taps_x, taps_y, src_row0, src_rows, flip ? 1 : 0,
                    swap_rb ? 1 : 0};
  return preprocess_surface(out, sf, format, t, sh, YuvCoeffs{yoff, iy, irv, igu, igv, ibu}, stream, &table);
}

// what both rig entry points do (roll: the rolled one's table, one row per camera, or null)
static int preprocess_rig(void* out, const void* image_table, const Tables& t, const simpb_rig_camera* cams, int num_cams,
                          int num_images, int out_height, int out_width, int kx_len, int x_len, int ky_len, int y_len, int mid_rows,
                          int swap_rb, void* stream, const RollTable* roll) {
  if (!cams || num_cams <= 0 || num_cams > SIMPB_RIG_MAX_CAMS || num_images <= 0 || num_images % num_cams) return SIMPB_EINVAL;
  if (kx_len <= 0 || x_len <= 0 || ky_len <= 0 || y_len <= 0 || mid_rows <= 0) return SIMPB_EINVAL;
  if (reinterpret_cast<size_t>(image_table) & 7) return SIMPB_EINVAL;
  int max_rows = 0;
  for (int i = 0; i < num_cams; ++i) {
    const simpb_rig_camera& c = cams[i];
    // (the rules of simpb_preprocess_surface_nhwc4_f16 in its address-table form, camera by camera)
    const Shape cs = {num_images, c.src_height, c.src_width, out_height, out_width, c.taps_x, c.taps_y, c.src_row0, c.src_rows,
                      c.flip ? 1 : 0, swap_rb ? 1 : 0};
    if (bad_arguments(out, image_table, t, cs)) return SIMPB_EINVAL;
    if (!known_format(c.format)) return SIMPB_EINVAL;
    long long chroma_pitch = c.chroma_pitch, chroma_offset = c.chroma_offset, chroma2_offset = c.chroma2_offset;
    if (surface_extent(c.format, c.src_height, c.src_width, c.pitch, chroma_pitch, chroma_offset, chroma2_offset, c.iy) < 0)
      return SIMPB_EINVAL;
    // the camera's tables and intermediate rows lie inside the arrays given ...
    if (c.kx_offset < 0 || c.x_offset < 0 || c.ky_offset < 0 || c.y_offset < 0 || c.mid_row < 0) return SIMPB_EINVAL;
    if ((long long)c.kx_offset + (long long)out_width * c.taps_x > kx_len || (long long)c.x_offset + out_width > x_len ||
        (long long)c.ky_offset + (long long)out_height * c.taps_y > ky_len || (long long)c.y_offset + out_height > y_len ||
        (long long)c.mid_row + c.src_rows > mid_rows)
      return SIMPB_EINVAL;
    // ... and apart from every other camera's
    for (int j = 0; j < i; ++j) {
      const simpb_rig_camera& d = cams[j];
      if (ranges_overlap(c.kx_offset, (long long)out_width * c.taps_x, d.kx_offset, (long long)out_width * d.taps_x) ||
          ranges_overlap(c.x_offset, out_width, d.x_offset, out_width) ||
          ranges_overlap(c.ky_offset, (long long)out_height * c.taps_y, d.ky_offset, (long long)out_height * d.taps_y) ||
          ranges_overlap(c.y_offset, out_height, d.y_offset, out_height) || ranges_overlap(c.mid_row, c.src_rows, d.mid_row, d.src_rows))
        return SIMPB_EINVAL;
    }
    max_rows = c.src_rows > max_rows ? c.src_rows : max_rows;
  }
  const unsigned long long* table = static_cast<const unsigned long long*>(image_table);
  Rig rig = {};
  for (int i = 0; i < num_cams; ++i) {
    rig.cam[i] = cams[i];
    rig.cam[i].flip = cams[i].flip ? 1 : 0;
  }
  const int pitch = mid_pitch(out_width);
  // LDS for the rig at hand (validated above: at most kMaxSrcW * 3 + kMaxOutW * 3 + 16 + 2 * kMaxSrcW * 2 = 34832 bytes; a 4-byte
  // row of the widest source is as long as the two P010 planes of one)
  // (behind the two planes, the far chroma row of the widest camera that stages one: at most kMaxSrcW bytes more)
  int src_bytes = 0, planes = 0, far_bytes = 0;
  for (int i = 0; i < num_cams; ++i) {
    const int plane = plane_bytes(cams[i].format, cams[i].src_width);
    src_bytes = cams[i].src_width * 3 > src_bytes ? cams[i].src_width * 3 : src_bytes;
    planes = plane > planes ? plane : planes;
    if (far_plane(cams[i].format) && plane > far_bytes) far_bytes = plane;
  }
  const RigLds lds = {(src_bytes + 15) / 16 * 16, pitch + 16, planes};
  hipStream_t s = static_cast<hipStream_t>(stream);
  (void)hipGetLastError();
  hipLaunchKernelGGL(resample_rows_rig_kernel, dim3(max_rows, num_images), dim3(kThreads),
                     (size_t)(lds.src_bytes + lds.out_bytes + 2 * lds.plane_bytes + far_bytes), s, static_cast<unsigned char*>(t.mid), table, rig,
                     num_cams, t.kx, t.xlo, t.xn, out_width, pitch, mid_rows, lds);
  return launch_vertical(num_images, out_height, out_width, roll, [&](dim3 grid, dim3 block, auto r) {
    hipLaunchKernelGGL(resample_cols_lut_rig_kernel<decltype(r)>, grid, block, 0, s, static_cast<_Float16*>(out),
                       static_cast<const unsigned char*>(t.mid), table, rig, num_cams, t.ky, t.ylo, t.yn,
                       static_cast<const _Float16*>(t.lut), out_height, out_width, swap_rb ? 1 : 0, pitch, mid_rows, r);
  });
}

extern "C" int simpb_preprocess_rig_nhwc4_f16(void* out, const void* image_table, void* mid, const int* kx, const int* xlo,
                                              const int* xn, const int* ky, const int* ylo, const int* yn, const void* lut,
                                              const simpb_rig_camera* cams, int num_cams, int num_images, int out_height,
                                              int out_width, int kx_len, int x_len, int ky_len, int y_len, int mid_rows, int swap_rb,
                                              void* stream) {
  const Tables t = {mid, kx, xlo, xn, ky, ylo, yn, lut};
  return preprocess_rig(out, image_table, t, cams, num_cams, num_images, out_height, out_width, kx_len, x_len, ky_len, y_len, mid_rows,
                        swap_rb, stream, nullptr);
}

extern "C" int simpb_preprocess_rig_roll_nhwc4_f16(void* out, const void* image_table, void* mid, const int* kx, const int* xlo,
                                                   const int* xn, const int* ky, const int* ylo, const int* yn, const void* lut,
                                                   const simpb_rig_camera* cams, int num_cams, int num_images, int out_height,
                                                   int out_width, int kx_len, int x_len, int ky_len, int y_len, int mid_rows,
                                                   int swap_rb, const int* roll, void* stream) {
  RollTable table;
  if (bad_roll(table, roll, num_cams, out_height, out_width)) return SIMPB_EINVAL;
  const Tables t = {mid, kx, xlo, xn, ky, ylo, yn, lut};
  return preprocess_rig(out, image_table, t, cams, num_cams, num_images, out_height, out_width, kx_len, x_len, ky_len, y_len, mid_rows,
                        swap_rb, stream, &table);
}
