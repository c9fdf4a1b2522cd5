// Camera frame ingest (gfx950): raw u8 [N, Hs, Ws, 3] frames as an image decoder delivers them -> the stem's operand, f16
// [N, h, w, 4] with channel 3 = 0 (what simpb_stem_conv7x7_pool_f16 reads). It replaces the reference's test pipeline on
// the host, ResizeCropFlipImage (datasets/pipelines/augment.py:86-106: PIL resize + crop + left-right flip) and
// NormalizeMultiviewImage (transform_3d.py:438-466), and the fp32 cast pass of csrc/stem.hip behind it.
//
// The resize is Pillow's 8-bit resampler restated: integer coefficients with 22 fractional bits (computed by the host in
// float64, simpb_amd/preprocess.py), a horizontal pass whose results are rounded and clamped to u8, then a vertical pass
// over those u8 values with the same rule. All arithmetic is int32, so the result is Pillow's byte for byte. Crop and flip
// are index arithmetic: only the kept columns and the source rows the kept output rows need are ever computed. Channel
// order, mean / std and the f16 rounding sit in a [3][256] table made by the host, so that no floating-point
// instruction (and no contraction rule of the compiler) enters the result.
//
// Two launches with a u8 intermediate [N, rows, pitch] in HBM (1.2 MB per camera at 1600 x 900 -> 704 x 256):
//   1. horizontal: one workgroup per (needed source row, image). The row (Ws x 3 bytes) is staged in LDS in 16-byte chunks
//      (neighbouring output columns share almost all of their taps), a thread makes whole output pixels, the resampled row
//      goes through LDS again and leaves as 16-byte chunks.
//   2. vertical + table: a thread owns 4 neighbouring output pixels = 12 intermediate bytes per tap row (three aligned
//      dwords), and writes them as two 16-byte stores.
// Every load of a thread is retired before its stores are issued (store_fence.h).
#include <hip/hip_runtime.h>
#include "../../include/simpb_hip.h"
#include "store_fence.h"

extern "C" int simpb_check_launch(void);

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));

constexpr int kThreads = 256;
constexpr int kMaxSrcW = 4096;    // staged source row: 12 KB
constexpr int kMaxOutW = 2048;    // staged resampled row: 6 KB
constexpr int kMaxTaps = SIMPB_PREPROCESS_MAX_TAPS;
constexpr int kPrecision = 22;

__device__ __forceinline__ int clip8(int acc) { return min(max(acc >> kPrecision, 0), 255); }

// mid[n][r][j][c] = clip8(2^21 + sum_t src[n][row0 + r][xlo[jj] + t][c] * kx[jj][t]),  jj = flip ? w - 1 - j : j
__global__ __launch_bounds__(kThreads) void resample_rows_kernel(unsigned char* __restrict__ mid, const unsigned char* __restrict__ src,
                                                                 const int* __restrict__ kx, const int* __restrict__ xlo,
                                                                 const int* __restrict__ xn, int Hs, int Ws, int row0, int rows,
                                                                 int w, int taps, int flip, int pitch, int vec16) {
  __shared__ __attribute__((aligned(16))) unsigned char s_src[kMaxSrcW * 3];
  __shared__ __attribute__((aligned(16))) unsigned char s_out[kMaxOutW * 3 + 16];
  const int tid = threadIdx.x, r = blockIdx.x, n = blockIdx.y;
  const size_t row_bytes = (size_t)Ws * 3;
  const unsigned char* p = src + ((size_t)n * Hs + row0 + r) * row_bytes;
  if (vec16) {
    const uint4* p16 = reinterpret_cast<const uint4*>(p);
    uint4* s16 = reinterpret_cast<uint4*>(s_src);
    for (int i = tid; i < (int)(row_bytes >> 4); i += kThreads) s16[i] = p16[i];
  } else {
    for (int i = tid; i < (int)row_bytes; i += kThreads) s_src[i] = p[i];
  }
  __syncthreads();
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
      v0 = clip8(a0); v1 = clip8(a1); v2 = clip8(a2);
    }
    s_out[j * 3] = (unsigned char)v0;
    s_out[j * 3 + 1] = (unsigned char)v1;
    s_out[j * 3 + 2] = (unsigned char)v2;
  }
  for (int i = wpad * 3 + tid; i < pitch; i += kThreads) s_out[i] = 0;
  simpb::loads_retired();
  __syncthreads();
  uint4* o16 = reinterpret_cast<uint4*>(mid + ((size_t)n * rows + r) * pitch);   // pitch % 16 == 0, mid 16-byte aligned
  const uint4* s16 = reinterpret_cast<const uint4*>(s_out);
  for (int i = tid; i < (pitch >> 4); i += kThreads) o16[i] = s16[i];
}

// out[n][y][x][c] = lut[c][clip8(2^21 + sum_t mid[n][ylo[y] - row0 + t][x][swap ? 2 - c : c] * ky[y][t])], out[..][3] = 0
__global__ __launch_bounds__(kThreads) void resample_cols_lut_kernel(_Float16* __restrict__ out, const unsigned char* __restrict__ mid,
                                                                     const int* __restrict__ ky, const int* __restrict__ ylo,
                                                                     const int* __restrict__ yn, const _Float16* __restrict__ lut,
                                                                     int row0, int rows, int h, int w, int taps, int swap_rb, int pitch) {
  __shared__ _Float16 s_lut[3 * 256];
  __shared__ int s_k[kMaxTaps];
  const int tid = threadIdx.x, y = blockIdx.y, n = blockIdx.z;
  for (int i = tid; i < 3 * 256; i += kThreads) s_lut[i] = lut[i];
  const int cnt = min(min(yn[y], taps), rows);
  if (tid < cnt) s_k[tid] = ky[(size_t)y * taps + tid];
  __syncthreads();
  const int g = blockIdx.x * kThreads + tid;   // group of 4 output pixels
  if (4 * g >= w) return;
  const int first = min(max(ylo[y] - row0, 0), rows - cnt);   // (clamped like the horizontal pass: never outside `mid`)
  const unsigned int* p = reinterpret_cast<const unsigned int*>(mid + ((size_t)n * rows + first) * pitch) + 3 * g;
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
  h8 v[2];
#pragma unroll
  for (int px = 0; px < 4; ++px) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int ci = swap_rb ? 2 - c : c;
      v[px >> 1][(px & 1) * 4 + c] = s_lut[c * 256 + clip8(acc[px * 3 + ci])];
    }
    v[px >> 1][(px & 1) * 4 + 3] = (_Float16)0.f;
  }
  simpb::pin(v[0]);
  simpb::pin(v[1]);
  simpb::loads_retired();
  _Float16* o = out + (((size_t)n * h + y) * w + 4 * g) * 4;
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

}  // namespace

// bytes of one intermediate row: whole groups of 4 pixels, rounded up to 16 bytes
static int mid_pitch(int out_width) { return ((out_width + 3) / 4 * 12 + 15) / 16 * 16; }

extern "C" int simpb_preprocess_mid_pitch(int out_width) {
  return (out_width <= 0 || out_width > kMaxOutW) ? 0 : mid_pitch(out_width);
}

extern "C" int simpb_preprocess_u8_nhwc4_f16(void* out, const void* src, void* mid, const int* kx, const int* xlo, const int* xn,
                                             const int* ky, const int* ylo, const int* yn, const void* lut, int num_images,
                                             int src_height, int src_width, int out_height, int out_width, int taps_x, int taps_y,
                                             int src_row0, int src_rows, int flip, int swap_rb, void* stream) {
  if (!out || !src || !mid || !kx || !xlo || !xn || !ky || !ylo || !yn || !lut) return SIMPB_EINVAL;
  if (num_images <= 0 || num_images > 65535 || src_height <= 0 || src_width <= 0 || out_height <= 0 || out_width <= 0 ||
      out_height > 65535 || src_width > kMaxSrcW || out_width > kMaxOutW)
    return SIMPB_EINVAL;
  if (taps_x <= 0 || taps_y <= 0 || taps_x > kMaxTaps || taps_y > kMaxTaps) return SIMPB_EINVAL;
  if (src_row0 < 0 || src_rows <= 0 || (long long)src_row0 + src_rows > src_height) return SIMPB_EINVAL;
  if ((reinterpret_cast<size_t>(out) | reinterpret_cast<size_t>(mid)) & 15) return SIMPB_EINVAL;
  if ((reinterpret_cast<size_t>(kx) | reinterpret_cast<size_t>(xlo) | reinterpret_cast<size_t>(xn) | reinterpret_cast<size_t>(ky) |
       reinterpret_cast<size_t>(ylo) | reinterpret_cast<size_t>(yn)) & 3)
    return SIMPB_EINVAL;
  if (reinterpret_cast<size_t>(lut) & 1) return SIMPB_EINVAL;
  const int pitch = mid_pitch(out_width);
  const int vec16 = ((size_t)src_width * 3 % 16 == 0 && (reinterpret_cast<size_t>(src) & 15) == 0) ? 1 : 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  (void)hipGetLastError();
  hipLaunchKernelGGL(resample_rows_kernel, dim3(src_rows, num_images), dim3(kThreads), 0, s, static_cast<unsigned char*>(mid),
                     static_cast<const unsigned char*>(src), kx, xlo, xn, src_height, src_width, src_row0, src_rows, out_width,
                     taps_x, flip ? 1 : 0, pitch, vec16);
  const int groups = (out_width + 3) / 4;
  hipLaunchKernelGGL(resample_cols_lut_kernel, dim3((groups + kThreads - 1) / kThreads, out_height, num_images), dim3(kThreads), 0, s,
                     static_cast<_Float16*>(out), static_cast<const unsigned char*>(mid), ky, ylo, yn,
                     static_cast<const _Float16*>(lut), src_row0, src_rows, out_height, out_width, taps_y, swap_rb ? 1 : 0, pitch);
  return simpb_check_launch();
}
