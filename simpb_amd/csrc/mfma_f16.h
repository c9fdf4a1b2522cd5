// FP16 matrix-core step used by conv1x1.hip, linear_split.hip and the split-fp16 variant of gemm.hip:
// D[32x32] += A[32x16] . B[16x32], fp32 accumulate, lane (r32, kb) holding k = 8*kb .. 8*kb+7 of its row/column.
//
// gfx950 has this as ONE instruction, v_mfma_f32_32x32x16_f16 (twice the K of gfx942's 32x32x8). Round 2 measurement
// (tools/daf_stress.py, profiles/r02_mfma_x16_interference/): while any wave of the chip executes that instruction,
// OTHER kernels' plain vector arithmetic goes wrong in lanes 48-63 of a wave now and then -- daf_fwd_rows beside a loop of
// conv1x1 or linear_split: 90-97 % of its launches return wrong channels 192-255 for ~10 anchors; beside fp32-MFMA
// kernels (linear_f32, hipBLASLt), MIOpen's fp16 3x3 convolution, copies or elementwise kernels: 0 of 1 500. This is
// what the "eager two-stream fault" of round 1 was. A register-only burner (tools/mfma_burn.hip) shows the same for all four
// double-K 16-bit instructions gfx950 adds (f16 / bf16, 32x32x16 / 16x16x32) and for none of the older ones. The same product as TWO v_mfma_f32_32x32x8f16 steps (each lane's
// eight k-values split into its low and high four: both operands use the same lane -> k map, so the products pair up
// and only the summation order changes) does not disturb other waves. SIMPB_MFMA_F16_K16=1 selects the single
// instruction again (for the measurement above, never for the product).
#pragma once
#include <hip/hip_runtime.h>

namespace simpb {

typedef _Float16 h16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 h16x4_t __attribute__((ext_vector_type(4)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));

#ifndef SIMPB_MFMA_F16_K16
#define SIMPB_MFMA_F16_K16 0
#endif

template <class A8, class C16>
__device__ __forceinline__ C16 mfma_32x32x16_f16(const A8& a, const A8& b, const C16& c) {
#if SIMPB_MFMA_F16_K16
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
#else
  const h16x4_t a0 = {a[0], a[1], a[2], a[3]}, a1 = {a[4], a[5], a[6], a[7]};
  const h16x4_t b0 = {b[0], b[1], b[2], b[3]}, b1 = {b[4], b[5], b[6], b[7]};
  C16 d = __builtin_amdgcn_mfma_f32_32x32x8f16(a0, b0, c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x8f16(a1, b1, d, 0, 0, 0);
#endif
}

// C/D layout of the 32x32 tile: register r of lane (column lane & 31, half = lane >> 5) holds this row
__device__ __forceinline__ constexpr int acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// Workgroups are numbered so that each XCD (blockIdx.x % 8) walks a contiguous range of `per_xcd` tiles: neighbouring
// tiles share operand rows in that XCD's L2. The tile of this workgroup, or -1 past the last of `total`.
__device__ __forceinline__ int xcd_tile(int per_xcd, int total) {
  const int tile = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
  return ((int)(blockIdx.x >> 3) >= per_xcd || tile >= total) ? -1 : tile;
}

// THE split of the split-operand kernels: s = h + l / 2^11. The trailing part is kept scaled by 2^11 so that it stays a
// normal half (no dependence on how the matrix pipe treats fp16 subnormals). plugin/dense.py _split_weights is its host twin.
__device__ __forceinline__ void split_halfs(float s, _Float16& h, _Float16& l) {
  h = (_Float16)s;
  l = (_Float16)((s - (float)h) * 2048.f);
}

// Range window of the split operands x = half(x) + half((x - half(x)) * 2^11) / 2^11 (csrc/gemm.hip, csrc/linear_split.hip):
// a row whose largest |x| lies in [2^-10, 2^15) (or is 0) splits to 22 bits as it is; any other finite row is staged as
// x * 2^-e with e = split_row_exp, and its sum multiplied by 2^e. (NaN / inf: nothing to gain, e = 0.)
__device__ __forceinline__ bool split_row_outside(float m) {   // m = largest |x| of a row
  return (m >= 32768.f && m <= 3.402823466e38f) || (m > 0.f && m < 0.0009765625f);
}
__device__ __forceinline__ int split_row_exp(float m) {
  return split_row_outside(m) ? __builtin_amdgcn_frexp_expf(m) - 1 : 0;   // m * 2^-e in [1, 2)
}

// One element of x while it is staged. First pass (kScaled = false): split as it is and collect the largest |x| of the
// row in `xmax`; second pass: split x * 2^-e, e the row's exponent.
template <bool kScaled>
__device__ __forceinline__ void split_staged(float s, int e, float& xmax, _Float16& h, _Float16& l) {
  if constexpr (kScaled) s = __builtin_amdgcn_ldexpf(s, -e);
  else xmax = fmaxf(xmax, fabsf(s));
  split_halfs(s, h, l);
}

// After the first pass: does this workgroup need the second one? Each thread staged NR rows (tile rows row + step * i),
// LANES consecutive lanes of a wave sharing a row; they meet on the row's largest |x|. The flag is a plain LDS word
// (zeroed before the first pass, whose barriers order that) behind a barrier the epilogue needs anyway. When a row lies
// outside the window, every row's exponent goes to `xe` and, from the lane with `writer`, to s_rowexp; it reaches the
// epilogue through the second pass's barriers. The answer is workgroup-uniform.
template <int LANES, int NR>
__device__ __forceinline__ bool split_needs_second_pass(float (&xmax)[NR], int (&xe)[NR], int& s_any, int* s_rowexp,
                                                        int row, int step, bool writer) {
#pragma unroll
  for (int i = 0; i < NR; ++i) {
#pragma unroll
    for (int m = 1; m < LANES; m <<= 1) xmax[i] = fmaxf(xmax[i], __shfl_xor(xmax[i], m));
    if (split_row_outside(xmax[i])) s_any = 1;
  }
  __syncthreads();
  const bool scaled = s_any != 0;
  if (scaled) {
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      xe[i] = split_row_exp(xmax[i]);
      if (writer) s_rowexp[row + step * i] = xe[i];
    }
  }
  return scaled;
}

}  // namespace simpb
