// Parts that the deformable samplers share, each written once (csrc/deform_agg.hip, deform_agg_fused.hip, deform_agg_bwd.hip,
// dfa_prep.hip, msda.hip, msda_lin.hip, msda_bwd.hip and msda_prep_kernel of rowops.hip):
//   kWaves / kThreads      the workgroup of the row kernels: 4 waves, one per level
//   Bilinear               fractions, clamped corners and tap-valid flags of one location on one map, filled by
//     taps_gated             the 3D rule (double 0.5, plain conversion, one-sided tests: the caller has passed the gate)
//     taps_free              the 2D rule (float 0.5f, clamped conversion, two-sided tests: any location, infinities too)
//   tap_weights            the four forward tap weights, zero where the tap is outside: scale * hh * hw, ...
//   Tap4, ld_row, issue_taps<FEAT>, tap_sum, accumulate     one sample of the 3D gather: 4 row loads in flight, then consumed
//                          by a sum whose every rounding is stated
//   in_image, RowLocations, load_locations, pop_sample, sample_location     the gate and the ballot walk of a row's samples
//   gather_levels<BATCH>   the 3D gather walk of a wave over its levels and the row's valid samples
//   meet_and_store         the four waves' partial rows meet in LDS, one store per channel
//   key_point, project     key point of an anchor and its projection into a camera (dfa_points_kernel, daf_fused_rows)
//   msda_operand<LP>       softmax over LP neighbouring lanes and reference point + offset / (W_l, H_l)
// NOT merged, on purpose:
//   * the two pixel rules: (float)((double)(l * size) - 0.5) rounds differently from l * size - 0.5f at a few inputs, the
//     reference has each (deformable_aggregation_cuda.cu:180-181, mmcv's ms_deform_attn), and one body that branches on its
//     caller is not simpler than two of twelve lines;
//   * the weight softmax of dfa_weights_kernel (an LDS tree over any layout) and of daf_fused_rows (shuffles over a
//     compile-time layout): different algorithms with different summation trees, and the tests use the three-launch route
//     as the reference for the fused one.
// What was measured about sharing them: profiles/sampler_shared_parts.md.
#pragma once
#include <hip/hip_runtime.h>

namespace simpb {
namespace sampler {

constexpr int kWaves = 4;
constexpr int kThreads = kWaves * 64;

// ---- one location on one H x W map. Tap k = 2 * row + column: (y0, x0), (y0, x1), (y1, x0), (y1, x1).
struct Bilinear {
  float lh, lw, hh, hw;   // fractions towards the lower row / right column, and 1 - them
  int y0, y1, x0, x1;     // the corner coordinates clamped into the map: an invalid tap still has a valid address
  bool in[4];             // tap k lies inside the map
  __device__ __forceinline__ int pixel(int k, int W) const { return ((k & 2) ? y1 : y0) * W + ((k & 1) ? x1 : x0); }
};

// 3D rule (deformable_aggregation_cuda.cu:180-181 with :35-53): the 0.5 is a double literal there. Only for locations
// inside (0, 1): the conversion to int is not clamped.
__device__ __forceinline__ Bilinear taps_gated(float lx, float ly, int H, int W) {
  Bilinear b;
  const float h_im = (float)((double)(ly * (float)H) - 0.5);
  const float w_im = (float)((double)(lx * (float)W) - 0.5);
  const float hf = floorf(h_im), wf = floorf(w_im);
  const int h0 = (int)hf, w0 = (int)wf;
  b.lh = h_im - hf; b.lw = w_im - wf;
  b.hh = 1.f - b.lh; b.hw = 1.f - b.lw;
  const bool y0 = h0 >= 0, y1 = h0 + 1 <= H - 1, x0 = w0 >= 0, x1 = w0 + 1 <= W - 1;
  b.y0 = max(h0, 0); b.y1 = min(h0 + 1, H - 1); b.x0 = max(w0, 0); b.x1 = min(w0 + 1, W - 1);
  b.in[0] = y0 && x0; b.in[1] = y0 && x1; b.in[2] = y1 && x0; b.in[3] = y1 && x1;
  return b;
}

// 2D rule (mmcv's CUDA op = grid_sample(bilinear, zeros, align_corners=False)): any location.
__device__ __forceinline__ Bilinear taps_free(float lx, float ly, int H, int W) {
  Bilinear b;
  const float h_im = ly * (float)H - 0.5f;
  const float w_im = lx * (float)W - 0.5f;
  const float hf = floorf(h_im), wf = floorf(w_im);
  // far-away locations: keep the int conversion defined, every tap ends up invalid anyway
  const int h0 = (int)fminf(fmaxf(hf, -2.f), (float)H);
  const int w0 = (int)fminf(fmaxf(wf, -2.f), (float)W);
  b.lh = h_im - hf; b.lw = w_im - wf;
  b.hh = 1.f - b.lh; b.hw = 1.f - b.lw;
  const bool y0 = h0 >= 0 && h0 <= H - 1, y1 = h0 + 1 >= 0 && h0 + 1 <= H - 1;
  const bool x0 = w0 >= 0 && w0 <= W - 1, x1 = w0 + 1 >= 0 && w0 + 1 <= W - 1;
  b.y0 = min(max(h0, 0), H - 1); b.y1 = min(max(h0 + 1, 0), H - 1);
  b.x0 = min(max(w0, 0), W - 1); b.x1 = min(max(w0 + 1, 0), W - 1);
  b.in[0] = y0 && x0; b.in[1] = y0 && x1; b.in[2] = y1 && x0; b.in[3] = y1 && x1;
  return b;
}

// Forward tap weights, multiplied left to right: scale * hh * hw (3D: scale = 1, which changes no bit; 2D: the attention
// weight). Taps outside the map get weight zero, so their (clamped) loads carry no branch.
__device__ __forceinline__ void tap_weights(float (&w)[4], const Bilinear& b, float scale = 1.f) {
  w[0] = b.in[0] ? scale * b.hh * b.hw : 0.f;
  w[1] = b.in[1] ? scale * b.hh * b.lw : 0.f;
  w[2] = b.in[2] ? scale * b.lh * b.hw : 0.f;
  w[3] = b.in[3] ? scale * b.lh * b.lw : 0.f;
}

// ---- one sample of the 3D gather: a lane's 4 channels of the 4 taps, and the tap weights
struct Tap4 {
  float4 v[4];
  float w[4];
};

__device__ __forceinline__ float4 ld_row(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 ld_row(const _Float16* p) {
  typedef _Float16 h4 __attribute__((ext_vector_type(4)));
  const h4 v = *reinterpret_cast<const h4*>(p);
  return make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
}

// Issue the 4 tap loads of one sample. Taps outside the map are redirected to a clamped (valid) address and their weight
// is zeroed, so the loads carry no branch and can all be in flight.
template <class FEAT>
__device__ __forceinline__ void issue_taps(Tap4& t, const FEAT* __restrict__ base, int H, int W, int C, float lx, float ly,
                                           int coff) {
  const Bilinear b = taps_gated(lx, ly, H, W);
  tap_weights(t.w, b);
#pragma unroll
  for (int k = 0; k < 4; ++k) t.v[k] = ld_row(base + (size_t)b.pixel(k, W) * C + coff);
}

// acc + wgt * (w0 v0 + w1 v1 + w2 v2 + w3 v3) of the 3D kernels, with every rounding stated. As a plain expression the
// compiler was free to choose which product stays a multiply and which become fused multiply-adds, and it chose by the
// code around the expression (the outputs are compared bit for bit between builds: tools/sampler_bits.py). The order the
// kernels have always had: w1 v1 rounded, then + w0 v0, + w2 v2, + w3 v3 and + acc, one fma each. FROM00: w0 v0 is the
// rounded product and w1 v1 the first fma (what the second sample of daf_fwd_rows' pairs always had).
template <bool FROM00 = false>
__device__ __forceinline__ float tap_sum(float acc, float wgt, const float (&w)[4], float v0, float v1, float v2, float v3) {
  float s = FROM00 ? fmaf(w[1], v1, w[0] * v0) : fmaf(w[0], v0, w[1] * v1);
  s = fmaf(w[2], v2, s);
  s = fmaf(w[3], v3, s);
  return fmaf(wgt, s, acc);
}

template <bool FROM00 = false>
__device__ __forceinline__ void accumulate(float4& acc, const Tap4& t, float wgt) {
  acc.x = tap_sum<FROM00>(acc.x, wgt, t.w, t.v[0].x, t.v[1].x, t.v[2].x, t.v[3].x);
  acc.y = tap_sum<FROM00>(acc.y, wgt, t.w, t.v[0].y, t.v[1].y, t.v[2].y, t.v[3].y);
  acc.z = tap_sum<FROM00>(acc.z, wgt, t.w, t.v[0].z, t.v[1].z, t.v[2].z, t.v[3].z);
  acc.w = tap_sum<FROM00>(acc.w, wgt, t.w, t.v[0].w, t.v[1].w, t.v[2].w, t.v[3].w);
}

// ---- the sampling locations of one (batch, anchor) row, up to 128 of them, held by EVERY wave: two ballots, no LDS, no
// barrier, and the valid ones are walked with scalar bit scans.
__device__ __forceinline__ bool in_image(float2 l) { return l.x > 0.f && l.x < 1.f && l.y > 0.f && l.y < 1.f; }   // cu:169-171

struct RowLocations {
  float2 l0, l1;               // lane i holds locations i and i + 64; (-1, -1) past the end of the row
  unsigned long long m0, m1;   // bit i: location i / i + 64 passes the gate
};

// `src` holds n <= 128 locations (global memory, or LDS padded to 128); on0 / on1 = false drops the lane's pair whatever it
// holds (a masked camera).
__device__ __forceinline__ RowLocations load_locations(const float2* src, int lane, int n, bool on0 = true, bool on1 = true) {
  RowLocations r;
  r.l0 = r.l1 = make_float2(-1.f, -1.f);
  if (lane < n) r.l0 = src[lane];
  if (lane + 64 < n) r.l1 = src[lane + 64];
  r.m0 = __ballot(on0 && in_image(r.l0));
  r.m1 = __ballot(on1 && in_image(r.l1));
  return r;
}

// index of the next valid sample in ascending order, -1 when none is left
__device__ __forceinline__ int pop_sample(unsigned long long& ma, unsigned long long& mb) {
  int i = -1;
  if (ma) { i = __builtin_ctzll(ma); ma &= ma - 1; }
  else if (mb) { i = 64 + __builtin_ctzll(mb); mb &= mb - 1; }
  return i;
}

// location i (wave-uniform) broadcast from the lane that holds it
__device__ __forceinline__ float2 sample_location(const RowLocations& r, int i) {
  return make_float2(i < 64 ? __shfl(r.l0.x, i) : __shfl(r.l1.x, i - 64), i < 64 ? __shfl(r.l0.y, i) : __shfl(r.l1.y, i - 64));
}

// ---- the 3D gather walk of one wave: levels wave, wave + 4, ...; within a level the row's valid samples in ascending
// order, BATCH of them (x 4 taps) requested before any is consumed, so a trip of the inner loop is one memory round trip.
// Sample i belongs to camera i % cams. weight(i, lvl) is the caller's weight of (sample, level) for this lane's group.
// FROM00: bit j set = the j-th sample of a batch is summed by accumulate<true>.
template <int BATCH, unsigned FROM00 = 0u, class FEAT, class Weight>
__device__ __forceinline__ void gather_levels(float4& acc, const RowLocations& r, const FEAT* __restrict__ featb,
                                              const int* __restrict__ spatial_shape, const int* __restrict__ scale_start,
                                              int cams, int L, int C, int ld_off, int wave, Weight weight) {
  for (int lvl = wave; lvl < L; lvl += kWaves) {
    unsigned long long ma = r.m0, mb = r.m1;
    while (ma | mb) {
      int idx[BATCH];
#pragma unroll
      for (int j = 0; j < BATCH; ++j) idx[j] = pop_sample(ma, mb);
      Tap4 t[BATCH];
      float wg[BATCH];
#pragma unroll
      for (int j = 0; j < BATCH; ++j) {
        wg[j] = 0.f;
        if (j == 0 || idx[j] >= 0) {   // wave-uniform; the first sample of a trip exists (the loop's condition)
          const int i = idx[j];
          const float2 l = sample_location(r, i);
          const int cs = (i % cams) * L + lvl;
          issue_taps(t[j], featb + (size_t)scale_start[cs] * C, spatial_shape[2 * cs], spatial_shape[2 * cs + 1], C, l.x, l.y,
                     ld_off);
          wg[j] = weight(i, lvl);
        }
      }
#pragma unroll
      for (int j = 0; j < BATCH; ++j)
        if (j == 0 || idx[j] >= 0) {
          if ((FROM00 >> j) & 1u) accumulate<true>(acc, t[j], wg[j]);
          else accumulate<false>(acc, t[j], wg[j]);
        }
    }
  }
}

// ---- the 4 waves meet once in LDS and the row is written once -> deterministic. 256 threads, one channel each: thread t
// sums component (t & 3) of lane (t >> 2) over the waves and stores channel first + t of the row if it is below n. A caller
// that comes back for another 256 channels puts a barrier in front.
__device__ __forceinline__ void meet_and_store(float4 (&s_red)[kWaves][64], const float4& acc, int wave, int lane,
                                               float* __restrict__ row, int first, int n) {
  s_red[wave][lane] = acc;
  __syncthreads();
  const int c = first + threadIdx.x;
  if (c < n) {
    const float* r = reinterpret_cast<const float*>(s_red);
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s += r[w * 256 + threadIdx.x];
    row[c] = s;
  }
}

// ---- SparseBox3DKeyPointsGenerator.forward (detection3d/blocks.py:181-222) for one key point: av = the anchor's first 8
// values (centre, log sizes, sin / cos of yaw); f = a fix_scale row (fixed) or raw learnable offsets (sigmoid applied here).
__device__ __forceinline__ float3 key_point(const float (&av)[8], float f0, float f1, float f2, bool fixed) {
  const float sw = expf(av[3]), sl = expf(av[4]), sh = expf(av[5]);
  float kx, ky, kz;
  if (fixed) {
    kx = f0 * sw; ky = f1 * sl; kz = f2 * sh;
  } else {
    kx = (1.f / (1.f + expf(-f0)) - 0.5f) * sw;
    ky = (1.f / (1.f + expf(-f1)) - 0.5f) * sl;
    kz = (1.f / (1.f + expf(-f2)) - 0.5f) * sh;
  }
  const float sn = av[6], cs = av[7];
  return make_float3(cs * kx - sn * ky + av[0], sn * kx + cs * ky + av[1], kz + av[2]);
}

// DeformableFeatureAggregation.project_points (models/blocks.py:198-213): m = the first three rows of the camera's
// matrix, (w0, w1) = the image's width and height.
__device__ __forceinline__ float2 project(const float (&m)[12], const float3& p, float w0, float w1) {
  const float u = m[0] * p.x + m[1] * p.y + m[2] * p.z + m[3];
  const float v = m[4] * p.x + m[5] * p.y + m[6] * p.z + m[7];
  const float d = fmaxf(m[8] * p.x + m[9] * p.y + m[10] * p.z + m[11], 1e-5f);
  return make_float2(u / d / w0, v / d / w1);
}

// ---- operands of the 2D sampler from the fused projection (group_attn.py:181-201), one lane per (head, level, point):
// softmax of the logit over the LP neighbouring lanes (xor shuffles LP/2 .. 1, max then sum) and location = reference point
// + offset / (W_l, H_l). live = false: the lane's exp counts as 0 (its logit should be -inf).
struct MsdaOperand {
  float x, y, a;
};
template <int LP>
__device__ __forceinline__ MsdaOperand msda_operand(float lg, float ox, float oy, float rx, float ry, float wl, float hl,
                                                    bool live = true) {
  float mx = lg;
#pragma unroll
  for (int m = LP / 2; m >= 1; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
  const float ex = live ? expf(lg - mx) : 0.f;
  float sum = ex;
#pragma unroll
  for (int m = LP / 2; m >= 1; m >>= 1) sum += __shfl_xor(sum, m);
  return {rx + ox / wl, ry + oy / hl, ex / sum};
}

}  // namespace sampler
}  // namespace simpb
