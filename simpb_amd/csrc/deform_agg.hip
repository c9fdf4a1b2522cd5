// 3D deformable feature aggregation, forward (gfx950).
//
// Semantics follow deformable_aggregation_kernel
// (/root/reference/projects/mmdet3d_plugin/ops/src/deformable_aggregation_cuda.cu:129-187):
//   out[b,a,c] = sum over (p, cam, lvl) of w[b,a,p,cam,lvl,c/(C/G)] * bilinear(feat, loc[b,a,p,cam])
// with a sample dropped unless 0 < x < 1 and 0 < y < 1 (:169-171), pixel = loc*size - 0.5
// (:180-181, the 0.5 is a double literal there) and each tap zero outside the map (:35-53).
//
// Mapping (not the reference's one-thread-per-(a,p,cam,lvl,c) + atomicAdd): one workgroup of 4
// waves per (batch, anchor). Every wave tests all P*cam locations itself (two ballots, no LDS,
// no barrier) and walks the valid ones with scalar bit scans; wave w takes levels w, w+4, ...
// so a wave's map geometry is scalar. One lane owns 4 consecutive channels: a tap is one
// 16-byte load per lane = one coalesced 1-KiB row per wave-instruction at C = 256. Sums stay in
// registers; the 4 waves meet once in LDS and the row is written once -> deterministic.
// The gate, the tap rule, the walk and the meeting are stated in csrc/sampler_parts.h.
#include <hip/hip_runtime.h>
#include "store_fence.h"
#include "../../include/simpb_hip.h"
#include "launch.h"
#include "sampler_parts.h"

namespace {

using namespace simpb::sampler;

// Fast path: C % 4 == 0, C <= 256, (C/G) % 4 == 0, P*cams <= 128.
__global__ __launch_bounds__(kThreads) void daf_fwd_rows(
    float* __restrict__ out, const float* __restrict__ feat, const int* __restrict__ spatial_shape,
    const int* __restrict__ scale_start, const float* __restrict__ loc, const float* __restrict__ weights,
    int num_cams, int num_feat, int C, int L, int A, int P, int G) {
  __shared__ float4 s_red[kWaves][64];
  const int a = blockIdx.x, b = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int PK = P * num_cams;
  const size_t row = (size_t)b * A + a;
  const RowLocations r = load_locations(reinterpret_cast<const float2*>(loc) + row * PK, lane, PK);

  const int coff = lane * 4;
  const int ld_off = coff < C ? coff : 0;
  const int g = ld_off / (C / G);
  const float* wrow = weights + row * PK * L * G + g;

  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  // two samples at a time: their 8 row loads are in flight together
  gather_levels<2, 0b10u>(acc, r, feat + (size_t)b * num_feat * C, spatial_shape, scale_start, num_cams, L, C, ld_off, wave,
                   [&](int i, int lvl) { return wrow[((size_t)i * L + lvl) * G]; });
  meet_and_store(s_red, acc, wave, lane, out + row * C, 0, C);
}

// Generic path for any (C, G, P*cams): one thread per channel, plain loops.
__global__ void daf_fwd_generic(float* __restrict__ out, const float* __restrict__ feat,
                                const int* __restrict__ spatial_shape, const int* __restrict__ scale_start,
                                const float* __restrict__ loc, const float* __restrict__ weights, int num_cams,
                                int num_feat, int C, int L, int A, int P, int G) {
  const int a = blockIdx.x, b = blockIdx.y;
  const size_t row = (size_t)b * A + a;
  const float* featb = feat + (size_t)b * num_feat * C;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    const int g = c / (C / G);
    float acc = 0.f;
    for (int p = 0; p < P; ++p)
      for (int cam = 0; cam < num_cams; ++cam) {
        const size_t li = (row * P + p) * num_cams + cam;
        const float2 l = make_float2(loc[2 * li], loc[2 * li + 1]);
        if (!in_image(l)) continue;
        for (int lvl = 0; lvl < L; ++lvl) {
          const int cs = cam * L + lvl;
          const int H = spatial_shape[2 * cs], W = spatial_shape[2 * cs + 1];
          const float* base = featb + (size_t)scale_start[cs] * C + c;
          const Bilinear t = taps_gated(l.x, l.y, H, W);
          float tw[4], v[4];
          tap_weights(tw, t);
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = t.in[k] ? base[(size_t)t.pixel(k, W) * C] : 0.f;
          acc = tap_sum(acc, weights[(li * L + lvl) * G + g], tw, v[0], v[1], v[2], v[3]);
        }
      }
    simpb::pin(acc);
    simpb::loads_retired();  // store_fence.h (channel loop: the next channel's loads start with nothing in flight)
    out[row * C + c] = acc;
    simpb::loads_retired();
  }
}

}  // namespace

extern "C" int simpb_deformable_aggregation_forward(
    float* output, const float* mc_ms_feat, const int* spatial_shape, const int* scale_start_index,
    const float* sample_location, const float* weights, int batch_size, int num_cams, int num_feat, int num_embeds,
    int num_scale, int num_anchors, int num_pts, int num_groups, void* stream) {
  if (!output || !mc_ms_feat || !spatial_shape || !scale_start_index || !sample_location || !weights)
    return SIMPB_EINVAL;
  if (batch_size <= 0 || num_cams <= 0 || num_feat <= 0 || num_embeds <= 0 || num_scale <= 0 || num_anchors <= 0 ||
      num_pts <= 0 || num_groups <= 0 || num_embeds % num_groups != 0 || batch_size > 65535)
    return SIMPB_EINVAL;
  (void)hipGetLastError();  // drop a stale error left by earlier runtime calls of the caller
  hipStream_t s = static_cast<hipStream_t>(stream);
  dim3 grid(num_anchors, batch_size);
  const int gd = num_embeds / num_groups;
  const int tslot = simpb_timing_begin(SIMPB_KERNEL_DAF, stream);
  const bool fast = num_embeds % 4 == 0 && num_embeds <= 256 && gd % 4 == 0 && num_pts * num_cams <= 128;
  if (fast) {
    hipLaunchKernelGGL(daf_fwd_rows, grid, dim3(kThreads), 0, s, output, mc_ms_feat, spatial_shape, scale_start_index,
                       sample_location, weights, num_cams, num_feat, num_embeds, num_scale, num_anchors, num_pts,
                       num_groups);
  } else {
    const int threads = num_embeds >= 256 ? 256 : ((num_embeds + 63) / 64) * 64;
    hipLaunchKernelGGL(daf_fwd_generic, grid, dim3(threads), 0, s, output, mc_ms_feat, spatial_shape,
                       scale_start_index, sample_location, weights, num_cams, num_feat, num_embeds, num_scale,
                       num_anchors, num_pts, num_groups);
  }
  simpb_timing_end(tslot, stream);
  return simpb_check_launch();
}
