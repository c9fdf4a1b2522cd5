// Camera-grouped multi-scale deformable attention, forward (gfx950).
//
// Replaces the per-camera Python loop over mmcv's ms_deform_attn_forward
// (/root/reference/projects/mmdet3d_plugin/models/group_attn.py:222-235) with ONE launch: query
// slot q samples the value map of camera query_cam[q]. Per (query, head):
//   out[q, head, :] = sum over (lvl, pt) of attn[q,head,lvl,pt] * bilinear(value[cam, lvl, :, head, :], loc)
// Sampling rule = mmcv's CUDA op = grid_sample(bilinear, padding zeros, align_corners=False):
// pixel = loc*size - 0.5, each tap zero outside the map (csrc/sampler_parts.h: taps_free).
//
// Mapping: one workgroup of 4 waves per (batch, query); wave w takes levels w, w+4, ...; a lane
// owns 4 consecutive channels of one head, so one wave-instruction fetches, for every head, the
// 128-byte head slice of that head's own tap (8 heads x 128 B at the shipped 8x32 layout).
// All points of a level are issued before any is consumed (4 points x 4 taps in flight per lane).
#include <hip/hip_runtime.h>
#include "../../include/simpb_hip.h"

#include "launch.h"
#include "sampler_parts.h"

namespace {

using namespace simpb::sampler;

template <int PTS>
__device__ __forceinline__ void level_points(float4& acc, const float* __restrict__ vbase, int H, int W, int HC,
                                             int coff, const float2* __restrict__ locp,
                                             const float* __restrict__ attp) {
  float4 v[PTS][4];
  float tw[PTS][4];
#pragma unroll
  for (int pt = 0; pt < PTS; ++pt) {
    const float2 l = locp[pt];
    const float aw = attp[pt];
    const Bilinear t = taps_free(l.x, l.y, H, W);
    tap_weights(tw[pt], t, aw);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[pt][k] = ld_row(vbase + (size_t)t.pixel(k, W) * HC + coff);
  }
#pragma unroll
  for (int pt = 0; pt < PTS; ++pt)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      acc.x += tw[pt][k] * v[pt][k].x;
      acc.y += tw[pt][k] * v[pt][k].y;
      acc.z += tw[pt][k] * v[pt][k].z;
      acc.w += tw[pt][k] * v[pt][k].w;
    }
}

template <int PTS>
__global__ __launch_bounds__(kThreads) void msda_grouped_fwd(
    float* __restrict__ out, const float* __restrict__ value, const long long* __restrict__ spatial_shapes,
    const long long* __restrict__ level_start, const float* __restrict__ loc, const float* __restrict__ attn,
    const int* __restrict__ query_cam, int num_cams, int num_value, int heads, int ch, int L, int P, int nq) {
  __shared__ float4 s_red[kWaves][64];
  const int q = blockIdx.x, b = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int HC = heads * ch;
  int cam = query_cam[q];
  if (cam < 0) {  // capacity slot outside every camera group: defined output, no sampling
    for (int c = threadIdx.x; c < HC; c += kThreads) out[((size_t)b * nq + q) * HC + c] = 0.f;
    return;
  }
  cam = min(cam, num_cams - 1);
  const float* vcam = value + ((size_t)b * num_cams + cam) * num_value * HC;
  const size_t qrow = (size_t)b * nq + q;

  for (int cbase = 0; cbase < HC; cbase += 256) {  // one pass at the shipped 8 heads x 32 channels
    const int coff = cbase + lane * 4;
    const bool active = coff < HC;
    const int ld_off = active ? coff : 0;
    const int head = ld_off / ch;
    const float2* locq = reinterpret_cast<const float2*>(loc) + (qrow * heads + head) * L * P;
    const float* attq = attn + (qrow * heads + head) * L * P;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int lvl = wave; lvl < L; lvl += kWaves) {
      const int H = (int)spatial_shapes[2 * lvl], W = (int)spatial_shapes[2 * lvl + 1];
      const float* vbase = vcam + (size_t)level_start[lvl] * HC;
      if (PTS > 0) {
        level_points<(PTS > 0 ? PTS : 1)>(acc, vbase, H, W, HC, ld_off, locq + lvl * P, attq + lvl * P);
      } else {
        for (int pt = 0; pt < P; ++pt) level_points<1>(acc, vbase, H, W, HC, ld_off, locq + lvl * P + pt, attq + lvl * P + pt);
      }
    }
    if (cbase) __syncthreads();
    meet_and_store(s_red, acc, wave, lane, out + qrow * HC, cbase, HC);
  }
}

}  // namespace

extern "C" int simpb_ms_deform_attn_grouped_forward(
    float* output, const float* value, const long long* spatial_shapes, const long long* level_start,
    const float* sampling_loc, const float* attn_weight, const int* query_cam, int batch_size, int num_cams,
    int num_value, int num_heads, int channels, int num_levels, int num_points, int num_query, void* stream) {
  if (!output || !value || !spatial_shapes || !level_start || !sampling_loc || !attn_weight || !query_cam)
    return SIMPB_EINVAL;
  if (batch_size <= 0 || num_cams <= 0 || num_value <= 0 || num_heads <= 0 || channels <= 0 || num_levels <= 0 ||
      num_points <= 0 || num_query <= 0 || batch_size > 65535 || channels % 4 != 0)
    return SIMPB_EINVAL;
  (void)hipGetLastError();  // drop a stale error left by earlier runtime calls of the caller
  hipStream_t s = static_cast<hipStream_t>(stream);
  dim3 grid(num_query, batch_size), block(kThreads);
  const int tslot = simpb_timing_begin(SIMPB_KERNEL_MSDA, stream);
#define SIMPB_MSDA_LAUNCH(PTS)                                                                                   \
  hipLaunchKernelGGL(msda_grouped_fwd<PTS>, grid, block, 0, s, output, value, spatial_shapes, level_start,       \
                     sampling_loc, attn_weight, query_cam, num_cams, num_value, num_heads, channels, num_levels, \
                     num_points, num_query)
  if (num_points == 4) SIMPB_MSDA_LAUNCH(4);
  else if (num_points == 8) SIMPB_MSDA_LAUNCH(8);
  else SIMPB_MSDA_LAUNCH(0);
#undef SIMPB_MSDA_LAUNCH
  simpb_timing_end(tslot, stream);
  return simpb_check_launch();
}
