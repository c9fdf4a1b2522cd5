// World record: the 3D detection record of a frame (decode.hip: rec3d, boxes in the lidar frame) as a serving caller wants
// it -- boxes in the global frame, score threshold and per-class range limit applied, the surviving rows packed in rank
// order, a row count per stream -- in one launch behind the decoder, inside the captured graph. Restates
// datasets/nuscenes_dataset.py:504-586 (`_format_bbox`) with `output_to_nusc_box` (:824-874) and
// `lidar_nusc_box_to_global` (:877-899) of the reference, which simpb_amd/results.py::format_sample runs per box in Python
// (7-10 ms per sample of 300 boxes on the host, against a frame of ~2.5 ms). All arithmetic in double, like there.
#include <hip/hip_runtime.h>
#include "../../include/simpb_hip.h"
#include "store_fence.h"

#include "launch.h"

namespace {

constexpr int kCapK = 512;   // rows per stream = threads per workgroup (decode.hip: kCapK)
constexpr int kW = SIMPB_WORLD_WIDTH;

// results.py quat_rotmat: the matrix of q / |q|
__device__ __forceinline__ void rotmat(const double* q, double* m) {
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
  m[0] = 1.0 - 2.0 * (y * y + z * z); m[1] = 2.0 * (x * y - z * w); m[2] = 2.0 * (x * z + y * w);
  m[3] = 2.0 * (x * y + z * w); m[4] = 1.0 - 2.0 * (x * x + z * z); m[5] = 2.0 * (y * z - x * w);
  m[6] = 2.0 * (x * z - y * w); m[7] = 2.0 * (y * z + x * w); m[8] = 1.0 - 2.0 * (x * x + y * y);
}

// One workgroup per stream, one thread per rec3d row.
__global__ __launch_bounds__(512) void world_record_kernel(unsigned long long* __restrict__ world, int* __restrict__ count,
                                                           const float* __restrict__ rec3d, const double* __restrict__ pose,
                                                           const unsigned char* __restrict__ active,
                                                           const simpb_world_tables tab) {
  __shared__ int s_wave[8];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = tab.num_output;
  const bool row = tid < K;
  // operands into registers (a thread without a row reads row 0: in bounds, never kept)
  const float* in = rec3d + ((size_t)b * K + (row ? tid : 0)) * SIMPB_RECORD3D_WIDTH;
  float v[SIMPB_RECORD3D_WIDTH];
#pragma unroll
  for (int k = 0; k < SIMPB_RECORD3D_WIDTH; ++k) v[k] = in[k];
  double p[14];
#pragma unroll
  for (int k = 0; k < 14; ++k) p[k] = pose[(size_t)b * 14 + k];
  const bool live = active == nullptr || active[b] != 0;
  simpb::loads_retired();  // store_fence.h

  // the class's row of the tables: selected, not indexed (the struct sits in scalar registers)
  const int label = (int)v[11];
  float range = -1.f;
  unsigned code_moving = 0u, code_still = 0u;
#pragma unroll
  for (int c = 0; c < SIMPB_WORLD_MAX_CLASSES; ++c) {
    if (label == c) { range = tab.class_range[c]; code_moving = tab.attr_moving[c]; code_still = tab.attr_still[c]; }
  }

  // lidar -> ego (:887-888): centre and velocity by the matrix of q / |q|, orientation by the raw quaternion
  double r1[9], r2[9];
  rotmat(p, r1);
  rotmat(p + 7, r2);
  const double x = v[0], y = v[1], z = v[2], vx = v[7], vy = v[8];
  const double cx = r1[0] * x + r1[1] * y + r1[2] * z + p[4];
  const double cy = r1[3] * x + r1[4] * y + r1[5] * z + p[5];
  const double cz = r1[6] * x + r1[7] * y + r1[8] * z + p[6];
  const double ux = r1[0] * vx + r1[1] * vy, uy = r1[3] * vx + r1[4] * vy, uz = r1[6] * vx + r1[7] * vy;
  double sn, cs;
  sincos(0.5 * (double)v[6], &sn, &cs);
  // (w, x, y, z) of q_l2e * (cs, 0, 0, sn)
  const double aw = p[0] * cs - p[3] * sn, ax = p[1] * cs + p[2] * sn, ay = p[2] * cs - p[1] * sn, az = p[3] * cs + p[0] * sn;
  // score threshold on the score before the re-score (:830-838), class range on the ego-frame distance (:890-894)
  bool keep = row && live && range >= 0.f && !(sqrt(cx * cx + cy * cy) > (double)range);
  if (tab.has_threshold) keep = keep && v[12] >= tab.threshold;
  // ego -> global (:896-897)
  const double gx = r2[0] * cx + r2[1] * cy + r2[2] * cz + p[11];
  const double gy = r2[3] * cx + r2[4] * cy + r2[5] * cz + p[12];
  const double gz = r2[6] * cx + r2[7] * cy + r2[8] * cz + p[13];
  const double wx = r2[0] * ux + r2[1] * uy + r2[2] * uz, wy = r2[3] * ux + r2[4] * uy + r2[5] * uz;
  const double bw = p[7], bx = p[8], by = p[9], bz = p[10];
  const double qw = bw * aw - bx * ax - by * ay - bz * az, qx = bw * ax + bx * aw + by * az - bz * ay;
  const double qy = bw * ay - bx * az + by * aw + bz * ax, qz = bw * az + bx * ay - by * ax + bz * aw;
  const unsigned code = hypot(wx, wy) > 0.2 ? code_moving : code_still;   // :526-549

  unsigned long long o[kW];
  o[0] = __double_as_longlong(gx); o[1] = __double_as_longlong(gy); o[2] = __double_as_longlong(gz);
  o[3] = __double_as_longlong((double)v[4]); o[4] = __double_as_longlong((double)v[3]);   // wlh = dims[[1, 0, 2]] (:849)
  o[5] = __double_as_longlong((double)v[5]);
  o[6] = __double_as_longlong(qw); o[7] = __double_as_longlong(qx); o[8] = __double_as_longlong(qy);
  o[9] = __double_as_longlong(qz);
  o[10] = __double_as_longlong(wx); o[11] = __double_as_longlong(wy);
  o[12] = __double_as_longlong((double)v[10]);
  o[13] = __double_as_longlong((double)label);
  o[14] = __double_as_longlong((double)code);
  o[15] = ((unsigned long long)__float_as_uint(v[14]) << 32) | (unsigned long long)__float_as_uint(v[13]);   // the int64 id
#pragma unroll
  for (int k = 0; k < kW; ++k) simpb::pin(o[k]);

  // stable compaction: ballot within the wave, prefix over the 8 waves in LDS
  const unsigned long long m = __ballot(keep);
  if (lane == 0) s_wave[wave] = __popcll(m);
  __syncthreads();
  int off = 0, total = 0;
#pragma unroll
  for (int w = 0; w < 8; ++w) {
    const int n = s_wave[w];
    if (w < wave) off += n;
    total += n;
  }
  const int dst = off + __popcll(m & ((1ull << lane) - 1ull));
  simpb::loads_retired();
  unsigned long long* out = world + (size_t)b * K * kW;
  if (keep) {   // dst < total <= K
    ulonglong2* d = reinterpret_cast<ulonglong2*>(out + (size_t)dst * kW);
#pragma unroll
    for (int k = 0; k < kW / 2; ++k) d[k] = make_ulonglong2(o[2 * k], o[2 * k + 1]);
  }
  if (row && tid >= total) {   // pad rows behind the kept ones: zeros, label -1
    ulonglong2* d = reinterpret_cast<ulonglong2*>(out + (size_t)tid * kW);
    const unsigned long long minus_one = (unsigned long long)__double_as_longlong(-1.0);
#pragma unroll
    for (int k = 0; k < kW / 2; ++k) d[k] = make_ulonglong2(0ull, 2 * k + 1 == 13 ? minus_one : 0ull);
  }
  if (tid == 0) count[b] = live ? total : -1;
}

}  // namespace

extern "C" int simpb_world_record(double* world, int* count, const float* rec3d, const double* pose,
                                  const unsigned char* active, simpb_world_tables tables, int num_streams, void* stream) {
  if (!world || !count || !rec3d || !pose || num_streams <= 0 || num_streams > 65535 || tables.num_output <= 0 ||
      tables.num_output > kCapK || (reinterpret_cast<size_t>(world) & 15))
    return SIMPB_EINVAL;
  (void)hipGetLastError();
  hipLaunchKernelGGL(world_record_kernel, dim3(num_streams), dim3(512), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<unsigned long long*>(world), count, rec3d, pose, active, tables);
  return simpb_check_launch();
}
