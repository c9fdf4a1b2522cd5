// DeformableFeatureAggregation.forward between its Linear layers, ONE launch (gfx950): key points
// (/root/reference/projects/mmdet3d_plugin/models/detection3d/blocks.py:181-222) -> project_points
// (models/blocks.py:198-213) -> the softmax of _get_weights (blocks.py:177-187) -> the aggregation kernel
// (ops/src/deformable_aggregation_cuda.cu:129-187). What csrc/dfa_prep.hip + csrc/deform_agg.hip do in three launches
// through two HBM tensors (loc 0.56 MB, weights 9 MB written and read back per layer), here in one: the workgroup that
// aggregates anchor `a` computes that anchor's 13 x 6 sampling locations in registers and its 312 x 8 softmax weights
// in LDS first. Key point, projection, gate, tap rule and gather walk are the same functions as in the three kernels
// (csrc/sampler_parts.h); the weight softmax is this kernel's own (tests compare the two routes).
//
// Mapping as daf_fwd_rows: one workgroup of 4 waves per (batch, anchor), wave w = level w, lane = 4 channels, a tap = one
// coalesced row per wave-instruction, sums in registers, one LDS meeting, one store. FEAT = float reads the decoder's
// fp32 token rows (1 KiB per tap); FEAT = _Float16 reads the f16 copy the FPN's output convolutions leave beside them
// (512 B per tap): the tokens ARE f16 numbers (the backbone runs in fp16, simpb.py:63), widening is exact, so both give
// the same bits at half the gather bytes.
#include <hip/hip_runtime.h>
#include "../../include/simpb_hip.h"
#include "store_fence.h"
#include "launch.h"
#include "sampler_parts.h"

namespace {

using namespace simpb::sampler;

constexpr int kMaxW = 4096;   // floats of LDS for the softmax weights: cams * L * P * G

struct DfaArgs {
  float* out;                 // [bs, A, C]
  const void* feat;           // FEAT [bs, num_feat, C]
  const int* spatial_shape;   // [cams, L, 2]
  const int* scale_start;     // [cams, L]
  const float* anchor;        // [bs, A, 11]
  const float* learn;         // [bs, A, num_learn * 3] raw learnable_fc output (sigmoid applied here)
  const float* fix_scale;     // [num_fix, 3]
  const float* proj;          // [bs, cams, 4, 4]
  const float* image_wh;      // [bs, cams, 2]
  const float* feat_logits;   // [bs, A, L * P * G]       weights_fc(feature + anchor_embed)
  const float* cam_logits;    // [bs, cams, L * P * G]    camera_embed . weights_fc.weight^T
  float* loc_out;             // optional [bs, A, P, cams, 2]      (tests / measurement)
  float* w_out;               // optional [bs, A, P, cams, L, G]   (tests)
  int cams, num_feat, C, L, A, num_fix, num_learn, G;
  const unsigned char* cam_valid;   // optional u8 [bs, cams] (masked instantiation only): 0 = the camera delivered no frame
};

// operands of one sampling location (key point p in camera cam), fetched before anything is computed from them
struct PointOps {
  float f0, f1, f2;   // fix_scale row or raw learnable offsets
  float m[12];        // first three rows of the camera's projection matrix
  float w0, w1;       // image width / height
  bool fixed;
};

// vmask (masked form): bit c = camera c of this stream is valid; `spare` a valid camera (or 0). The rows of a masked camera
// are not read: its loads go to the spare camera's rows and their results are dropped.
template <int CAMS, int NUM_FIX, int NUM_LEARN, bool MASKED>
__device__ __forceinline__ void fetch_point(PointOps& o, const DfaArgs& k, size_t row, int b, int i, unsigned vmask, int spare) {
  const int p = i / CAMS;
  int cam = i - p * CAMS;
  if (MASKED) cam = ((vmask >> cam) & 1u) ? cam : spare;
  o.fixed = p < NUM_FIX;
  const float* f = o.fixed ? k.fix_scale + p * 3 : k.learn + (row * NUM_LEARN + (p - NUM_FIX)) * 3;
  o.f0 = f[0]; o.f1 = f[1]; o.f2 = f[2];
  const float* M = k.proj + ((size_t)b * CAMS + cam) * 16;
#pragma unroll
  for (int j = 0; j < 12; ++j) o.m[j] = M[j];
  const float* wh = k.image_wh + ((size_t)b * CAMS + cam) * 2;
  o.w0 = wh[0]; o.w1 = wh[1];
}

// CAMS / L / NUM_FIX / NUM_LEARN / G / C are compile-time: the index arithmetic of the prologue (entry -> (cam, level, point))
// is then shifts and multiplies; with run-time divisors it was ~3 000 instructions per thread and as long as the gather.
//
// MASKED (k.cam_valid given): the mask row of stream b is workgroup-uniform and loaded once. A masked camera's logits are
// -inf by substitution (its cam_logits row is not read), so its weights are exactly 0.0 and the softmax runs over the valid
// cameras; its sampling locations are (-1, -1) without its matrix being read, and its bits are cleared from the tap
// ballots, so no tap of its tokens is ever issued (they may hold NaN). A stream with no valid camera (refused on the host)
// gives zeros: no division by the zero sum. MASKED = false is the kernel as it was.
template <class FEAT, int CAMS, int L, int NUM_FIX, int NUM_LEARN, int G, int C, bool MASKED>
__global__ __launch_bounds__(kThreads) void daf_fused_rows(DfaArgs k) {
  __shared__ float s_w[kMaxW];            // [(p * cams + cam) * L + lvl][G]: exp(logit - max), NOT yet divided by the sum
  __shared__ float4 s_red[kWaves][64];    // softmax reductions first, the waves' partial rows at the end
  __shared__ float2 s_loc[128];           // sampling locations, i = p * cams + cam
  const int a = blockIdx.x, b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  constexpr int cams = CAMS, P = NUM_FIX + NUM_LEARN, PK = P * cams;
  constexpr int LP = L * P, LPG = LP * G, n = cams * LP, slices = kThreads / G;
  static_assert(PK <= 128 && n * G <= kMaxW && (G & (G - 1)) == 0 && G <= 64 && C <= 256 && (C / G) % 4 == 0,
                "layout");
  const size_t row = (size_t)b * k.A + a;
  const int g_sm = tid % G, slice = tid / G;

  // ---- every global operand of the prologue is requested up front (indices clamped, loads unconditional): the
  // prologue then costs ONE memory round trip, not one per dependent step (all workgroups of the launch are resident at
  // once and walk their phases in step, so prologue latency adds to the launch time in full)
  unsigned vmask = (1u << CAMS) - 1u;   // bit c: camera c of this stream delivered a frame
  int spare = 0;
  if (MASKED) {
    vmask = 0u;
#pragma unroll
    for (int cam = 0; cam < CAMS; ++cam) vmask |= (k.cam_valid[b * CAMS + cam] ? 1u : 0u) << cam;
    vmask = __builtin_amdgcn_readfirstlane(vmask);
    spare = vmask ? __builtin_ctz(vmask) : 0;
  }
  float av[8];
  {
    const float* an = k.anchor + row * 11;
#pragma unroll
    for (int j = 0; j < 8; ++j) av[j] = an[j];
  }
  PointOps op;   // thread i < PK computes sampling location i = p * cams + cam, once per workgroup
  fetch_point<CAMS, NUM_FIX, NUM_LEARN, MASKED>(op, k, row, b, min(tid, PK - 1), vmask, spare);
  // softmax entries of this thread: group g_sm, (level, point) pairs lp = slice + j * slices, every camera
  constexpr int NJ = (LP + slices - 1) / slices;
  float lg[NJ][CAMS];
  {
    const float* fl = k.feat_logits + row * LPG;
    const float* cl = k.cam_logits + (size_t)b * cams * LPG;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int lp = min(slice + j * slices, LP - 1);
      const float f = fl[lp * G + g_sm];
#pragma unroll
      for (int cam = 0; cam < CAMS; ++cam) {
        if (MASKED) {   // a masked camera: -inf by substitution, the load goes to the spare camera's row
          const bool on = (vmask >> cam) & 1u;
          const float c = cl[(on ? cam : spare) * LPG + lp * G + g_sm];
          lg[j][cam] = on ? f + c : -INFINITY;
        } else {
          lg[j][cam] = f + cl[cam * LPG + lp * G + g_sm];   // (blocks.py:177-179)
        }
      }
    }
  }

  // ---- sampling locations (the functions of dfa_points_kernel), published through LDS
  {
    const bool on = !MASKED || ((vmask >> (min(tid, PK - 1) % CAMS)) & 1u);
    if (tid < PK) s_loc[tid] = on ? project(op.m, key_point(av, op.f0, op.f1, op.f2, op.fixed), op.w0, op.w1) : make_float2(-1.f, -1.f);
    else if (tid < 128) s_loc[tid] = make_float2(-1.f, -1.f);
  }

  // ---- softmax over the cams * L * P entries of each group (dfa_weights_kernel's result by another tree): thread -> (group, slice);
  // lanes of one group sit G apart inside a wave, so a group's reduction is xor shuffles + one LDS meeting. The division
  // by the sum is applied once to the finished channel sums (every channel belongs to one group).
  float inv_sum;
  {
    float* red = reinterpret_cast<float*>(s_red);   // [2][kWaves][64]: max, then sum
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
      if (slice + j * slices < LP) {
#pragma unroll
        for (int cam = 0; cam < CAMS; ++cam) m = fmaxf(m, lg[j][cam]);
      }
    for (int s = G; s < 64; s <<= 1) m = fmaxf(m, __shfl_xor(m, s));
    if (lane < G) red[wave * 64 + lane] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[g_sm], red[64 + g_sm]), fmaxf(red[128 + g_sm], red[192 + g_sm]));
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int lp = slice + j * slices;
      if (lp < LP) {
        const int lvl = lp / P, pt = lp - lvl * P;
        float* w = s_w + (pt * cams * L + lvl) * G + g_sm;   // [(pt * cams + cam) * L + lvl][G]
#pragma unroll
        for (int cam = 0; cam < CAMS; ++cam) {
          float v = expf(lg[j][cam] - m);
          if (MASKED && !((vmask >> cam) & 1u)) v = 0.f;   // exactly 0.0 (and not exp(-inf - -inf) when no camera is valid)
          w[cam * L * G] = v;
          sum += v;
        }
      }
    }
    for (int s = G; s < 64; s <<= 1) sum += __shfl_xor(sum, s);
    if (lane < G) red[256 + wave * 64 + lane] = sum;
    __syncthreads();   // s_w and s_loc complete, sums in place
    if (k.w_out) {
      float inv = 1.f / (red[256 + g_sm] + red[256 + 64 + g_sm] + red[256 + 128 + g_sm] + red[256 + 192 + g_sm]);
      if (MASKED && vmask == 0u) inv = 0.f;
      float* wo = k.w_out + row * (size_t)n * G;
      for (int e = slice; e < n; e += slices) wo[e * G + g_sm] = s_w[e * G + g_sm] * inv;   // (same layout)
      simpb::stores_retired();
    }
    const int gch = (lane * 4 < C ? lane * 4 : 0) / (C / G);   // group of this lane's channels in the aggregation below
    inv_sum = 1.f / (red[256 + gch] + red[256 + 64 + gch] + red[256 + 128 + gch] + red[256 + 192 + gch]);
    if (MASKED && vmask == 0u) inv_sum = 0.f;   // no valid camera: zeros out, not 0 x inf
  }
  // lane i (and i + 64) of EVERY wave holds location i
  // (masked form: location i belongs to camera i % cams; a masked camera's bit is cleared whatever its location holds)
  const RowLocations r = load_locations(s_loc, lane, 128, !MASKED || ((vmask >> (lane % CAMS)) & 1u),
                                        !MASKED || ((vmask >> ((lane + 64) % CAMS)) & 1u));
  if (k.loc_out && wave == 0) {
    float2* lo = reinterpret_cast<float2*>(k.loc_out) + row * PK;
    if (lane < PK) lo[lane] = r.l0;
    if (lane + 64 < PK) lo[lane + 64] = r.l1;
    simpb::stores_retired();   // (measurement-only output: nothing of it in flight beside the gather's counted waits)
  }

  // ---- the aggregation itself (daf_fwd_rows' walk with the weights in LDS), four samples at a time
  const int coff = lane * 4;
  const int ld_off = coff < C ? coff : 0;
  const int g = ld_off / (C / G);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  gather_levels<4>(acc, r, static_cast<const FEAT*>(k.feat) + (size_t)b * k.num_feat * C, k.spatial_shape, k.scale_start, cams, L,
                   C, ld_off, wave, [&](int i, int lvl) { return s_w[(i * L + lvl) * G + g]; });
  __syncthreads();   // every wave has read the sums out of s_red
  acc.x *= inv_sum; acc.y *= inv_sum; acc.z *= inv_sum; acc.w *= inv_sum;
  meet_and_store(s_red, acc, wave, lane, k.out + row * C, 0, C);
}

// the shipped layout (config :221-238: 4 levels, 7 fixed + 6 learnable key points, 8 groups of 32 channels) at CAMS cameras;
// CAMS = 6 is the shipped rig, and both the shipped-layout entries and the rig entry launch these very instantiations for it
template <class FEAT, int CAMS>
void launch_fused(bool masked, dim3 grid, hipStream_t s, const DfaArgs& k) {
  if (masked) hipLaunchKernelGGL((daf_fused_rows<FEAT, CAMS, 4, 7, 6, 8, 256, true>), grid, dim3(kThreads), 0, s, k);
  else hipLaunchKernelGGL((daf_fused_rows<FEAT, CAMS, 4, 7, 6, 8, 256, false>), grid, dim3(kThreads), 0, s, k);
}

constexpr int kMaxRigCams = 8;   // 13 * CAMS <= 128 locations per row and CAMS * 416 <= kMaxW hold up to 9; the allocation kernels end at 8

template <int CAMS>
void launch_fused_cams(bool f16, bool masked, dim3 grid, hipStream_t s, const DfaArgs& k) {
  if (f16) launch_fused<_Float16, CAMS>(masked, grid, s, k);
  else launch_fused<float, CAMS>(masked, grid, s, k);
}

bool operands_given(const float* output, const void* mc_ms_feat, const int* spatial_shape, const int* scale_start_index,
                    const float* anchor, const float* learnable, const float* fix_scale, const float* projection_mat,
                    const float* image_wh, const float* feat_logits, const float* cam_logits, int batch_size, int num_cams,
                    int num_feat, int num_scale, int num_anchors, int num_fix, int num_learn, int num_groups) {
  if (!output || !mc_ms_feat || !spatial_shape || !scale_start_index || !anchor || !fix_scale || !projection_mat ||
      !image_wh || !feat_logits || !cam_logits || (num_learn > 0 && !learnable))
    return false;
  return !(batch_size <= 0 || batch_size > 65535 || num_cams <= 0 || num_feat <= 0 || num_scale <= 0 || num_anchors <= 0 ||
           num_fix < 0 || num_learn < 0 || num_fix + num_learn <= 0 || num_groups <= 0);
}

// num_cams in 1..kMaxRigCams, the rest of the layout as shipped (validated by the callers; the count once more here, in front of
// any HIP call: no count without a case of its own reaches a kernel compiled for another)
int launch_rig(float* output, const void* mc_ms_feat, int feat_is_f16, const int* spatial_shape, const int* scale_start_index,
               const float* anchor, const float* learnable, const float* fix_scale, const float* projection_mat,
               const float* image_wh, const float* feat_logits, const float* cam_logits, float* loc_out, float* weights_out,
               int batch_size, int num_cams, int num_feat, int num_embeds, int num_scale, int num_anchors, int num_fix,
               int num_learn, int num_groups, const unsigned char* cam_valid, void* stream) {
  if (num_cams < 1 || num_cams > kMaxRigCams) return SIMPB_EINVAL;
  (void)hipGetLastError();
  DfaArgs k;
  k.out = output; k.feat = mc_ms_feat; k.spatial_shape = spatial_shape; k.scale_start = scale_start_index;
  k.anchor = anchor; k.learn = learnable; k.fix_scale = fix_scale; k.proj = projection_mat; k.image_wh = image_wh;
  k.feat_logits = feat_logits; k.cam_logits = cam_logits; k.loc_out = loc_out; k.w_out = weights_out;
  k.cams = num_cams; k.num_feat = num_feat; k.C = num_embeds; k.L = num_scale; k.A = num_anchors; k.num_fix = num_fix;
  k.num_learn = num_learn; k.G = num_groups; k.cam_valid = cam_valid;
  hipStream_t s = static_cast<hipStream_t>(stream);
  dim3 grid(num_anchors, batch_size);
  const bool f16 = feat_is_f16 != 0, masked = cam_valid != nullptr;
  const int tslot = simpb_timing_begin(SIMPB_KERNEL_DAF, stream);
  switch (num_cams) {
    case 1: launch_fused_cams<1>(f16, masked, grid, s, k); break;
    case 2: launch_fused_cams<2>(f16, masked, grid, s, k); break;
    case 3: launch_fused_cams<3>(f16, masked, grid, s, k); break;
    case 4: launch_fused_cams<4>(f16, masked, grid, s, k); break;
    case 5: launch_fused_cams<5>(f16, masked, grid, s, k); break;
    case 6: launch_fused_cams<6>(f16, masked, grid, s, k); break;
    case 7: launch_fused_cams<7>(f16, masked, grid, s, k); break;
    case 8: launch_fused_cams<8>(f16, masked, grid, s, k); break;
    default: break;   // (refused above)
  }
  static_assert(kMaxRigCams == 8, "one case per camera count");
  simpb_timing_end(tslot, stream);
  return simpb_check_launch();
}

}  // namespace

extern "C" int simpb_dfa_fused_forward_rig(
    float* output, const void* mc_ms_feat, int feat_is_f16, const int* spatial_shape, const int* scale_start_index,
    const float* anchor, const float* learnable, const float* fix_scale, const float* projection_mat, const float* image_wh,
    const float* feat_logits, const float* cam_logits, float* loc_out, float* weights_out, int batch_size, int num_cams,
    int num_feat, int num_embeds, int num_scale, int num_anchors, int num_fix, int num_learn, int num_groups,
    const unsigned char* cam_valid, void* stream) {
  if (!operands_given(output, mc_ms_feat, spatial_shape, scale_start_index, anchor, learnable, fix_scale, projection_mat, image_wh,
                      feat_logits, cam_logits, batch_size, num_cams, num_feat, num_scale, num_anchors, num_fix, num_learn, num_groups))
    return SIMPB_EINVAL;
  // the camera count is the one free dimension: a kernel per count, the rest compiled for the shipped layout
  if (num_cams > kMaxRigCams || num_scale != 4 || num_fix != 7 || num_learn != 6 || num_groups != 8 || num_embeds != 256)
    return SIMPB_EINVAL;
  return launch_rig(output, mc_ms_feat, feat_is_f16, spatial_shape, scale_start_index, anchor, learnable, fix_scale, projection_mat,
                    image_wh, feat_logits, cam_logits, loc_out, weights_out, batch_size, num_cams, num_feat, num_embeds, num_scale,
                    num_anchors, num_fix, num_learn, num_groups, cam_valid, stream);
}

extern "C" int simpb_dfa_fused_forward_cams(
    float* output, const void* mc_ms_feat, int feat_is_f16, const int* spatial_shape, const int* scale_start_index,
    const float* anchor, const float* learnable, const float* fix_scale, const float* projection_mat, const float* image_wh,
    const float* feat_logits, const float* cam_logits, float* loc_out, float* weights_out, int batch_size, int num_cams,
    int num_feat, int num_embeds, int num_scale, int num_anchors, int num_fix, int num_learn, int num_groups,
    const unsigned char* cam_valid, void* stream) {
  if (!operands_given(output, mc_ms_feat, spatial_shape, scale_start_index, anchor, learnable, fix_scale, projection_mat, image_wh,
                      feat_logits, cam_logits, batch_size, num_cams, num_feat, num_scale, num_anchors, num_fix, num_learn, num_groups))
    return SIMPB_EINVAL;
  // the shipped layout only (six cameras); simpb_dfa_fused_forward_rig takes 1..8 cameras, the three-launch route
  // (simpb_dfa_points / simpb_dfa_weights / simpb_deformable_aggregation_forward) any other layout
  if (num_cams != 6 || num_scale != 4 || num_fix != 7 || num_learn != 6 || num_groups != 8 || num_embeds != 256)
    return SIMPB_EINVAL;
  return launch_rig(output, mc_ms_feat, feat_is_f16, spatial_shape, scale_start_index, anchor, learnable, fix_scale, projection_mat,
                    image_wh, feat_logits, cam_logits, loc_out, weights_out, batch_size, num_cams, num_feat, num_embeds, num_scale,
                    num_anchors, num_fix, num_learn, num_groups, cam_valid, stream);
}

extern "C" int simpb_dfa_fused_forward(
    float* output, const void* mc_ms_feat, int feat_is_f16, const int* spatial_shape, const int* scale_start_index,
    const float* anchor, const float* learnable, const float* fix_scale, const float* projection_mat, const float* image_wh,
    const float* feat_logits, const float* cam_logits, float* loc_out, float* weights_out, int batch_size, int num_cams,
    int num_feat, int num_embeds, int num_scale, int num_anchors, int num_fix, int num_learn, int num_groups, void* stream) {
  return simpb_dfa_fused_forward_cams(output, mc_ms_feat, feat_is_f16, spatial_shape, scale_start_index, anchor, learnable,
                                      fix_scale, projection_mat, image_wh, feat_logits, cam_logits, loc_out, weights_out,
                                      batch_size, num_cams, num_feat, num_embeds, num_scale, num_anchors, num_fix, num_learn,
                                      num_groups, nullptr, stream);
}
