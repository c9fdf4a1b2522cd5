// Fused small-MLP chains (gfx950): a whole `linear_relu_ln` stack of the reference
// (projects/mmdet3d_plugin/models/blocks.py:32-43) -- [Linear, ReLU]*, LayerNorm,
// ..., optional last Linear + Scale -- in ONE launch, with the activations of a row tile living in
// LDS between layers. Used for the 3D anchor encoder (detection3d/blocks.py:57-74: 4 branches x 4 x
// [Linear, ReLU, LN] = 48 tiny kernels in the reference, 7 times per frame), the 2D sine encoder
// (detection2d/blocks.py:48-63 + utils.py:40-63), the refinement heads (detection3d/blocks.py:123-154,
// detection2d/blocks.py:117-144) and the camera encoder (blocks.py:93-99).
//
// These chains are tiny (<= 1.5k rows x 256 wide): the cost in the reference is launch count, not
// FLOPs, so the kernels are organised for latency: one workgroup = R rows, the row tile stays in LDS,
// weights come straight from L2 into registers. Up to 8 independent chains (SIMPB_MLP_MAX_CHAINS; e.g. the
// 4 encoder branches) share a launch through blockIdx.y.
//
// One program, four kernels. `chain_walk<Form>` is the program: dead-row exit, input stage, one barrier
// per op, output stage. The stages (load_tile, lead_norm_rows, layernorm_rows, linear_per_column,
// store_tile) are written once. A Form states what is its own: rows R, waves, LDS row stride, its
// LayerNorm stage (layernorm_rows over its reducer), whether it has the leading norm, and `linear`:
// how a Linear layer with a "nice" K is multiplied (row tile, weight layout, matrix instruction).
// Three kernels are chain_walk over a Form; the shipped 4-row kernel keeps its own walk over the same
// stages (the reason is at the kernel). The table `kForms` at the end maps args.weights_transposed to
// a kernel. A new form is a `linear` body and a line in that table.
#include <hip/hip_runtime.h>
#include <type_traits>
#include "../../include/simpb_hip.h"

#include "launch.h"

#ifdef SIMPB_CHAIN_STAMPS
// diagnostic build only (tools/chain_stamps.py): s_memtime of workgroup (0, 0), wave 0 at the walk's phase boundaries:
// 0 start, 1 input staged, per op o: 2 + 4o start, 3 + 4o first weights requested (matrix paths), 4 + 4o done, 5 + 4o past
// the barrier; 126 / 127 around the output stage
__device__ unsigned long long g_chain_stamps[128];
#define SIMPB_STAMP(i)                                                                       \
  do {                                                                                       \
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && (i) < 128)                 \
      g_chain_stamps[(i)] = __builtin_amdgcn_s_memtime();                                    \
  } while (0)
extern "C" int simpb_debug_chain_stamps(unsigned long long* host_out) {
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_chain_stamps), sizeof(g_chain_stamps));
}
#else
#define SIMPB_STAMP(i) do {} while (0)
#endif

namespace {

constexpr int kMaxDim = 256;
constexpr int kLdAct = kMaxDim + 4;   // row stride = 4 mod 64 floats: the 16 lanes of a ds_read_b128 phase hit 16 distinct 4-bank slots

using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x16 = __attribute__((ext_vector_type(16))) float;

// compile-time loop (register-set indices must be constants in the front end: csrc/gemm.hip)
template <int D, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (D < N) {
    f(std::integral_constant<int, D>{});
    static_for<D + 1, N>(f);
  }
}

// ---------------------------------------------------------------------------------------------- shared stages
// optional last stage on one output value (see SIMPB_MLP_POST_* in the header)
__device__ __forceinline__ float post_stage(const simpb_mlp_chain& ch, float v, int row, int t) {
  if (ch.post == SIMPB_MLP_POST_REFINE3D) {
    if (ch.div && t >= ch.div_col0) v = v / ch.div[row / ch.div_rows];
    if (t < ch.res_cols) v += ch.res[(size_t)row * ch.ldres + t];
  } else if (ch.post == SIMPB_MLP_POST_REFINE2D) {
    if (t < ch.res_cols) {
      float a = ch.res[(size_t)row * ch.ldres + t];
      a = fminf(fmaxf(a, 0.f), 1.f);
      v += logf(fmaxf(a, 1e-5f) / fmaxf(1.f - a, 1e-5f));
    }
    v = 1.f / (1.f + expf(-v));
  } else if (ch.post == SIMPB_MLP_POST_SIGMOID) {
    v = 1.f / (1.f + expf(-v));
  }
  return v;
}

// Rows >= *m_live are capacity slots of the static 2D query set (no camera, nothing reads them): a workgroup whose rows are
// all dead writes zeros and leaves -- a quarter of the 1 536-slot launches' workgroups at N2 ~ 1 130.
__device__ __forceinline__ bool skip_dead_rows(const simpb_mlp_args& args, const simpb_mlp_chain& ch, int row0, int rows,
                                               int tid, int nthreads) {
  if (!args.m_live || row0 < *args.m_live) return false;
  int width = ch.in_mode == SIMPB_MLP_IN_SINE2D ? 256 : ch.in_dim;
  for (int o = 0; o < ch.n_ops; ++o)
    if (ch.ops[o].type == SIMPB_MLP_LINEAR) width = ch.ops[o].out_dim;
  if (ch.out)   // (NULL: the leading LayerNorm stage alone, below)
    for (int idx = tid; idx < rows * width; idx += nthreads) {
      const int r = idx / width, t = idx - r * width;
      if (row0 + r < args.num_rows) ch.out[(size_t)(row0 + r) * ch.ldo + t] = 0.f;
    }
  if (ch.in_mode == SIMPB_MLP_IN_ROWS_LN && ch.ln_out)
    for (int idx = tid; idx < rows * ch.in_dim; idx += nthreads) {
      const int r = idx / ch.in_dim, t = idx - r * ch.in_dim;
      if (row0 + r < args.num_rows) ch.ln_out[(size_t)(row0 + r) * ch.ld_ln_out + t] = 0.f;
    }
  return true;
}

// Input stage: the chain's input rows into the tile, zeros for rows past N. VEC16 (the 16-row form only) adds a path of
// 16-byte loads for power-of-two widths; it produces the same values.
template <int R, int LD, int THREADS, bool VEC16>
__device__ __forceinline__ void load_tile(float (&tile)[R][LD], const simpb_mlp_chain& ch, int row0, int N, int tid) {
  if (ch.in_mode == SIMPB_MLP_IN_SINE2D) {
    // pos2posemb2d (utils.py:40-63) of a 2-d point: 128 features of y then 128 of x;
    // feature i of an axis = sin or cos (even / odd i) of coord * 2*pi / 10000^(2*(i/2)/128)
    for (int idx = tid; idx < R * 256; idx += THREADS) {
      const int r = idx >> 8, j = idx & 255;
      const int row = row0 + r;
      float v = 0.f;
      if (row < N) {
        const int axis = j < 128 ? 1 : 0, i = j & 127;
        const float coord = ch.x[(size_t)row * ch.ldx + axis] * 6.283185307179586f;
        const float dim_t = powf(10000.f, (float)(2 * (i >> 1)) / 128.f);
        const float p = coord / dim_t;
        v = (i & 1) ? cosf(p) : sinf(p);
      }
      tile[r][j] = v;
    }
    return;
  }
  if constexpr (VEC16) {
    if ((ch.in_dim & (ch.in_dim - 1)) == 0 && ch.in_dim >= 4 && (ch.ldx & 3) == 0 && (ch.ldx2 & 3) == 0 &&
        ((reinterpret_cast<size_t>(ch.x) | reinterpret_cast<size_t>(ch.x2)) & 15) == 0) {
      // power-of-two width: 16-byte loads, shifts instead of divisions, every load of the tile in flight at once
      const int q = ch.in_dim >> 2, sh = __ffs(q) - 1;
#pragma unroll 2
      for (int idx = tid; idx < R * q; idx += THREADS) {
        const int r = idx >> sh, c4 = idx & (q - 1);
        const int row = row0 + r;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < N) {
          v = *reinterpret_cast<const float4*>(ch.x + (size_t)row * ch.ldx + 4 * c4);
          if (ch.x2) {
            const float4 u = *reinterpret_cast<const float4*>(ch.x2 + (size_t)row * ch.ldx2 + 4 * c4);
            v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
          }
        }
        *reinterpret_cast<float4*>(&tile[r][4 * c4]) = v;
      }
      return;
    }
  }
  for (int idx = tid; idx < R * ch.in_dim; idx += THREADS) {
    const int r = idx / ch.in_dim, k = idx - r * ch.in_dim;
    const int row = row0 + r;
    float v = 0.f;
    if (row < N) {
      v = ch.x[(size_t)row * ch.ldx + k];
      if (ch.x2) v += ch.x2[(size_t)row * ch.ldx2 + k];
    }
    tile[r][k] = v;
  }
}

// Output stage: out_scale, post stage, store; rows past N are not written.
template <int R, int LD, int THREADS>
__device__ __forceinline__ void store_tile(const float (&tile)[R][LD], int width, const simpb_mlp_chain& ch, int row0, int N,
                                           int tid) {
  for (int idx = tid; idx < R * width; idx += THREADS) {
    const int r = idx / width, t = idx - r * width;
    const int row = row0 + r;
    if (row < N) {
      float v = tile[r][t];
      if (ch.out_scale) v *= ch.out_scale[t];
      if (ch.post) v = post_stage(ch, v, row, t);
      ch.out[(size_t)row * ch.ldo + t] = v;
    }
  }
}

// Sums over the LANES lanes that share a row, the result in every one of them. Three, because their summation trees differ
// and the kernels' bits are pinned: the xor butterfly 32..1 (VALU form), DPP steps over a half wave (16-row form), and the
// half-wave sum + one xor 32 (4- and 32-row forms, leading norm).
template <int CTRL>
__device__ __forceinline__ float dpp_add(float x) {
  const int y = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xF, 0xF, true);
  return x + __builtin_bit_cast(float, y);
}
// sum over the 32 lanes of a half wave (lanes 0-31 / 32-63): four DPP steps (register moves, no LDS crossbar) + one ds_bpermute
struct HalfWaveSum {
  static __device__ __forceinline__ float sum(float x) {
    x = dpp_add<0xB1>(x);    // quad_perm [1,0,3,2]: lane ^ 1
    x = dpp_add<0x4E>(x);    // quad_perm [2,3,0,1]: lane ^ 2
    x = dpp_add<0x141>(x);   // row_half_mirror: i <-> 7 - i inside 8 lanes (every quad already holds its sum)
    x = dpp_add<0x140>(x);   // row_mirror: i <-> 15 - i inside the 16-lane row
    return x + __shfl_xor(x, 16);
  }
};
struct WaveSum {
  static __device__ __forceinline__ float sum(float x) { x = HalfWaveSum::sum(x); return x + __shfl_xor(x, 32); }
};
struct ButterflySum {
  static __device__ __forceinline__ float sum(float x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
    return x;
  }
};

// Moments of one row of D values held as v[j] = element l + LANES * j (zeros past D): mean and 1 / sqrt(var + eps), eps 1e-5,
// biased variance (torch.nn.LayerNorm).
template <int LANES, class Reduce>
__device__ __forceinline__ void row_moments(const float (&v)[kMaxDim / LANES], int l, int D, float& mean, float& inv) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < kMaxDim / LANES; ++j) s += v[j];
  s = Reduce::sum(s);
  mean = s / (float)D;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < kMaxDim / LANES; ++j) {
    const float d = (l + LANES * j) < D ? v[j] - mean : 0.f;
    q += d * d;
  }
  q = Reduce::sum(q);
  inv = 1.f / sqrtf(q / (float)D + 1e-5f);
}

// LayerNorm stage, in place: LANES lanes per row (64: one wave per row, 4 elements per lane; 32: a half wave per row, 8
// elements, all 16 rows of the 16-row form at once -- one wave per row with two rows in sequence was ~1.5 us of dependent
// ds_bpermute latency per LayerNorm there). gamma and beta are requested before the reductions need them.
template <int R, int LD, int THREADS, int LANES, class Reduce>
__device__ __forceinline__ void layernorm_rows(float (&tile)[R][LD], const simpb_mlp_op& op, int tid) {
  constexpr int NJ = kMaxDim / LANES;
  const int D = op.in_dim, l = tid & (LANES - 1);
  // kOneRow (the 16-row and VALU forms: at most one row per lane group) keeps the request order those kernels had before the
  // stage was shared: gamma, beta and the row under one condition per j. The other arm keeps the 32-row kernel's: gamma and
  // beta once, in front of its eight rows. Keep both: a loop of its own for gamma and beta in front of a single row made
  // the compiler wait for the first pair before it issued the next (measured in the 4-row kernel, +0.3 us per launch).
  constexpr bool kOneRow = R * LANES <= THREADS;
  float g[NJ], be[NJ];
  if constexpr (!kOneRow) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int e = l + LANES * j;
      g[j] = e < D ? op.w[e] : 0.f;
      be[j] = e < D ? op.b[e] : 0.f;
    }
  }
#pragma unroll 2
  for (int r = tid / LANES; r < R; r += THREADS / LANES) {
    float v[NJ], mean, inv;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int e = l + LANES * j;
      const bool in = e < D;
      if constexpr (kOneRow) {
        g[j] = in ? op.w[e] : 0.f;
        be[j] = in ? op.b[e] : 0.f;
      }
      v[j] = in ? tile[r][e] : 0.f;
    }
    row_moments<LANES, Reduce>(v, l, D, mean, inv);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int e = l + LANES * j;
      if (e < D) tile[r][e] = (v[j] - mean) * inv * g[j] + be[j];
    }
  }
}

// IN_ROWS_LN input stage: the decoder's `norm` operator in front of a head, inside the launch. One wave per row (the
// LayerNorm stage's arithmetic), + x2 afterwards; the chain that carries ln_out writes the operator's output.
template <int R, int LD, int WAVES>
__device__ __forceinline__ void lead_norm_rows(float (&tile)[R][LD], const simpb_mlp_args& args, const simpb_mlp_chain& ch,
                                               int row0, int tid) {
  constexpr int NJ = kMaxDim / 64;
  const int lane = tid & 63, D = ch.in_dim, N = args.num_rows;
  const int live = args.m_live ? min(N, *args.m_live) : N;
  constexpr bool kOneRow = R <= WAVES;   // as in layernorm_rows: gamma, beta, x and x2 under one condition per j
  float g[NJ], be[NJ];
  if constexpr (!kOneRow) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int e = lane + 64 * j;
      g[j] = e < D ? ch.ln_w[e] : 0.f;
      be[j] = e < D ? ch.ln_b[e] : 0.f;
    }
  }
  for (int r = tid >> 6; r < R; r += WAVES) {
    const int row = row0 + r;
    const bool in_rows = row < N, alive = row < live;
    float v[NJ], x2v[NJ], mean, inv;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int e = lane + 64 * j;
      const bool in = e < D;
      if constexpr (kOneRow) {
        g[j] = in ? ch.ln_w[e] : 0.f;
        be[j] = in ? ch.ln_b[e] : 0.f;
      }
      v[j] = (in && in_rows) ? ch.x[(size_t)row * ch.ldx + e] : 0.f;
      x2v[j] = (in && in_rows && ch.x2) ? ch.x2[(size_t)row * ch.ldx2 + e] : 0.f;
    }
    row_moments<64, WaveSum>(v, lane, D, mean, inv);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int e = lane + 64 * j;
      if (e < D) {
        const float y = alive ? (v[j] - mean) * inv * g[j] + be[j] : 0.f;   // (capacity rows: zeros, as the LayerNorm launch wrote)
        if (ch.ln_out && in_rows) ch.ln_out[(size_t)row * ch.ld_ln_out + e] = y;
        tile[r][e] = y + x2v[j];
      }
    }
  }
}

// Linear layer, one thread per output column (narrow / odd K: 2, 3, 12, ...): bias first, then fmaf over ascending k.
// `w` = the column's first weight, `kstride` = floats between k and k + 1: (op.w + tid * K, 1) on nn.Linear's [D][K],
// (op.w + tid, D) on [K][D].
template <int R, int LD>
__device__ __forceinline__ void linear_per_column(const float (&in)[R][LD], float (&out)[R][LD], const simpb_mlp_op& op,
                                                  const float* w, size_t kstride, int tid) {
  if (tid >= op.out_dim) return;
  float acc[R];
  const float b = op.b ? op.b[tid] : 0.f;
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = b;
  for (int k = 0; k < op.in_dim; ++k) {
    const float wv = w[(size_t)k * kstride];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = fmaf(in[r][k], wv, acc[r]);
  }
#pragma unroll
  for (int r = 0; r < R; ++r) out[r][tid] = op.relu ? fmaxf(acc[r], 0.f) : acc[r];
}

// ---------------------------------------------------------------------------------------------- the walk
template <class F>
__device__ __forceinline__ void chain_walk(const simpb_mlp_args& args) {
  constexpr int R = F::R, LD = F::LD, kThreads = F::WAVES * 64;
  __shared__ float act[2][R][LD];
  const simpb_mlp_chain& ch = args.chain[blockIdx.y];
  const int tid = threadIdx.x;
  const int row0 = blockIdx.x * R;
  if (skip_dead_rows(args, ch, row0, R, tid, kThreads)) return;
  SIMPB_STAMP(0);

  if (F::kLeadNorm && ch.in_mode == SIMPB_MLP_IN_ROWS_LN) {
    lead_norm_rows<R, LD, F::WAVES>(act[0], args, ch, row0, tid);
    if (!ch.out) return;   // the `norm` operator alone (no chain behind it, workgroup-uniform): ln_out is the job's product
  } else {
    load_tile<R, LD, kThreads, F::kVecInput>(act[0], ch, row0, args.num_rows, tid);
  }
  __syncthreads();
  SIMPB_STAMP(1);

  int cur = 0;
  int width = ch.in_mode == SIMPB_MLP_IN_SINE2D ? 256 : ch.in_dim;
  for (int o = 0; o < ch.n_ops; ++o) {
    const simpb_mlp_op& op = ch.ops[o];
    SIMPB_STAMP(2 + 4 * o);
    if (op.type == SIMPB_MLP_LINEAR) {
      F::linear(act[cur], act[cur ^ 1], op, tid, o);
      cur ^= 1;
      width = op.out_dim;
    } else {  // LayerNorm over `width` (= op.in_dim)
      F::layernorm(act[cur], op, tid);
    }
    SIMPB_STAMP(4 + 4 * o);
    __syncthreads();
    SIMPB_STAMP(5 + 4 * o);
  }
  SIMPB_STAMP(126);
  store_tile<R, LD, kThreads>(act[cur], width, ch, row0, args.num_rows, tid);
  SIMPB_STAMP(127);
}

// ---------------------------------------------------------------------------------------------- the forms
// ---- VALU form (weights_transposed == 1): weights pre-transposed ([in][out], one coalesced 1-KiB wave-load per k,
// L2-resident and shared by all workgroups), the row tile broadcast from LDS.
template <int R_, int WAVES_>
struct ValuForm {
  static constexpr int R = R_, WAVES = WAVES_, LD = kMaxDim;
  static constexpr bool kLeadNorm = false, kVecInput = false;
  static __device__ __forceinline__ void layernorm(float (&tile)[R][LD], const simpb_mlp_op& op, int tid) {
    layernorm_rows<R, LD, WAVES * 64, 64, ButterflySum>(tile, op, tid);
  }

  static __device__ __forceinline__ void linear(const float (&in)[R][LD], float (&out)[R][LD], const simpb_mlp_op& op, int tid,
                                                int o) {
    __shared__ float part[WAVES][R][kMaxDim];  // per-wave partial sums of the split-K linear
    const int K = op.in_dim, D = op.out_dim;
    if (!((D & 3) == 0 && K >= 16)) {
      linear_per_column<R, LD>(in, out, op, op.w + tid, D, tid);
      return;
    }
    // Wide form. What bounds a layer is streaming W^T (up to 256 KiB) from L2 into ONE workgroup,
    // so the reduction is split over the WAVES waves and each lane takes 4 adjacent columns: every
    // load is 16 B per lane (a 1-KiB row of W^T per wave-instruction), 4x the bytes in flight of a
    // scalar-column layout. Partial sums meet in LDS.
    const int lane = tid & 63, wave = tid >> 6;
    const int c4 = lane * 4;
    const int kq = (K + WAVES - 1) / WAVES;    // k-range per wave, in rows
    const int kb = wave * kq, ke = min(K, kb + kq);
    float4 acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c4 < D) {
      const float* wt = op.w + c4;
      constexpr int KU = 8;
      float4 wa[KU], wb[KU];
      int k = kb;
      const int kfull = kb + ((ke - kb) / KU) * KU;
      if (kfull > kb) {
#pragma unroll
        for (int j = 0; j < KU; ++j) wa[j] = *reinterpret_cast<const float4*>(wt + (size_t)(k + j) * D);
      }
      SIMPB_STAMP(3 + 4 * o);
      for (; k < kfull; k += KU) {
        const bool more = k + KU < kfull;
        if (more) {
#pragma unroll
          for (int j = 0; j < KU; ++j) wb[j] = *reinterpret_cast<const float4*>(wt + (size_t)(k + KU + j) * D);
        }
#pragma unroll
        for (int j = 0; j < KU; ++j) {
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const float a = in[r][k + j];
            acc[r].x = fmaf(a, wa[j].x, acc[r].x);
            acc[r].y = fmaf(a, wa[j].y, acc[r].y);
            acc[r].z = fmaf(a, wa[j].z, acc[r].z);
            acc[r].w = fmaf(a, wa[j].w, acc[r].w);
          }
        }
        if (more) {
#pragma unroll
          for (int j = 0; j < KU; ++j) wa[j] = wb[j];
        }
      }
      for (; k < ke; ++k) {
        const float4 w4 = *reinterpret_cast<const float4*>(wt + (size_t)k * D);
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const float a = in[r][k];
          acc[r].x = fmaf(a, w4.x, acc[r].x);
          acc[r].y = fmaf(a, w4.y, acc[r].y);
          acc[r].z = fmaf(a, w4.z, acc[r].z);
          acc[r].w = fmaf(a, w4.w, acc[r].w);
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r) *reinterpret_cast<float4*>(&part[wave][r][c4]) = acc[r];
    }
    __syncthreads();
    // thread t = column t: sum the WAVES partials (fixed order), bias, activation
    if (tid < D) {
      const float b = op.b ? op.b[tid] : 0.f;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float v = part[0][r][tid];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) v += part[w][r][tid];  // fixed order: deterministic
        v += b;
        out[r][tid] = op.relu ? fmaxf(v, 0.f) : v;
      }
    }
  }
};

// ---- 16-row matrix-core form (weights_transposed == 0): 8 waves; wave w owns output columns [32w, 32w+32)
// of a Linear layer as two 16x16 tiles of v_mfma_f32_16x16x4_f32 (exact fp32). Operands use the
// ORIGINAL weight layout [out][in] with the k-order permuted inside each 64-wide k-chunk: load j of
// lane quarter kq is the float4 at k = 16*j + 4*kq, so the four lanes of a weight row read 64
// CONTIGUOUS bytes per instruction (16 half-lines per wave-load; with k = 16*kq + 4*j it was four
// scattered 16-byte pieces per row = 32 lines per wave-load). A and B use the same permutation, so
// the sum is unchanged.
struct R16Form {
  static constexpr int R = 16, WAVES = 8, LD = kLdAct;   // LD: rows 16 B apart in bank space for the b128 reads
  static constexpr bool kLeadNorm = false, kVecInput = true;
  static __device__ __forceinline__ void layernorm(float (&tile)[R][LD], const simpb_mlp_op& op, int tid) {
    layernorm_rows<R, LD, WAVES * 64, 32, HalfWaveSum>(tile, op, tid);
  }

  static __device__ __forceinline__ void linear(const float (&in)[R][LD], float (&out)[R][LD], const simpb_mlp_op& op, int tid,
                                                int o) {
    const int K = op.in_dim, D = op.out_dim;
    if ((K & 63) != 0) {  // narrow / odd layers (K = 2, 3, 12, 32; D = 2..11)
      linear_per_column<R, LD>(in, out, op, op.w + (size_t)tid * K, 1, tid);
      return;
    }
    // any D: columns past D are fed zeros and not stored (D = 2..11 heads use wave 0 only)
    const int lane = tid & 63, wave = tid >> 6;
    const int col0 = wave * 32;
    if (col0 >= D) return;
    const int r16 = lane & 15, kq = lane >> 4;
    const bool cv0 = col0 + r16 < D, cv1 = col0 + 16 + r16 < D;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    const float* w0 = op.w + (size_t)(cv0 ? col0 + r16 : 0) * K + 4 * kq;         // original layout [D][K]
    const float* w1 = op.w + (size_t)(cv1 ? col0 + 16 + r16 : 0) * K + 4 * kq;
    const float m0 = cv0 ? 1.f : 0.f, m1 = cv1 ? 1.f : 0.f;
    const float* ar = &in[r16][4 * kq];
    const int c0 = col0 + r16, c1 = col0 + 16 + r16;
    const float bias0 = (op.b && cv0) ? op.b[c0] : 0.f, bias1 = (op.b && cv1) ? op.b[c1] : 0.f;  // in flight with the weights
    // Two register sets of weights (one 64-wide k-chunk each) ahead of the matrix work. Every
    // request is UNCONDITIONAL (chunk index clamped; a layer narrower than 256 re-requests its last
    // chunk) and the four chunk steps are unrolled at compile time, so the compiler can count the
    // loads in flight and wait for the older set only. (Requesting the whole layer in one burst of
    // four sets was measured too: no faster -- the CU's 64 B/clk load path serialises the eight
    // waves' bursts, 256 KB = 4k cycles per layer, and the last wave starts late.) Measured before (s_memtime stamps,
    // tools/chain_stamps.py): with the next chunk requested behind `if (more)` it waited for
    // everything in front of the matrix instructions, each chunk paid a full round trip (~2.7k
    // cycles) on top of its ~2k cycles of matrix work, and a 256x256 layer took ~23k cycles.
    const int nchunk = K >> 6;
    f32x4 wa[2][4], wb[2][4];
    auto fetch = [&](auto set_c, int chunk) __attribute__((always_inline)) {
      constexpr int set = decltype(set_c)::value;
      const int kc = (chunk < nchunk ? chunk : nchunk - 1) * 64;
      static_for<0, 4>([&](auto j) __attribute__((always_inline)) {
        constexpr int jj = decltype(j)::value;
        wa[set][jj] = *reinterpret_cast<const f32x4*>(w0 + kc + 16 * jj);
        wb[set][jj] = *reinterpret_cast<const f32x4*>(w1 + kc + 16 * jj);
      });
    };
    fetch(std::integral_constant<int, 0>{}, 0);
    fetch(std::integral_constant<int, 1>{}, 1);
    SIMPB_STAMP(3 + 4 * o);
    static_for<0, 4>([&](auto c_c) __attribute__((always_inline)) {
      constexpr int c = decltype(c_c)::value;
      constexpr int set = c & 1;
      if (c < nchunk) {
        static_for<0, 4>([&](auto j) __attribute__((always_inline)) {
          constexpr int jj = decltype(j)::value;
          const float4 a = *reinterpret_cast<const float4*>(ar + c * 64 + 16 * jj);
          const f32x4 b0 = wa[set][jj], b1 = wb[set][jj];
          acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b0[0] * m0, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b1[0] * m1, acc1, 0, 0, 0);
          acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b0[1] * m0, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b1[1] * m1, acc1, 0, 0, 0);
          acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b0[2] * m0, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b1[2] * m1, acc1, 0, 0, 0);
          acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b0[3] * m0, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b1[3] * m1, acc1, 0, 0, 0);
        });
      }
      if constexpr (c + 2 < 4) fetch(std::integral_constant<int, set>{}, c + 2);
    });
    // C/D of the 16x16 tile: column = lane & 15, row = 4 * (lane >> 4) + reg
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v0 = acc0[r] + bias0, v1 = acc1[r] + bias1;
      if (cv0) out[4 * kq + r][c0] = op.relu ? fmaxf(v0, 0.f) : v0;
      if (cv1) out[4 * kq + r][c1] = op.relu ? fmaxf(v1, 0.f) : v1;
    }
  }
};

// ---- 4-row form on the 4x4 matrix blocks (weights_transposed == 2). The shipped one.
// Why: a chain over M = 900 rows in 16-row workgroups is 57 workgroups on 256 CUs (round-1 profile: MFMA busy 0.066, 64 %
// of wave cycles waiting), and a 16x16 tile cannot be made shorter without wasting it. v_mfma_f32_4x4x1f32 multiplies
// SIXTEEN independent 4x4 blocks per instruction at the same flop rate: block b = output columns 4b..4b+3 of a wave's 64
// columns, the four rows of the block = the four rows of the workgroup, k advances by one per instruction. So 4 rows per
// workgroup lose nothing: 225 workgroups for 900 rows, each with a quarter of the matrix work per layer.
//   lane l = 4*b + j: A operand = x[row j][k] (LDS), B operand = W[column 64*wave + l][k], D[i] = out[row i][column].
// Weights come k4-packed, Wp[k / 4][column][k % 4] (host repack, plugin/fused.py): the B operands of four k for a
// lane are one 16-byte load, and a wave-load is 1 KiB contiguous. No weight staging through LDS, no barrier inside a layer.
// Measured (tools/chain_stamps.py, tools/bench_chain.py): ~10.4k cycles per 256x256 layer against ~19k for the 16-row kernel
// (refine3d chain 29.6 us vs 42.3 us, anchor encoder 14.1 vs 18.6, 2D encoder 20.1 vs 28.6). The layer time is the same for
// ONE busy wave (a 256 -> 11 head) as for four and does not change with eight accumulators, a branch-free step, or a
// rotated k order across workgroups: v_mfma_f32_4x4x1f32 issues once per ~38 cycles on gfx950, i.e. at a quarter of the
// 16x16x4 flop rate, so 4 rows per CU cost as many matrix cycles as 16 do. What is gained is the 4x CU count, not
// matrix efficiency; the floor left is the 256 KB of weights per layer through one CU's 64 B/clk load path (4k cycles).
// Also measured and dropped: 16 waves per workgroup with K split four ways and every weight of a layer requested up front
// (partials meeting in LDS): the single wide chain gains (refine3d 29.6 -> 24.2 us, ~7k cycles per layer) but launches of
// several chains lose more (anchor encoder 14.1 -> 60.6 us, refine2d 50.5 -> 78 us: 1024-thread workgroups, two per CU).
// This kernel keeps its OWN walk and LayerNorm stage over the shared load_tile, lead_norm_rows, linear_per_column and
// store_tile: through chain_walk<Form> and layernorm_rows (same arithmetic, same bits, same registers) the anchor encoder
// launch, which the frame runs seven times, took 14.8 us for the parent's 14.4 us -- 0.3 us in the LayerNorm stage, 0.1-0.2 us
// in the walk (profiles/mlp_chain_shared_parts.md, "What went back"). A change to the walk is made here as well.
__global__ __launch_bounds__(256) void mlp_chain_r4_kernel(simpb_mlp_args args) {
  constexpr int R = 4, LD = kLdAct, kThreads = 256;
  __shared__ float act[2][R][LD];
  const simpb_mlp_chain& ch = args.chain[blockIdx.y];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int row0 = blockIdx.x * R;
  if (skip_dead_rows(args, ch, row0, R, tid, kThreads)) return;
  const int N = args.num_rows;

  SIMPB_STAMP(0);
  if (ch.in_mode == SIMPB_MLP_IN_ROWS_LN) {
    lead_norm_rows<R, LD, 4>(act[0], args, ch, row0, tid);
    if (!ch.out) return;   // the `norm` operator alone (no chain behind it, workgroup-uniform): ln_out is the job's product
  } else {
    load_tile<R, LD, kThreads, false>(act[0], ch, row0, N, tid);
  }
  __syncthreads();
  SIMPB_STAMP(1);

  int cur = 0;
  int width = ch.in_mode == SIMPB_MLP_IN_SINE2D ? 256 : ch.in_dim;
  for (int o = 0; o < ch.n_ops; ++o) {
    const simpb_mlp_op& op = ch.ops[o];
    SIMPB_STAMP(2 + 4 * o);
    if (op.type == SIMPB_MLP_LINEAR) {
      const int K = op.in_dim, D = op.out_dim;
      if ((K & 3) == 0) {  // k4-packed weights
        if (wave * 64 < D) {
          const int n = tid;
          const bool cv = n < D;
          const float4* wp = reinterpret_cast<const float4*>(op.w) + (cv ? n : 0);
          const float* ar = &act[cur][lane & 3][0];
          const float bias = (op.b && cv) ? op.b[n] : 0.f;
          const int steps = K >> 2;                 // one step = 4 k = one 16-byte B load + one 16-byte A read
          f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
          constexpr int G = 8;                      // steps per register set; two sets in flight
          float4 wa[G], wb[G];
          auto fetch = [&](float4* dst, int g) __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < G; ++j) dst[j] = wp[(size_t)min(g * G + j, steps - 1) * D];  // unconditional, clamped
          };
          auto work = [&](const float4* w, int g) __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < G; ++j) {
              const int st = g * G + j;
              if (st < steps) {  // wave-uniform
                const float4 a = *reinterpret_cast<const float4*>(ar + 4 * st);
                acc0 = __builtin_amdgcn_mfma_f32_4x4x1f32(a.x, w[j].x, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_4x4x1f32(a.y, w[j].y, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_4x4x1f32(a.z, w[j].z, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_4x4x1f32(a.w, w[j].w, acc1, 0, 0, 0);
              }
            }
          };
          const int groups = (steps + G - 1) / G;
          fetch(wa, 0);
          SIMPB_STAMP(3 + 4 * o);
          for (int g = 0; g < groups; g += 2) {
            fetch(wb, g + 1);
            work(wa, g);
            fetch(wa, g + 2);
            if (g + 1 < groups) work(wb, g + 1);
          }
          if (cv) {
#pragma unroll
            for (int i = 0; i < R; ++i) {
              const float v = acc0[i] + acc1[i] + bias;
              act[cur ^ 1][i][n] = op.relu ? fmaxf(v, 0.f) : v;
            }
          }
        }
      } else {  // K = 2, 3, ...: weights as stored, [D][K]
        linear_per_column<R, LD>(act[cur], act[cur ^ 1], op, op.w + (size_t)tid * K, 1, tid);
      }
      SIMPB_STAMP(4 + 4 * o);
      __syncthreads();
      SIMPB_STAMP(5 + 4 * o);
      cur ^= 1;
      width = D;
    } else {
      // LayerNorm written out: wave r = row r, 64 lanes x 4 elements (layernorm_rows' arithmetic and request order)
      const int D = op.in_dim;
      const int r = wave;
      float g[kMaxDim / 64], be[kMaxDim / 64], v[kMaxDim / 64];
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < kMaxDim / 64; ++j) {
        const int e = lane + 64 * j;
        const bool in = e < D;
        g[j] = in ? op.w[e] : 0.f;
        be[j] = in ? op.b[e] : 0.f;
        v[j] = in ? act[cur][r][e] : 0.f;
        sum += v[j];
      }
      sum = WaveSum::sum(sum);
      const float mean = sum / (float)D;
      float q = 0.f;
#pragma unroll
      for (int j = 0; j < kMaxDim / 64; ++j) {
        const float d = (lane + 64 * j) < D ? v[j] - mean : 0.f;
        q += d * d;
      }
      q = WaveSum::sum(q);
      const float inv = 1.f / sqrtf(q / (float)D + 1e-5f);
#pragma unroll
      for (int j = 0; j < kMaxDim / 64; ++j) {
        const int e = lane + 64 * j;
        if (e < D) act[cur][r][e] = (v[j] - mean) * inv * g[j] + be[j];
      }
      SIMPB_STAMP(4 + 4 * o);
      __syncthreads();
      SIMPB_STAMP(5 + 4 * o);
    }
  }
  SIMPB_STAMP(126);
  store_tile<R, LD, kThreads>(act[cur], width, ch, row0, N, tid);
  SIMPB_STAMP(127);
}

// ---- 32-row form on the 32x32 matrix tiles (weights_transposed == 3), for launches with thousands of rows (a batch of
// camera streams per launch, runner independent_streams). The 4-row kernel above exists to spread ~1 k rows over 256 CUs; its
// v_mfma_f32_4x4x1f32 issues at a quarter of the fp32 matrix rate, and at ~9 k rows (bs = 8) that IS the bound: measured
// 33-36 TFLOP/s on every chain (refine2d 213 us, 2D encoder 64 us, per step of 8 frames), the 4x4x1 issue peak. Here:
//   one workgroup = 32 rows x 4 waves; the row tile lives in LDS between layers (two buffers, 66 KB: two workgroups per CU);
//   wave w owns output columns 64w..64w+63 = two 32x32 tiles of v_mfma_f32_32x32x2f32 (full fp32 matrix rate);
//   lane (r32, half) holds k = 16 * half + 0..15 of a 32-deep chunk of its A row (LDS, four ds_read_b128) and of its B
//   column (the same k permutation on both operands, as in csrc/gemm.hip), sixteen matrix steps per tile and chunk;
//   weights arrive FRAGMENT-PACKED by the host (plugin/fused.py): Wq[tile][chunk][q][lane][4] = W[32 tile + r32][32 chunk +
//   16 half + 4 q + 0..3], columns past out_dim as zeros -- a wave's B operand of a chunk is four fully coalesced 1-KiB
//   loads straight into registers (no staging, no barrier inside a layer), two chunks in flight, every request
//   unconditional with a clamped index so that the waits are counted.
// Layers with in_dim % 32 != 0 (the 2-, 3- and 12-wide first layers) take nn.Linear's layout on the vector units.
// Its LayerNorm stages run one wave per row, eight rows per wave.
struct R32Form {
  static constexpr int R = 32, WAVES = 4, LD = kLdAct;
  static constexpr bool kLeadNorm = true, kVecInput = false;
  static __device__ __forceinline__ void layernorm(float (&tile)[R][LD], const simpb_mlp_op& op, int tid) {
    layernorm_rows<R, LD, WAVES * 64, 64, WaveSum>(tile, op, tid);
  }

  static __device__ __forceinline__ void linear(const float (&in)[R][LD], float (&out)[R][LD], const simpb_mlp_op& op, int tid,
                                                int o) {
    const int K = op.in_dim, D = op.out_dim;
    if ((K & 31) != 0) {  // K = 2, 3, 12: weights as stored, [D][K]
      linear_per_column<R, LD>(in, out, op, op.w + (size_t)tid * K, 1, tid);
      return;
    }
    // fragment-packed weights
    const int lane = tid & 63, wave = tid >> 6;
    const int r32 = lane & 31, half = lane >> 5;
    const int ntile = (D + 31) >> 5, nchunk = K >> 5;
    const int t0 = 2 * wave;
    if (t0 >= ntile) return;
    const bool two = t0 + 1 < ntile;                  // wave-uniform
    const int t1 = two ? t0 + 1 : t0;                 // (a lone last tile is loaded twice and multiplied once)
    const f32x4* w0 = reinterpret_cast<const f32x4*>(op.w) + (size_t)t0 * nchunk * 256 + lane;
    const f32x4* w1 = reinterpret_cast<const f32x4*>(op.w) + (size_t)t1 * nchunk * 256 + lane;
    const float* ar = &in[r32][16 * half];
    f32x16 acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
    f32x4 wa[2][4], wb[2][4];
    auto fetch = [&](auto set_c, int chunk) __attribute__((always_inline)) {
      constexpr int set = decltype(set_c)::value;
      const int c = min(chunk, nchunk - 1);           // unconditional, clamped: past the end the last chunk again
      static_for<0, 4>([&](auto q) __attribute__((always_inline)) {
        constexpr int qq = decltype(q)::value;
        wa[set][qq] = w0[(size_t)c * 256 + 64 * qq];
        wb[set][qq] = w1[(size_t)c * 256 + 64 * qq];
      });
    };
    auto work = [&](auto set_c, int chunk) __attribute__((always_inline)) {
      constexpr int set = decltype(set_c)::value;
      f32x4 a[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) a[q] = *reinterpret_cast<const f32x4*>(ar + 32 * chunk + 4 * q);
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q][e], wa[set][q][e], acc0, 0, 0, 0);
      if (two) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q][e], wb[set][q][e], acc1, 0, 0, 0);
      }
    };
    fetch(std::integral_constant<int, 0>{}, 0);
    SIMPB_STAMP(3 + 4 * o);
    for (int c = 0; c < nchunk; c += 2) {
      fetch(std::integral_constant<int, 1>{}, c + 1);
      work(std::integral_constant<int, 0>{}, c);
      fetch(std::integral_constant<int, 0>{}, c + 2);
      if (c + 1 < nchunk) work(std::integral_constant<int, 1>{}, c + 1);
    }
    // C/D of a 32x32 tile: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * half
    const int c0 = 32 * t0 + r32, c1 = 32 * t0 + 32 + r32;
    const bool cv0 = c0 < D, cv1 = two && c1 < D;
    const float bias0 = (op.b && cv0) ? op.b[c0] : 0.f, bias1 = (op.b && cv1) ? op.b[c1] : 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int rr = (i & 3) + 8 * (i >> 2) + 4 * half;
      const float v0 = acc0[i] + bias0, v1 = acc1[i] + bias1;
      if (cv0) out[rr][c0] = op.relu ? fmaxf(v0, 0.f) : v0;
      if (cv1) out[rr][c1] = op.relu ? fmaxf(v1, 0.f) : v1;
    }
  }
};

// ---------------------------------------------------------------------------------------------- the kernels
template <int R, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void mlp_chain_kernel(simpb_mlp_args args) { chain_walk<ValuForm<R, WAVES>>(args); }
__global__ __launch_bounds__(R16Form::WAVES * 64) void mlp_chain_mfma_kernel(simpb_mlp_args args) { chain_walk<R16Form>(args); }
__global__ __launch_bounds__(256, 2) void mlp_chain_r32_kernel(simpb_mlp_args args) { chain_walk<R32Form>(args); }

// args.weights_transposed -> kernel, threads, rows per workgroup, leading norm
struct ChainForm {
  void (*kernel)(simpb_mlp_args);
  int threads, rows;
  bool lead_norm;
};
template <class F>
constexpr ChainForm form_of(void (*kernel)(simpb_mlp_args)) { return {kernel, F::WAVES * 64, F::R, F::kLeadNorm}; }
const ChainForm kForms[4] = {
    form_of<R16Form>(mlp_chain_mfma_kernel),        // 0: nn.Linear's own [out][in] layout
    form_of<ValuForm<4, 8>>(mlp_chain_kernel<4, 8>),  // 1: weights [in][out], split-K with 16-byte weight loads
    {mlp_chain_r4_kernel, 256, 4, true},            // 2: k4-packed weights (the kernel with its own walk)
    // 3: fragment-packed weights, launches with thousands of rows. (Four register sets = three chunks in flight ahead of the
    // one multiplied: 152 vs 147 us for refine2d, no better; 8 waves with one column tile each were measured too: refine2d
    // 204 us against 147 us at 8.9 k rows -- every wave re-reads the A tile, and half the B registers in flight per wave.)
    form_of<R32Form>(mlp_chain_r32_kernel),
};

}  // namespace

extern "C" int simpb_mlp_chain_forward(const simpb_mlp_args* args, void* stream) {
  if (!args || args->num_rows <= 0 || args->num_chains <= 0 || args->num_chains > SIMPB_MLP_MAX_CHAINS)
    return SIMPB_EINVAL;
  const int wt = args->weights_transposed;
  const ChainForm& form = kForms[wt == 2 || wt == 3 ? wt : wt != 0];   // (any other non-zero value: the VALU form)
  for (int c = 0; c < args->num_chains; ++c) {
    const simpb_mlp_chain& ch = args->chain[c];
    if (!ch.x || ch.n_ops < 0 || ch.n_ops > SIMPB_MLP_MAX_OPS) return SIMPB_EINVAL;
    // no `out`: the leading LayerNorm stage alone -- IN_ROWS_LN with ln_out and no op behind it
    if (!ch.out && (ch.in_mode != SIMPB_MLP_IN_ROWS_LN || !ch.ln_out || ch.n_ops != 0)) return SIMPB_EINVAL;
    int width = ch.in_mode == SIMPB_MLP_IN_SINE2D ? 256 : ch.in_dim;
    if (width <= 0 || width > kMaxDim) return SIMPB_EINVAL;
    if (ch.post < 0 || ch.post > SIMPB_MLP_POST_SIGMOID) return SIMPB_EINVAL;
    if ((ch.post == SIMPB_MLP_POST_REFINE3D || ch.post == SIMPB_MLP_POST_REFINE2D) && (!ch.res || ch.ldres < ch.res_cols))
      return SIMPB_EINVAL;
    if (ch.post == SIMPB_MLP_POST_REFINE3D && ch.div && ch.div_rows <= 0) return SIMPB_EINVAL;
    if (ch.in_mode == SIMPB_MLP_IN_SINE2D && ch.ldx < 2) return SIMPB_EINVAL;
    if (ch.in_mode == SIMPB_MLP_IN_ROWS_LN && (!form.lead_norm || !ch.ln_w || !ch.ln_b || (ch.ln_out && ch.ld_ln_out < ch.in_dim)))
      return SIMPB_EINVAL;
    if (ch.in_mode < 0 || ch.in_mode > SIMPB_MLP_IN_ROWS_LN) return SIMPB_EINVAL;
    for (int o = 0; o < ch.n_ops; ++o) {
      const simpb_mlp_op& op = ch.ops[o];
      if (op.type == SIMPB_MLP_LINEAR) {
        if (!op.w || op.in_dim != width || op.out_dim <= 0 || op.out_dim > kMaxDim) return SIMPB_EINVAL;
        width = op.out_dim;
      } else if (op.type == SIMPB_MLP_LAYERNORM) {
        if (!op.w || !op.b || op.in_dim != width) return SIMPB_EINVAL;
      } else {
        return SIMPB_EINVAL;
      }
    }
  }
  (void)hipGetLastError();
  dim3 grid((args->num_rows + form.rows - 1) / form.rows, args->num_chains);
  hipLaunchKernelGGL(form.kernel, grid, dim3(form.threads), 0, static_cast<hipStream_t>(stream), *args);
  return simpb_check_launch();
}
