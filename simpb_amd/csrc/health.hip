// Camera health (include/simpb_hip.h, "Camera health"): integer statistics of every image the ingest wrote, and the verdict
// that turns them into the camera mask the decoder of the same frame reads. Two launches behind the ingest, on its stream.
//
// image_health_stats_kernel: one workgroup per (image, band) -- a band is an eighth of the rows of one cell row, so 64 bands
// an image and 384 workgroups at six 256 x 704 images. A band's rows are one contiguous run of 8-byte pixels: it is read once
// with 16-byte loads (two pixels a lane, consecutive lanes consecutive pairs); an image starts on an 8-byte boundary only, so
// a run that begins or ends off a 16-byte one has its first / last pixel taken by one lane with an 8-byte load. Each lane
// keeps the 8 x 3 cell-column sums, its hash part and its non-finite count in registers; the waves reduce by shuffles, the
// workgroup through LDS, and 26 threads write the band's ONE partial row with plain stores. No global atomics, nothing to
// zero between frames, no ticket: the verdict launch adds the rows in band order (integers: any order gives the same bits).
//
// camera_health_verdict_kernel: one workgroup per stream, its cameras in turn. float64 with one rounding per operation
// (contraction off for this file), so numpy float64 gives the same bits.
#include <hip/hip_runtime.h>
#include "../../include/simpb_hip.h"
#include "store_fence.h"

#include "launch.h"

#pragma clang fp contract(off)

namespace {

constexpr int kG = SIMPB_HEALTH_GRID;
constexpr int kSub = SIMPB_HEALTH_BANDS / kG;
constexpr int kWords = SIMPB_HEALTH_PARTIAL_WORDS;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxCams = 64;
static_assert(kWords == kG * 3 + 2 && SIMPB_HEALTH_BANDS == kG * kSub, "partial row layout");

__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

struct Acc {
  long long s[kG * 3];
  unsigned long long hash;
  unsigned nonfinite;
};

// One pixel: lo = channels 0 | 1 << 16, hi = channel 2 (its upper half, channel 3, is dropped here). q: the pixel's index in
// its image, col: its cell column.
__device__ __forceinline__ void take(Acc& a, unsigned lo, unsigned hi, unsigned q, int col) {
  const unsigned bits[3] = {lo & 0xFFFFu, lo >> 16, hi & 0xFFFFu};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const unsigned b = bits[k], e = (b >> 10) & 31u, m = b & 1023u;
    // x * 2^24: a subnormal is m * 2^-24, a normal (1024 + m) * 2^(e - 25)
    long long v = e ? (long long)((unsigned long long)(1024u | m) << (e - 1u)) : (long long)m;
    if (b & 0x8000u) v = -v;
    if (e == 31u) { v = 0; a.nonfinite += 1u; }
#pragma unroll
    for (int j = 0; j < kG; ++j) a.s[j * 3 + k] += (j == col) ? v : 0ll;   // selected, not indexed: the sums stay in registers
    a.hash += mix64((unsigned long long)b | ((unsigned long long)(q * 3u + (unsigned)k) << 16));
  }
}

__device__ __forceinline__ int cell_column(unsigned x, int width) {
  int col = 0;
#pragma unroll
  for (int j = 1; j < kG; ++j) col += x >= (unsigned)(j * width / kG) ? 1 : 0;
  return col;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += (unsigned long long)__shfl_xor((long long)v, d, 64);
  return v;
}

__global__ __launch_bounds__(kThreads) void image_health_stats_kernel(unsigned long long* __restrict__ partials,
                                                                      const uint2* __restrict__ images, int height, int width) {
  __shared__ unsigned long long s_part[kWaves][kWords];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int band = blockIdx.x, n = blockIdx.y;
  const int i = band / kSub, sub = band % kSub;
  const int r0 = i * height / kG, rows = (i + 1) * height / kG - r0;
  const unsigned p0 = (unsigned)(r0 + sub * rows / kSub) * (unsigned)width;         // the band's pixels: [p0, p1) of the image
  const unsigned p1 = (unsigned)(r0 + (sub + 1) * rows / kSub) * (unsigned)width;
  const uint2* img = images + (size_t)n * height * width;
  // the first pixel that sits on a 16-byte boundary (p1 where the band is empty or ends before one)
  unsigned pa = p0 + ((reinterpret_cast<size_t>(img + p0) & 15) ? 1u : 0u);
  if (pa > p1) pa = p1;
  const unsigned pairs = (p1 - pa) >> 1;

  Acc a;
#pragma unroll
  for (int k = 0; k < kG * 3; ++k) a.s[k] = 0;
  a.hash = 0ull;
  a.nonfinite = 0u;

  if (tid == 0 && pa > p0) {   // head: one pixel in front of the boundary
    const uint2 v = img[p0];
    take(a, v.x, v.y, p0, cell_column(p0 % (unsigned)width, width));
  }
  if (tid == 64 && ((p1 - pa) & 1u)) {   // tail: one pixel behind the last whole pair
    const uint2 v = img[p1 - 1u];
    take(a, v.x, v.y, p1 - 1u, cell_column((p1 - 1u) % (unsigned)width, width));
  }
  const uint4* pair = reinterpret_cast<const uint4*>(img + pa);
  for (unsigned t = tid; t < pairs; t += kThreads) {
    const uint4 v = pair[t];
    const unsigned q = pa + 2u * t;
    const unsigned x = q % (unsigned)width;
    const unsigned x1 = x + 1u == (unsigned)width ? 0u : x + 1u;
    take(a, v.x, v.y, q, cell_column(x, width));
    take(a, v.z, v.w, q + 1u, cell_column(x1, width));
  }
  simpb::loads_retired();   // store_fence.h: nothing below loads from global memory

  unsigned long long w[kWords];
#pragma unroll
  for (int k = 0; k < kG * 3; ++k) w[k] = wave_sum((unsigned long long)a.s[k]);
  w[kG * 3] = wave_sum(a.hash);
  w[kG * 3 + 1] = wave_sum((unsigned long long)a.nonfinite);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kWords; ++k) s_part[wave][k] = w[k];
  }
  __syncthreads();
  if (tid < kWords) {
    unsigned long long sum = 0ull;
#pragma unroll
    for (int v = 0; v < kWaves; ++v) sum += s_part[v][tid];
    simpb::pin(sum);
    partials[((size_t)n * SIMPB_HEALTH_BANDS + band) * kWords + tid] = sum;
  }
}

// ((sum / denom) * std + mean) per channel, then the mean of the three: one rounding per operation. Plain operators under
// this file's `fp contract(off)` (the __dmul_rn family of the HIP headers is compiled under the headers' own setting and
// does get contracted into an FMA once inlined).
__device__ __forceinline__ double level_of(const long long* sum3, double denom, const simpb_health_params& p) {
  double l[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) l[k] = ((double)sum3[k] / denom) * p.std[k] + p.mean[k];
  return ((l[0] + l[1]) + l[2]) / 3.0;
}

__global__ __launch_bounds__(kThreads) void camera_health_verdict_kernel(
    unsigned char* __restrict__ cam_out, unsigned char* __restrict__ flags, simpb_health_state* __restrict__ state,
    const long long* __restrict__ partials, const unsigned char* __restrict__ cam_in,
    const unsigned char* __restrict__ active, const simpb_health_params p, int num_cams, int height, int width) {
  __shared__ long long s_cell[kG][kWords];     // cell row i of the camera in hand: S[i][j][k], hash part, non-finite count
  __shared__ double s_lc[kG * kG];
  __shared__ unsigned char s_flags[kMaxCams], s_in[kMaxCams], s_considered[kMaxCams];
  __shared__ unsigned long long s_hash[kMaxCams];
  __shared__ unsigned s_repeats[kMaxCams], s_frames[kMaxCams];
  const int s = blockIdx.x, tid = threadIdx.x;
  const bool on = active == nullptr || active[s] != 0;

#pragma nounroll
  for (int c = 0; c < num_cams; ++c) {   // (every condition below is the same for the whole workgroup)
    const size_t n = (size_t)s * num_cams + c;
    const bool in = cam_in == nullptr || cam_in[n] != 0;
    const bool considered = on && in;
    if (tid == 0) { s_in[c] = in; s_considered[c] = considered; s_flags[c] = 0; }
    if (!considered) continue;
    if (tid < kG * kWords) {   // the camera's 64 partial rows, added in band order
      const int i = tid / kWords, wd = tid % kWords;
      const long long* row = partials + (n * SIMPB_HEALTH_BANDS + (size_t)i * kSub) * kWords + wd;
      long long sum = 0;
#pragma unroll
      for (int b = 0; b < kSub; ++b) sum += row[(size_t)b * kWords];
      s_cell[i][wd] = sum;
    }
    __syncthreads();
    if (tid < kG * kG) {
      const int i = tid / kG, j = tid % kG;
      const int nr = (i + 1) * height / kG - i * height / kG, nc = (j + 1) * width / kG - j * width / kG;
      s_lc[tid] = level_of(&s_cell[i][j * 3], (double)(nr * nc) * 16777216.0, p);
    }
    __syncthreads();
    if (tid == 0) {
      long long total[3] = {0, 0, 0};
      unsigned long long hash = 0ull;
      long long nonfinite = 0;
      double lo = s_lc[0], hi = s_lc[0];
#pragma nounroll
      for (int i = 0; i < kG; ++i) {
#pragma nounroll
        for (int j = 0; j < kG; ++j) {
#pragma unroll
          for (int k = 0; k < 3; ++k) total[k] += s_cell[i][j * 3 + k];
          const double v = s_lc[i * kG + j];
          lo = v < lo ? v : lo;
          hi = v > hi ? v : hi;
        }
        hash += (unsigned long long)s_cell[i][kG * 3];
        nonfinite += s_cell[i][kG * 3 + 1];
      }
      const double level = level_of(total, (double)(height * width) * 16777216.0, p);
      const simpb_health_state st = state[n];
      const unsigned repeats = (st.frames > 0u && st.prev_hash == hash) ? st.repeats + 1u : 0u;
      unsigned f = 0u;
      if (p.check_dark && level < p.dark_below) f |= SIMPB_HEALTH_DARK;
      if (p.check_bright && level > p.bright_above) f |= SIMPB_HEALTH_BRIGHT;
      if (p.check_flat && hi - lo < p.flat_below) f |= SIMPB_HEALTH_FLAT;
      if (p.check_frozen && repeats >= (unsigned)p.frozen_after) f |= SIMPB_HEALTH_FROZEN;
      if (nonfinite > 0) f |= SIMPB_HEALTH_NONFINITE;
      s_flags[c] = (unsigned char)f;
      s_hash[c] = hash;
      s_repeats[c] = repeats;
      s_frames[c] = st.frames + 1u;
    }
    __syncthreads();   // (s_cell and s_lc are the next camera's from here)
  }
  __syncthreads();
  simpb::loads_retired();   // store_fence.h: every partial row and state row is in; only stores from here

  if (tid < num_cams) {
    bool any = false, all_fault = true;
    for (int c = 0; c < num_cams; ++c) {
      if (s_considered[c]) { any = true; all_fault = all_fault && s_flags[c] != 0; }
    }
    const bool fail_open = any && all_fault;
    const size_t n = (size_t)s * num_cams + tid;
    unsigned f = s_flags[tid];
    if (s_considered[tid]) {
      if (fail_open) f |= SIMPB_HEALTH_FAIL_OPEN;
      simpb_health_state st;
      st.prev_hash = s_hash[tid];
      st.repeats = s_repeats[tid];
      st.frames = s_frames[tid];
      state[n] = st;
    }
    const bool drop = (f & ~(unsigned)SIMPB_HEALTH_FAIL_OPEN) != 0u && p.act != 0 && !fail_open;
    flags[n] = (unsigned char)f;
    cam_out[n] = (s_in[tid] && !drop) ? 1 : 0;
  }
}

bool sizes_ok(int num_images, int height, int width) {
  return num_images >= 1 && num_images <= 65535 && height >= kG && width >= kG && height <= 16384 && width <= 16384;
}

bool is_finite(double v) { return v == v && v - v == 0.0; }

}  // namespace

extern "C" int simpb_image_health_partials_bytes(int num_images, int height, int width) {
  if (!sizes_ok(num_images, height, width)) return SIMPB_EINVAL;
  return num_images * SIMPB_HEALTH_BANDS * kWords * 8;
}

extern "C" int simpb_image_health_stats(long long* partials, const void* images, int num_images, int height, int width,
                                        void* stream) {
  if (!partials || !images || !sizes_ok(num_images, height, width) || (reinterpret_cast<size_t>(partials) & 7) ||
      (reinterpret_cast<size_t>(images) & 7))
    return SIMPB_EINVAL;
  (void)hipGetLastError();
  hipLaunchKernelGGL(image_health_stats_kernel, dim3(SIMPB_HEALTH_BANDS, num_images), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), reinterpret_cast<unsigned long long*>(partials),
                     static_cast<const uint2*>(images), height, width);
  return simpb_check_launch();
}

extern "C" int simpb_camera_health_verdict(unsigned char* cam_out, unsigned char* flags, simpb_health_state* state,
                                           const long long* partials, const unsigned char* cam_in,
                                           const unsigned char* active, simpb_health_params params, int batch_size,
                                           int num_cams, int height, int width, void* stream) {
  if (!cam_out || !flags || !state || !partials || batch_size < 1 || batch_size > 65535 || num_cams < 1 || num_cams > kMaxCams ||
      !sizes_ok(1, height, width) || (long long)batch_size * num_cams > 65535 || (reinterpret_cast<size_t>(partials) & 7) ||
      (reinterpret_cast<size_t>(state) & 7))
    return SIMPB_EINVAL;
  if ((params.check_dark && !is_finite(params.dark_below)) || (params.check_bright && !is_finite(params.bright_above)) ||
      (params.check_flat && !is_finite(params.flat_below)) || (params.check_frozen && params.frozen_after < 1))
    return SIMPB_EINVAL;
  for (int k = 0; k < 3; ++k)
    if (!is_finite(params.mean[k]) || !is_finite(params.std[k]) || !(params.std[k] > 0.0)) return SIMPB_EINVAL;
  (void)hipGetLastError();
  hipLaunchKernelGGL(camera_health_verdict_kernel, dim3(batch_size), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     cam_out, flags, state, partials, cam_in, active, params, num_cams, height, width);
  return simpb_check_launch();
}
