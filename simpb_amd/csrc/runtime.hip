// Host-side runtime of the library, no kernel: the ABI version, the launch check with the last error's text, and the
// optional per-launch HIP-event timing. The internal prototypes are in csrc/launch.h.
#include <hip/hip_runtime.h>
#include "../../include/simpb_hip.h"
#include "launch.h"

// 2: simpb_mlp_chain gained the post stage (8 chains per launch); 3: simpb_bank_cache takes the hold flags, the 3D
// record carries the int64 track id in two lanes (15 columns); 5: simpb_gemm_job gained the LayerNorm prologue fields,
// new entry points simpb_dfa_fused_forward / simpb_aggregate_2d_to_3d_alpha
extern "C" int simpb_abi_version(void) { return 7; }

// ---- optional per-launch HIP-event timing (bench.py's roofline leg). Events are recorded on the
// launch stream immediately around the kernel launch, inside the same C call, so the interval
// holds the kernel and not the host's time to get from one Python statement to the next.
namespace {
struct TimingSlot { hipEvent_t start, stop; int kernel_id; };
TimingSlot* g_slots = nullptr;
int g_capacity = 0, g_used = 0;
}  // namespace

extern "C" int simpb_timing_enable(int capacity) {
  if (capacity < 0) return SIMPB_EINVAL;
  for (int i = 0; i < g_capacity; ++i) { hipEventDestroy(g_slots[i].start); hipEventDestroy(g_slots[i].stop); }
  delete[] g_slots;
  g_slots = nullptr; g_capacity = 0; g_used = 0;
  if (capacity == 0) return SIMPB_OK;
  g_slots = new TimingSlot[capacity];
  for (int i = 0; i < capacity; ++i) {
    if (hipEventCreate(&g_slots[i].start) != hipSuccess || hipEventCreate(&g_slots[i].stop) != hipSuccess) return SIMPB_ELAUNCH;
    g_slots[i].kernel_id = -1;
  }
  g_capacity = capacity;
  return SIMPB_OK;
}

extern "C" int simpb_timing_begin(int kernel_id, void* stream) {  // returns slot or -1
  if (g_used >= g_capacity) return -1;
  const int i = g_used++;
  g_slots[i].kernel_id = kernel_id;
  hipEventRecord(g_slots[i].start, static_cast<hipStream_t>(stream));
  return i;
}

extern "C" void simpb_timing_end(int slot, void* stream) {
  if (slot >= 0 && slot < g_capacity) hipEventRecord(g_slots[slot].stop, static_cast<hipStream_t>(stream));
}

extern "C" int simpb_timing_read(int kernel_id, float* ms_out, int max_n) {
  if (!ms_out || max_n < 0) return -1;
  int n = 0;
  for (int i = 0; i < g_used && n < max_n; ++i) {
    if (g_slots[i].kernel_id != kernel_id) continue;
    float ms = 0.f;
    if (hipEventSynchronize(g_slots[i].stop) != hipSuccess) return -1;
    if (hipEventElapsedTime(&ms, g_slots[i].start, g_slots[i].stop) != hipSuccess) return -1;
    ms_out[n++] = ms;
  }
  return n;
}

extern "C" void simpb_timing_reset(void) { g_used = 0; }

// Text of the last HIP error seen by simpb_check_launch() on this thread ("" if none).
static thread_local const char* g_last_error = "";
extern "C" const char* simpb_last_error(void) { return g_last_error; }
extern "C" int simpb_check_launch(void) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return SIMPB_OK;
  g_last_error = hipGetErrorString(e);
  return SIMPB_ELAUNCH;
}
