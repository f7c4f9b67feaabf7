// Shared helpers for libvqvae_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <mutex>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../include/vqvae_hip.h"

namespace vq {

void set_error(const char* fmt, ...);

#define VQ_CHECK_HIP(expr)                                                        \
  do {                                                                            \
    hipError_t _e = (expr);                                                       \
    if (_e != hipSuccess) {                                                       \
      vq::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr,                 \
                    hipGetErrorString(_e));                                       \
      return (int)_e;                                                             \
    }                                                                             \
  } while (0)

#define VQ_REQUIRE(cond, ...)                                                     \
  do {                                                                            \
    if (!(cond)) {                                                                \
      vq::set_error(__VA_ARGS__);                                                 \
      return VQVAE_E_INVALID;                                                     \
    }                                                                             \
  } while (0)

#define VQ_LAUNCH_CHECK()                                                         \
  do {                                                                            \
    hipError_t _e = hipGetLastError();                                            \
    if (_e != hipSuccess) {                                                       \
      vq::set_error("%s:%d: kernel launch -> %s", __FILE__, __LINE__,             \
                    hipGetErrorString(_e));                                       \
      return (int)_e;                                                             \
    }                                                                             \
  } while (0)

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// Offsets into a caller-provided workspace, handed out in order; every piece starts on a 256-byte boundary and is padded
// to the next one.  One plan function per entry-point family builds a struct of named offsets with it, and both the
// *_workspace_bytes query and the entry point call that function.
struct WsPlan {
  size_t total = 0;
  size_t take(size_t bytes, size_t align = 256) {      // returns the piece's offset, advances total
    const size_t at = align_up(total, align);
    total = at + align_up(bytes, align);
    return at;
  }
};

// Makes `lds` bytes of dynamic LDS launchable for `Kernel` on the CURRENT device (64 KB or less needs no asking).  Cheap
// after the first call for a (kernel, device) pair; asks again only when a larger size is needed than was granted before.
// The state is per kernel, not per kernel type.  Errors carry the caller's file and line.
template <auto Kernel>
int lds_opt_in(size_t lds, const char* file = __builtin_FILE(), int line = __builtin_LINE()) {
  if (lds <= 64 * 1024) return 0;
  constexpr int kDevices = 64;                           // devices beyond the table are asked for every time
  static std::atomic<size_t> granted[kDevices] = {};
  static std::mutex mu;                                  // a smaller request must not land after a larger one
  int dev = -1;
  hipError_t e = hipGetDevice(&dev);
  const bool tabled = e == hipSuccess && dev >= 0 && dev < kDevices;
  if (tabled && granted[dev].load(std::memory_order_acquire) >= lds) return 0;
  if (e == hipSuccess) {
    std::lock_guard<std::mutex> lock(mu);
    if (tabled && granted[dev].load(std::memory_order_relaxed) >= lds) return 0;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess && tabled) granted[dev].store(lds, std::memory_order_release);
  }
  if (e != hipSuccess) set_error("%s:%d: %zu bytes of dynamic LDS -> %s", file, line, lds, hipGetErrorString(e));
  return (int)e;
}

// profiling hooks (runtime.hip): bracket a launch with events when enabled
void prof_begin(int tag, hipStream_t s);
void prof_end(int tag, hipStream_t s);

struct ProfScope {
  int tag; hipStream_t s;
  ProfScope(int t, hipStream_t st) : tag(t), s(st) { if (tag) prof_begin(tag, s); }
  ~ProfScope() { if (tag) prof_end(tag, s); }
};

// A launch timed by the events of its OWN dispatch packet (hipExtLaunchKernelGGL(start, stop)): no event packets
// before and after the kernel on the stream -- those cost ~5.6 us of idle queue each, 0.22 ms per step when the 20 gate
// launches of the bench are timed (tools/phase_trace.py).  prof_attach returns false when the tag is not enabled.
bool prof_attach(int tag, hipEvent_t* start, hipEvent_t* stop);
bool prof_enabled(int tag);

}  // namespace vq
