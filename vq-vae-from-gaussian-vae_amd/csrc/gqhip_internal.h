// gqhip_internal.h -- what the translation units of libgqhip.so share on the host side.
#pragma once
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include "gqhip.h"

namespace gqhip {
extern thread_local int g_last_hip_error;   // last hipError_t seen by a failing call on this thread (gqhip_last_hip_error)
int check_launch();                          // hipGetLastError() -> GQHIP_OK / GQHIP_ERR_LAUNCH

// A start / stop event pair of the profiling recorder (gqhip.hip), taken for one dispatch; `on` is false when profiling is off,
// `enable` is, or the pool is empty.
struct ProfScope {
  hipEvent_t a = nullptr, b = nullptr;
  bool on = false;
  explicit ProfScope(bool enable = true);
  ~ProfScope();
  ProfScope(const ProfScope &) = delete;
  ProfScope &operator=(const ProfScope &) = delete;
};

// The one launch path.  `kernel` is what a kernel-choice function returned: nullptr (no instantiation serves the shape) is
// GQHIP_ERR_INVALID_ARG.  Arguments are converted to the kernel's parameter types, as a direct call would.
template <class... P, class... A>
int launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, A &&...args) {
  if (!kernel) return GQHIP_ERR_INVALID_ARG;
  hipLaunchKernelGGL(kernel, grid, block, lds, st, static_cast<P>(args)...);
  return check_launch();
}
// ... with the event pair of `prof` attached to the dispatch when it holds one
template <class... P, class... A>
int launch(const ProfScope &prof, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, A &&...args) {
  if (!prof.on) return launch(kernel, grid, block, lds, st, static_cast<A &&>(args)...);
  if (!kernel) return GQHIP_ERR_INVALID_ARG;
  hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)lds, st, prof.a, prof.b, 0, static_cast<P>(args)...);
  return check_launch();
}
}  // namespace gqhip
