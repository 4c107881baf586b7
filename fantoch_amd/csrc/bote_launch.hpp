// bote_launch.hpp — the two host helpers every kernel family's launcher
// shares (bote_group.hip, bote_sweep.hip, bote_kernels.hip).  A family keeps
// one selector that maps its arguments to a kernel (`const void*`); the
// occupancy query and the launch both go through it, so the persistent grid
// is sized by the kernel that runs.
#pragma once
#include <hip/hip_runtime.h>

namespace bote {

// Workgroups per CU of kernel `k` at `bd` threads and `shm` bytes of dynamic
// LDS; `on_fail` when the runtime refuses the query or reports none.
inline int kernel_occupancy(const void* k, uint32_t bd, size_t shm, int on_fail) {
  int nb = 0;
  if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm) != hipSuccess) return on_fail;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k, (int)bd, shm) != hipSuccess) return on_fail;
  return nb > 0 ? nb : on_fail;
}

// Launches kernel `k`, whose one parameter is `args` by value.  Timed
// launches (e0, e1) carry their events in the dispatch: no marker packets
// before and after the kernel, which cost ~10 us of idle GPU each.
template <class Args>
inline hipError_t launch_kernel(const void* k, Args args, uint32_t grid, uint32_t bd, size_t shm, hipStream_t st,
                                hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr) {
  hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
  if (e != hipSuccess) return e;
  void* params[] = {&args};
  if (e0) (void)hipExtLaunchKernel(k, dim3(grid), dim3(bd), params, (uint32_t)shm, st, e0, e1, 0);
  else (void)hipLaunchKernel(k, dim3(grid), dim3(bd), params, shm, st);
  return hipGetLastError();
}

}  // namespace bote
