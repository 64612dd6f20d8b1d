// rl_env_history.hip - the observation-history launch of the env library (include/rl_env.h rl_env_set_obs_history), gfx950.
//
// A translation unit of its own: it includes nothing a step kernel includes, so the step kernels' code objects do not depend on it.
// Pure data movement: one thread per output element (env, column) of the flattened [N][hist_dim] row spaces of both groups, the
// policy group's elements first, 256-thread workgroups.  Consecutive threads handle consecutive columns of a row, so the dword
// stores of a wavefront are one contiguous run and the loads from the previous slot are, too, inside a term block (the rows - 45 x H
// columns, terms of 3 - are not 16-byte aligned: nothing wider than a dword is used).  No LDS, no atomics, no loop.
#include <hip/hip_runtime.h>

#include "env_history.h"

namespace {
__global__ __launch_bounds__(256) void history_kernel(rl::HistArgsT<float> A) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < A.total) rl::history_element(A, i);
}
}  // namespace

// launcher for csrc/rl_env.hip (Backend::launch_history); returns the hipError_t of the launch
extern "C" __attribute__((visibility("hidden"))) int rl_env_launch_history(const void* args, void* stream) {
  const rl::HistArgsT<float>& A = *static_cast<const rl::HistArgsT<float>*>(args);
  if (A.total == 0u) return (int)hipSuccess;
  hipLaunchKernelGGL(history_kernel, dim3((A.total + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, A);
  return (int)hipGetLastError();
}
