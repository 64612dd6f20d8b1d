// rl_rnd.hip - the intrinsic reward of random network distillation inside the collection loop, for gfx950 (MI355X).  C-ABI, the rule and the
// order of every sum: include/rl_rnd.h (the definition is robot_lab_amd/rnd.py).
//
//   rows / step  a workgroup of 256 is 16 rows x 16 lanes: lane j of a row adds (double)d * d over the columns j, j + 16, ... (consecutive lanes
//                read consecutive floats of both embeddings), the 16 sums fold through the xor butterfly 8, 4, 2, 1.  K = 1 (rsl_rl's default)
//                leaves 15 lanes of a row idle: at 4096 envs that is 256 workgroups of a few hundred cycles, behind an env step of tens of us.
//   finish       one thread per row.
//   sums         one workgroup of 64 over the (step, workgroup) partials in order.
// Built with -ffp-contract=off: avg gamma + r, r / std, r weight and slot + r are separate fp32 roundings, as in torch.
#include <hip/hip_runtime.h>

#include <math.h>
#include <cmath>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/rl_rnd.h"

#pragma clang fp contract(off)

struct rl_rnd_reward {
  int N = 0, K = 0, T = 0, device = 0;
  float gamma = 0.f;
  float *r = nullptr, *avg = nullptr, *weights = nullptr;
  double* part = nullptr;  // [T][row_blocks][2]: per workgroup the sums of r_int and of the new slot values
  double* sums = nullptr;  // [2]
  int row_blocks = 0;      // workgroups of the 16-row launches (the stride of `part`; the finish launch uses fewer)
  int used_blocks = 0;     // workgroups per step that wrote partials in the last loop
  std::vector<float> host_weights;
};

namespace {

constexpr int BLOCK = 256, ROW_LANES = 16, ROWS_PER_BLOCK = BLOCK / ROW_LANES;

thread_local std::string g_err;
int fail(const std::string& m) {
  g_err = m;
  return -1;
}

// sqrt(sum_k d_k^2) of row `row` in every one of its 16 lanes (rows past the end: 0, nothing is read)
__device__ __forceinline__ float row_norm(const float* pred, const float* targ, int row, int j, int N, int K) {
  double s = 0.0;
  if (row < N) {
    const float* p = pred + (size_t)row * K;
    const float* t = targ + (size_t)row * K;
    for (int k = j; k < K; k += ROW_LANES) {
      const float d = t[k] - p[k];
      s += (double)d * (double)d;
    }
  }
  for (int w = ROW_LANES / 2; w > 0; w >>= 1) s += __shfl_xor(s, w, ROW_LANES);
  return (float)sqrt(s);
}

// the rule's steps 3 (division), 4 and 5 for one row; returns the weighted reward, *total = the new slot value
__device__ __forceinline__ float finish_row(float r, const float* std_dev, float weight, float* slot, float* total) {
  if (std_dev) {
    const float sd = *std_dev;
    if (sd > 0.f) r = r / sd;
  }
  r = r * weight;
  const float v = *slot + r;
  *slot = v;
  *total = v;
  return r;
}

// FINISH: the same launch adds into the reward slot of step t (no reward normalisation); otherwise only r and avg are written
template <bool FINISH>
__global__ __launch_bounds__(BLOCK) void rnd_rows_kernel(const float* pred, const float* targ, float* r_out, float* avg, float gamma, int N, int K,
                                                         const float* weight, float* slot, double* part) {
  const int q = threadIdx.x / ROW_LANES, j = threadIdx.x % ROW_LANES;
  const int row = (int)blockIdx.x * ROWS_PER_BLOCK + q;
  const float r = row_norm(pred, targ, row, j, N, K);
  __shared__ double sh[ROWS_PER_BLOCK][2];
  if (j == 0) {
    double a = 0.0, b = 0.0;
    if (row < N) {
      r_out[row] = r;
      avg[row] = avg[row] * gamma + r;
      if (FINISH) {
        float total;
        a = (double)finish_row(r, nullptr, *weight, slot + row, &total);
        b = (double)total;
      }
    }
    if (FINISH) {
      sh[q][0] = a;
      sh[q][1] = b;
    }
  }
  if (FINISH) {
    __syncthreads();
    if (threadIdx.x < 2) {
      double s = 0.0;
      for (int i = 0; i < ROWS_PER_BLOCK; ++i) s += sh[i][threadIdx.x];  // rows in order
      part[(size_t)blockIdx.x * 2 + threadIdx.x] = s;
    }
  }
}

__global__ __launch_bounds__(BLOCK) void rnd_finish_kernel(const float* r_in, const float* std_dev, const float* weight, float* slot, int N, double* part) {
  __shared__ double sh[2][BLOCK];
  const int row = (int)blockIdx.x * BLOCK + threadIdx.x;
  double a = 0.0, b = 0.0;
  if (row < N) {
    float total;
    a = (double)finish_row(r_in[row], std_dev, *weight, slot + row, &total);
    b = (double)total;
  }
  sh[0][threadIdx.x] = a;
  sh[1][threadIdx.x] = b;
  __syncthreads();
  for (int w = BLOCK / 2; w > 0; w >>= 1) {  // the halving tree: thread t < w adds entry t + w to its own
    if ((int)threadIdx.x < w) {
      sh[0][threadIdx.x] += sh[0][threadIdx.x + w];
      sh[1][threadIdx.x] += sh[1][threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x < 2) part[(size_t)blockIdx.x * 2 + threadIdx.x] = sh[threadIdx.x][0];
}

// out[c] = sum over t < n_steps, b < blocks of part[t][b][c]: lane l adds its entries (t, b) with (t blocks + b) % 64 == l in order, then the tree
__global__ __launch_bounds__(64) void rnd_sums_kernel(const double* part, int n_steps, int blocks, int stride, double* out) {
  __shared__ double sh[2][64];
  double a = 0.0, b = 0.0;
  const long total = (long)n_steps * blocks;
  for (long i = threadIdx.x; i < total; i += 64) {
    const long t = i / blocks, k = i - t * blocks;
    a += part[((size_t)t * stride + k) * 2];
    b += part[((size_t)t * stride + k) * 2 + 1];
  }
  sh[0][threadIdx.x] = a;
  sh[1][threadIdx.x] = b;
  __syncthreads();
  for (int w = 32; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      sh[0][threadIdx.x] += sh[0][threadIdx.x + w];
      sh[1][threadIdx.x] += sh[1][threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x < 2) out[threadIdx.x] = sh[threadIdx.x][0];
}

int check_launch() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(hipGetErrorString(e));
}

int enter(rl_rnd_reward* h, const char* what) {
  if (!h) return fail(std::string(what) + ": null handle");
  if (hipSetDevice(h->device) != hipSuccess) return fail("hipSetDevice failed");
  return 0;
}

int check_step(const rl_rnd_reward* h, int t, const char* what) {
  if (t < 0 || t >= h->T) return fail(std::string(what) + ": step " + std::to_string(t) + " outside 0.." + std::to_string(h->T - 1));
  return 0;
}

}  // namespace

extern "C" {

const char* rl_rnd_reward_last_error(void) { return g_err.c_str(); }

int rl_rnd_reward_destroy(rl_rnd_reward* h) {
  if (!h) return 0;
  (void)hipSetDevice(h->device);
  for (void* q : {(void*)h->r, (void*)h->avg, (void*)h->weights, (void*)h->part, (void*)h->sums})
    if (q) (void)hipFree(q);
  delete h;
  return 0;
}

int rl_rnd_reward_create(int32_t num_envs, int32_t num_outputs, int32_t num_steps, float gamma_r, int32_t device, rl_rnd_reward** out) {
  if (out) *out = nullptr;
  if (!out) return fail("rl_rnd_reward_create: null argument");
  if (num_envs < 1) return fail("rl_rnd_reward_create: num_envs " + std::to_string(num_envs) + " must be >= 1");
  if (num_outputs < 1 || num_outputs > RL_RND_MAX_OUTPUTS)
    return fail("rl_rnd_reward_create: num_outputs " + std::to_string(num_outputs) + " outside 1.." + std::to_string(RL_RND_MAX_OUTPUTS));
  if (num_steps < 1) return fail("rl_rnd_reward_create: num_steps " + std::to_string(num_steps) + " must be >= 1");
  if (!std::isfinite(gamma_r) || gamma_r < 0.f || gamma_r > 1.f) return fail("rl_rnd_reward_create: gamma_r must be finite and in [0, 1]");
  if (hipSetDevice(device) != hipSuccess) return fail("hipSetDevice failed (the RND reward kernels need a GPU; there is no CPU path)");
  rl_rnd_reward* h = new rl_rnd_reward();
  h->N = num_envs; h->K = num_outputs; h->T = num_steps; h->device = device; h->gamma = gamma_r;
  h->row_blocks = (num_envs + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
  h->host_weights.assign((size_t)num_steps, 0.f);
  const size_t n = (size_t)num_envs, np = (size_t)num_steps * h->row_blocks * 2;
  bool ok = hipMalloc((void**)&h->r, n * 4) == hipSuccess && hipMalloc((void**)&h->avg, n * 4) == hipSuccess &&
            hipMalloc((void**)&h->weights, (size_t)num_steps * 4) == hipSuccess && hipMalloc((void**)&h->part, np * 8) == hipSuccess &&
            hipMalloc((void**)&h->sums, 2 * 8) == hipSuccess;
  ok = ok && hipMemset(h->r, 0, n * 4) == hipSuccess && hipMemset(h->avg, 0, n * 4) == hipSuccess &&
       hipMemset(h->weights, 0, (size_t)num_steps * 4) == hipSuccess && hipMemset(h->part, 0, np * 8) == hipSuccess &&
       hipMemset(h->sums, 0, 2 * 8) == hipSuccess;
  if (!ok) {
    rl_rnd_reward_destroy(h);
    return fail("rl_rnd_reward_create: device allocation failed");
  }
  *out = h;
  return 0;
}

int rl_rnd_reward_set_weights(rl_rnd_reward* h, const float* weights_host, void* stream) {
  if (!h || !weights_host) return fail("rl_rnd_reward_set_weights: null argument");
  for (int t = 0; t < h->T; ++t)
    if (!std::isfinite(weights_host[t])) return fail("rl_rnd_reward_set_weights: weight " + std::to_string(t) + " is not finite");
  if (hipSetDevice(h->device) != hipSuccess) return fail("hipSetDevice failed");
  h->host_weights.assign(weights_host, weights_host + h->T);
  // (pageable source: the runtime stages it before the call returns, so the next iteration may overwrite host_weights)
  const hipError_t e = hipMemcpyAsync(h->weights, h->host_weights.data(), (size_t)h->T * 4, hipMemcpyHostToDevice, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail(hipGetErrorString(e));
}

int rl_rnd_reward_rows(rl_rnd_reward* h, const float* predictor_dev, const float* target_dev, void* stream) {
  if (!h || !predictor_dev || !target_dev) return fail("rl_rnd_reward_rows: null argument");
  if (enter(h, "rl_rnd_reward_rows")) return -1;
  hipLaunchKernelGGL(rnd_rows_kernel<false>, dim3(h->row_blocks), dim3(BLOCK), 0, (hipStream_t)stream, predictor_dev, target_dev, h->r, h->avg, h->gamma, h->N,
                     h->K, (const float*)nullptr, (float*)nullptr, (double*)nullptr);
  return check_launch();
}

int rl_rnd_reward_finish(rl_rnd_reward* h, int32_t t, const float* std_dev, float* reward_slot_dev, void* stream) {
  if (!h || !reward_slot_dev) return fail("rl_rnd_reward_finish: null argument");
  if (check_step(h, t, "rl_rnd_reward_finish") || enter(h, "rl_rnd_reward_finish")) return -1;
  const int blocks = (h->N + BLOCK - 1) / BLOCK;  // (<= row_blocks)
  h->used_blocks = blocks;
  hipLaunchKernelGGL(rnd_finish_kernel, dim3(blocks), dim3(BLOCK), 0, (hipStream_t)stream, h->r, std_dev, h->weights + t, reward_slot_dev, h->N,
                     h->part + (size_t)t * h->row_blocks * 2);
  return check_launch();
}

int rl_rnd_reward_step(rl_rnd_reward* h, const float* predictor_dev, const float* target_dev, int32_t t, float* reward_slot_dev, void* stream) {
  if (!h || !predictor_dev || !target_dev || !reward_slot_dev) return fail("rl_rnd_reward_step: null argument");
  if (check_step(h, t, "rl_rnd_reward_step") || enter(h, "rl_rnd_reward_step")) return -1;
  h->used_blocks = h->row_blocks;
  hipLaunchKernelGGL(rnd_rows_kernel<true>, dim3(h->row_blocks), dim3(BLOCK), 0, (hipStream_t)stream, predictor_dev, target_dev, h->r, h->avg, h->gamma, h->N,
                     h->K, (const float*)(h->weights + t), reward_slot_dev, h->part + (size_t)t * h->row_blocks * 2);
  return check_launch();
}

int rl_rnd_reward_pointers(rl_rnd_reward* h, float** r, float** avg, float** weights) {
  if (!h) return fail("rl_rnd_reward_pointers: null handle");
  if (r) *r = h->r;
  if (avg) *avg = h->avg;
  if (weights) *weights = h->weights;
  return 0;
}

int rl_rnd_reward_reset(rl_rnd_reward* h, void* stream) {
  if (enter(h, "rl_rnd_reward_reset")) return -1;
  const hipError_t e = hipMemsetAsync(h->avg, 0, (size_t)h->N * 4, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail(hipGetErrorString(e));
}

int rl_rnd_reward_sums(rl_rnd_reward* h, int32_t n_steps, double* out, void* stream) {
  if (!h || !out) return fail("rl_rnd_reward_sums: null argument");
  if (n_steps < 1 || n_steps > h->T) return fail("rl_rnd_reward_sums: n_steps " + std::to_string(n_steps) + " outside 1.." + std::to_string(h->T));
  if (h->used_blocks < 1) return fail("rl_rnd_reward_sums: no step has run on this handle");
  if (enter(h, "rl_rnd_reward_sums")) return -1;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(rnd_sums_kernel, dim3(1), dim3(64), 0, s, h->part, n_steps, h->used_blocks, h->row_blocks, h->sums);
  if (check_launch()) return -1;
  if (hipStreamSynchronize(s) != hipSuccess) return fail("stream synchronisation failed");
  if (hipMemcpy(out, h->sums, 2 * 8, hipMemcpyDeviceToHost) != hipSuccess) return fail("rl_rnd_reward_sums: copy failed");
  return 0;
}

}  // extern "C"
