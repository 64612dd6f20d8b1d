// rl_distill.inl - the distillation learner for gfx950 (MI355X): `Distillation.update` of robot_lab_amd/distill.py (rsl_rl's rule for a
// feed-forward student) as HIP kernels.  C-ABI: include/rl_distill.h.  Included at the end of rl_ppo.hip: GEMMs (ppo_gemm_kernel, the plain
// sides), column sums, reduce, sum of squares and clip + Adam are the PPO learner's kernels; new here are the behaviour-cloning head, its
// finish kernel and the row index of a group that wraps the epoch boundary.
//
// One group of g <= gradient_length time steps is a fixed sequence of launches on the caller's stream:
//   (index)  only for a group whose steps are not consecutive: idx[j N + r] = step_j N + r
//   forward  per layer one launch, rows = g N: the contiguous range obs + t0 N obs_dim, or the gather through idx
//   head     grid (blocks of 256 envs, g steps): dmean and, per block, the fp64 partial loss sum of ITS step through block_sum
//   finish   one workgroup: per step, in the group's order, the partials -> l_t in fp32 -> total, cnt; the Adam step is counted
//   dX, dW, column sums, reduce, sum of squares, clip + Adam: as a PPO mini-batch of one network (n_std = 0)
// The left-over steps of an update run (index) forward, head, finish and nothing else.
#include "../../../include/rl_distill.h"

namespace {

// DevState as this learner uses it: lr, step, grad_norm as the PPO learner (ppo_adam_kernel reads and writes them); acc[0] = total (the sum of
// the steps' fp32 losses), n_minibatches = cnt, acc[1] = optimiser steps of the update
struct DistillHeadArgs {
  const float* mean;    // [rows][A]
  const float* target;  // teacher actions: row m, or row idx[m]
  const int64_t* idx;   // null: contiguous
  float* dmean;         // [rows][A]
  double* partials;     // [n_steps][blocks per step]
  int N, A, huber;
};

// the behaviour-cloning head: row m = blockIdx.y N + blockIdx.x 256 + threadIdx.x (a block never straddles two steps)
__global__ __launch_bounds__(256) void distill_head_kernel(DistillHeadArgs a) {
  __shared__ double sh[256];
  const int r = (int)blockIdx.x * 256 + threadIdx.x;
  double s = 0.0;
  if (r < a.N) {
    const size_t m = (size_t)blockIdx.y * a.N + r;
    const size_t g = a.idx ? (size_t)a.idx[m] : m;
    const float inv = 1.0f / ((float)a.N * (float)a.A);
    const float two_inv = 2.0f / ((float)a.N * (float)a.A);
    for (int k = 0; k < a.A; ++k) {
      const float d = a.mean[m * a.A + k] - a.target[g * a.A + k];
      float gm;
      if (a.huber) {
        const float ad = fabsf(d);
        gm = ad <= 1.0f ? inv * d : (d > 0.f ? inv : -inv);
        s += ad <= 1.0f ? 0.5 * (double)d * (double)d : (double)ad - 0.5;
      } else {
        gm = two_inv * d;
        s += (double)d * (double)d;
      }
      a.dmean[m * a.A + k] = gm;
    }
  }
  sh[threadIdx.x] = s;
  block_sum<256, 1>(sh);
  if (threadIdx.x == 0) a.partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = sh[0];
}

// one workgroup of 64: per step of the group, in order, the head's partials -> l_t = fp32(sum / (N A)) (what `float(l_t)` of the rule is);
// `book`: total and cnt take it; `count_step`: an optimiser step follows (the Adam step counter and the update's step count move)
__global__ __launch_bounds__(64) void distill_finish_kernel(const double* partials, int n_steps, int blocks, double count, DevState* st, int book, int count_step) {
  __shared__ double sh[64];
  for (int j = 0; j < n_steps; ++j) {
    double s = 0.0;
    for (int b = threadIdx.x; b < blocks; b += 64) s += partials[(size_t)j * blocks + b];
    sh[threadIdx.x] = s;
    block_sum<64, 1>(sh);
    if (threadIdx.x == 0 && book) {
      st->acc[0] += (double)(float)(sh[0] / count);
      st->n_minibatches += 1;
    }
  }
  if (threadIdx.x == 0 && count_step) {
    st->step += 1;
    st->acc[1] += 1.0;
  }
}

// idx[j N + r] = step_j N + r with step_j = steps[j], or (c0 + j) % T without a list (the rule's count c0 + j across the epochs)
__global__ __launch_bounds__(256) void distill_rows_kernel(int64_t* idx, const int* steps, int c0, int T, int N, long rows) {
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  if (m >= rows) return;
  const int j = (int)(m / N), r = (int)(m - (long)j * N);
  const int t = steps ? steps[j] : (c0 + j) % T;
  idx[m] = (int64_t)t * N + r;
}

}  // namespace

struct rl_distill {
  int device = 0, L = 0, A = 0, N = 0;
  rl_distill_hyper hp{};
  Net net;
  long n_params = 0;
  long max_rows = 0;  // gradient_length x num_envs
  float *params = nullptr, *grads = nullptr, *m1 = nullptr, *m2 = nullptr;
  double *head_part = nullptr, *norm_part = nullptr;
  int64_t* idx = nullptr;  // [max_rows]
  int* steps = nullptr;    // [gradient_length] (rl_distill_group_grad)
  DevState* st = nullptr;
  std::vector<void*> allocs;
};

namespace {

// one group: `steps_dev` (a list on the device), or the counts c0 .. c0 + g - 1 of an update over T steps; `contiguous`: its first step t0
// starts ONE row range.  mode 0: forward + head + finish(book) - a left-over; 1: + backward into the flat gradient (no statistics); 2: + statistics,
// the step count and the optimiser
int distill_group(rl_distill* p, const float* obs, const float* ta, int N, int g, bool contiguous, int t0, const int* steps_dev, int c0, int T, int mode,
                  hipStream_t s) {
  const int L = p->L;
  const long rows_l = (long)g * N;
  const int rows = (int)rows_l;
  const Net& Nt = p->net;
  const int64_t* gidx = nullptr;
  const float* x0 = obs;
  if (contiguous) {
    x0 = obs + (size_t)t0 * N * Nt.dims[0];
    ta = ta + (size_t)t0 * N * p->A;
  } else {
    hipLaunchKernelGGL(distill_rows_kernel, dim3((unsigned)((rows_l + 255) / 256)), dim3(256), 0, s, p->idx, steps_dev, c0, T, N, rows_l);
    gidx = p->idx;
  }
  for (int l = 0; l < L; ++l) {
    GemmBatch gb{};
    net_prob(gb.p[0], Nt, p->params, L, x0, G_FWD, l, rows);
    if (l == 0) gb.p[0].gidx = gidx;
    hipLaunchKernelGGL((ppo_gemm_kernel<G_FWD, false>), dim3(gb.p[0].ntiles, 1, 1), dim3(256), 0, s, gb);
  }
  const int blocks = (N + 255) / 256;
  {
    DistillHeadArgs a{};
    a.mean = Nt.h[L]; a.target = ta; a.idx = gidx; a.dmean = Nt.dz[L]; a.partials = p->head_part; a.N = N; a.A = p->A;
    a.huber = p->hp.loss_type == RL_DISTILL_LOSS_HUBER;
    hipLaunchKernelGGL(distill_head_kernel, dim3(blocks, g), dim3(256), 0, s, a);
    if (mode != 1)
      hipLaunchKernelGGL(distill_finish_kernel, dim3(1), dim3(64), 0, s, p->head_part, g, blocks, (double)N * (double)p->A, p->st, 1, mode == 2 ? 1 : 0);
  }
  if (mode == 0) return check_launch();
  for (int l = L - 1; l >= 1; --l) {
    GemmBatch gb{};
    net_prob(gb.p[0], Nt, p->params, L, x0, G_DX, l, rows);
    hipLaunchKernelGGL((ppo_gemm_kernel<G_DX, false>), dim3(gb.p[0].ntiles, 1, 1), dim3(256), 0, s, gb);
  }
  {
    GemmBatch gb{};
    ColBatch cb{};
    RedBatch rb{};
    int tiles = 0, Smax = 1, colx = 1;
    long redmax = 1;
    for (int l = 0; l < L; ++l) {
      const int Nn = Nt.dims[l + 1], K = Nt.dims[l];
      GemmProb& q = gb.p[l];
      net_prob(q, Nt, p->params, L, x0, G_DW, l, rows);
      if (l == 0) q.gidx = gidx;
      ColProb& c = cb.p[l];
      c.Z = Nt.dz[l + 1]; c.part = Nt.part[l]; c.N = Nn; c.M = q.R; c.ld = Nn; c.S = q.S; c.chunk = q.chunk; c.stride = q.cstride; c.off = (long)Nn * K;
      RedProb& r = rb.p[l];
      r.part = Nt.part[l]; r.out = p->grads + Nt.w_off[l]; r.count = q.cstride; r.stride = q.cstride; r.S = q.S;  // (b follows W in the flat layout)
      tiles = std::max(tiles, q.ntiles); Smax = std::max(Smax, q.S); colx = std::max(colx, (Nn + 63) / 64); redmax = std::max(redmax, r.count);
    }
    hipLaunchKernelGGL((ppo_gemm_kernel<G_DW, false>), dim3(tiles, Smax, L), dim3(256), 0, s, gb);
    hipLaunchKernelGGL(ppo_colsum_kernel, dim3(colx, Smax, L), dim3(256), 0, s, cb);
    hipLaunchKernelGGL(ppo_reduce_kernel, dim3((unsigned)std::min<long>((redmax + 255) / 256, 512), L), dim3(256), 0, s, rb);
  }
  if (mode == 2) {
    hipLaunchKernelGGL(ppo_sumsq_kernel<false>, dim3(NORM_BLOCKS), dim3(256), 0, s, p->grads, p->n_params, p->norm_part, 1.0f);
    // max_grad_norm unset: +inf / (norm + 1e-6) is +inf for every finite norm, and min(+inf, 1) is exactly 1
    const float max_norm = p->hp.max_grad_norm > 0.f ? p->hp.max_grad_norm : INFINITY;
    hipLaunchKernelGGL(ppo_adam_kernel<false>, dim3((unsigned)((p->n_params + 255) / 256)), dim3(256), 0, s, p->params, p->grads, p->m1, p->m2, p->n_params, 0,
                       p->norm_part, p->st, max_norm, 1.0f);
  }
  return check_launch();
}

int distill_enter(rl_distill* p, const float* obs, const float* ta, int n_envs) {
  if (!p || !obs || !ta) return fail("null argument");
  if (n_envs < 1 || n_envs > p->N) return fail("n_envs " + std::to_string(n_envs) + " outside 1..num_envs (" + std::to_string(p->N) + ") of rl_distill_create");
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  return 0;
}

int distill_read_state(rl_distill* p, void* stream, DevState* st, const char* what) {
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return fail("stream synchronisation failed");
  if (hipMemcpy(st, p->st, sizeof(*st), hipMemcpyDeviceToHost) != hipSuccess) return fail(std::string(what) + " copy failed");
  return 0;
}

int distill_copy_parameters(rl_distill* p, const float* const* w, const float* const* b, bool to_flat, hipStream_t s) {
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  auto cp = [&](const float* user, long off, size_t count) {
    if (!user) return fail("null layer pointer");
    float* flat = p->params + off;
    const hipError_t e = to_flat ? hipMemcpyAsync(flat, user, count * 4, hipMemcpyDeviceToDevice, s)
                                 : hipMemcpyAsync(const_cast<float*>(user), flat, count * 4, hipMemcpyDeviceToDevice, s);
    return e == hipSuccess ? 0 : fail(hipGetErrorString(e));
  };
  for (int l = 0; l < p->L; ++l) {
    if (w && cp(w[l], p->net.w_off[l], (size_t)p->net.dims[l] * p->net.dims[l + 1])) return -1;
    if (b && cp(b[l], p->net.b_off[l], (size_t)p->net.dims[l + 1])) return -1;
  }
  return 0;
}

}  // namespace

extern "C" {

const char* rl_distill_last_error(void) { return err().c_str(); }

int rl_distill_destroy(rl_distill* p) {
  if (!p) return 0;
  (void)hipSetDevice(p->device);
  for (void* q : p->allocs) (void)hipFree(q);
  delete p;
  return 0;
}

int rl_distill_create(const int32_t* dims, int32_t n_layers, int32_t activation, const rl_distill_hyper* hyper, int32_t num_envs, int32_t device,
                      rl_distill** out) {
  if (out) *out = nullptr;
  if (!dims || !hyper || !out) return fail("null argument");
  if (n_layers < 1 || n_layers > RL_DISTILL_MAX_LAYERS)
    return fail("unsupported layer count " + std::to_string(n_layers) + " (1.." + std::to_string(RL_DISTILL_MAX_LAYERS) + ")");
  if (activation != RL_DISTILL_ACT_ELU)
    return fail("unsupported activation: the HIP distillation learner implements ELU only (use the torch learner of robot_lab_amd/distill.py)");
  for (int l = 0; l <= n_layers; ++l)
    if (dims[l] < 1 || dims[l] > RL_DISTILL_MAX_WIDTH)
      return fail("unsupported layer width " + std::to_string(dims[l]) + " (1.." + std::to_string(RL_DISTILL_MAX_WIDTH) + ")");
  if (hyper->gradient_length < 1) return fail("gradient_length " + std::to_string(hyper->gradient_length) + " must be >= 1");
  if (hyper->num_learning_epochs < 1) return fail("num_learning_epochs " + std::to_string(hyper->num_learning_epochs) + " must be >= 1");
  if (!std::isfinite(hyper->learning_rate) || !(hyper->learning_rate > 0.0)) return fail("the learning rate must be finite and > 0");
  if (hyper->loss_type != RL_DISTILL_LOSS_MSE && hyper->loss_type != RL_DISTILL_LOSS_HUBER)
    return fail("unknown loss type " + std::to_string(hyper->loss_type) + " (0: mse, 1: huber)");
  if (!(hyper->max_grad_norm >= 0.f)) return fail("max_grad_norm must be > 0, or 0 for none");
  if (num_envs < 1) return fail("num_envs " + std::to_string(num_envs) + " must be >= 1");
  if ((long long)hyper->gradient_length * num_envs > 0x7fffffffLL) return fail("gradient_length x num_envs rows do not fit 31 bits");
  if (hipSetDevice(device) != hipSuccess) return fail("hipSetDevice failed (the HIP learner needs a GPU; there is no CPU path)");
  rl_distill* p = new rl_distill();
  p->device = device; p->L = n_layers; p->A = dims[n_layers]; p->N = num_envs; p->hp = *hyper;
  p->max_rows = (long)hyper->gradient_length * num_envs;
  Net& N = p->net;
  long off = 0;
  for (int l = 0; l <= n_layers; ++l) N.dims[l] = dims[l];
  for (int l = 0; l < n_layers; ++l) {
    N.w_off[l] = off; off += (long)dims[l] * dims[l + 1];
    N.b_off[l] = off; off += dims[l + 1];
  }
  p->n_params = off;
  const size_t rows = (size_t)p->max_rows;
  bool ok = dalloc(p->allocs, &p->params, (size_t)off) && dalloc(p->allocs, &p->grads, (size_t)off) && dalloc(p->allocs, &p->m1, (size_t)off) &&
            dalloc(p->allocs, &p->m2, (size_t)off) && dalloc(p->allocs, &p->norm_part, (size_t)NORM_BLOCKS) && dalloc(p->allocs, &p->st, 1) &&
            dalloc(p->allocs, &p->idx, rows) && dalloc(p->allocs, &p->steps, (size_t)hyper->gradient_length) &&
            dalloc(p->allocs, &p->head_part, (size_t)hyper->gradient_length * (size_t)((num_envs + 255) / 256));
  const int s_cap = (int)std::max<size_t>(1, (rows + TK - 1) / TK);  // no chunk shorter than a slice
  for (int l = 0; l < n_layers && ok; ++l) {
    const int Nn = N.dims[l + 1], K = N.dims[l];
    ok = dalloc(p->allocs, &N.h[l + 1], rows * Nn) && dalloc(p->allocs, &N.dz[l + 1], rows * Nn);
    N.S[l] = std::max(1, std::min(256 / (tiles_of(Nn) * tiles_of(K)), s_cap));  // one network: ~256 workgroups per layer in the dW launch
    ok = ok && dalloc(p->allocs, &N.part[l], (size_t)N.S[l] * ((size_t)Nn * K + Nn));
  }
  if (ok) {
    DevState st{};
    st.lr = hyper->learning_rate;
    ok = hipMemcpy(p->st, &st, sizeof(st), hipMemcpyHostToDevice) == hipSuccess;
  }
  if (!ok) {
    rl_distill_destroy(p);
    return fail("device allocation failed");
  }
  *out = p;
  return 0;
}

int64_t rl_distill_num_parameters(const rl_distill* p) { return p ? p->n_params : 0; }

int rl_distill_set_parameters(rl_distill* p, const float* const* w_dev, const float* const* b_dev, void* stream) {
  if (!p) return fail("null argument");
  return distill_copy_parameters(p, w_dev, b_dev, true, (hipStream_t)stream);
}

int rl_distill_get_parameters(rl_distill* p, float* const* w_dev, float* const* b_dev, void* stream) {
  if (!p) return fail("null argument");
  return distill_copy_parameters(p, w_dev, b_dev, false, (hipStream_t)stream);
}

int rl_distill_parameter_pointers(rl_distill* p, const float** w_dev, const float** b_dev) {
  if (!p) return fail("null argument");
  for (int l = 0; l < p->L; ++l) {
    if (w_dev) w_dev[l] = p->params + p->net.w_off[l];
    if (b_dev) b_dev[l] = p->params + p->net.b_off[l];
  }
  return 0;
}

int rl_distill_get_flat(rl_distill* p, int32_t which, float* dst_dev, void* stream) {
  if (!p || !dst_dev) return fail("null argument");
  if (which < 0 || which > 3) return fail("rl_distill_get_flat: which must be 0..3");
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  const float* src[4] = {p->params, p->grads, p->m1, p->m2};
  const hipError_t e = hipMemcpyAsync(dst_dev, src[which], (size_t)p->n_params * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail(hipGetErrorString(e));
}

int rl_distill_set_flat(rl_distill* p, int32_t which, const float* src_dev, void* stream) {
  if (!p || !src_dev) return fail("null argument");
  if (which != 2 && which != 3) return fail("rl_distill_set_flat: which must be 2 or 3 (the Adam moments; parameters go through rl_distill_set_parameters)");
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  const hipError_t e = hipMemcpyAsync(which == 2 ? p->m1 : p->m2, src_dev, (size_t)p->n_params * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail(hipGetErrorString(e));
}

int rl_distill_get_optimizer(rl_distill* p, double* lr, int64_t* step, void* stream) {
  if (!p || !lr || !step) return fail("null argument");
  DevState st{};
  if (distill_read_state(p, stream, &st, "optimiser state")) return -1;
  *lr = st.lr;
  *step = (int64_t)st.step;
  return 0;
}

int rl_distill_set_optimizer(rl_distill* p, double lr, int64_t step, void* stream) {
  if (!p) return fail("null argument");
  if (!std::isfinite(lr) || !(lr > 0.0)) return fail("rl_distill_set_optimizer: the learning rate must be finite and > 0");
  if (step < 0) return fail("rl_distill_set_optimizer: the step counter must be >= 0");
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  hipLaunchKernelGGL(ppo_set_optimizer_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, p->st, lr, (long long)step);
  return check_launch();
}

int rl_distill_group_grad(rl_distill* p, const float* obs_dev, const float* teacher_actions_dev, int32_t n_envs, const int32_t* steps_host, int32_t n_steps,
                          void* stream) {
  if (distill_enter(p, obs_dev, teacher_actions_dev, n_envs)) return -1;
  if (!steps_host) return fail("null argument");
  if (n_steps < 1 || n_steps > p->hp.gradient_length) return fail("rl_distill_group_grad: n_steps outside 1..gradient_length");
  bool contiguous = true;
  for (int j = 0; j < n_steps; ++j) {
    if (steps_host[j] < 0 || (long long)(steps_host[j] + 1) * n_envs > 0x7fffffffLL) return fail("rl_distill_group_grad: step " + std::to_string(steps_host[j]) + " is no row range of 31 bits");
    contiguous = contiguous && steps_host[j] == steps_host[0] + j;
  }
  hipStream_t s = (hipStream_t)stream;
  if (!contiguous) {
    if (hipStreamSynchronize(s) != hipSuccess || hipMemcpy(p->steps, steps_host, (size_t)n_steps * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
      return fail("rl_distill_group_grad: cannot copy the step list");
  }
  return distill_group(p, obs_dev, teacher_actions_dev, n_envs, n_steps, contiguous, steps_host[0], p->steps, 0, 1, 1, s);
}

int rl_distill_update(rl_distill* p, const float* obs_dev, const float* teacher_actions_dev, int32_t T, int32_t n_envs, void* stream) {
  if (distill_enter(p, obs_dev, teacher_actions_dev, n_envs)) return -1;
  if (T < 1 || (long long)T * n_envs > 0x7fffffffLL) return fail("rl_distill_update: T x n_envs outside 1..2^31 - 1 rows");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(p->st->acc, 0, sizeof(double) * 4, s) != hipSuccess || hipMemsetAsync(&p->st->n_minibatches, 0, sizeof(long long), s) != hipSuccess)
    return fail("cannot reset the statistics block");
  const long long total = (long long)p->hp.num_learning_epochs * T;
  const int gl = p->hp.gradient_length;
  for (long long c0 = 0; c0 < total; c0 += gl) {
    const int g = (int)std::min<long long>(gl, total - c0);
    const int t0 = (int)(c0 % T);
    const bool contiguous = t0 + g <= T;
    if (distill_group(p, obs_dev, teacher_actions_dev, n_envs, g, contiguous, t0, nullptr, (int)(c0 % T), T, g == gl ? 2 : 0, s)) return -1;
  }
  return 0;
}

int rl_distill_stats(rl_distill* p, double* out, void* stream) {
  if (!p || !out) return fail("null argument");
  DevState st{};
  if (distill_read_state(p, stream, &st, "statistics")) return -1;
  out[0] = st.acc[0] / (st.n_minibatches > 0 ? (double)st.n_minibatches : 1.0);
  out[1] = st.lr; out[2] = st.grad_norm; out[3] = st.acc[1]; out[4] = (double)st.step;
  return 0;
}

}  // extern "C"
