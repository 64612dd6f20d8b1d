// rl_rnd.inl - the update of random network distillation for gfx950 (MI355X): `update_minibatch` of robot_lab_amd/rnd.py (rsl_rl's rule) as HIP
// kernels.  C-ABI: include/rl_rnd_learner.h.  Included at the end of rl_ppo.hip, behind rl_distill.inl: GEMMs (ppo_gemm_kernel, the plain sides),
// column sums, reduce, sum of squares and clip + Adam are the PPO learner's kernels, the MSE head (distill_head_kernel: one "step" of n rows against
// the target network's output, gradient 2 (p - t) / (n K)) and its finish kernel are the distillation learner's.  Nothing is instantiated twice and
// no kernel is new: what is new is the sequence.
//
// One mini-batch of n rows idx is a fixed sequence of launches on the caller's stream:
//   forward  per layer one launch with the predictor's and the target's problem side by side (blockIdx.z), the rows gathered through idx in layer 0
//   head     blocks of 256 rows: dL/dp into the predictor's dz and, per block, the fp64 partial sum of squares through block_sum
//   finish   one workgroup: the partials -> L in fp32 -> the update's loss sum, the mini-batch count, the Adam step counter
//   dX, dW, column sums, reduce of the predictor, sum of squares, Adam with max_norm = +inf (the clip coefficient is exactly 1)
#include "../../../include/rl_rnd_learner.h"

struct rl_rnd {
  int device = 0, Lp = 0, Lt = 0, K = 0, max_rows = 0;
  rl_rnd_hyper hp{};
  Net pred, targ;  // (targ: dims, offsets into tparams and h only)
  long n_params = 0, n_tparams = 0;
  float *params = nullptr, *grads = nullptr, *m1 = nullptr, *m2 = nullptr, *tparams = nullptr;
  double *head_part = nullptr, *norm_part = nullptr;
  DevState* st = nullptr;  // lr, step as the PPO learner; acc[0] = the sum of the mini-batches' fp32 losses, n_minibatches their count
  std::vector<void*> allocs;
};

namespace {

// mode 1: the gradient alone; 2: + statistics, the step count and the optimiser
int rnd_minibatch(rl_rnd* p, const float* state, const int64_t* idx, int n, int mode, hipStream_t s) {
  const Net &P = p->pred, &T = p->targ;
  const int Lp = p->Lp, Lt = p->Lt;
  for (int l = 0; l < std::max(Lp, Lt); ++l) {
    GemmBatch gb{};
    int nz = 0, tiles = 0;
    if (l < Lp) {
      net_prob(gb.p[nz], P, p->params, Lp, state, G_FWD, l, n);
      if (l == 0) gb.p[nz].gidx = idx;
      tiles = std::max(tiles, gb.p[nz++].ntiles);
    }
    if (l < Lt) {
      net_prob(gb.p[nz], T, p->tparams, Lt, state, G_FWD, l, n);
      if (l == 0) gb.p[nz].gidx = idx;
      tiles = std::max(tiles, gb.p[nz++].ntiles);
    }
    hipLaunchKernelGGL((ppo_gemm_kernel<G_FWD, false>), dim3(tiles, 1, nz), dim3(256), 0, s, gb);
  }
  const int blocks = (n + 255) / 256;
  {
    DistillHeadArgs a{};
    a.mean = P.h[Lp]; a.target = T.h[Lt]; a.idx = nullptr; a.dmean = P.dz[Lp]; a.partials = p->head_part; a.N = n; a.A = p->K; a.huber = 0;
    hipLaunchKernelGGL(distill_head_kernel, dim3(blocks, 1), dim3(256), 0, s, a);
    if (mode == 2) hipLaunchKernelGGL(distill_finish_kernel, dim3(1), dim3(64), 0, s, p->head_part, 1, blocks, (double)n * (double)p->K, p->st, 1, 1);
  }
  for (int l = Lp - 1; l >= 1; --l) {
    GemmBatch gb{};
    net_prob(gb.p[0], P, p->params, Lp, state, G_DX, l, n);
    hipLaunchKernelGGL((ppo_gemm_kernel<G_DX, false>), dim3(gb.p[0].ntiles, 1, 1), dim3(256), 0, s, gb);
  }
  {
    GemmBatch gb{};
    ColBatch cb{};
    RedBatch rb{};
    int tiles = 0, Smax = 1, colx = 1;
    long redmax = 1;
    for (int l = 0; l < Lp; ++l) {
      const int Nn = P.dims[l + 1], Kk = P.dims[l];
      GemmProb& q = gb.p[l];
      net_prob(q, P, p->params, Lp, state, G_DW, l, n);
      if (l == 0) q.gidx = idx;
      ColProb& c = cb.p[l];
      c.Z = P.dz[l + 1]; c.part = P.part[l]; c.N = Nn; c.M = q.R; c.ld = Nn; c.S = q.S; c.chunk = q.chunk; c.stride = q.cstride; c.off = (long)Nn * Kk;
      RedProb& r = rb.p[l];
      r.part = P.part[l]; r.out = p->grads + P.w_off[l]; r.count = q.cstride; r.stride = q.cstride; r.S = q.S;  // (b follows W in the flat layout)
      tiles = std::max(tiles, q.ntiles); Smax = std::max(Smax, q.S); colx = std::max(colx, (Nn + 63) / 64); redmax = std::max(redmax, r.count);
    }
    hipLaunchKernelGGL((ppo_gemm_kernel<G_DW, false>), dim3(tiles, Smax, Lp), dim3(256), 0, s, gb);
    hipLaunchKernelGGL(ppo_colsum_kernel, dim3(colx, Smax, Lp), dim3(256), 0, s, cb);
    hipLaunchKernelGGL(ppo_reduce_kernel, dim3((unsigned)std::min<long>((redmax + 255) / 256, 512), Lp), dim3(256), 0, s, rb);
  }
  if (mode == 2) {
    hipLaunchKernelGGL(ppo_sumsq_kernel<false>, dim3(NORM_BLOCKS), dim3(256), 0, s, p->grads, p->n_params, p->norm_part, 1.0f);
    // no clipping: +inf / (norm + 1e-6) is +inf for every finite norm, and min(+inf, 1) is exactly 1
    hipLaunchKernelGGL(ppo_adam_kernel<false>, dim3((unsigned)((p->n_params + 255) / 256)), dim3(256), 0, s, p->params, p->grads, p->m1, p->m2, p->n_params, 0,
                       p->norm_part, p->st, INFINITY, 1.0f);
  }
  return check_launch();
}

int rnd_enter(rl_rnd* p, const float* state, const int64_t* idx, int n, const char* what) {
  if (!p || !state || !idx) return fail("null argument");
  if (n < 1 || n > p->max_rows) return fail(std::string(what) + " " + std::to_string(n) + " outside 1..max_rows_per_minibatch (" + std::to_string(p->max_rows) + ") of rl_rnd_create");
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  return 0;
}

int rnd_read_state(rl_rnd* p, void* stream, DevState* st, const char* what) {
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return fail("stream synchronisation failed");
  if (hipMemcpy(st, p->st, sizeof(*st), hipMemcpyDeviceToHost) != hipSuccess) return fail(std::string(what) + " copy failed");
  return 0;
}

int rnd_copy_parameters(rl_rnd* p, const float* const* pw, const float* const* pb, const float* const* tw, const float* const* tb, bool to_flat, hipStream_t s) {
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  auto cp = [&](const float* user, float* flat, size_t count) {
    if (!user) return fail("null layer pointer");
    const hipError_t e = to_flat ? hipMemcpyAsync(flat, user, count * 4, hipMemcpyDeviceToDevice, s)
                                 : hipMemcpyAsync(const_cast<float*>(user), flat, count * 4, hipMemcpyDeviceToDevice, s);
    return e == hipSuccess ? 0 : fail(hipGetErrorString(e));
  };
  for (int l = 0; l < p->Lp; ++l) {
    if (pw && cp(pw[l], p->params + p->pred.w_off[l], (size_t)p->pred.dims[l] * p->pred.dims[l + 1])) return -1;
    if (pb && cp(pb[l], p->params + p->pred.b_off[l], (size_t)p->pred.dims[l + 1])) return -1;
  }
  for (int l = 0; l < p->Lt; ++l) {
    if (tw && cp(tw[l], p->tparams + p->targ.w_off[l], (size_t)p->targ.dims[l] * p->targ.dims[l + 1])) return -1;
    if (tb && cp(tb[l], p->tparams + p->targ.b_off[l], (size_t)p->targ.dims[l + 1])) return -1;
  }
  return 0;
}

int rnd_check_dims(const char* who, const int32_t* dims, int n_layers) {
  if (n_layers < 1 || n_layers > RL_RND_MAX_LAYERS)
    return fail(std::string("unsupported layer count ") + std::to_string(n_layers) + " of the " + who + " (1.." + std::to_string(RL_RND_MAX_LAYERS) + ")");
  for (int l = 0; l <= n_layers; ++l)
    if (dims[l] < 1 || dims[l] > RL_RND_MAX_WIDTH)
      return fail(std::string("unsupported layer width ") + std::to_string(dims[l]) + " of the " + who + " (1.." + std::to_string(RL_RND_MAX_WIDTH) + ")");
  return 0;
}

long rnd_layout(Net& N, const int32_t* dims, int n_layers) {
  long off = 0;
  for (int l = 0; l <= n_layers; ++l) N.dims[l] = dims[l];
  for (int l = 0; l < n_layers; ++l) {
    N.w_off[l] = off; off += (long)dims[l] * dims[l + 1];
    N.b_off[l] = off; off += dims[l + 1];
  }
  return off;
}

}  // namespace

extern "C" {

const char* rl_rnd_last_error(void) { return err().c_str(); }

int rl_rnd_destroy(rl_rnd* p) {
  if (!p) return 0;
  (void)hipSetDevice(p->device);
  for (void* q : p->allocs) (void)hipFree(q);
  delete p;
  return 0;
}

int rl_rnd_create(const int32_t* predictor_dims, int32_t n_predictor_layers, const int32_t* target_dims, int32_t n_target_layers, int32_t activation,
                  const rl_rnd_hyper* hyper, int32_t max_rows_per_minibatch, int32_t device, rl_rnd** out) {
  if (out) *out = nullptr;
  if (!predictor_dims || !target_dims || !hyper || !out) return fail("null argument");
  if (rnd_check_dims("predictor", predictor_dims, n_predictor_layers) || rnd_check_dims("target", target_dims, n_target_layers)) return -1;
  if (activation != RL_RND_ACT_ELU)
    return fail("unsupported activation: the HIP RND learner implements ELU only (use the torch learner of robot_lab_amd/rnd.py)");
  if (predictor_dims[0] != target_dims[0] || predictor_dims[n_predictor_layers] != target_dims[n_target_layers])
    return fail("the predictor and the target differ in their state width or their number of outputs");
  if (!std::isfinite(hyper->learning_rate) || !(hyper->learning_rate > 0.0)) return fail("the learning rate must be finite and > 0");
  if (hyper->num_learning_epochs < 1) return fail("num_learning_epochs " + std::to_string(hyper->num_learning_epochs) + " must be >= 1");
  if (hyper->num_mini_batches < 1) return fail("num_mini_batches " + std::to_string(hyper->num_mini_batches) + " must be >= 1");
  if (max_rows_per_minibatch < 1) return fail("max_rows_per_minibatch " + std::to_string(max_rows_per_minibatch) + " must be >= 1");
  if (hipSetDevice(device) != hipSuccess) return fail("hipSetDevice failed (the HIP learner needs a GPU; there is no CPU path)");
  rl_rnd* p = new rl_rnd();
  p->device = device; p->Lp = n_predictor_layers; p->Lt = n_target_layers; p->K = predictor_dims[n_predictor_layers]; p->hp = *hyper;
  p->max_rows = max_rows_per_minibatch;
  p->n_params = rnd_layout(p->pred, predictor_dims, n_predictor_layers);
  p->n_tparams = rnd_layout(p->targ, target_dims, n_target_layers);
  const size_t rows = (size_t)p->max_rows, np = (size_t)p->n_params;
  bool ok = dalloc(p->allocs, &p->params, np) && dalloc(p->allocs, &p->grads, np) && dalloc(p->allocs, &p->m1, np) && dalloc(p->allocs, &p->m2, np) &&
            dalloc(p->allocs, &p->tparams, (size_t)p->n_tparams) && dalloc(p->allocs, &p->norm_part, (size_t)NORM_BLOCKS) && dalloc(p->allocs, &p->st, 1) &&
            dalloc(p->allocs, &p->head_part, (rows + 255) / 256);
  const int s_cap = (int)std::max<size_t>(1, (rows + TK - 1) / TK);  // no chunk shorter than a slice
  for (int l = 0; l < p->Lp && ok; ++l) {
    Net& N = p->pred;
    const int Nn = N.dims[l + 1], K = N.dims[l];
    ok = dalloc(p->allocs, &N.h[l + 1], rows * Nn) && dalloc(p->allocs, &N.dz[l + 1], rows * Nn);
    N.S[l] = std::max(1, std::min(256 / (tiles_of(Nn) * tiles_of(K)), s_cap));  // one network: ~256 workgroups per layer in the dW launch
    ok = ok && dalloc(p->allocs, &N.part[l], (size_t)N.S[l] * ((size_t)Nn * K + Nn));
  }
  for (int l = 0; l < p->Lt && ok; ++l) ok = dalloc(p->allocs, &p->targ.h[l + 1], rows * p->targ.dims[l + 1]);
  if (ok) {
    DevState st{};
    st.lr = hyper->learning_rate;
    ok = hipMemcpy(p->st, &st, sizeof(st), hipMemcpyHostToDevice) == hipSuccess;
  }
  if (!ok) {
    rl_rnd_destroy(p);
    return fail("device allocation failed");
  }
  *out = p;
  return 0;
}

int64_t rl_rnd_num_parameters(const rl_rnd* p) { return p ? p->n_params : 0; }

int rl_rnd_set_parameters(rl_rnd* p, const float* const* predictor_w_dev, const float* const* predictor_b_dev, const float* const* target_w_dev,
                          const float* const* target_b_dev, void* stream) {
  if (!p) return fail("null argument");
  return rnd_copy_parameters(p, predictor_w_dev, predictor_b_dev, target_w_dev, target_b_dev, true, (hipStream_t)stream);
}

int rl_rnd_get_parameters(rl_rnd* p, float* const* predictor_w_dev, float* const* predictor_b_dev, float* const* target_w_dev, float* const* target_b_dev,
                          void* stream) {
  if (!p) return fail("null argument");
  return rnd_copy_parameters(p, predictor_w_dev, predictor_b_dev, target_w_dev, target_b_dev, false, (hipStream_t)stream);
}

int rl_rnd_parameter_pointers(rl_rnd* p, const float** predictor_w_dev, const float** predictor_b_dev) {
  if (!p) return fail("null argument");
  for (int l = 0; l < p->Lp; ++l) {
    if (predictor_w_dev) predictor_w_dev[l] = p->params + p->pred.w_off[l];
    if (predictor_b_dev) predictor_b_dev[l] = p->params + p->pred.b_off[l];
  }
  return 0;
}

int rl_rnd_get_flat(rl_rnd* p, int32_t which, float* dst_dev, void* stream) {
  if (!p || !dst_dev) return fail("null argument");
  if (which < 0 || which > 3) return fail("rl_rnd_get_flat: which must be 0..3");
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  const float* src[4] = {p->params, p->grads, p->m1, p->m2};
  const hipError_t e = hipMemcpyAsync(dst_dev, src[which], (size_t)p->n_params * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail(hipGetErrorString(e));
}

int rl_rnd_set_flat(rl_rnd* p, int32_t which, const float* src_dev, void* stream) {
  if (!p || !src_dev) return fail("null argument");
  if (which != 2 && which != 3) return fail("rl_rnd_set_flat: which must be 2 or 3 (the Adam moments; parameters go through rl_rnd_set_parameters)");
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  const hipError_t e = hipMemcpyAsync(which == 2 ? p->m1 : p->m2, src_dev, (size_t)p->n_params * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail(hipGetErrorString(e));
}

int rl_rnd_get_optimizer(rl_rnd* p, double* lr, int64_t* step, void* stream) {
  if (!p || !lr || !step) return fail("null argument");
  DevState st{};
  if (rnd_read_state(p, stream, &st, "optimiser state")) return -1;
  *lr = st.lr;
  *step = (int64_t)st.step;
  return 0;
}

int rl_rnd_set_optimizer(rl_rnd* p, double lr, int64_t step, void* stream) {
  if (!p) return fail("null argument");
  if (!std::isfinite(lr) || !(lr > 0.0)) return fail("rl_rnd_set_optimizer: the learning rate must be finite and > 0");
  if (step < 0) return fail("rl_rnd_set_optimizer: the step counter must be >= 0");
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  hipLaunchKernelGGL(ppo_set_optimizer_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, p->st, lr, (long long)step);
  return check_launch();
}

int rl_rnd_minibatch_grad(rl_rnd* p, const float* state_dev, const int64_t* idx_dev, int32_t n_idx, void* stream) {
  if (rnd_enter(p, state_dev, idx_dev, n_idx, "n_idx")) return -1;
  return rnd_minibatch(p, state_dev, idx_dev, n_idx, 1, (hipStream_t)stream);
}

int rl_rnd_update(rl_rnd* p, const float* state_dev, const int64_t* perm_dev, int32_t n_rows, void* stream) {
  const int mb = p ? n_rows / p->hp.num_mini_batches : 0;
  if (rnd_enter(p, state_dev, perm_dev, mb, "rows per mini-batch")) return -1;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(p->st->acc, 0, sizeof(double) * 4, s) != hipSuccess || hipMemsetAsync(&p->st->n_minibatches, 0, sizeof(long long), s) != hipSuccess)
    return fail("cannot reset the statistics block");
  for (int e = 0; e < p->hp.num_learning_epochs; ++e)
    for (int i = 0; i < p->hp.num_mini_batches; ++i)
      if (rnd_minibatch(p, state_dev, perm_dev + (size_t)i * mb, mb, 2, s)) return -1;
  return 0;
}

int rl_rnd_stats(rl_rnd* p, double* out, void* stream) {
  if (!p || !out) return fail("null argument");
  DevState st{};
  if (rnd_read_state(p, stream, &st, "statistics")) return -1;
  out[0] = st.acc[0] / (st.n_minibatches > 0 ? (double)st.n_minibatches : 1.0);
  out[1] = st.lr; out[2] = (double)st.n_minibatches; out[3] = (double)st.step;
  return 0;
}

}  // extern "C"
