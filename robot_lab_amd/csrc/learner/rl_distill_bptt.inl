// rl_distill_bptt.inl - the recurrent distillation learner for gfx950 (MI355X): `RecurrentDistillation.update` of robot_lab_amd/distill_recurrent.py
// (an LSTM in front of the student's MLP, truncated back-propagation through time over groups of gradient_length steps) as HIP kernels.
// C-ABI: include/rl_distill_bptt.h.  Included at the end of rl_ppo.hip behind rl_distill.inl and rl_bptt.inl: the step kernels
// (bptt_step_kernel<false|true>, launched with ONE network: a grid of one in z) are the recurrent PPO learner's, the behaviour-cloning head and
// its finish kernel the distillation learner's, GEMMs, column sums, reduce, sum of squares and clip + Adam the PPO learner's; new here is the
// prep kernel alone (the row index of a group that wraps an epoch boundary, and b_ih + b_hh of ONE memory).
//
// One group of g <= gradient_length steps (rows [j N, (j + 1) N) of the workspace are step j of the group) is a fixed sequence of launches:
//   prep      idx[j N + r] = step_j N + r (only where the steps are not consecutive); bsum = b_ih + b_hh
//   zx        ONE forward GEMM without activation: zx = X W_ih^T + bsum over the g N rows
//   forward   g step launches.  hprev / cprev: h0 / c0 where step_j = 0 (no reset: its own is applied), else the carried buffers (j = 0) or
//             step j - 1's outputs, with reset = dones[step_j - 1]
//   head      the MLP's layers on the contiguous h buffer, the behaviour-cloning head + finish; dX per layer, dL/dh = dZ_0 W_0 (G_DXLIN)
//   backward  g step launches, j descending; dzn is null at j = g - 1 and wherever step_{j+1} = 0 (an epoch begins: nothing flows into h0)
//   dW        the two LSTM weight matrices (dz^T X gathered, dz^T h~), the column sums of dz into b_ih AND b_hh, reduce; the head's dW
//   step      sum of squares, clip + Adam; then the group's last (h, c) -> the carried buffers (two device-to-device copies)
// The left-over steps of an update run prep, zx, forward, head, finish and the carry copy.
#include "../../../include/rl_distill_bptt.h"

namespace {

// idx[j N + r] = step_j N + r with step_j = steps[j], or (c0 + j) % T without a list; idx null: a contiguous group.  bs = bih + bhh [H4]
__global__ __launch_bounds__(256) void rdistill_prep_kernel(int64_t* idx, const int* steps, int c0, int T, int N, long rows, const float* bih, const float* bhh,
                                                            float* bs, int H4) {
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx && m < rows) {
    const int j = (int)(m / N), r = (int)(m - (long)j * N);
    const int t = steps ? steps[j] : (c0 + j) % T;
    idx[m] = (int64_t)t * N + r;
  }
  if (m < H4) bs[m] = bih[m] + bhh[m];
}

}  // namespace

struct rl_rdistill {
  int device = 0, L = 0, A = 0, H = 0, N = 0, last_n = 0;
  rl_distill_hyper hp{};
  Mem mem;  // ZX .. dHh sized by max_rows; DC [N][H]
  Net net;  // the head; h[0] = the memory's h buffer, dz[0] = dL/dh
  long n_params = 0;
  long max_rows = 0;  // gradient_length x num_envs
  float *params = nullptr, *grads = nullptr, *m1 = nullptr, *m2 = nullptr;
  float *h_carry = nullptr, *c_carry = nullptr;  // [N][H]: the state behind the last step of the last group
  double *head_part = nullptr, *norm_part = nullptr;
  int64_t* idx = nullptr;  // [max_rows]
  int* steps = nullptr;    // [gradient_length] (the entry points with a step list)
  DevState* st = nullptr;
  std::vector<void*> allocs;
};

namespace {

struct RdBatch {
  const float *obs, *ta;
  const uint8_t* dones;
  const float *h0, *c0;
};

enum { RD_LEFTOVER = 0, RD_GRAD = 1, RD_UPDATE = 2, RD_FORWARD = 3 };

// one group over the epoch-relative steps st[0 .. g) (host); `steps_dev`: the same list on the device, or null for the counts c0 .. c0 + g - 1 of an
// update over T steps.  RD_LEFTOVER: forward + head + finish(book); RD_GRAD: + backward into the flat gradient (no statistics); RD_UPDATE: +
// statistics, the step count and the optimiser; RD_FORWARD: forward + the head's layers, the means copied to mean_out
int rdistill_group(rl_rdistill* p, const RdBatch& b, int N, const int* st, int g, const int* steps_dev, int c0, int T, int mode, float* mean_out, hipStream_t s) {
  const int L = p->L, H = p->H, H4 = 4 * H;
  const long rows_l = (long)g * N;
  const int rows = (int)rows_l;
  const Mem& M = p->mem;
  const Net& Nt = p->net;
  bool contiguous = true;
  for (int j = 1; j < g; ++j) contiguous = contiguous && st[j] == st[0] + j;
  const int64_t* gidx = contiguous ? nullptr : p->idx;
  const float* x0 = contiguous ? b.obs + (size_t)st[0] * N * M.D : b.obs;
  const float* ta = contiguous && b.ta ? b.ta + (size_t)st[0] * N * p->A : b.ta;
  hipLaunchKernelGGL(rdistill_prep_kernel, dim3((unsigned)((std::max<long>(contiguous ? 0 : rows_l, H4) + 255) / 256)), dim3(256), 0, s,
                     contiguous ? (int64_t*)nullptr : p->idx, steps_dev, c0, T, N, rows_l, p->params + M.bih, p->params + M.bhh, M.bsum, H4);
  {  // the input half of the gates
    GemmBatch gb{};
    GemmProb& q = gb.p[0];
    q.A = x0; q.lda = M.D; q.B = p->params + M.wih; q.ldb = M.D; q.aux = M.bsum; q.C = M.ZX; q.ldc = H4;
    q.I = rows; q.J = H4; q.R = M.D; q.act = 0; q.gidx = gidx;
    q.tilesJ = tiles_of(q.J); q.ntiles = tiles_of(q.I) * q.tilesJ;
    hipLaunchKernelGGL((ppo_gemm_kernel<G_FWD, false>), dim3(q.ntiles, 1, 1), dim3(256), 0, s, gb);
  }
  const dim3 step_grid(tiles_of(N), (H + 31) / 32, 1);
  auto step_args = [&](int j) {
    StepArgs a{};
    a.n = N;
    StepNet& q = a.net[0];
    const size_t oH = (size_t)j * N * H, oG = (size_t)j * N * H4;
    const bool begins = st[j] == 0;                         // t = 0 of an epoch: the saved state, its own reset applied
    const bool flows = j + 1 < g && st[j + 1] != 0;         // step j + 1 continues this one inside the group
    q.Whh = p->params + M.whh; q.H = H;
    q.hprev = begins ? b.h0 : (j > 0 ? M.Hout + oH - (size_t)N * H : p->h_carry);
    q.cprev = begins ? b.c0 : (j > 0 ? M.C + oH - (size_t)N * H : p->c_carry);
    q.reset = begins ? nullptr : b.dones + (size_t)(st[j] - 1) * N;
    q.cut = flows ? b.dones + (size_t)st[j] * N : nullptr;
    q.zx = M.ZX + oG; q.G = M.G + oG; q.Gnext = flows ? M.G + oG + (size_t)N * H4 : nullptr;
    q.HS = M.HS + oH; q.Hout = M.Hout + oH; q.C = M.C + oH;
    q.dzn = flows ? M.DZ + oG + (size_t)N * H4 : nullptr;
    q.dH = M.dHh + oH; q.dz = M.DZ + oG; q.dc = M.DC;
    return a;
  };
  for (int j = 0; j < g; ++j) hipLaunchKernelGGL(bptt_step_kernel<false>, step_grid, dim3(256), 0, s, step_args(j));
  auto carry = [&]() {  // the group's last (h, c) is what the next group continues from (every launch that read the old one is behind us on the stream)
    const size_t last = (size_t)(g - 1) * N * H, bytes = (size_t)N * H * 4;
    p->last_n = N;
    if (hipMemcpyAsync(p->h_carry, M.Hout + last, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess ||
        hipMemcpyAsync(p->c_carry, M.C + last, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess)
      return fail("cannot carry the state");
    return check_launch();
  };
  for (int l = 0; l < L; ++l) {
    GemmBatch gb{};
    net_prob(gb.p[0], Nt, p->params, L, M.Hout, G_FWD, l, rows);
    hipLaunchKernelGGL((ppo_gemm_kernel<G_FWD, false>), dim3(gb.p[0].ntiles, 1, 1), dim3(256), 0, s, gb);
  }
  if (mode == RD_FORWARD) {
    if (hipMemcpyAsync(mean_out, Nt.h[L], (size_t)rows * p->A * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return fail("rl_rdistill_forward: cannot copy the outputs");
    return carry();
  }
  const int blocks = (N + 255) / 256;
  {
    DistillHeadArgs a{};
    a.mean = Nt.h[L]; a.target = ta; a.idx = gidx; a.dmean = Nt.dz[L]; a.partials = p->head_part; a.N = N; a.A = p->A;
    a.huber = p->hp.loss_type == RL_DISTILL_LOSS_HUBER;
    hipLaunchKernelGGL(distill_head_kernel, dim3(blocks, g), dim3(256), 0, s, a);
    if (mode != RD_GRAD)
      hipLaunchKernelGGL(distill_finish_kernel, dim3(1), dim3(64), 0, s, p->head_part, g, blocks, (double)N * (double)p->A, p->st, 1, mode == RD_UPDATE ? 1 : 0);
  }
  if (mode == RD_LEFTOVER) return carry();
  for (int l = L - 1; l >= 0; --l) {  // l = 0: dL/dh of the memory's outputs, no elu' factor
    GemmBatch gb{};
    net_prob(gb.p[0], Nt, p->params, L, M.Hout, G_DX, l, rows);
    hipLaunchKernelGGL(side<GemmK>(l == 0, ppo_gemm_kernel<G_DXLIN, false>, ppo_gemm_kernel<G_DX, false>), dim3(gb.p[0].ntiles, 1, 1), dim3(256), 0, s, gb);
  }
  for (int j = g - 1; j >= 0; --j) hipLaunchKernelGGL(bptt_step_kernel<true>, step_grid, dim3(256), 0, s, step_args(j));
  {  // the memory's weight gradients: problems ih, hh; the column sums of dz go to b_ih and b_hh behind dW_hh
    GemmBatch gb{};
    ColBatch cb{};
    RedBatch rb{};
    int tiles = 0, Smax = 1;
    long redmax = 1;
    for (int w = 0; w < 2; ++w) {
      const int K = w == 0 ? M.D : H;
      GemmProb& q = gb.p[w];
      q.A = M.DZ; q.lda = H4; q.B = w == 0 ? x0 : M.HS; q.ldb = K; q.C = w == 0 ? M.part_ih : M.part_hh; q.ldc = K;
      q.I = H4; q.J = K; q.R = rows; q.S = w == 0 ? M.S_ih : M.S_hh; q.chunk = chunk_rows(rows, q.S);
      q.cstride = w == 0 ? (long)H4 * K : (long)H4 * K + 2 * H4;
      q.gidx = w == 0 ? gidx : nullptr;
      q.tilesJ = tiles_of(q.J); q.ntiles = tiles_of(q.I) * q.tilesJ;
      RedProb& r = rb.p[w];
      r.part = q.C; r.out = p->grads + (w == 0 ? M.wih : M.whh); r.count = q.cstride; r.stride = q.cstride; r.S = q.S;  // (b_ih, b_hh follow W_hh)
      tiles = std::max(tiles, q.ntiles); Smax = std::max(Smax, q.S); redmax = std::max(redmax, r.count);
      ColProb& c = cb.p[w];  // w = 0: b_ih's copy, w = 1: b_hh's; both in the chunks of the hh problem
      c.Z = M.DZ; c.part = M.part_hh; c.N = H4; c.M = rows; c.ld = H4; c.S = M.S_hh; c.chunk = chunk_rows(rows, M.S_hh);
      c.stride = (long)H4 * H + 2 * H4; c.off = (long)H4 * H + (long)w * H4;
    }
    hipLaunchKernelGGL((ppo_gemm_kernel<G_DW, false>), dim3(tiles, Smax, 2), dim3(256), 0, s, gb);
    hipLaunchKernelGGL(ppo_colsum_kernel, dim3((H4 + 63) / 64, Smax, 2), dim3(256), 0, s, cb);
    hipLaunchKernelGGL(ppo_reduce_kernel, dim3((unsigned)std::min<long>((redmax + 255) / 256, 512), 2), dim3(256), 0, s, rb);
  }
  {  // the head's weight gradients
    GemmBatch gb{};
    ColBatch cb{};
    RedBatch rb{};
    int tiles = 0, Smax = 1, colx = 1;
    long redmax = 1;
    for (int l = 0; l < L; ++l) {
      const int Nn = Nt.dims[l + 1], K = Nt.dims[l];
      GemmProb& q = gb.p[l];
      net_prob(q, Nt, p->params, L, M.Hout, G_DW, l, rows);
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
  if (mode == RD_UPDATE) {
    hipLaunchKernelGGL(ppo_sumsq_kernel<false>, dim3(NORM_BLOCKS), dim3(256), 0, s, p->grads, p->n_params, p->norm_part, 1.0f);
    // max_grad_norm unset: +inf / (norm + 1e-6) is +inf for every finite norm, and min(+inf, 1) is exactly 1
    const float max_norm = p->hp.max_grad_norm > 0.f ? p->hp.max_grad_norm : INFINITY;
    hipLaunchKernelGGL(ppo_adam_kernel<false>, dim3((unsigned)((p->n_params + 255) / 256)), dim3(256), 0, s, p->params, p->grads, p->m1, p->m2, p->n_params, 0,
                       p->norm_part, p->st, max_norm, 1.0f);
  }
  return carry();
}

int rdistill_enter(rl_rdistill* p, const RdBatch& b, bool need_ta, int n_envs) {
  if (!p || !b.obs || (need_ta && !b.ta) || !b.dones || !b.h0 || !b.c0) return fail("null argument");
  if (n_envs < 1 || n_envs > p->N) return fail("n_envs " + std::to_string(n_envs) + " outside 1..num_envs (" + std::to_string(p->N) + ") of rl_rdistill_create");
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  return 0;
}

// the step list of the test entry points: checked, copied to the device, the input state into the carried buffers
int rdistill_list(rl_rdistill* p, const char* who, const float* h_in, const float* c_in, int n_envs, const int32_t* steps_host, int n_steps, hipStream_t s) {
  if (!steps_host) return fail("null argument");
  if (n_steps < 1 || n_steps > p->hp.gradient_length) return fail(std::string(who) + ": n_steps outside 1..gradient_length");
  for (int j = 0; j < n_steps; ++j) {
    if (steps_host[j] < 0 || (long long)(steps_host[j] + 1) * n_envs > 0x7fffffffLL) return fail(std::string(who) + ": step " + std::to_string(steps_host[j]) + " is no row range of 31 bits");
    if (j > 0 && steps_host[j] != 0 && steps_host[j] != steps_host[j - 1] + 1)
      return fail(std::string(who) + ": step " + std::to_string(steps_host[j]) + " behind step " + std::to_string(steps_host[j - 1]) + " is neither its successor nor 0 (an epoch's first)");
  }
  if (steps_host[0] != 0 && (!h_in || !c_in)) return fail(std::string(who) + ": the group does not begin an epoch and has no input state");
  if (hipStreamSynchronize(s) != hipSuccess || hipMemcpy(p->steps, steps_host, (size_t)n_steps * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
    return fail(std::string(who) + ": cannot copy the step list");
  if (steps_host[0] != 0) {
    const size_t bytes = (size_t)n_envs * p->H * 4;
    if (hipMemcpyAsync(p->h_carry, h_in, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess || hipMemcpyAsync(p->c_carry, c_in, bytes, hipMemcpyDeviceToDevice, s) != hipSuccess)
      return fail(std::string(who) + ": cannot copy the input state");
  }
  return 0;
}

int rdistill_read_state(rl_rdistill* p, void* stream, DevState* st, const char* what) {
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return fail("stream synchronisation failed");
  if (hipMemcpy(st, p->st, sizeof(*st), hipMemcpyDeviceToHost) != hipSuccess) return fail(std::string(what) + " copy failed");
  return 0;
}

int rdistill_copy_parameters(rl_rdistill* p, const float* const* lstm, const float* const* w, const float* const* b, bool to_flat, hipStream_t s) {
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  auto cp = [&](const float* user, long off, size_t count) {
    if (!user) return fail("null parameter pointer");
    float* flat = p->params + off;
    const hipError_t e = to_flat ? hipMemcpyAsync(flat, user, count * 4, hipMemcpyDeviceToDevice, s)
                                 : hipMemcpyAsync(const_cast<float*>(user), flat, count * 4, hipMemcpyDeviceToDevice, s);
    return e == hipSuccess ? 0 : fail(hipGetErrorString(e));
  };
  const size_t H4 = (size_t)4 * p->H;
  const long off[4] = {p->mem.wih, p->mem.whh, p->mem.bih, p->mem.bhh};
  const size_t count[4] = {H4 * p->mem.D, H4 * p->H, H4, H4};
  for (int j = 0; j < 4 && lstm; ++j)
    if (cp(lstm[j], off[j], count[j])) return -1;
  for (int l = 0; l < p->L; ++l) {
    if (w && cp(w[l], p->net.w_off[l], (size_t)p->net.dims[l] * p->net.dims[l + 1])) return -1;
    if (b && cp(b[l], p->net.b_off[l], (size_t)p->net.dims[l + 1])) return -1;
  }
  return 0;
}

}  // namespace

extern "C" {

const char* rl_rdistill_last_error(void) { return err().c_str(); }

int rl_rdistill_destroy(rl_rdistill* p) {
  if (!p) return 0;
  (void)hipSetDevice(p->device);
  for (void* q : p->allocs) (void)hipFree(q);
  delete p;
  return 0;
}

int rl_rdistill_create(int32_t obs_dim, int32_t hidden, const int32_t* head_dims, int32_t n_layers, int32_t activation, const rl_distill_hyper* hyper,
                       int32_t num_envs, int32_t device, rl_rdistill** out) {
  if (out) *out = nullptr;
  if (!head_dims || !hyper || !out) return fail("null argument");
  if (n_layers < 1 || n_layers > RL_RDISTILL_MAX_LAYERS)
    return fail("unsupported layer count " + std::to_string(n_layers) + " (1.." + std::to_string(RL_RDISTILL_MAX_LAYERS) + ")");
  if (activation != RL_DISTILL_ACT_ELU)
    return fail("unsupported activation: the HIP recurrent distillation learner implements ELU only (use the torch learner of robot_lab_amd/distill_recurrent.py)");
  const int32_t widths[2] = {obs_dim, hidden};
  for (int w : widths)
    if (w < 1 || w > RL_RDISTILL_MAX_WIDTH)
      return fail("unsupported width " + std::to_string(w) + " of the observation row or the hidden state (1.." + std::to_string(RL_RDISTILL_MAX_WIDTH) + ")");
  for (int l = 0; l <= n_layers; ++l)
    if (head_dims[l] < 1 || head_dims[l] > RL_RDISTILL_MAX_WIDTH)
      return fail("unsupported layer width " + std::to_string(head_dims[l]) + " (1.." + std::to_string(RL_RDISTILL_MAX_WIDTH) + ")");
  if (head_dims[0] != hidden) return fail("the head's input width must be the hidden size " + std::to_string(hidden));
  if (hyper->gradient_length < 1) return fail("gradient_length " + std::to_string(hyper->gradient_length) + " must be >= 1");
  if (hyper->num_learning_epochs < 1) return fail("num_learning_epochs " + std::to_string(hyper->num_learning_epochs) + " must be >= 1");
  if (!std::isfinite(hyper->learning_rate) || !(hyper->learning_rate > 0.0)) return fail("the learning rate must be finite and > 0");
  if (hyper->loss_type != RL_DISTILL_LOSS_MSE && hyper->loss_type != RL_DISTILL_LOSS_HUBER)
    return fail("unknown loss type " + std::to_string(hyper->loss_type) + " (0: mse, 1: huber)");
  if (!(hyper->max_grad_norm >= 0.f)) return fail("max_grad_norm must be > 0, or 0 for none");
  if (num_envs < 1) return fail("num_envs " + std::to_string(num_envs) + " must be >= 1");
  if ((long long)hyper->gradient_length * num_envs > 0x7fffffffLL) return fail("gradient_length x num_envs rows do not fit 31 bits");
  if (hipSetDevice(device) != hipSuccess) return fail("hipSetDevice failed (the HIP learner needs a GPU; there is no CPU path)");
  rl_rdistill* p = new rl_rdistill();
  p->device = device; p->L = n_layers; p->A = head_dims[n_layers]; p->H = hidden; p->N = num_envs; p->hp = *hyper;
  p->max_rows = (long)hyper->gradient_length * num_envs;
  const long H4 = 4L * hidden;
  Mem& M = p->mem;
  Net& Nt = p->net;
  long off = 0;
  M.D = obs_dim;
  M.wih = off; off += H4 * obs_dim;
  M.whh = off; off += H4 * hidden;
  M.bih = off; off += H4;
  M.bhh = off; off += H4;
  for (int l = 0; l <= n_layers; ++l) Nt.dims[l] = head_dims[l];
  for (int l = 0; l < n_layers; ++l) {
    Nt.w_off[l] = off; off += (long)head_dims[l] * head_dims[l + 1];
    Nt.b_off[l] = off; off += head_dims[l + 1];
  }
  p->n_params = off;
  const size_t rows = (size_t)p->max_rows, nH = (size_t)num_envs * hidden;
  std::vector<void*>& own = p->allocs;
  bool ok = dalloc(own, &p->params, (size_t)off) && dalloc(own, &p->grads, (size_t)off) && dalloc(own, &p->m1, (size_t)off) && dalloc(own, &p->m2, (size_t)off) &&
            dalloc(own, &p->norm_part, (size_t)NORM_BLOCKS) && dalloc(own, &p->st, 1) && dalloc(own, &p->idx, rows) &&
            dalloc(own, &p->steps, (size_t)hyper->gradient_length) &&
            dalloc(own, &p->head_part, (size_t)hyper->gradient_length * (size_t)((num_envs + 255) / 256)) && dalloc(own, &p->h_carry, nH) &&
            dalloc(own, &p->c_carry, nH);
  const int s_cap = (int)std::max<size_t>(1, (rows + TK - 1) / TK);  // no chunk shorter than a slice
  ok = ok && dalloc(own, &M.ZX, rows * H4) && dalloc(own, &M.G, rows * H4) && dalloc(own, &M.DZ, rows * H4) && dalloc(own, &M.HS, rows * hidden) &&
       dalloc(own, &M.Hout, rows * hidden) && dalloc(own, &M.C, rows * hidden) && dalloc(own, &M.dHh, rows * hidden) && dalloc(own, &M.DC, nH) &&
       dalloc(own, &M.bsum, (size_t)H4);
  M.S_ih = std::max(1, std::min(256 / (tiles_of((int)H4) * tiles_of(M.D)), s_cap));  // one network: ~256 workgroups per problem in the dW launch
  M.S_hh = std::max(1, std::min(256 / (tiles_of((int)H4) * tiles_of(hidden)), s_cap));
  ok = ok && dalloc(own, &M.part_ih, (size_t)M.S_ih * (size_t)(H4 * M.D)) && dalloc(own, &M.part_hh, (size_t)M.S_hh * (size_t)(H4 * hidden + 2 * H4));
  Nt.h[0] = M.Hout;
  Nt.dz[0] = M.dHh;
  for (int l = 0; l < n_layers && ok; ++l) {
    const int Nn = Nt.dims[l + 1], K = Nt.dims[l];
    ok = dalloc(own, &Nt.h[l + 1], rows * Nn) && dalloc(own, &Nt.dz[l + 1], rows * Nn);
    Nt.S[l] = std::max(1, std::min(256 / (tiles_of(Nn) * tiles_of(K)), s_cap));
    ok = ok && dalloc(own, &Nt.part[l], (size_t)Nt.S[l] * ((size_t)Nn * K + Nn));
  }
  if (ok) {
    DevState st{};
    st.lr = hyper->learning_rate;
    ok = hipMemcpy(p->st, &st, sizeof(st), hipMemcpyHostToDevice) == hipSuccess;
  }
  if (!ok) {
    rl_rdistill_destroy(p);
    return fail("device allocation failed");
  }
  *out = p;
  return 0;
}

int64_t rl_rdistill_num_parameters(const rl_rdistill* p) { return p ? p->n_params : 0; }

int rl_rdistill_set_parameters(rl_rdistill* p, const float* const* lstm_dev, const float* const* w_dev, const float* const* b_dev, void* stream) {
  if (!p) return fail("null argument");
  return rdistill_copy_parameters(p, lstm_dev, w_dev, b_dev, true, (hipStream_t)stream);
}

int rl_rdistill_get_parameters(rl_rdistill* p, float* const* lstm_dev, float* const* w_dev, float* const* b_dev, void* stream) {
  if (!p) return fail("null argument");
  return rdistill_copy_parameters(p, lstm_dev, w_dev, b_dev, false, (hipStream_t)stream);
}

int rl_rdistill_parameter_pointers(rl_rdistill* p, const float** lstm_dev, const float** w_dev, const float** b_dev) {
  if (!p) return fail("null argument");
  const long off[4] = {p->mem.wih, p->mem.whh, p->mem.bih, p->mem.bhh};
  for (int j = 0; j < 4 && lstm_dev; ++j) lstm_dev[j] = p->params + off[j];
  for (int l = 0; l < p->L; ++l) {
    if (w_dev) w_dev[l] = p->params + p->net.w_off[l];
    if (b_dev) b_dev[l] = p->params + p->net.b_off[l];
  }
  return 0;
}

int rl_rdistill_get_flat(rl_rdistill* p, int32_t which, float* dst_dev, void* stream) {
  if (!p || !dst_dev) return fail("null argument");
  if (which < 0 || which > 3) return fail("rl_rdistill_get_flat: which must be 0..3");
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  const float* src[4] = {p->params, p->grads, p->m1, p->m2};
  const hipError_t e = hipMemcpyAsync(dst_dev, src[which], (size_t)p->n_params * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail(hipGetErrorString(e));
}

int rl_rdistill_set_flat(rl_rdistill* p, int32_t which, const float* src_dev, void* stream) {
  if (!p || !src_dev) return fail("null argument");
  if (which != 2 && which != 3) return fail("rl_rdistill_set_flat: which must be 2 or 3 (the Adam moments; parameters go through rl_rdistill_set_parameters)");
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  const hipError_t e = hipMemcpyAsync(which == 2 ? p->m1 : p->m2, src_dev, (size_t)p->n_params * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail(hipGetErrorString(e));
}

int rl_rdistill_get_optimizer(rl_rdistill* p, double* lr, int64_t* step, void* stream) {
  if (!p || !lr || !step) return fail("null argument");
  DevState st{};
  if (rdistill_read_state(p, stream, &st, "optimiser state")) return -1;
  *lr = st.lr;
  *step = (int64_t)st.step;
  return 0;
}

int rl_rdistill_set_optimizer(rl_rdistill* p, double lr, int64_t step, void* stream) {
  if (!p) return fail("null argument");
  if (!std::isfinite(lr) || !(lr > 0.0)) return fail("rl_rdistill_set_optimizer: the learning rate must be finite and > 0");
  if (step < 0) return fail("rl_rdistill_set_optimizer: the step counter must be >= 0");
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  hipLaunchKernelGGL(ppo_set_optimizer_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, p->st, lr, (long long)step);
  return check_launch();
}

int rl_rdistill_group_grad(rl_rdistill* p, const float* obs_dev, const float* teacher_actions_dev, const uint8_t* dones_dev, const float* h0_dev,
                           const float* c0_dev, const float* h_in_dev, const float* c_in_dev, int32_t n_envs, const int32_t* steps_host, int32_t n_steps,
                           void* stream) {
  const RdBatch b{obs_dev, teacher_actions_dev, dones_dev, h0_dev, c0_dev};
  if (rdistill_enter(p, b, true, n_envs)) return -1;
  hipStream_t s = (hipStream_t)stream;
  if (rdistill_list(p, "rl_rdistill_group_grad", h_in_dev, c_in_dev, n_envs, steps_host, n_steps, s)) return -1;
  return rdistill_group(p, b, n_envs, steps_host, n_steps, p->steps, 0, 1, RD_GRAD, nullptr, s);
}

int rl_rdistill_forward(rl_rdistill* p, const float* obs_dev, const uint8_t* dones_dev, const float* h0_dev, const float* c0_dev, const float* h_in_dev,
                        const float* c_in_dev, int32_t n_envs, const int32_t* steps_host, int32_t n_steps, float* mean_out_dev, void* stream) {
  const RdBatch b{obs_dev, nullptr, dones_dev, h0_dev, c0_dev};
  if (rdistill_enter(p, b, false, n_envs)) return -1;
  if (!mean_out_dev) return fail("null argument");
  hipStream_t s = (hipStream_t)stream;
  if (rdistill_list(p, "rl_rdistill_forward", h_in_dev, c_in_dev, n_envs, steps_host, n_steps, s)) return -1;
  return rdistill_group(p, b, n_envs, steps_host, n_steps, p->steps, 0, 1, RD_FORWARD, mean_out_dev, s);
}

int rl_rdistill_update(rl_rdistill* p, const float* obs_dev, const float* teacher_actions_dev, const uint8_t* dones_dev, const float* h0_dev,
                       const float* c0_dev, int32_t T, int32_t n_envs, void* stream) {
  const RdBatch b{obs_dev, teacher_actions_dev, dones_dev, h0_dev, c0_dev};
  if (rdistill_enter(p, b, true, n_envs)) return -1;
  if (T < 1 || (long long)T * n_envs > 0x7fffffffLL) return fail("rl_rdistill_update: T x n_envs outside 1..2^31 - 1 rows");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(p->st->acc, 0, sizeof(double) * 4, s) != hipSuccess || hipMemsetAsync(&p->st->n_minibatches, 0, sizeof(long long), s) != hipSuccess)
    return fail("cannot reset the statistics block");
  const long long total = (long long)p->hp.num_learning_epochs * T;
  const int gl = p->hp.gradient_length;
  std::vector<int> st((size_t)std::min<long long>(gl, total));
  for (long long c0 = 0; c0 < total; c0 += gl) {
    const int g = (int)std::min<long long>(gl, total - c0);
    for (int j = 0; j < g; ++j) st[j] = (int)((c0 + j) % T);
    if (rdistill_group(p, b, n_envs, st.data(), g, nullptr, (int)(c0 % T), T, g == gl ? RD_UPDATE : RD_LEFTOVER, nullptr, s)) return -1;
  }
  return 0;
}

int rl_rdistill_final_state(rl_rdistill* p, float* h_dev, float* c_dev, void* stream) {
  if (!p || !h_dev || !c_dev) return fail("null argument");
  if (p->last_n < 1) return fail("rl_rdistill_final_state: no group has run yet");
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  const size_t bytes = (size_t)p->last_n * p->H * 4;
  if (hipMemcpyAsync(h_dev, p->h_carry, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess ||
      hipMemcpyAsync(c_dev, p->c_carry, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess)
    return fail("rl_rdistill_final_state: copy failed");
  return 0;
}

int rl_rdistill_stats(rl_rdistill* p, double* out, void* stream) {
  if (!p || !out) return fail("null argument");
  DevState st{};
  if (rdistill_read_state(p, stream, &st, "statistics")) return -1;
  out[0] = st.acc[0] / (st.n_minibatches > 0 ? (double)st.n_minibatches : 1.0);
  out[1] = st.lr; out[2] = st.grad_norm; out[3] = st.acc[1]; out[4] = (double)st.step;
  return 0;
}

}  // extern "C"
