// rl_bptt.inl - the recurrent PPO learner for gfx950 (MI355X): `RecurrentPPO.update` of robot_lab_amd/recurrent.py (an LSTM in front of the actor's
// and the critic's MLP, back-propagation through time) as HIP kernels.  C-ABI: include/rl_bptt.h.  Included at the end of rl_ppo.hip: the GEMMs
// (ppo_gemm_kernel, the plain sides, plus the G_DXLIN instantiation for dL/dh behind the heads), the PPO head and its finish kernel, column sums,
// reduce, sum of squares and clip + Adam are the PPO learner's kernels; new here are the two step kernels and the row index.
//
// One block (n envs x T steps, rows in [T][n] order) is a fixed sequence of launches on the caller's stream:
//   prep      idx[t n + j] = t N + lo + j; bsum = b_ih + b_hh of both memories
//   zx        ONE forward GEMM without activation for both networks: zx = X W_ih^T + bsum over the T n gathered rows
//   forward   T launches of bptt_step_kernel<false>, both networks each: z_t = h~_{t-1} W_hh^T + zx_t, the reset as a select on the operand
//             fetch, the gate nonlinearities in the epilogue; kept for backward: the four activated gates, h~_{t-1}, c_t, h_t
//   heads     forward per layer on the contiguous h buffer, the PPO head + finish, dX per layer, and dL/dh = dZ_0 W_0 (G_DXLIN: no elu' factor)
//   backward  T launches of bptt_step_kernel<true>, t descending: dz_{t+1} W_hh on the matrix cores, the cell's backward in the epilogue, the
//             dc carry in place (element (row, unit) belongs to one thread)
//   dW        one launch for the four LSTM weight matrices (dz^T X gathered, dz^T h~), the column sums of dz into b_ih AND b_hh, reduce; the
//             heads' dW launch as a PPO mini-batch; sum of squares, clip + Adam, floor of std
// Tiles.  A workgroup is four wavefronts, each 32 rows x (NT x 32) columns of v_mfma_f32_32x32x2_f32 accumulators, 16-deep slices through
// LDS as ppo_gemm_kernel.  Forward: NT = 4, the four column blocks are the gates i, f, g, o of the SAME 32 hidden units, so a lane holds all four
// gates of its (row, unit) pairs and the epilogue needs no exchange; 128 rows x 32 units per workgroup = (n / 128) x (H / 32) x 2 workgroups:
// 128 at n = 1024, H = 256, where a 128 x 128-unit tile would give 32.  Backward: NT = 1 (128 rows x 32 units over the 4H-deep contraction): the
// same 128 workgroups; two LDS reads per MFMA of 64 cycles leave the matrix pipe the bottleneck.
#include "../../../include/rl_bptt.h"

namespace {

struct StepNet {
  const float* Whh;      // [4H][H]
  const float* hprev;    // forward: h_{t-1} [n][H] (t = 0: rows of h0)
  const float* cprev;    // c_{t-1} [n][H] (t = 0: rows of c0)
  const uint8_t* reset;  // reset_t of the block's rows = their dones[t - 1]; null at t = 0
  const uint8_t* cut;    // backward: reset_{t+1} = dones[t]; null at t = T - 1 (nothing is carried)
  const float* zx;       // forward: [n][4H]
  float* G;              // [n][4H] activated gates of step t (forward writes, backward reads)
  const float* Gnext;    // backward: the gates of step t + 1
  float *HS, *Hout, *C;  // [n][H]: h~_{t-1}, h_t, c_t of step t
  const float* dzn;      // backward: dz_{t+1} [n][4H]; null at t = T - 1
  const float* dH;       // backward: dL/dh_t from the heads [n][H]
  float* dz;             // backward: dz_t [n][4H], columns q H + u as W_ih / W_hh rows
  float* dc;             // backward: the carry dc_{t+1} -> dc_t, in place [n][H]
  int H;
};
struct StepArgs {
  StepNet net[2];
  int n;
};

__device__ __forceinline__ float bptt_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

template <bool BWD>
__global__ __launch_bounds__(256, 2) void bptt_step_kernel(StepArgs a) {
  constexpr int NT = BWD ? 1 : 4;      // column blocks of 32 per wavefront
  constexpr int LDB = 32 * NT + 4;     // LDS row stride of the B slice
  const StepNet& P = a.net[blockIdx.z];
  const int H = P.H, n = a.n, H4 = 4 * H;
  const int i0 = (int)blockIdx.x * TB, u0 = (int)blockIdx.y * 32;
  if (u0 >= H || i0 >= n) return;  // (uniform for the workgroup)
  __shared__ float As[TK * LD];
  __shared__ float Bs[TK * LDB];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int R = BWD ? (P.dzn ? H4 : 0) : H;  // contraction length; the last step of the backward pass carries nothing
  const int lda = BWD ? H4 : H;
  const float* A = BWD ? P.dzn : P.hprev;

  // A: 16 r x 16 rows per pass, eight passes (contraction-contiguous).  Forward: the reset is a select here, a reset row contributes exact zeros
  const int a_r = t & 15, a_o = t >> 4;
  size_t a_row[8];
  bool a_ok[8];
  for (int p = 0; p < 8; ++p) {
    const int i = i0 + a_o + 16 * p;
    a_ok[p] = i < n && !(!BWD && P.reset && P.reset[i]);
    a_row[p] = i < n ? (size_t)i * lda : 0;
  }
  // B forward: column j = 32 q + v is gate q of unit u0 + v: W_hh[q H + u0 + v][r], 16 r x 16 columns per pass, eight passes
  // B backward: column v is unit u0 + v: W_hh[r][u0 + v], 32 columns x 8 r per pass, two passes
  constexpr int NB = BWD ? 2 : 8;
  const int b_r = BWD ? (t >> 5) : (t & 15), b_o = BWD ? (t & 31) : (t >> 4);
  size_t b_row[NB];
  bool b_ok[NB];
  for (int p = 0; p < NB; ++p) {
    if (BWD) {
      b_ok[p] = u0 + b_o < H;
      b_row[p] = 0;
    } else {
      const int j = b_o + 16 * p, u = u0 + (j & 31);
      b_ok[p] = u < H;
      b_row[p] = u < H ? (size_t)((j >> 5) * H + u) * H : 0;
    }
  }
  float ra[8], rb[NB];
  auto fetch = [&](int r0) {
#pragma unroll
    for (int p = 0; p < 8; ++p) ra[p] = (a_ok[p] && r0 + a_r < R) ? A[a_row[p] + r0 + a_r] : 0.f;
#pragma unroll
    for (int p = 0; p < NB; ++p) {
      if (BWD) {
        const int r = r0 + b_r + 8 * p;
        rb[p] = (b_ok[p] && r < R) ? P.Whh[(size_t)r * H + u0 + b_o] : 0.f;
      } else {
        rb[p] = (b_ok[p] && r0 + b_r < R) ? P.Whh[b_row[p] + r0 + b_r] : 0.f;
      }
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int p = 0; p < 8; ++p) As[a_r * LD + a_o + 16 * p] = ra[p];
#pragma unroll
    for (int p = 0; p < NB; ++p) {
      if (BWD) Bs[(b_r + 8 * p) * LDB + b_o] = rb[p];
      else Bs[b_r * LDB + b_o + 16 * p] = rb[p];
    }
  };

  f32x16 acc[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[q][e] = 0.f;
  const int lr = lane >> 5, lc = lane & 31;  // MFMA operand maps: A[row = lane & 31][k = lane >> 5], B[k = lane >> 5][col = lane & 31]
  if (R > 0) fetch(0);
  for (int r0 = 0; r0 < R; r0 += TK) {
    stash();
    __syncthreads();
    if (r0 + TK < R) fetch(r0 + TK);  // the next slice travels while this one is multiplied
#pragma unroll
    for (int kk = 0; kk < TK / 2; ++kk) {
      const float a0 = As[(2 * kk + lr) * LD + 32 * wave + lc];
      const float* bp = Bs + (2 * kk + lr) * LDB + lc;
#pragma unroll
      for (int q = 0; q < NT; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bp[32 * q], acc[q], 0, 0, 0);
    }
    __syncthreads();
  }

  // D map of v_mfma_f32_32x32x2_f32: register e holds row 8 (e >> 2) + 4 (lane >> 5) + (e & 3), column lane & 31
  const int u = u0 + lc;
  if (u >= H) return;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int i = i0 + 32 * wave + 8 * (e >> 2) + 4 * lr + (e & 3);
    if (i >= n) continue;
    const size_t ru = (size_t)i * H + u, rg = (size_t)i * H4 + u;
    const bool rs = P.reset && P.reset[i];
    const float cs = rs ? 0.f : P.cprev[ru];  // c~_{t-1}
    if (!BWD) {
      const float hs = rs ? 0.f : P.hprev[ru];
      const float gi = bptt_sigmoid(acc[0][e] + P.zx[rg]), gf = bptt_sigmoid(acc[NT > 1 ? 1 : 0][e] + P.zx[rg + H]);
      const float gg = tanhf(acc[NT > 2 ? 2 : 0][e] + P.zx[rg + 2 * H]), go = bptt_sigmoid(acc[NT > 3 ? 3 : 0][e] + P.zx[rg + 3 * H]);
      const float c = gf * cs + gi * gg;
      P.G[rg] = gi; P.G[rg + H] = gf; P.G[rg + 2 * H] = gg; P.G[rg + 3 * H] = go;
      P.HS[ru] = hs;
      P.C[ru] = c;
      P.Hout[ru] = go * tanhf(c);
    } else {
      const bool carry = P.dzn && !P.cut[i];  // keep_{t+1}: no gradient crosses a done
      const float gi = P.G[rg], gf = P.G[rg + H], gg = P.G[rg + 2 * H], go = P.G[rg + 3 * H];
      const float tc = tanhf(P.C[ru]);
      const float dh = P.dH[ru] + (carry ? acc[0][e] : 0.f);
      const float dc = dh * go * (1.f - tc * tc) + (carry ? P.Gnext[rg + H] * P.dc[ru] : 0.f);
      P.dz[rg] = dc * gg * gi * (1.f - gi);
      P.dz[rg + H] = dc * cs * gf * (1.f - gf);
      P.dz[rg + 2 * H] = dc * gi * (1.f - gg * gg);
      P.dz[rg + 3 * H] = dh * tc * go * (1.f - go);
      P.dc[ru] = dc;
    }
  }
}

// idx[t n + j] = t N + lo + j: what the layer-0 row gather and the PPO head read as they read a permutation; bsum = b_ih + b_hh of both memories
__global__ __launch_bounds__(256) void bptt_prep_kernel(int64_t* idx, int n, int N, int lo, long rows, const float* bih_a, const float* bhh_a, float* bs_a,
                                                        const float* bih_c, const float* bhh_c, float* bs_c, int H4) {
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  if (m < rows) {
    const long tt = m / n;
    idx[m] = (int64_t)(tt * N + lo + (m - tt * n));
  }
  if (m < H4) {
    bs_a[m] = bih_a[m] + bhh_a[m];
    bs_c[m] = bih_c[m] + bhh_c[m];
  }
}

struct Mem {  // one memory (LSTM) of the learner
  int D = 0;                                             // input width
  long wih = 0, whh = 0, bih = 0, bhh = 0;               // offsets into the flat buffers
  float *ZX = nullptr, *G = nullptr, *DZ = nullptr;      // [rows][4H]
  float *HS = nullptr, *Hout = nullptr, *C = nullptr, *dHh = nullptr;  // [rows][H]
  float *DC = nullptr, *bsum = nullptr;                  // [n][H], [4H]
  float *part_ih = nullptr, *part_hh = nullptr;          // dW partials: [S_ih][4H D], [S_hh][4H H + 4H + 4H] (the column sums twice: b_ih, b_hh)
  int S_ih = 1, S_hh = 1;
};

}  // namespace

struct rl_bptt {
  int device = 0, L = 0, A = 0, H = 0, T = 0, N = 0, n = 0;
  long rows = 0;  // T n
  rl_ppo_hyper hp{};
  Mem mem[2];
  Net net[2];  // the heads; h[0] = the memory's h buffer, dz[0] = dL/dh
  long n_params = 0;
  float *params = nullptr, *grads = nullptr, *m1 = nullptr, *m2 = nullptr;
  float *dstd_rows = nullptr, *std_part = nullptr;
  int S_std = 1;
  double *head_part = nullptr, *norm_part = nullptr;
  int64_t* idx = nullptr;
  DevState* st = nullptr;
  std::vector<void*> allocs;
};

namespace {

enum { BPTT_FORWARD = 0, BPTT_GRAD = 1, BPTT_UPDATE = 2 };

// the launches of one block (see the head of this file)
int bptt_block(rl_bptt* p, const rl_bptt_batch* b, int lo, int mode, float* mean_out, float* value_out, hipStream_t s) {
  const int L = p->L, H = p->H, H4 = 4 * H, T = p->T, N = p->N, n = p->n, rows = (int)p->rows;
  const float* X[2] = {b->observations, b->privileged_observations};
  const float* h0[2] = {b->h0_a, b->h0_c};
  const float* c0[2] = {b->c0_a, b->c0_c};
  hipLaunchKernelGGL(bptt_prep_kernel, dim3((unsigned)((std::max<long>(p->rows, H4) + 255) / 256)), dim3(256), 0, s, p->idx, n, N, lo, p->rows,
                     p->params + p->mem[0].bih, p->params + p->mem[0].bhh, p->mem[0].bsum, p->params + p->mem[1].bih, p->params + p->mem[1].bhh, p->mem[1].bsum, H4);
  {  // the input half of the gates
    GemmBatch gb{};
    int tiles = 0;
    for (int k = 0; k < 2; ++k) {
      const Mem& M = p->mem[k];
      GemmProb& g = gb.p[k];
      g.A = X[k]; g.lda = M.D; g.B = p->params + M.wih; g.ldb = M.D; g.aux = M.bsum; g.C = M.ZX; g.ldc = H4;
      g.I = rows; g.J = H4; g.R = M.D; g.act = 0; g.gidx = p->idx;
      g.tilesJ = tiles_of(g.J); g.ntiles = tiles_of(g.I) * g.tilesJ;
      tiles = std::max(tiles, g.ntiles);
    }
    hipLaunchKernelGGL((ppo_gemm_kernel<G_FWD, false>), dim3(tiles, 1, 2), dim3(256), 0, s, gb);
  }
  const dim3 step_grid(tiles_of(n), (H + 31) / 32, 2);
  auto step_args = [&](int t) {
    StepArgs a{};
    a.n = n;
    for (int k = 0; k < 2; ++k) {
      const Mem& M = p->mem[k];
      StepNet& q = a.net[k];
      const size_t oH = (size_t)t * n * H, oG = (size_t)t * n * H4;
      q.Whh = p->params + M.whh; q.H = H;
      q.hprev = t > 0 ? M.Hout + oH - (size_t)n * H : h0[k] + (size_t)lo * H;
      q.cprev = t > 0 ? M.C + oH - (size_t)n * H : c0[k] + (size_t)lo * H;
      q.reset = t > 0 ? b->dones + (size_t)(t - 1) * N + lo : nullptr;
      q.cut = t + 1 < T ? b->dones + (size_t)t * N + lo : nullptr;
      q.zx = M.ZX + oG; q.G = M.G + oG; q.Gnext = t + 1 < T ? M.G + oG + (size_t)n * H4 : nullptr;
      q.HS = M.HS + oH; q.Hout = M.Hout + oH; q.C = M.C + oH;
      q.dzn = t + 1 < T ? M.DZ + oG + (size_t)n * H4 : nullptr;
      q.dH = M.dHh + oH; q.dz = M.DZ + oG; q.dc = M.DC;
    }
    return a;
  };
  for (int t = 0; t < T; ++t) hipLaunchKernelGGL(bptt_step_kernel<false>, step_grid, dim3(256), 0, s, step_args(t));
  for (int l = 0; l < L; ++l) {
    GemmBatch gb{};
    int tiles = 0;
    for (int k = 0; k < 2; ++k) {
      net_prob(gb.p[k], p->net[k], p->params, L, p->mem[k].Hout, G_FWD, l, rows);
      tiles = std::max(tiles, gb.p[k].ntiles);
    }
    hipLaunchKernelGGL((ppo_gemm_kernel<G_FWD, false>), dim3(tiles, 1, 2), dim3(256), 0, s, gb);
  }
  if (mode == BPTT_FORWARD) {
    if (hipMemcpyAsync(mean_out, p->net[0].h[L], (size_t)rows * p->A * 4, hipMemcpyDeviceToDevice, s) != hipSuccess ||
        hipMemcpyAsync(value_out, p->net[1].h[L], (size_t)rows * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
      return fail("rl_bptt_forward: cannot copy the outputs");
    return check_launch();
  }
  {
    HeadArgs a{};
    a.mean = p->net[0].h[L]; a.value = p->net[1].h[L];
    a.b.observations = b->observations; a.b.privileged_observations = b->privileged_observations; a.b.actions = b->actions; a.b.values = b->values;
    a.b.returns = b->returns; a.b.advantages = b->advantages; a.b.actions_log_prob = b->actions_log_prob; a.b.mu = b->mu; a.b.sigma = b->sigma;
    a.idx = p->idx; a.std = p->params;
    a.dmean = p->net[0].dz[L]; a.dvalue = p->net[1].dz[L]; a.dstd_rows = p->dstd_rows; a.partials = p->head_part;
    a.n = rows; a.A = p->A; a.clip = p->hp.clip_param; a.value_loss_coef = p->hp.value_loss_coef; a.entropy_coef = p->hp.entropy_coef;
    a.use_clipped_value_loss = p->hp.use_clipped_value_loss; a.n0 = rows; a.n_terms = rows;
    const int blocks = (rows + 255) / 256;
    hipLaunchKernelGGL(ppo_head_kernel<false>, dim3(blocks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(ppo_head_finish_kernel<false>, dim3(1), dim3(64), 0, s, p->head_part, blocks, rows, rows, p->params, p->A, p->st,
                       mode == BPTT_UPDATE ? 1 : 0, p->hp.schedule == RL_PPO_SCHEDULE_ADAPTIVE ? 1 : 0, p->hp.desired_kl, (float*)nullptr);
  }
  for (int l = L - 1; l >= 0; --l) {  // l = 0: dL/dh of the memories' outputs, no elu' factor
    GemmBatch gb{};
    int tiles = 0;
    for (int k = 0; k < 2; ++k) {
      net_prob(gb.p[k], p->net[k], p->params, L, p->mem[k].Hout, G_DX, l, rows);
      tiles = std::max(tiles, gb.p[k].ntiles);
    }
    hipLaunchKernelGGL(side<GemmK>(l == 0, ppo_gemm_kernel<G_DXLIN, false>, ppo_gemm_kernel<G_DX, false>), dim3(tiles, 1, 2), dim3(256), 0, s, gb);
  }
  for (int t = T - 1; t >= 0; --t) hipLaunchKernelGGL(bptt_step_kernel<true>, step_grid, dim3(256), 0, s, step_args(t));
  {  // the memories' weight gradients: problems (k, ih), (k, hh); the column sums of dz go to b_ih and b_hh behind dW_hh
    GemmBatch gb{};
    ColBatch cb{};
    RedBatch rb{};
    int tiles = 0, Smax = 1;
    long redmax = 1;
    for (int k = 0; k < 2; ++k) {
      const Mem& M = p->mem[k];
      for (int w = 0; w < 2; ++w) {
        const int K = w == 0 ? M.D : H;
        GemmProb& g = gb.p[2 * k + w];
        g.A = M.DZ; g.lda = H4; g.B = w == 0 ? X[k] : M.HS; g.ldb = K; g.C = w == 0 ? M.part_ih : M.part_hh; g.ldc = K;
        g.I = H4; g.J = K; g.R = rows; g.S = w == 0 ? M.S_ih : M.S_hh; g.chunk = chunk_rows(rows, g.S);
        g.cstride = w == 0 ? (long)H4 * K : (long)H4 * K + 2 * H4;
        g.gidx = w == 0 ? p->idx : nullptr;
        g.tilesJ = tiles_of(g.J); g.ntiles = tiles_of(g.I) * g.tilesJ;
        RedProb& r = rb.p[2 * k + w];
        r.part = g.C; r.out = p->grads + (w == 0 ? M.wih : M.whh); r.count = g.cstride; r.stride = g.cstride; r.S = g.S;  // (b_ih, b_hh follow W_hh)
        tiles = std::max(tiles, g.ntiles); Smax = std::max(Smax, g.S); redmax = std::max(redmax, r.count);
        ColProb& c = cb.p[2 * k + w];  // w = 0: b_ih's copy, w = 1: b_hh's; both in the chunks of the hh problem
        c.Z = M.DZ; c.part = M.part_hh; c.N = H4; c.M = rows; c.ld = H4; c.S = M.S_hh; c.chunk = chunk_rows(rows, M.S_hh);
        c.stride = (long)H4 * H + 2 * H4; c.off = (long)H4 * H + (long)w * H4;
      }
    }
    hipLaunchKernelGGL((ppo_gemm_kernel<G_DW, false>), dim3(tiles, Smax, 4), dim3(256), 0, s, gb);
    hipLaunchKernelGGL(ppo_colsum_kernel, dim3((H4 + 63) / 64, Smax, 4), dim3(256), 0, s, cb);
    hipLaunchKernelGGL(ppo_reduce_kernel, dim3((unsigned)std::min<long>((redmax + 255) / 256, 512), 4), dim3(256), 0, s, rb);
  }
  {  // the heads' weight gradients and dL/dstd, as a PPO mini-batch
    GemmBatch gb{};
    ColBatch cb{};
    RedBatch rb{};
    int tiles = 0, Smax = 1, colx = 1, np = 0;
    long redmax = 1;
    for (int k = 0; k < 2; ++k)
      for (int l = 0; l < L; ++l, ++np) {
        const Net& Nt = p->net[k];
        const int Nn = Nt.dims[l + 1], K = Nt.dims[l];
        GemmProb& g = gb.p[np];
        net_prob(g, Nt, p->params, L, p->mem[k].Hout, G_DW, l, rows);
        ColProb& c = cb.p[np];
        c.Z = Nt.dz[l + 1]; c.part = Nt.part[l]; c.N = Nn; c.M = g.R; c.ld = Nn; c.S = g.S; c.chunk = g.chunk; c.stride = g.cstride; c.off = (long)Nn * K;
        RedProb& r = rb.p[np];
        r.part = Nt.part[l]; r.out = p->grads + Nt.w_off[l]; r.count = g.cstride; r.stride = g.cstride; r.S = g.S;  // (b follows W in the flat layout)
        tiles = std::max(tiles, g.ntiles); Smax = std::max(Smax, g.S); colx = std::max(colx, (Nn + 63) / 64); redmax = std::max(redmax, r.count);
      }
    ColProb& c = cb.p[np];
    c.Z = p->dstd_rows; c.part = p->std_part; c.N = p->A; c.M = rows; c.ld = p->A; c.S = p->S_std; c.chunk = chunk_rows(rows, c.S); c.stride = p->A; c.off = 0;
    RedProb& r = rb.p[np];
    r.part = p->std_part; r.out = p->grads; r.count = p->A; r.stride = p->A; r.S = p->S_std;
    colx = std::max(colx, (p->A + 63) / 64); Smax = std::max(Smax, p->S_std);
    hipLaunchKernelGGL((ppo_gemm_kernel<G_DW, false>), dim3(tiles, Smax, np), dim3(256), 0, s, gb);
    hipLaunchKernelGGL(ppo_colsum_kernel, dim3(colx, Smax, np + 1), dim3(256), 0, s, cb);
    hipLaunchKernelGGL(ppo_reduce_kernel, dim3((unsigned)std::min<long>((redmax + 255) / 256, 512), np + 1), dim3(256), 0, s, rb);
  }
  if (mode == BPTT_UPDATE) {
    hipLaunchKernelGGL(ppo_sumsq_kernel<false>, dim3(NORM_BLOCKS), dim3(256), 0, s, p->grads, p->n_params, p->norm_part, 1.0f);
    hipLaunchKernelGGL(ppo_adam_kernel<false>, dim3((unsigned)((p->n_params + 255) / 256)), dim3(256), 0, s, p->params, p->grads, p->m1, p->m2, p->n_params,
                       p->A, p->norm_part, p->st, p->hp.max_grad_norm, 1.0f);
  }
  return check_launch();
}

int bptt_enter(rl_bptt* p, const rl_bptt_batch* b, int lo) {
  if (!p) return fail("null argument");
  if (!b || !b->observations || !b->privileged_observations || !b->actions || !b->values || !b->returns || !b->advantages || !b->actions_log_prob || !b->mu ||
      !b->sigma || !b->dones || !b->h0_a || !b->c0_a || !b->h0_c || !b->c0_c)
    return fail("null batch pointer");
  if (lo < 0 || lo + p->n > p->N) return fail("block " + std::to_string(lo) + " .. " + std::to_string(lo + p->n - 1) + " outside the " + std::to_string(p->N) + " envs");
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  return 0;
}

int bptt_read_state(rl_bptt* p, void* stream, DevState* st, const char* what) {
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return fail("stream synchronisation failed");
  if (hipMemcpy(st, p->st, sizeof(*st), hipMemcpyDeviceToHost) != hipSuccess) return fail(std::string(what) + " copy failed");
  return 0;
}

// (offset, count) of the four tensors of memory k in the flat buffers
void bptt_mem_slots(const rl_bptt* p, int k, long off[4], size_t count[4]) {
  const Mem& M = p->mem[k];
  const size_t H4 = (size_t)4 * p->H;
  off[0] = M.wih; off[1] = M.whh; off[2] = M.bih; off[3] = M.bhh;
  count[0] = H4 * M.D; count[1] = H4 * p->H; count[2] = H4; count[3] = H4;
}

int bptt_copy_parameters(rl_bptt* p, const float* const* la, const float* const* lc, const float* const* aw, const float* const* ab, const float* const* cw,
                         const float* const* cb, const float* sd, bool to_flat, hipStream_t s) {
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  auto cp = [&](const float* user, long off, size_t count) {
    if (!user) return fail("null parameter pointer");
    float* flat = p->params + off;
    const hipError_t e = to_flat ? hipMemcpyAsync(flat, user, count * 4, hipMemcpyDeviceToDevice, s)
                                 : hipMemcpyAsync(const_cast<float*>(user), flat, count * 4, hipMemcpyDeviceToDevice, s);
    return e == hipSuccess ? 0 : fail(hipGetErrorString(e));
  };
  const float* const* Lm[2] = {la, lc};
  const float* const* W[2] = {aw, cw};
  const float* const* B[2] = {ab, cb};
  for (int k = 0; k < 2; ++k) {
    long off[4];
    size_t count[4];
    bptt_mem_slots(p, k, off, count);
    for (int j = 0; j < 4 && Lm[k]; ++j)
      if (cp(Lm[k][j], off[j], count[j])) return -1;
    for (int l = 0; l < p->L; ++l) {
      const Net& Nt = p->net[k];
      if (W[k] && cp(W[k][l], Nt.w_off[l], (size_t)Nt.dims[l] * Nt.dims[l + 1])) return -1;
      if (B[k] && cp(B[k][l], Nt.b_off[l], (size_t)Nt.dims[l + 1])) return -1;
    }
  }
  if (sd && cp(sd, 0, (size_t)p->A)) return -1;
  return 0;
}

}  // namespace

extern "C" {

const char* rl_bptt_last_error(void) { return err().c_str(); }

int rl_bptt_destroy(rl_bptt* p) {
  if (!p) return 0;
  (void)hipSetDevice(p->device);
  for (void* q : p->allocs) (void)hipFree(q);
  delete p;
  return 0;
}

int rl_bptt_create(int32_t obs_dim, int32_t critic_obs_dim, int32_t hidden, const int32_t* actor_dims, const int32_t* critic_dims, int32_t n_layers,
                   int32_t activation, const rl_ppo_hyper* hyper, int32_t T, int32_t num_envs, int32_t device, rl_bptt** out) {
  if (out) *out = nullptr;
  if (!actor_dims || !critic_dims || !hyper || !out) return fail("null argument");
  if (n_layers < 1 || n_layers > RL_BPTT_MAX_LAYERS)
    return fail("unsupported layer count " + std::to_string(n_layers) + " (1.." + std::to_string(RL_BPTT_MAX_LAYERS) + ")");
  if (activation != RL_PPO_ACT_ELU) return fail("unsupported activation: the HIP recurrent learner implements ELU only (use the torch learner of robot_lab_amd/recurrent.py)");
  if (hyper->std_type != RL_PPO_STD_SCALAR) return fail("unsupported noise_std_type: the HIP recurrent learner implements \"scalar\" only (use the torch learner)");
  const int32_t widths[3] = {obs_dim, critic_obs_dim, hidden};
  for (int w : widths)
    if (w < 1 || w > RL_BPTT_MAX_WIDTH) return fail("unsupported width " + std::to_string(w) + " of an observation row or the hidden state (1.." + std::to_string(RL_BPTT_MAX_WIDTH) + ")");
  for (int l = 0; l <= n_layers; ++l)
    if (actor_dims[l] < 1 || actor_dims[l] > RL_BPTT_MAX_WIDTH || critic_dims[l] < 1 || critic_dims[l] > RL_BPTT_MAX_WIDTH)
      return fail("unsupported layer width " + std::to_string(std::max(actor_dims[l], critic_dims[l])) + " (1.." + std::to_string(RL_BPTT_MAX_WIDTH) + ")");
  if (actor_dims[0] != hidden || critic_dims[0] != hidden) return fail("the heads' input width must be the hidden size " + std::to_string(hidden));
  if (critic_dims[n_layers] != 1) return fail("the critic's output width must be 1");
  if (hyper->num_learning_epochs < 1 || hyper->num_mini_batches < 1) return fail("num_learning_epochs and num_mini_batches must be positive");
  if (hyper->schedule != RL_PPO_SCHEDULE_FIXED && hyper->schedule != RL_PPO_SCHEDULE_ADAPTIVE) return fail("unknown schedule");
  if (hyper->schedule == RL_PPO_SCHEDULE_ADAPTIVE && !(hyper->desired_kl > 0.0))
    return fail("the adaptive schedule needs desired_kl > 0 (no target: pass RL_PPO_SCHEDULE_FIXED)");
  if (!(hyper->learning_rate > 0.0) || !(hyper->clip_param > 0.f) || !(hyper->max_grad_norm > 0.f)) return fail("learning_rate, clip_param and max_grad_norm must be positive");
  if (num_envs < hyper->num_mini_batches)
    return fail(std::to_string(num_envs) + " envs do not fill " + std::to_string(hyper->num_mini_batches) + " mini-batches of whole trajectories (num_envs < num_mini_batches)");
  if (T < 1) return fail("T " + std::to_string(T) + " must be >= 1");
  if ((long long)T * num_envs > 0x7fffffffLL) return fail("T x num_envs rows do not fit 31 bits");
  if (hipSetDevice(device) != hipSuccess) return fail("hipSetDevice failed (the HIP learner needs a GPU; there is no CPU path)");
  rl_bptt* p = new rl_bptt();
  p->device = device; p->L = n_layers; p->A = actor_dims[n_layers]; p->H = hidden; p->T = T; p->N = num_envs; p->hp = *hyper;
  p->n = num_envs / hyper->num_mini_batches;
  p->rows = (long)T * p->n;
  const long H4 = 4L * hidden;
  long off = p->A;  // std first: the order of ActorCriticRecurrent.parameters()
  for (int k = 0; k < 2; ++k) {
    Mem& M = p->mem[k];
    M.D = k == 0 ? obs_dim : critic_obs_dim;
    M.wih = off; off += H4 * M.D;
    M.whh = off; off += H4 * hidden;
    M.bih = off; off += H4;
    M.bhh = off; off += H4;
  }
  for (int k = 0; k < 2; ++k) {
    Net& Nt = p->net[k];
    const int32_t* d = k == 0 ? actor_dims : critic_dims;
    for (int l = 0; l <= n_layers; ++l) Nt.dims[l] = d[l];
    for (int l = 0; l < n_layers; ++l) {
      Nt.w_off[l] = off; off += (long)d[l] * d[l + 1];
      Nt.b_off[l] = off; off += d[l + 1];
    }
  }
  p->n_params = off;
  const size_t rows = (size_t)p->rows;
  std::vector<void*>& own = p->allocs;
  bool ok = dalloc(own, &p->params, (size_t)off) && dalloc(own, &p->grads, (size_t)off) && dalloc(own, &p->m1, (size_t)off) && dalloc(own, &p->m2, (size_t)off) &&
            dalloc(own, &p->norm_part, (size_t)NORM_BLOCKS) && dalloc(own, &p->st, 1) && dalloc(own, &p->idx, rows);
  const int s_cap = (int)std::max<size_t>(1, (rows + TK - 1) / TK);  // no chunk shorter than a slice
  for (int k = 0; k < 2 && ok; ++k) {
    Mem& M = p->mem[k];
    ok = dalloc(own, &M.ZX, rows * H4) && dalloc(own, &M.G, rows * H4) && dalloc(own, &M.DZ, rows * H4) && dalloc(own, &M.HS, rows * hidden) &&
         dalloc(own, &M.Hout, rows * hidden) && dalloc(own, &M.C, rows * hidden) && dalloc(own, &M.dHh, rows * hidden) &&
         dalloc(own, &M.DC, (size_t)p->n * hidden) && dalloc(own, &M.bsum, (size_t)H4);
    M.S_ih = std::max(1, std::min(128 / (tiles_of((int)H4) * tiles_of(M.D)), s_cap));
    M.S_hh = std::max(1, std::min(128 / (tiles_of((int)H4) * tiles_of(hidden)), s_cap));
    ok = ok && dalloc(own, &M.part_ih, (size_t)M.S_ih * (size_t)(H4 * M.D)) && dalloc(own, &M.part_hh, (size_t)M.S_hh * (size_t)(H4 * hidden + 2 * H4));
    Net& Nt = p->net[k];
    Nt.h[0] = M.Hout;
    Nt.dz[0] = M.dHh;
    for (int l = 0; l < n_layers && ok; ++l) {
      const int Nn = Nt.dims[l + 1], K = Nt.dims[l];
      ok = dalloc(own, &Nt.h[l + 1], rows * Nn) && dalloc(own, &Nt.dz[l + 1], rows * Nn);
      Nt.S[l] = std::max(1, std::min(128 / (tiles_of(Nn) * tiles_of(K)), s_cap));
      ok = ok && dalloc(own, &Nt.part[l], (size_t)Nt.S[l] * ((size_t)Nn * K + Nn));
    }
  }
  p->S_std = std::max(1, std::min(64, s_cap));
  ok = ok && dalloc(own, &p->dstd_rows, rows * p->A) && dalloc(own, &p->std_part, (size_t)p->S_std * p->A) && dalloc(own, &p->head_part, ((rows + 255) / 256) * 3);
  if (ok) {
    std::vector<float> ones((size_t)p->A, 1.0f);
    DevState st{};
    st.lr = hyper->learning_rate;
    ok = hipMemcpy(p->params, ones.data(), ones.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(p->st, &st, sizeof(st), hipMemcpyHostToDevice) == hipSuccess;
  }
  if (!ok) {
    rl_bptt_destroy(p);
    return fail("device allocation failed");
  }
  *out = p;
  return 0;
}

int64_t rl_bptt_num_parameters(const rl_bptt* p) { return p ? p->n_params : 0; }

int rl_bptt_set_parameters(rl_bptt* p, const float* const* lstm_a_dev, const float* const* lstm_c_dev, const float* const* actor_w_dev,
                           const float* const* actor_b_dev, const float* const* critic_w_dev, const float* const* critic_b_dev, const float* std_dev,
                           void* stream) {
  if (!p) return fail("null argument");
  return bptt_copy_parameters(p, lstm_a_dev, lstm_c_dev, actor_w_dev, actor_b_dev, critic_w_dev, critic_b_dev, std_dev, true, (hipStream_t)stream);
}

int rl_bptt_get_parameters(rl_bptt* p, float* const* lstm_a_dev, float* const* lstm_c_dev, float* const* actor_w_dev, float* const* actor_b_dev,
                           float* const* critic_w_dev, float* const* critic_b_dev, float* std_dev, void* stream) {
  if (!p) return fail("null argument");
  return bptt_copy_parameters(p, lstm_a_dev, lstm_c_dev, actor_w_dev, actor_b_dev, critic_w_dev, critic_b_dev, std_dev, false, (hipStream_t)stream);
}

int rl_bptt_parameter_pointers(rl_bptt* p, const float** lstm_a_dev, const float** lstm_c_dev, const float** actor_w_dev, const float** actor_b_dev,
                               const float** critic_w_dev, const float** critic_b_dev, const float** std_dev) {
  if (!p) return fail("null argument");
  const float** Lm[2] = {lstm_a_dev, lstm_c_dev};
  const float** W[2] = {actor_w_dev, critic_w_dev};
  const float** B[2] = {actor_b_dev, critic_b_dev};
  for (int k = 0; k < 2; ++k) {
    long off[4];
    size_t count[4];
    bptt_mem_slots(p, k, off, count);
    for (int j = 0; j < 4 && Lm[k]; ++j) Lm[k][j] = p->params + off[j];
    for (int l = 0; l < p->L; ++l) {
      if (W[k]) W[k][l] = p->params + p->net[k].w_off[l];
      if (B[k]) B[k][l] = p->params + p->net[k].b_off[l];
    }
  }
  if (std_dev) *std_dev = p->params;
  return 0;
}

int rl_bptt_get_flat(rl_bptt* p, int32_t which, float* dst_dev, void* stream) {
  if (!p || !dst_dev) return fail("null argument");
  if (which < 0 || which > 3) return fail("rl_bptt_get_flat: which must be 0..3");
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  const float* src[4] = {p->params, p->grads, p->m1, p->m2};
  const hipError_t e = hipMemcpyAsync(dst_dev, src[which], (size_t)p->n_params * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail(hipGetErrorString(e));
}

int rl_bptt_set_flat(rl_bptt* p, int32_t which, const float* src_dev, void* stream) {
  if (!p || !src_dev) return fail("null argument");
  if (which != 2 && which != 3) return fail("rl_bptt_set_flat: which must be 2 or 3 (the Adam moments; parameters go through rl_bptt_set_parameters)");
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  const hipError_t e = hipMemcpyAsync(which == 2 ? p->m1 : p->m2, src_dev, (size_t)p->n_params * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail(hipGetErrorString(e));
}

int rl_bptt_get_optimizer(rl_bptt* p, double* lr, int64_t* step, void* stream) {
  if (!p || !lr || !step) return fail("null argument");
  DevState st{};
  if (bptt_read_state(p, stream, &st, "optimiser state")) return -1;
  *lr = st.lr;
  *step = (int64_t)st.step;
  return 0;
}

int rl_bptt_set_optimizer(rl_bptt* p, double lr, int64_t step, void* stream) {
  if (!p) return fail("null argument");
  if (!std::isfinite(lr) || !(lr > 0.0)) return fail("rl_bptt_set_optimizer: the learning rate must be finite and > 0");
  if (step < 0) return fail("rl_bptt_set_optimizer: the step counter must be >= 0");
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  hipLaunchKernelGGL(ppo_set_optimizer_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, p->st, lr, (long long)step);
  return check_launch();
}

int rl_bptt_block_grad(rl_bptt* p, const rl_bptt_batch* batch, int32_t lo, void* stream) {
  if (bptt_enter(p, batch, lo)) return -1;
  return bptt_block(p, batch, lo, BPTT_GRAD, nullptr, nullptr, (hipStream_t)stream);
}

int rl_bptt_forward(rl_bptt* p, const rl_bptt_batch* batch, int32_t lo, float* mean_out_dev, float* value_out_dev, void* stream) {
  if (bptt_enter(p, batch, lo)) return -1;
  if (!mean_out_dev || !value_out_dev) return fail("null argument");
  return bptt_block(p, batch, lo, BPTT_FORWARD, mean_out_dev, value_out_dev, (hipStream_t)stream);
}

int rl_bptt_update(rl_bptt* p, const rl_bptt_batch* batch, void* stream) {
  if (bptt_enter(p, batch, 0)) return -1;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(p->st->acc, 0, sizeof(double) * 4, s) != hipSuccess || hipMemsetAsync(&p->st->n_minibatches, 0, sizeof(long long), s) != hipSuccess)
    return fail("cannot reset the statistics block");
  for (int e = 0; e < p->hp.num_learning_epochs; ++e)
    for (int i = 0; i < p->hp.num_mini_batches; ++i)
      if (bptt_block(p, batch, i * p->n, BPTT_UPDATE, nullptr, nullptr, s)) return -1;
  return 0;
}

int rl_bptt_stats(rl_bptt* p, double* out, void* stream) {
  if (!p || !out) return fail("null argument");
  DevState st{};
  if (bptt_read_state(p, stream, &st, "statistics")) return -1;
  const double nb = st.n_minibatches > 0 ? (double)st.n_minibatches : 1.0;
  out[0] = st.acc[0] / nb; out[1] = st.acc[1] / nb; out[2] = st.acc[2] / nb; out[3] = st.acc[3] / nb;
  out[4] = st.lr; out[5] = st.grad_norm; out[6] = (double)st.n_minibatches; out[7] = (double)st.step;
  return 0;
}

}  // extern "C"
