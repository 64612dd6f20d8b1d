// rl_ppo.hip - the PPO learner for gfx950 (MI355X): `PPO.update` of robot_lab_amd/ppo.py (rsl_rl's update rule) as HIP kernels.
// C-ABI: include/rl_ppo.h.
//
// One mini-batch is a fixed sequence of launches on the caller's stream, nothing of it returns to the host:
//   forward   per layer ONE launch for actor and critic (blockIdx.z): Y = elu(X W^T + b), rows of layer 0 gathered through the permutation
//   head      mean, value + the stored batch -> dL/dmean, dL/dvalue, the per-row terms of dL/dstd, partial loss / KL sums; a one-block
//             kernel orders the partials, moves the learning-rate word (KL-adaptive schedule) and the Adam step counter
//   dX        per hidden layer one launch for both networks: dZ_l = (dZ_{l+1} W_l) * elu'(H_l)   (elu' from the stored output: h > 0 ? 1 : h + 1)
//   dW        ONE launch for every layer of both networks: partial[s] = dZ^T X over the s-th chunk of rows (the deterministic split that
//             fills the CUs); column sums of dZ (bias gradients, dL/dstd) alike; one reduce launch adds the partials in chunk order
//   symmetry  (rl_ppo_set_symmetry) a mini-batch of n rows becomes n_sym n VIRTUAL rows, copy s in rows s n .. (s + 1) n: row v reads the
//             stored row idx[v % n] through the signed column permutation s = v / n.  The mirror lives in the operand fetch of the layer-0
//             forward and dW problems and in the head's action read (template flag SYM; one table word per column: source column |
//             sign bit); no mirrored copy of the batch exists in memory, every later stage only sees more rows
//   mirror    (rl_ppo_set_mirror_loss) rsl_rl's mirror loss on the same tables: the head's MIRROR instantiation reads, for a row of copy s >= 1,
//             the target S_s^act(mean of its copy-0 row) from the SAME mean buffer (written by the forward launch before it) and adds
//             c dL_mirror / dmean to its own row of dmean; a fourth per-block partial carries sum (mu - tau)^2.  Without the augmentation
//             only the ACTOR's problems keep n_sym n rows: the critic's problems, the std column sum and the loss means are those of the n
//             stored rows, and a row of a copy >= 1 carries the mirror gradient alone
//   obsnorm   (rl_ppo_set_obs_normalization) the batch holds RAW rows: the layer-0 forward and dW launches are the NORM instantiations of the GEMM, whose
//             fetch of X (or, without SYM, its stash into LDS) puts every loaded element - after the mirror - through y = (x - mean[c]) / (std[c] + eps) with the statistics of the
//             DESTINATION column c, rl_obsnorm_apply's three fp32 roundings; the statistics are read from the normalisers' own device vectors
//             at launch time; a group without statistics passes through the same launch unnormalised; no normalised copy of the batch exists
//   step      sum of squares in fixed blocks -> every block of the Adam kernel adds the same partials in the same order: norm, clip
//             coefficient, Adam, floor of std
//   world     (rl_ppo_set_world) one rank among several: rl_ppo_minibatch_local ends after the reduce launch and leaves the flat gradient and,
//             in word [P] behind it, the rank's KL statistic (the LOCAL side of the head-finish kernel) in the WIRE; the caller SUM-all-reduces
//             it; rl_ppo_minibatch_apply moves the learning rate from word [P] / world in a one-workgroup kernel and runs `step` on
//             g[i] / world (the SCALED sides of its two kernels; fp32 divisions, as the torch learner's `flat /= world_size`)
// The three GEMM shapes are one LDS-tiled kernel (128 x 128 output tile, 16-deep slices, four wavefronts of 64 x 64 = 2 x 2
// v_mfma_f32_32x32x2_f32 tiles: exact fp32 products, fp32 accumulation in contraction order).
#include <hip/hip_runtime.h>

#include <math.h>

#include <cmath>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/rl_ppo.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TB = 128;       // output tile edge
constexpr int TK = 16;        // contraction slice
constexpr int LD = TB + 4;    // LDS row stride: 4 r + i is a distinct bank for the 16 x 4 (r, i) pairs a wavefront stores at once
constexpr int MAXP = 2 * RL_PPO_MAX_LAYERS + 1;
constexpr float HALF_LOG_2PI = 0.9189385332046727f;
constexpr int tiles_of(int x) { return (x + TB - 1) / TB; }  // output tiles along an edge of x entries

enum { G_FWD = 0, G_DX = 1, G_DW = 2, G_DXLIN = 3 };

// C[I][J] = sum_r A(i, r) B(r, j):
//   G_FWD  i = row, j = output unit, r = input unit:  A = X[row(i)][r],  B = W[j][r];   C = act(. + bias[j])
//   G_DX   i = row, j = input unit,  r = output unit: A = dZ[i][r],      B = W[r][j];   C = . * elu'(H[i][j])
//   G_DXLIN  G_DX without the elu' factor: the gradient of a layer's INPUT that no activation produced (csrc/learner/rl_bptt.inl: dL/dh behind the heads)
//   G_DW   i = output unit, j = input unit, r = row:  A = dZ[r][i],      B = X[row(r)][j]; C = partial[s][i][j] over rows [s chunk, (s + 1) chunk)
struct GemmProb {
  const float* A;
  const float* B;
  float* C;
  const float* aux;     // G_FWD: bias; G_DX: H
  const int64_t* gidx;  // row gather of X (layer 0) or null
  int I, J, R;
  int lda, ldb, ldc, ldaux;
  int tilesJ, ntiles;
  int act;        // G_FWD: 1 = ELU follows
  int S, chunk;   // G_DW: number of row chunks, rows per chunk (multiple of TK)
  long cstride;   // G_DW: floats between the partials of consecutive chunks
  const int* sym; // SYM: [n_sym][columns of X] table words of the gathered operand (SYM_COL | SYM_NEG), or null (G_DW, layers past the first)
  int n0;         // SYM: stored rows of the mini-batch; virtual row v is copy v / n0 of row gidx[v % n0]
};
struct GemmBatch {
  GemmProb p[2 * RL_PPO_MAX_LAYERS];
};

// NORM: the statistics of the two observation groups, a second kernel argument of the NORM instantiations alone (GemmProb and the argument list of
// every other instantiation stay what they were); indexed like GemmBatch::p, a null mean = the problem's X is not normalised
struct NormProb {
  const float* mean;
  const float* std;
  float eps;
};
struct NormBatch {
  NormProb p[2 * RL_PPO_MAX_LAYERS];
};
// rl_obsnorm_apply's expression (csrc/rl_obsnorm.hip), bit for bit: an addition, a subtraction and a correctly rounded division in fp32, never fused
// and never a multiplication by a reciprocal.  The divisor of a column is formed once and kept
__device__ __forceinline__ float norm_divisor(float std, float eps) {
#pragma clang fp contract(off)
  return std + eps;
}
__device__ __forceinline__ float norm_apply(float x, float mean, float divisor) {
#pragma clang fp contract(off)
  return (x - mean) / divisor;
}
__device__ __forceinline__ const NormProb* norm_prob(int) { return nullptr; }
__device__ __forceinline__ const NormProb* norm_prob(int z, const NormBatch& nb) { return &nb.p[z]; }

// a symmetry table word: the source column, and the sign in the float's sign position (the mirror is an exact XOR)
constexpr int SYM_COL = 0x7fffffff, SYM_NEG = (int)0x80000000u;
__device__ __forceinline__ float sym_read(const float* row, int word) {
  return __int_as_float(__float_as_int(row[word & SYM_COL]) ^ (word & SYM_NEG));
}

// SYM (G_FWD, G_DW of a layer-0 launch): X is read through the symmetry tables, see GemmProb::sym.  SYM = false is the plain gather.
// NORM (G_FWD, G_DW of a layer-0 launch of a handle with rl_ppo_set_obs_normalization): the pack holds one NormBatch and every loaded element of X
// goes through norm_apply after the mirror; elements outside the problem stay 0.  An empty pack is the kernel of a learner without it, argument
// list included.
template <int MODE, bool SYM, class... NORM>
__global__ __launch_bounds__(256, 2) void ppo_gemm_kernel(GemmBatch batch, NORM... norm) {
  static_assert(!SYM || MODE != G_DX, "only the operands that read X are mirrored");
  constexpr bool NRM = sizeof...(NORM) != 0;
  static_assert(!NRM || MODE != G_DX, "only the operands that read X are normalised");
  const GemmProb& P = batch.p[blockIdx.z];
  if ((int)blockIdx.x >= P.ntiles || (int)blockIdx.y >= (MODE == G_DW ? P.S : 1)) return;  // (uniform for the workgroup)
  __shared__ float As[TK * LD];
  __shared__ float Bs[TK * LD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int i0 = ((int)blockIdx.x / P.tilesJ) * TB, j0 = ((int)blockIdx.x % P.tilesJ) * TB;
  const int r_begin = MODE == G_DW ? (int)blockIdx.y * P.chunk : 0;
  const int r_end = MODE == G_DW ? min(P.R, r_begin + P.chunk) : P.R;

  // a thread's eight elements of either operand tile: contraction-contiguous operands are read 16 r x 16 outer per pass, the others 128 outer x 2 r
  constexpr bool A_RC = MODE != G_DW, B_RC = MODE == G_FWD;
  const int a_r = A_RC ? (t & 15) : (t >> 7), a_o = A_RC ? (t >> 4) : (t & 127);
  const int b_r = B_RC ? (t & 15) : (t >> 7), b_o = B_RC ? (t >> 4) : (t & 127);
  size_t a_row[8];  // (A_RC) offsets of the eight outer rows
  size_t b_row[8];
  int a_tab[8];     // (SYM, G_FWD) offset of the row's copy in the table
  if (A_RC) {
    for (int p = 0; p < 8; ++p) {
      const int i = i0 + a_o + 16 * p;
      if (SYM && MODE == G_FWD) {  // the copy boundary falls anywhere in the tile: copy and row are per element
        const int s = i < P.I ? i / P.n0 : 0;
        a_row[p] = i < P.I ? (size_t)P.gidx[i - s * P.n0] * P.lda : 0;
        a_tab[p] = s * P.R;
      } else {
        a_row[p] = i < P.I ? (size_t)(MODE == G_FWD && P.gidx ? P.gidx[i] : i) * P.lda : 0;
      }
    }
  }
  const bool b_sym = SYM && MODE == G_DW && P.sym != nullptr;  // (uniform for the workgroup)
  const NormProb* NP = norm_prob((int)blockIdx.z, norm...);
  const bool normed = NRM && NP->mean != nullptr;            // (uniform for the workgroup)
  // (NORM, G_DW) a thread's column j0 + b_o of X is fixed for the whole kernel: its statistics are loaded once
  float b_mean = 0.f, b_div = 1.f;
  if constexpr (NRM && MODE == G_DW) {
    if (normed && j0 + b_o < P.J) {
      b_mean = NP->mean[j0 + b_o];
      b_div = norm_divisor(NP->std[j0 + b_o], NP->eps);
    }
  }
  if (B_RC) {
    for (int p = 0; p < 8; ++p) {
      const int j = j0 + b_o + 16 * p;
      b_row[p] = j < P.J ? (size_t)j * P.ldb : 0;
    }
  }
  float ra[8], rb[8];
  // (NORM) fetch loads the slice's elements and, G_FWD, the statistics of its column r0 + a_r (a thread's eight elements share it: one pair of loads
  // per slice, issued with the slice's own).  WHERE the divisions run is measured (profiles/ppo_hip_obsnorm_in_learner.txt): without SYM in stash, on
  // the way into LDS - after the multiply loop that the loads travel under, not in front of it, where they would wait for the loads (an update
  // with both groups normalised: +4 % instead of +13 %); with SYM in fetch - its dependent table-word and element loads are waited for there anyway, and
  // the later form costs registers (+2.8 % instead of +5.2 %)
  constexpr bool LATE = !SYM;
  float a_mean = 0.f, a_div = 1.f;
  int f_r0 = 0;  // the slice `ra` / `rb` hold
  // (NORM) element p of the held slice - of ra (G_FWD) or rb (G_DW) - in place, if it lies `inside` the problem: an element outside stays 0, never
  // (0 - mean) / divisor.  Called from fetch, where the load's own predicate says `inside`, or from stash, see LATE
  auto normalise = [&](int p, bool inside) {
    if constexpr (NRM) {
      if (!normed || !inside) return;
      if (MODE == G_FWD) ra[p] = norm_apply(ra[p], a_mean, a_div);
      else rb[p] = norm_apply(rb[p], b_mean, b_div);
    }
  };
  auto fetch = [&](int r0) {
    int sv = 0, mv = 0;  // (SYM, G_DW) copy and stored-row slot of the virtual row r0 + b_r + 2 p
    if (b_sym) {
      sv = (r0 + b_r) / P.n0;
      mv = (r0 + b_r) - sv * P.n0;
    }
    if constexpr (NRM && LATE) f_r0 = r0;
    if constexpr (NRM && MODE == G_FWD) {
      if (normed && r0 + a_r < r_end) {
        a_mean = NP->mean[r0 + a_r];
        a_div = norm_divisor(NP->std[r0 + a_r], NP->eps);
      }
    }
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      if (A_RC) {
        const int i = i0 + a_o + 16 * p, r = r0 + a_r;
        if (SYM && MODE == G_FWD) ra[p] = (i < P.I && r < r_end) ? sym_read(P.A + a_row[p], P.sym[a_tab[p] + r]) : 0.f;
        else ra[p] = (i < P.I && r < r_end) ? P.A[a_row[p] + r] : 0.f;
        if constexpr (NRM && MODE == G_FWD && !LATE) normalise(p, i < P.I && r < r_end);
      } else {
        const int i = i0 + a_o, r = r0 + a_r + 2 * p;
        ra[p] = (i < P.I && r < r_end) ? P.A[(size_t)r * P.lda + i] : 0.f;
      }
      if (B_RC) {
        const int j = j0 + b_o + 16 * p, r = r0 + b_r;
        rb[p] = (j < P.J && r < r_end) ? P.B[b_row[p] + r] : 0.f;
      } else {
        const int j = j0 + b_o, r = r0 + b_r + 2 * p;
        float v = 0.f;
        if (b_sym) {
          if (j < P.J && r < r_end) v = sym_read(P.B + (size_t)P.gidx[mv] * P.ldb, P.sym[sv * P.J + j]);
          for (mv += 2; mv >= P.n0; mv -= P.n0) ++sv;
        } else if (j < P.J && r < r_end) {
          const size_t row = MODE == G_DW && P.gidx ? (size_t)P.gidx[r] : (size_t)r;
          v = P.B[row * P.ldb + j];
        }
        rb[p] = v;
        if constexpr (NRM && MODE == G_DW && !LATE) normalise(p, j < P.J && r < r_end);
      }
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      if constexpr (NRM && LATE)
        normalise(p, MODE == G_FWD ? i0 + a_o + 16 * p < P.I && f_r0 + a_r < r_end : j0 + b_o < P.J && f_r0 + b_r + 2 * p < r_end);
      if (A_RC) As[a_r * LD + a_o + 16 * p] = ra[p];
      else As[(a_r + 2 * p) * LD + a_o] = ra[p];
      if (B_RC) Bs[b_r * LD + b_o + 16 * p] = rb[p];
      else Bs[(b_r + 2 * p) * LD + b_o] = rb[p];
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
  const int wi = (wave >> 1) * 64, wj = (wave & 1) * 64;
  const int lr = lane >> 5, lc = lane & 31;  // MFMA operand maps: A[row = lane & 31][k = lane >> 5], B[k = lane >> 5][col = lane & 31]

  if (r_begin < r_end) fetch(r_begin);
  for (int r0 = r_begin; r0 < r_end; r0 += TK) {
    stash();
    __syncthreads();
    if (r0 + TK < r_end) fetch(r0 + TK);  // the next slice travels while this one is multiplied
#pragma unroll
    for (int kk = 0; kk < TK / 2; ++kk) {
      const float* ap = As + (2 * kk + lr) * LD + wi + lc;
      const float* bp = Bs + (2 * kk + lr) * LD + wj + lc;
      const float a0 = ap[0], a1 = ap[32], b0 = bp[0], b1 = bp[32];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }

  // D map of v_mfma_f32_32x32x2_f32: register 4 g + e holds row 8 g + 4 (lane >> 5) + e, column lane & 31
  float* C = MODE == G_DW ? P.C + (size_t)blockIdx.y * P.cstride : P.C;
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
      const int j = j0 + wj + 32 * tj + lc;
      if (j >= P.J) continue;
      const float bias = MODE == G_FWD ? P.aux[j] : 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int i = i0 + wi + 32 * ti + 8 * (e >> 2) + 4 * lr + (e & 3);
        if (i >= P.I) continue;
        float v = acc[ti][tj][e];
        if (MODE == G_FWD) {
          v += bias;
          if (P.act) v = v > 0.f ? v : expm1f(v);
        } else if (MODE == G_DX) {
          const float h = P.aux[(size_t)i * P.ldaux + j];
          v *= h > 0.f ? 1.f : h + 1.f;
        }
        C[(size_t)i * P.ldc + j] = v;
      }
    }
}

// ---- column sums (bias gradients, dL/dstd): part[s][off + n] = sum over the rows of chunk s of Z[m][n], fp64 inside
struct ColProb {
  const float* Z;
  float* part;
  int N, M, ld, S, chunk;
  long stride, off;
};
struct ColBatch {
  ColProb p[MAXP];
};
__global__ __launch_bounds__(256) void ppo_colsum_kernel(ColBatch batch) {
  const ColProb& P = batch.p[blockIdx.z];
  if ((int)blockIdx.y >= P.S || (int)blockIdx.x * 64 >= P.N) return;
  __shared__ double sh[4][64];
  const int c = threadIdx.x & 63, q = threadIdx.x >> 6, n = (int)blockIdx.x * 64 + c;
  const int m0 = (int)blockIdx.y * P.chunk, m1 = min(P.M, m0 + P.chunk);
  double s = 0.0;
  if (n < P.N)
    for (int m = m0 + q; m < m1; m += 4) s += (double)P.Z[(size_t)m * P.ld + n];
  sh[q][c] = s;
  __syncthreads();
  if (q == 0 && n < P.N) P.part[(size_t)blockIdx.y * P.stride + P.off + n] = (float)(((sh[0][c] + sh[1][c]) + sh[2][c]) + sh[3][c]);
}

// ---- out[i] = sum_s part[s][i], s ascending, fp64 inside
struct RedProb {
  const float* part;
  float* out;
  long count, stride;
  int S;
};
struct RedBatch {
  RedProb p[MAXP];
};
__global__ __launch_bounds__(256) void ppo_reduce_kernel(RedBatch batch) {
  const RedProb& P = batch.p[blockIdx.y];
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < P.count; i += (long)gridDim.x * 256) {
    double s = 0.0;
    for (int k = 0; k < P.S; ++k) s += (double)P.part[(size_t)k * P.stride + i];
    P.out[i] = (float)s;
  }
}

// ---- sh[q * NT] = sum over t of sh[q * NT + t] for the Q rows of NT doubles in LDS at `rows`: THE halving tree of this file (thread t < w adds entry
// t + w to its own, w = NT / 2, NT / 4, .. 1), so every reduction adds in one order.  Called by all NT threads of the block after their writes to the rows.
// (The LDS pointer and the do-while keep the instruction streams of the hand-written trees this replaced: profiles/ppo_hip_refactor_isa_identity.txt.)
template <int NT, int Q>
__device__ __forceinline__ void block_sum(double* rows) {
  auto* sh = (__attribute__((address_space(3))) double*)rows;
  __syncthreads();
  for (int w = NT / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      int q = 0;
      do sh[q * NT + threadIdx.x] += sh[q * NT + threadIdx.x + w];
      while (++q < Q);
    }
    __syncthreads();
  }
}

// ---- loss head
struct DevState {
  double lr;           // the learning-rate word
  double acc[4];       // sums over the mini-batches of an update: value loss, surrogate, entropy, KL
  double grad_norm;    // last pre-clip gradient norm
  long long step;      // Adam step counter
  long long n_minibatches;
  double mirror_acc;   // sum over the mini-batches of an update of L_mirror (rl_ppo_set_mirror_loss)
};
struct HeadArgs {
  const float *mean, *value;  // [n][A], [n]
  rl_ppo_batch b;
  const int64_t* idx;
  const float* std;
  float *dmean, *dvalue, *dstd_rows;
  double* partials;  // [blocks][3]: surrogate, value loss, KL sums
  int n, A;          // n: the rows of mean / value (SYM: the n_sym n0 virtual rows)
  const int* asym;   // SYM: [n_sym][A] table words of the actions
  int n0;            // SYM: stored rows; virtual row m is copy m / n0 of row idx[m % n0]
  float clip, value_loss_coef, entropy_coef;
  int use_clipped_value_loss;
  // MIRROR: rows below n_terms carry the PPO terms (means over n_terms rows): n with the augmentation, n0 without - then value / dvalue /
  // dstd_rows hold n0 rows only; rows of copies >= 1 add mirror_coeff dL_mirror / dmean
  int n_terms;
  float mirror_coeff;
  double* mirror_partials;  // [blocks]: sum over the block's rows of copies >= 1 of (mu - tau)^2
};

// MIRROR (with SYM): the mirror loss, see HeadArgs::n_terms.  MIRROR = false is the code of a learner without rl_ppo_set_mirror_loss.
template <bool SYM, bool MIRROR = false>
__global__ __launch_bounds__(256) void ppo_head_kernel(HeadArgs a) {
  static_assert(SYM || !MIRROR, "the mirror loss reads the symmetry tables");
  __shared__ double sh[3][256];
  const int m = (int)blockIdx.x * 256 + threadIdx.x;
  double s_sur = 0.0, s_val = 0.0, s_kl = 0.0, s_mir = 0.0;
  if (m < a.n && (!MIRROR || m < a.n_terms)) {
    const int A = a.A;
    const int cp = SYM ? m / a.n0 : 0;  // the copy: every stored term of the row is repeated for it, the action is mirrored
    const size_t g = (size_t)a.idx[SYM ? m - cp * a.n0 : m];
    const int* aw = SYM ? a.asym + (size_t)cp * A : nullptr;
    auto action = [&](int k) { return SYM ? sym_read(a.b.actions + g * A, aw[k]) : a.b.actions[g * A + k]; };
    const float inv_n = 1.0f / (float)(MIRROR ? a.n_terms : a.n);
    float logp = 0.f, kl = 0.f;
    for (int k = 0; k < A; ++k) {
      const float sd = a.std[k], mu = a.mean[(size_t)m * A + k], d = action(k) - mu;
      logp += -0.5f * (d * d) / (sd * sd) - logf(sd) - HALF_LOG_2PI;
      const float so = a.b.sigma[g * A + k], dm = a.b.mu[g * A + k] - mu;
      kl += logf(sd / so + 1e-5f) + (so * so + dm * dm) / (2.0f * sd * sd) - 0.5f;
    }
    const float ratio = expf(logp - a.b.actions_log_prob[g]), adv = a.b.advantages[g];
    const float lo = 1.0f - a.clip, hi = 1.0f + a.clip;
    const float t1 = -adv * ratio, t2 = -adv * fminf(fmaxf(ratio, lo), hi);
    const float inr = (ratio >= lo && ratio <= hi) ? 1.f : 0.f;
    // d max(t1, t2) / d ratio as autograd has it: the larger branch; on a tie half of each
    const float gr = t1 > t2 ? -adv : (t1 < t2 ? -adv * inr : -adv * 0.5f * (1.f + inr));
    const float c = gr * ratio * inv_n;  // dL / dlogp
    const float v = a.value[m], ret = a.b.returns[g];
    float vloss, gv;
    if (a.use_clipped_value_loss) {
      const float vo = a.b.values[g], dv = v - vo;
      const float vc = vo + fminf(fmaxf(dv, -a.clip), a.clip);
      const float l1 = (v - ret) * (v - ret), l2 = (vc - ret) * (vc - ret);
      const float in2 = (dv >= -a.clip && dv <= a.clip) ? 1.f : 0.f;
      const float g1 = 2.f * (v - ret), g2 = 2.f * (vc - ret) * in2;
      vloss = fmaxf(l1, l2);
      gv = l1 > l2 ? g1 : (l1 < l2 ? g2 : 0.5f * (g1 + g2));
    } else {
      vloss = (ret - v) * (ret - v);
      gv = 2.f * (v - ret);
    }
    a.dvalue[m] = a.value_loss_coef * gv * inv_n;
    for (int k = 0; k < A; ++k) {
      const float sd = a.std[k], d = action(k) - a.mean[(size_t)m * A + k];
      a.dmean[(size_t)m * A + k] = c * d / (sd * sd);
      // dlogp / dstd and the entropy bonus (-entropy_coef * mean over rows of sum_k log std_k): the column sum over the rows is dL / dstd_k
      a.dstd_rows[(size_t)m * A + k] = c * (d * d / (sd * sd * sd) - 1.0f / sd) - a.entropy_coef * inv_n / sd;
    }
    s_sur = (double)fmaxf(t1, t2);
    s_val = (double)vloss;
    s_kl = SYM && cp != 0 ? 0.0 : (double)kl;  // the schedule's statistic is that of the stored rows (copy 0)
  }
  if (MIRROR && m < a.n && m >= a.n0) {
    // tau = S_cp^act(mean of the row's copy 0): rows of `mean` that the forward launch wrote and nobody writes here; this thread alone touches
    // row m of dmean (it wrote the PPO part above, or the row carries no PPO term)
    const int A = a.A, cp = m / a.n0, n_sym = a.n / a.n0;
    const float* src = a.mean + (size_t)(m - cp * a.n0) * A;
    const int* aw = a.asym + (size_t)cp * A;
    const float scale = a.mirror_coeff * 2.0f / ((float)(n_sym - 1) * (float)a.n0 * (float)A);
    for (int k = 0; k < A; ++k) {
      const float diff = a.mean[(size_t)m * A + k] - sym_read(src, aw[k]);
      const float gm = scale * diff;
      a.dmean[(size_t)m * A + k] = m < a.n_terms ? a.dmean[(size_t)m * A + k] + gm : gm;
      s_mir += (double)diff * (double)diff;
    }
  }
  sh[0][threadIdx.x] = s_sur; sh[1][threadIdx.x] = s_val; sh[2][threadIdx.x] = s_kl;
  block_sum<256, 3>(sh[0]);
  if (threadIdx.x < 3) a.partials[(size_t)blockIdx.x * 3 + threadIdx.x] = sh[threadIdx.x][0];
  if (MIRROR) {  // the fourth partial, through the same tree
    __syncthreads();
    sh[0][threadIdx.x] = s_mir;
    block_sum<256, 1>(sh[0]);
    if (threadIdx.x == 0) a.mirror_partials[blockIdx.x] = sh[0][0];
  }
}

// the KL-adaptive schedule and the counters of one mini-batch, by ONE thread (of ppo_head_finish_kernel<false>: the fused update; of
// ppo_world_apply_kernel: the split one): the learning-rate word moves on the statistic `kl`, which is booked; the Adam step and the mini-batch are counted
__device__ __forceinline__ void schedule_step(DevState* st, int adaptive, double desired_kl, float kl) {
  if (adaptive) {  // (rl_ppo_create: adaptive implies desired_kl > 0)
    // the host learner compares an fp32 statistic with thresholds formed in fp64
    if (kl > (float)(2.0 * desired_kl)) st->lr = fmax(1e-5, st->lr / 1.5);
    else if (kl > 0.f && kl < (float)(desired_kl / 2.0)) st->lr = fmin(1e-2, st->lr * 1.5);
    st->acc[3] += (double)kl;
  }
  st->step += 1;
  st->n_minibatches += 1;
}

// one workgroup of 64: orders the head's partial sums; with `apply` it books the statistics, moves the learning rate and counts the step.
// LOCAL (rl_ppo_minibatch_local, always with `apply`): it books the rank-local statistics and leaves the KL statistic in `kl_word` - the
// learning rate, the KL sum and the counters are ppo_world_apply_kernel's, after the caller's all-reduce.  LOCAL = false never reads `kl_word`
// (n: rows of the loss means; n_kl: rows of the KL mean - the stored rows under symmetry augmentation)
enum { APPLY_NONE = 0, APPLY_FUSED = 1, APPLY_LOCAL = 2 };
template <bool LOCAL>
__global__ __launch_bounds__(64) void ppo_head_finish_kernel(const double* partials, int nblocks, int n, int n_kl, const float* std, int A, DevState* st,
                                                            int apply, int adaptive, double desired_kl, float* kl_word) {
  __shared__ double sh[3][64];
  for (int q = 0; q < 3; ++q) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 64) s += partials[(size_t)b * 3 + q];
    sh[q][threadIdx.x] = s;
  }
  block_sum<64, 3>(sh[0]);
  if (threadIdx.x != 0 || !apply) return;
  float ent = 0.f;
  for (int k = 0; k < A; ++k) ent += 0.5f + HALF_LOG_2PI + logf(std[k]);
  const float kl = (float)(sh[2][0] / (double)n_kl);
  st->acc[0] += (double)(float)(sh[1][0] / (double)n);
  st->acc[1] += (double)(float)(sh[0][0] / (double)n);
  st->acc[2] += (double)ent;
  if (LOCAL) {
    *kl_word = adaptive ? kl : 0.f;
    return;
  }
  schedule_step(st, adaptive, desired_kl, kl);
}

// the mirror loss's statistic: orders the fourth partials and books L_mirror = sum / count (count = (n_sym - 1) n0 A)
__global__ __launch_bounds__(64) void ppo_mirror_finish_kernel(const double* partials, int nblocks, double count, DevState* st, int apply) {
  __shared__ double sh[64];
  double s = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += 64) s += partials[b];
  sh[threadIdx.x] = s;
  block_sum<64, 1>(sh);
  if (threadIdx.x == 0 && apply) st->mirror_acc += (double)(float)(sh[0] / count);
}

// what ppo_head_finish_kernel does under APPLY_FUSED past the local statistics, on the all-reduced wire word: the KL statistic is the ranks'
// SUM / world in fp32 (dist.py `LearnerGroup.mean`), the rule is schedule_step
__global__ __launch_bounds__(64) void ppo_world_apply_kernel(const float* kl_word, float world, DevState* st, int adaptive, double desired_kl) {
  if (threadIdx.x != 0) return;
  schedule_step(st, adaptive, desired_kl, adaptive ? *kl_word / world : 0.f);
}

__global__ void ppo_set_optimizer_kernel(DevState* st, double lr, long long step) {
  st->lr = lr;
  st->step = step;
}

// ---- optimiser step.  SCALED (rl_ppo_minibatch_apply with a world > 1): g holds the ranks' SUM and every entry is read as g[i] / world, a
// division in fp32 as `flat /= world_size` of the torch learner; SCALED = false never reads `world`
constexpr int NORM_BLOCKS = 256;
template <bool SCALED>
__device__ __forceinline__ float grad_read(const float* g, long i, float world) {
  return SCALED ? g[i] / world : g[i];
}
template <bool SCALED>
__global__ __launch_bounds__(256) void ppo_sumsq_kernel(const float* g, long n, double* partial, float world) {
  __shared__ double sh[256];
  const long per = (n + NORM_BLOCKS - 1) / NORM_BLOCKS, b0 = (long)blockIdx.x * per, b1 = b0 + per < n ? b0 + per : n;
  double s = 0.0;
  for (long i = b0 + threadIdx.x; i < b1; i += 256) {
    const float gi = grad_read<SCALED>(g, i, world);
    s += (double)gi * (double)gi;
  }
  sh[threadIdx.x] = s;
  block_sum<256, 1>(sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}

// clip_grad_norm_ (coef = min(1, max_norm / (norm + 1e-6))) + torch.optim.Adam's step (defaults) + the floor of std (the first n_std entries)
template <bool SCALED>
__global__ __launch_bounds__(256) void ppo_adam_kernel(float* p, const float* g, float* m1, float* m2, long n, int n_std, const double* partial, DevState* st,
                                                      float max_norm, float world) {
  __shared__ double sh[256];
  sh[threadIdx.x] = partial[threadIdx.x];  // NORM_BLOCKS == blockDim.x; every block adds the same numbers in the same order
  block_sum<256, 1>(sh);
  const float norm = (float)sqrt(sh[0]);
  const float coef = fminf(max_norm / (norm + 1e-6f), 1.0f);
  if (blockIdx.x == 0 && threadIdx.x == 0) st->grad_norm = (double)norm;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double step = (double)st->step;
  const double bc1 = 1.0 - pow(0.9, step), bc2 = 1.0 - pow(0.999, step);
  const float step_size = (float)(st->lr / bc1), bc2_sqrt = (float)sqrt(bc2);
  const float gi = grad_read<SCALED>(g, i, world) * coef;
  const float m = m1[i] + 0.1f * (gi - m1[i]);                       // exp_avg.lerp_(grad, 1 - beta1)
  const float v = m2[i] * 0.999f + (float)(1.0 - 0.999) * gi * gi;   // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
  m1[i] = m;
  m2[i] = v;
  const float denom = sqrtf(v) / bc2_sqrt + 1e-8f;
  float w = p[i] - step_size * (m / denom);
  if (i < n_std) w = fmaxf(w, 1e-6f);
  p[i] = w;
}

std::string& err() {
  static thread_local std::string e;
  return e;
}
int fail(const std::string& m) {
  err() = m;
  return -1;
}

struct Net {
  int dims[RL_PPO_MAX_LAYERS + 1] = {};
  long w_off[RL_PPO_MAX_LAYERS] = {}, b_off[RL_PPO_MAX_LAYERS] = {};  // into the flat buffers
  float* h[RL_PPO_MAX_LAYERS + 1] = {};   // h[l], l >= 1: output of layer l - 1 ([rows][dims[l]]); h[n_layers]: the network's output
  float* dz[RL_PPO_MAX_LAYERS + 1] = {};  // dz[l], l >= 1: dL / d(pre-activation of layer l - 1)
  float* part[RL_PPO_MAX_LAYERS] = {};    // dW / db partials of layer l: [S][N K + N]
  int S[RL_PPO_MAX_LAYERS] = {};
};

}  // namespace

struct rl_ppo {
  int device = 0, L = 0, A = 0, max_rows = 0;
  rl_ppo_hyper hp{};
  Net net[2];  // actor, critic
  long n_params = 0;
  float *params = nullptr, *grads = nullptr, *m1 = nullptr, *m2 = nullptr;
  float *dstd_rows = nullptr, *std_part = nullptr;
  int S_std = 1;
  double *head_part = nullptr, *norm_part = nullptr;
  DevState* st = nullptr;
  std::vector<void*> allocs;      // what lives as long as the handle
  std::vector<void*> row_allocs;  // what is sized by the rows of a mini-batch (alloc_rows, at the first mini-batch: n_sym is known by then)
  bool rows_ready = false;
  int n_sym = 0;                  // 0: rl_ppo_set_symmetry was not called
  int* sym[3] = {};               // table words [n_sym][width]: observations, critic observations, actions
  bool started = false;           // a mini-batch was enqueued: the symmetry is fixed from then on
  float mirror = 0.f;             // coefficient of the mirror loss; 0: rl_ppo_set_mirror_loss was not called
  bool augment = true;            // (mirror loss) the PPO terms see every copy; false: the stored rows only
  double* mirror_part = nullptr;  // the head's fourth partials
  bool norm = false;              // rl_ppo_set_obs_normalization was called: the batch holds raw rows, the layer-0 launches are the NORM kernels
  NormProb norm_of[2] = {};       // the caller's statistics of the actor's / the critic's input (a null mean: that group is not normalised)
  int world = 0;                  // ranks whose gradients the caller sums into the wire; 0: rl_ppo_set_world was not called (one rank)
  bool local_pending = false;     // rl_ppo_minibatch_local ran and rl_ppo_minibatch_apply has not yet
};

namespace {

template <class T>
bool dalloc(std::vector<void*>& owner, T** out, size_t count) {
  void* q = nullptr;
  if (hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) return false;
  owner.push_back(q);
  if (hipMemset(q, 0, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) return false;
  *out = (T*)q;
  return true;
}
template <class T>
bool dalloc(rl_ppo* p, T** out, size_t count) {
  return dalloc(p->allocs, out, count);
}

// activations, gradients of the activations and the partial buffers for mini-batches of up to `rows` rows (with symmetry: virtual rows)
bool alloc_rows(rl_ppo* p, size_t rows) {
  const size_t stored = (size_t)p->max_rows;  // what the critic and the std column sum see under a mirror loss without augmentation
  std::vector<void*>& own = p->row_allocs;
  for (void* q : own) (void)hipFree(q);  // (what a failed earlier attempt left)
  own.clear();
  p->rows_ready = false;
  bool ok = true;
  const int s_cap = (int)std::max<size_t>(1, (rows + TK - 1) / TK);  // no chunk shorter than a slice
  for (int k = 0; k < 2 && ok; ++k) {
    Net& N = p->net[k];
    const size_t rows_k = k == 1 && !p->augment ? stored : rows;
    for (int l = 0; l < p->L && ok; ++l) {
      const int Nn = N.dims[l + 1], K = N.dims[l];
      ok = dalloc(own, &N.h[l + 1], rows_k * Nn) && dalloc(own, &N.dz[l + 1], rows_k * Nn);
      const int tiles = tiles_of(Nn) * tiles_of(K);
      N.S[l] = std::max(1, std::min(128 / tiles, s_cap));  // ~128 workgroups per layer and network: 1024 in the one dW launch of the A1 networks
      ok = ok && dalloc(own, &N.part[l], (size_t)N.S[l] * ((size_t)Nn * K + Nn));
    }
  }
  p->S_std = std::max(1, std::min(64, s_cap));
  p->rows_ready = ok && dalloc(own, &p->dstd_rows, rows * p->A) && dalloc(own, &p->std_part, (size_t)p->S_std * p->A) &&
                  dalloc(own, &p->head_part, ((rows + 255) / 256) * 3);
  if (p->rows_ready && p->mirror > 0.f) p->rows_ready = dalloc(own, &p->mirror_part, (rows + 255) / 256);
  return p->rows_ready;
}

// the flat gradient buffer is the WIRE of a multi-rank update: P gradient words, the KL word [P], padded to a multiple of 64 floats
size_t wire_floats(long n_params) { return ((size_t)n_params + 1 + 63) / 64 * 64; }

int check_launch() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(hipGetErrorString(e));
}

int chunk_rows(int n, int S) {  // rows per chunk: a multiple of the GEMM's slice
  const int c = (n + S - 1) / S;
  return std::max(TK, (c + TK - 1) / TK * TK);
}

// the launch dispatcher: a runtime flag names the template side of a kernel, the launch that follows has ONE argument list
template <class K>
K* side(bool flag, K* on, K* off) {
  return flag ? on : off;
}
// the two argument lists of ppo_gemm_kernel (side<GemmK>(...) picks the instantiation with the empty NORM pack)
using GemmK = void(GemmBatch);
using GemmNormK = void(GemmBatch, NormBatch);

// sum of squares -> clip -> Adam -> floor of std on the flat gradient; with a world > 1 on g[i] / world (the wire holds the ranks' SUM)
void optimiser_step(rl_ppo* p, hipStream_t s) {
  const float world = (float)std::max(p->world, 1);
  const bool scaled = p->world > 1;
  hipLaunchKernelGGL(side(scaled, ppo_sumsq_kernel<true>, ppo_sumsq_kernel<false>), dim3(NORM_BLOCKS), dim3(256), 0, s, p->grads, p->n_params, p->norm_part,
                     world);
  hipLaunchKernelGGL(side(scaled, ppo_adam_kernel<true>, ppo_adam_kernel<false>), dim3((unsigned)((p->n_params + 255) / 256)), dim3(256), 0, s, p->params,
                     p->grads, p->m1, p->m2, p->n_params, p->A, p->norm_part, p->st, p->hp.max_grad_norm, world);
}

// fills (a zeroed) `g` with the problem of `mode` for layer l of network k over `rows` rows (see GemmProb): the operands of either network, the
// gather through the n0 indices at `idx` and the symmetry tables where the layer's input is the stored batch, the tile grid
// (net_prob: the same for ONE network of `L` layers whose first layer reads `x0` - what the distillation learner, csrc/learner/rl_distill.inl, shares)
void net_prob(GemmProb& g, const Net& N, const float* params, int L, const float* x0, int mode, int l, int rows) {
  const int K = N.dims[l], Nn = N.dims[l + 1];
  const float* x = l > 0 ? N.h[l] : x0;  // the layer's input [rows][K]
  const float* W = params + N.w_off[l];  // [Nn][K]
  if (mode == G_FWD) {
    g.A = x; g.lda = K; g.B = W; g.ldb = K; g.aux = params + N.b_off[l]; g.C = N.h[l + 1]; g.ldc = Nn;
    g.I = rows; g.J = Nn; g.R = K; g.act = l + 1 < L;
  } else if (mode == G_DX) {
    g.A = N.dz[l + 1]; g.lda = Nn; g.B = W; g.ldb = K; g.aux = N.h[l]; g.ldaux = K; g.C = N.dz[l]; g.ldc = K;
    g.I = rows; g.J = K; g.R = Nn;
  } else {
    g.A = N.dz[l + 1]; g.lda = Nn; g.B = x; g.ldb = K; g.C = N.part[l]; g.ldc = K;
    g.I = Nn; g.J = K; g.R = rows;
    g.S = N.S[l]; g.chunk = chunk_rows(rows, g.S); g.cstride = (long)Nn * K + Nn;
  }
  g.tilesJ = tiles_of(g.J); g.ntiles = tiles_of(g.I) * g.tilesJ;
}
void gemm_prob(GemmProb& g, const rl_ppo* p, const rl_ppo_batch* b, const int64_t* idx, int n0, int mode, int k, int l, int rows) {
  net_prob(g, p->net[k], p->params, p->L, k == 0 ? b->observations : b->privileged_observations, mode, l, rows);
  if (mode != G_DX && l == 0) {
    g.gidx = idx;
    if (p->n_sym > 0) { g.sym = p->sym[k]; g.n0 = n0; }
  }
}

// the launches of one mini-batch (see the head of this file); `apply`: APPLY_NONE (the gradient alone), APPLY_FUSED (statistics, learning rate
// and the optimiser step follow on the device), APPLY_LOCAL (the rank-local statistics and the KL word of the wire; no optimiser step)
int minibatch(rl_ppo* p, const rl_ppo_batch* b, const int64_t* idx, int n0, int apply, hipStream_t s) {
  const int L = p->L;
  const bool sym = p->n_sym > 0;
  const int n = sym ? p->n_sym * n0 : n0;  // the rows every stage past the layer-0 fetch sees
  const bool mirror = p->mirror > 0.f;
  const int n_terms = p->augment ? n : n0;          // rows of the PPO terms, of dstd_rows ...
  const int rows_of[2] = {n, n_terms};              // ... and of the actor's / the critic's problems
  if (!p->rows_ready && !alloc_rows(p, (size_t)(sym ? p->n_sym : 1) * (size_t)p->max_rows))
    return fail("device allocation of the mini-batch buffers failed");  // nothing is launched; a later call tries again
  p->started = true;
  for (int l = 0; l < L; ++l) {
    GemmBatch gb{};
    int tiles = 0;
    for (int k = 0; k < 2; ++k) {
      gemm_prob(gb.p[k], p, b, idx, n0, G_FWD, k, l, rows_of[k]);
      tiles = std::max(tiles, gb.p[k].ntiles);
    }
    if (p->norm && l == 0) {
      NormBatch nb{};
      nb.p[0] = p->norm_of[0]; nb.p[1] = p->norm_of[1];
      hipLaunchKernelGGL(side<GemmNormK>(sym, ppo_gemm_kernel<G_FWD, true>, ppo_gemm_kernel<G_FWD, false>), dim3(tiles, 1, 2), dim3(256), 0, s, gb, nb);
    } else {
      hipLaunchKernelGGL(side<GemmK>(sym && l == 0, ppo_gemm_kernel<G_FWD, true>, ppo_gemm_kernel<G_FWD, false>), dim3(tiles, 1, 2), dim3(256), 0, s, gb);
    }
  }
  {
    HeadArgs a{};
    a.mean = p->net[0].h[L]; a.value = p->net[1].h[L]; a.b = *b; a.idx = idx; a.std = p->params;
    a.dmean = p->net[0].dz[L]; a.dvalue = p->net[1].dz[L]; a.dstd_rows = p->dstd_rows; a.partials = p->head_part;
    a.n = n; a.A = p->A; a.clip = p->hp.clip_param; a.value_loss_coef = p->hp.value_loss_coef; a.entropy_coef = p->hp.entropy_coef;
    a.use_clipped_value_loss = p->hp.use_clipped_value_loss;
    a.asym = p->sym[2]; a.n0 = n0;
    a.n_terms = n_terms; a.mirror_coeff = p->mirror; a.mirror_partials = p->mirror_part;
    const int blocks = (n + 255) / 256;
    hipLaunchKernelGGL(side(mirror, ppo_head_kernel<true, true>, side(sym, ppo_head_kernel<true>, ppo_head_kernel<false>)), dim3(blocks), dim3(256), 0, s, a);
    const int adaptive = p->hp.schedule == RL_PPO_SCHEDULE_ADAPTIVE ? 1 : 0;
    const bool local = apply == APPLY_LOCAL;  // the KL word goes to the wire, behind the gradient
    hipLaunchKernelGGL(side(local, ppo_head_finish_kernel<true>, ppo_head_finish_kernel<false>), dim3(1), dim3(64), 0, s, p->head_part, blocks, n_terms, n0,
                       p->params, p->A, p->st, apply ? 1 : 0, adaptive, p->hp.desired_kl, local ? p->grads + p->n_params : (float*)nullptr);
    if (mirror)
      hipLaunchKernelGGL(ppo_mirror_finish_kernel, dim3(1), dim3(64), 0, s, p->mirror_part, blocks, (double)(p->n_sym - 1) * (double)n0 * (double)p->A, p->st,
                         apply ? 1 : 0);
  }
  for (int l = L - 1; l >= 1; --l) {
    GemmBatch gb{};
    int tiles = 0;
    for (int k = 0; k < 2; ++k) {
      gemm_prob(gb.p[k], p, b, idx, n0, G_DX, k, l, rows_of[k]);
      tiles = std::max(tiles, gb.p[k].ntiles);
    }
    hipLaunchKernelGGL((ppo_gemm_kernel<G_DX, false>), dim3(tiles, 1, 2), dim3(256), 0, s, gb);
  }
  {
    GemmBatch gb{};
    ColBatch cb{};
    RedBatch rb{};
    int tiles = 0, Smax = 1, colx = 1, np = 0;
    long redmax = 1;
    for (int k = 0; k < 2; ++k)
      for (int l = 0; l < L; ++l, ++np) {
        const Net& N = p->net[k];
        const int Nn = N.dims[l + 1], K = N.dims[l];
        GemmProb& g = gb.p[np];
        gemm_prob(g, p, b, idx, n0, G_DW, k, l, rows_of[k]);
        ColProb& c = cb.p[np];
        c.Z = N.dz[l + 1]; c.part = N.part[l]; c.N = Nn; c.M = g.R; c.ld = Nn; c.S = g.S; c.chunk = g.chunk; c.stride = g.cstride; c.off = (long)Nn * K;
        RedProb& r = rb.p[np];
        r.part = N.part[l]; r.out = p->grads + N.w_off[l]; r.count = g.cstride; r.stride = g.cstride; r.S = g.S;  // (b follows W in the flat layout)
        tiles = std::max(tiles, g.ntiles); Smax = std::max(Smax, g.S); colx = std::max(colx, (Nn + 63) / 64); redmax = std::max(redmax, r.count);
      }
    ColProb& c = cb.p[np];
    c.Z = p->dstd_rows; c.part = p->std_part; c.N = p->A; c.M = n_terms; c.ld = p->A; c.S = p->S_std; c.chunk = chunk_rows(n_terms, c.S); c.stride = p->A; c.off = 0;
    RedProb& r = rb.p[np];
    r.part = p->std_part; r.out = p->grads; r.count = p->A; r.stride = p->A; r.S = p->S_std;
    colx = std::max(colx, (p->A + 63) / 64); Smax = std::max(Smax, p->S_std);
    if (p->norm) {
      NormBatch nb{};  // (problem k L + l: the layer-0 problems of the two networks carry the statistics)
      nb.p[0] = p->norm_of[0]; nb.p[L] = p->norm_of[1];
      hipLaunchKernelGGL(side<GemmNormK>(sym, ppo_gemm_kernel<G_DW, true>, ppo_gemm_kernel<G_DW, false>), dim3(tiles, Smax, np), dim3(256), 0, s, gb, nb);
    } else {
      hipLaunchKernelGGL(side<GemmK>(sym, ppo_gemm_kernel<G_DW, true>, ppo_gemm_kernel<G_DW, false>), dim3(tiles, Smax, np), dim3(256), 0, s, gb);
    }
    hipLaunchKernelGGL(ppo_colsum_kernel, dim3(colx, Smax, np + 1), dim3(256), 0, s, cb);
    hipLaunchKernelGGL(ppo_reduce_kernel, dim3((unsigned)std::min<long>((redmax + 255) / 256, 512), np + 1), dim3(256), 0, s, rb);
  }
  if (apply == APPLY_FUSED) optimiser_step(p, s);
  return check_launch();
}

// the guard of the entry points that enqueue mini-batches: arguments, the batch's pointers, `rows` (named `what` in the refusal) per mini-batch, the
// device; last and only with `pending`: that refusal while an rl_ppo_minibatch_local waits for its rl_ppo_minibatch_apply
int enter(rl_ppo* p, const rl_ppo_batch* b, const int64_t* idx, int rows, const char* what, const char* pending) {
  if (!p || !idx) return fail("null argument");
  if (!b || !b->observations || !b->privileged_observations || !b->actions || !b->values || !b->returns || !b->advantages || !b->actions_log_prob ||
      !b->mu || !b->sigma)
    return fail("null batch pointer");
  if (rows < 1 || rows > p->max_rows) return fail(std::string(what) + " outside 1..max_rows_per_minibatch");
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  if (pending && p->local_pending) return fail(pending);
  return 0;
}

// waits for the stream and copies the state block to the host
int read_state(rl_ppo* p, void* stream, DevState* st, const char* what) {
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return fail("stream synchronisation failed");
  if (hipMemcpy(st, p->st, sizeof(*st), hipMemcpyDeviceToHost) != hipSuccess) return fail(std::string(what) + " copy failed");
  return 0;
}

// walks the per-layer images of both networks and std; `to_flat`: user -> flat
int copy_parameters(rl_ppo* p, const float* const* aw, const float* const* ab, const float* const* cw, const float* const* cb, const float* sd, bool to_flat,
                    hipStream_t s) {
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  auto cp = [&](const float* user, long off, size_t count) {
    if (!user) return fail("null layer pointer");
    float* flat = p->params + off;
    const hipError_t e = to_flat ? hipMemcpyAsync(flat, user, count * 4, hipMemcpyDeviceToDevice, s)
                                 : hipMemcpyAsync(const_cast<float*>(user), flat, count * 4, hipMemcpyDeviceToDevice, s);
    return e == hipSuccess ? 0 : fail(hipGetErrorString(e));
  };
  const float* const* W[2] = {aw, cw};
  const float* const* B[2] = {ab, cb};
  for (int k = 0; k < 2; ++k)
    for (int l = 0; l < p->L; ++l) {
      const Net& N = p->net[k];
      if (W[k] && cp(W[k][l], N.w_off[l], (size_t)N.dims[l] * N.dims[l + 1])) return -1;
      if (B[k] && cp(B[k][l], N.b_off[l], (size_t)N.dims[l + 1])) return -1;
    }
  if (sd && cp(sd, 0, (size_t)p->A)) return -1;
  return 0;
}

// the statistics of an update start at zero (stream-ordered: the previous update's are read by rl_ppo_stats before)
int reset_statistics(rl_ppo* p, hipStream_t s) {
  if (hipMemsetAsync(p->st->acc, 0, sizeof(double) * 4, s) != hipSuccess || hipMemsetAsync(&p->st->n_minibatches, 0, sizeof(long long), s) != hipSuccess)
    return fail("cannot reset the statistics block");
  if (p->mirror > 0.f && hipMemsetAsync(&p->st->mirror_acc, 0, sizeof(double), s) != hipSuccess) return fail("cannot reset the statistics block");
  return 0;
}

}  // namespace

extern "C" {

const char* rl_ppo_last_error(void) { return err().c_str(); }

int rl_ppo_destroy(rl_ppo* p) {
  if (!p) return 0;
  (void)hipSetDevice(p->device);
  for (void* q : p->allocs) (void)hipFree(q);
  for (void* q : p->row_allocs) (void)hipFree(q);
  delete p;
  return 0;
}

int rl_ppo_create(const int32_t* actor_dims, const int32_t* critic_dims, int32_t n_layers, int32_t activation, const rl_ppo_hyper* hyper,
                  int32_t max_rows_per_minibatch, int32_t device, rl_ppo** out) {
  if (!actor_dims || !critic_dims || !hyper || !out) return fail("null argument");
  if (n_layers < 1 || n_layers > RL_PPO_MAX_LAYERS) return fail("unsupported layer count " + std::to_string(n_layers) + " (1.." + std::to_string(RL_PPO_MAX_LAYERS) + ")");
  if (activation != RL_PPO_ACT_ELU) return fail("unsupported activation: the HIP learner implements ELU only (use the torch learner of robot_lab_amd/ppo.py)");
  if (hyper->std_type != RL_PPO_STD_SCALAR) return fail("unsupported noise_std_type: the HIP learner implements \"scalar\" only (use the torch learner)");
  for (int l = 0; l <= n_layers; ++l)
    if (actor_dims[l] < 1 || actor_dims[l] > RL_PPO_MAX_WIDTH || critic_dims[l] < 1 || critic_dims[l] > RL_PPO_MAX_WIDTH)
      return fail("unsupported layer width " + std::to_string(std::max(actor_dims[l], critic_dims[l])) + " (1.." + std::to_string(RL_PPO_MAX_WIDTH) + ")");
  if (critic_dims[n_layers] != 1) return fail("the critic's output width must be 1");
  if (max_rows_per_minibatch < 1) return fail("max_rows_per_minibatch must be positive");
  if (hyper->num_learning_epochs < 1 || hyper->num_mini_batches < 1) return fail("num_learning_epochs and num_mini_batches must be positive");
  if (hyper->schedule != RL_PPO_SCHEDULE_FIXED && hyper->schedule != RL_PPO_SCHEDULE_ADAPTIVE) return fail("unknown schedule");
  if (hyper->schedule == RL_PPO_SCHEDULE_ADAPTIVE && !(hyper->desired_kl > 0.0))
    return fail("the adaptive schedule needs desired_kl > 0 (no target: pass RL_PPO_SCHEDULE_FIXED)");
  if (!(hyper->learning_rate > 0.0) || !(hyper->clip_param > 0.f) || !(hyper->max_grad_norm > 0.f)) return fail("learning_rate, clip_param and max_grad_norm must be positive");
  if (hipSetDevice(device) != hipSuccess) return fail("hipSetDevice failed (the HIP learner needs a GPU; there is no CPU path)");
  rl_ppo* p = new rl_ppo();
  p->device = device; p->L = n_layers; p->A = actor_dims[n_layers]; p->max_rows = max_rows_per_minibatch; p->hp = *hyper;
  long off = p->A;  // std first: the order of ActorCritic.parameters()
  for (int k = 0; k < 2; ++k) {
    Net& N = p->net[k];
    const int32_t* d = k == 0 ? actor_dims : critic_dims;
    for (int l = 0; l <= n_layers; ++l) N.dims[l] = d[l];
    for (int l = 0; l < n_layers; ++l) {
      N.w_off[l] = off; off += (long)d[l] * d[l + 1];
      N.b_off[l] = off; off += d[l + 1];
    }
  }
  p->n_params = off;
  bool ok = dalloc(p, &p->params, (size_t)off) && dalloc(p, &p->grads, wire_floats(off)) && dalloc(p, &p->m1, (size_t)off) && dalloc(p, &p->m2, (size_t)off);
  ok = ok && dalloc(p, &p->norm_part, (size_t)NORM_BLOCKS) && dalloc(p, &p->st, 1);
  if (ok) {
    std::vector<float> ones((size_t)p->A, 1.0f);
    DevState st{};
    st.lr = hyper->learning_rate;
    ok = hipMemcpy(p->params, ones.data(), ones.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(p->st, &st, sizeof(st), hipMemcpyHostToDevice) == hipSuccess;
  }
  if (!ok) {
    rl_ppo_destroy(p);
    return fail("device allocation failed");
  }
  *out = p;
  return 0;
}

int64_t rl_ppo_num_parameters(const rl_ppo* p) { return p ? p->n_params : 0; }

int rl_ppo_set_symmetry(rl_ppo* p, int32_t n_sym, const int32_t* obs_perm, const float* obs_sign, const int32_t* critic_perm, const float* critic_sign,
                        const int32_t* act_perm, const float* act_sign) {
  if (!p) return fail("null argument");
  if (p->n_sym) return fail("rl_ppo_set_symmetry: the symmetry of this learner is already set (it is set once, before the first mini-batch)");
  if (p->started)
    return fail("rl_ppo_set_symmetry: refused after the first rl_ppo_minibatch_grad / rl_ppo_update - the buffers of the handle are sized by the "
                "number of copies at the first mini-batch; create a new learner");
  if (n_sym < 1 || n_sym > RL_PPO_MAX_SYM) return fail("rl_ppo_set_symmetry: n_sym " + std::to_string(n_sym) + " outside 1.." + std::to_string(RL_PPO_MAX_SYM));
  if (!obs_perm || !obs_sign || !act_perm || !act_sign) return fail("rl_ppo_set_symmetry: the observation and action tables are required");
  if ((critic_perm == nullptr) != (critic_sign == nullptr)) return fail("rl_ppo_set_symmetry: critic_perm and critic_sign are both given or both null");
  if ((long long)n_sym * p->max_rows > 0x7fffffffLL) return fail("rl_ppo_set_symmetry: n_sym x max_rows_per_minibatch does not fit 32 bits");
  const char* names[3] = {"obs", "critic", "act"};
  const int32_t* perm[3] = {obs_perm, critic_perm, act_perm};
  const float* sign[3] = {obs_sign, critic_sign, act_sign};
  const int width[3] = {p->net[0].dims[0], p->net[1].dims[0], p->A};
  std::vector<int> words[3];
  for (int t = 0; t < 3; ++t) {  // everything is checked before the device is touched: the words index device memory
    const int W = width[t];
    words[t].resize((size_t)n_sym * W);
    std::vector<char> seen((size_t)W);
    for (int s = 0; s < n_sym; ++s) {
      std::fill(seen.begin(), seen.end(), 0);
      for (int c = 0; c < W; ++c) {
        const std::string at = std::string(names[t]) + " table, copy " + std::to_string(s) + ", column " + std::to_string(c);
        if (!perm[t]) {  // "replicated": the identity for every copy
          words[t][(size_t)s * W + c] = c;
          continue;
        }
        const int src = perm[t][(size_t)s * W + c];
        const float sg = sign[t][(size_t)s * W + c];
        if (src < 0 || src >= W) return fail("rl_ppo_set_symmetry: " + at + ": source column " + std::to_string(src) + " outside 0.." + std::to_string(W - 1));
        if (seen[src]) return fail("rl_ppo_set_symmetry: " + at + ": source column " + std::to_string(src) + " is used twice (not a bijection)");
        seen[src] = 1;
        if (!(sg == 1.0f || sg == -1.0f)) return fail("rl_ppo_set_symmetry: " + at + ": sign " + std::to_string(sg) + " is not +1 or -1");
        if (s == 0 && (src != c || sg != 1.0f)) return fail("rl_ppo_set_symmetry: " + at + ": copy 0 must be the identity");
        words[t][(size_t)s * W + c] = src | (sg < 0.f ? SYM_NEG : 0);
      }
    }
  }
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  bool ok = true;
  for (int t = 0; t < 3 && ok; ++t)
    ok = dalloc(p, &p->sym[t], words[t].size()) && hipMemcpy(p->sym[t], words[t].data(), words[t].size() * sizeof(int), hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) return fail("rl_ppo_set_symmetry: device allocation of the tables failed (no symmetry is set: the handle is as it was)");
  p->n_sym = n_sym;  // (the mini-batch buffers are allocated at the first mini-batch, for n_sym x max_rows_per_minibatch rows)
  return 0;
}

int rl_ppo_set_mirror_loss(rl_ppo* p, float coeff, int32_t data_augmentation) {
  if (!p) return fail("null argument");
  if (p->mirror > 0.f) return fail("rl_ppo_set_mirror_loss: the mirror loss of this learner is already set (it is set once, before the first mini-batch)");
  if (p->started)
    return fail("rl_ppo_set_mirror_loss: refused after the first rl_ppo_minibatch_grad / rl_ppo_update - the buffers of the handle are sized at the "
                "first mini-batch; create a new learner");
  if (!p->n_sym) return fail("rl_ppo_set_mirror_loss: no symmetry is set (rl_ppo_set_symmetry comes first: its tables say what the mirrored action is)");
  if (p->n_sym < 2) return fail("rl_ppo_set_mirror_loss: the symmetry of this learner has n_sym = 1 (the identity alone): there is no mirrored copy");
  if (!std::isfinite(coeff) || !(coeff > 0.f)) return fail("rl_ppo_set_mirror_loss: the coefficient must be finite and > 0, got " + std::to_string(coeff));
  p->mirror = coeff;  // (no device work: the fourth partials are allocated with the other mini-batch buffers)
  p->augment = data_augmentation != 0;
  return 0;
}

int rl_ppo_set_obs_normalization(rl_ppo* p, const float* actor_mean_dev, const float* actor_std_dev, float actor_eps, const float* critic_mean_dev,
                                 const float* critic_std_dev, float critic_eps) {
  if (!p) return fail("null argument");
  if (p->norm)
    return fail("rl_ppo_set_obs_normalization: the observation normalisation of this learner is already set (it is set once, before the first mini-batch)");
  if (p->started)
    return fail("rl_ppo_set_obs_normalization: refused after the first rl_ppo_minibatch_grad / rl_ppo_update - the mini-batches before it read the "
                "batch unnormalised; create a new learner");
  const char* names[2] = {"actor", "critic"};
  const float* mean[2] = {actor_mean_dev, critic_mean_dev};
  const float* sd[2] = {actor_std_dev, critic_std_dev};
  const float eps[2] = {actor_eps, critic_eps};
  if (!mean[0] && !sd[0] && !mean[1] && !sd[1])
    return fail("rl_ppo_set_obs_normalization: both groups are null - a learner without normalisation is one on which this is not called");
  for (int k = 0; k < 2; ++k) {
    if ((mean[k] == nullptr) != (sd[k] == nullptr))
      return fail(std::string("rl_ppo_set_obs_normalization: ") + names[k] + " mean and std are both given or both null");
    if (mean[k] && (!std::isfinite(eps[k]) || !(eps[k] >= 0.f)))
      return fail(std::string("rl_ppo_set_obs_normalization: the ") + names[k] + " eps must be finite and >= 0, got " + std::to_string(eps[k]));
  }
  for (int k = 0; k < 2; ++k) p->norm_of[k] = NormProb{mean[k], sd[k], mean[k] ? eps[k] : 0.f};  // (no device work: the kernels read the vectors at launch time)
  p->norm = true;
  return 0;
}

int rl_ppo_set_parameters(rl_ppo* p, const float* const* actor_w_dev, const float* const* actor_b_dev, const float* const* critic_w_dev,
                          const float* const* critic_b_dev, const float* std_dev, void* stream) {
  if (!p) return fail("null argument");
  return copy_parameters(p, actor_w_dev, actor_b_dev, critic_w_dev, critic_b_dev, std_dev, true, (hipStream_t)stream);
}

int rl_ppo_get_parameters(rl_ppo* p, float* const* actor_w_dev, float* const* actor_b_dev, float* const* critic_w_dev, float* const* critic_b_dev,
                          float* std_dev, void* stream) {
  if (!p) return fail("null argument");
  return copy_parameters(p, actor_w_dev, actor_b_dev, critic_w_dev, critic_b_dev, std_dev, false, (hipStream_t)stream);
}

int rl_ppo_parameter_pointers(rl_ppo* p, const float** actor_w_dev, const float** actor_b_dev, const float** critic_w_dev, const float** critic_b_dev,
                              const float** std_dev) {
  if (!p) return fail("null argument");
  const float** W[2] = {actor_w_dev, critic_w_dev};
  const float** B[2] = {actor_b_dev, critic_b_dev};
  for (int k = 0; k < 2; ++k)
    for (int l = 0; l < p->L; ++l) {
      if (W[k]) W[k][l] = p->params + p->net[k].w_off[l];
      if (B[k]) B[k][l] = p->params + p->net[k].b_off[l];
    }
  if (std_dev) *std_dev = p->params;
  return 0;
}

int rl_ppo_get_flat(rl_ppo* p, int32_t which, float* dst_dev, void* stream) {
  if (!p || !dst_dev) return fail("null argument");
  if (which < 0 || which > 3) return fail("rl_ppo_get_flat: which must be 0..3");
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  const float* src[4] = {p->params, p->grads, p->m1, p->m2};
  const hipError_t e = hipMemcpyAsync(dst_dev, src[which], (size_t)p->n_params * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail(hipGetErrorString(e));
}

int rl_ppo_minibatch_grad(rl_ppo* p, const rl_ppo_batch* batch, const int64_t* idx_dev, int32_t n_idx, void* stream) {
  if (enter(p, batch, idx_dev, n_idx, "n_idx", nullptr)) return -1;
  return minibatch(p, batch, idx_dev, n_idx, APPLY_NONE, (hipStream_t)stream);
}

int rl_ppo_update(rl_ppo* p, const rl_ppo_batch* batch, const int64_t* perm_dev, int32_t n_rows, void* stream) {
  const int mb = p ? n_rows / p->hp.num_mini_batches : 0;
  if (enter(p, batch, perm_dev, mb, "rows per mini-batch", "rl_ppo_update: an rl_ppo_minibatch_local waits for its rl_ppo_minibatch_apply")) return -1;
  hipStream_t s = (hipStream_t)stream;
  if (reset_statistics(p, s)) return -1;
  for (int e = 0; e < p->hp.num_learning_epochs; ++e)
    for (int i = 0; i < p->hp.num_mini_batches; ++i)
      if (minibatch(p, batch, perm_dev + (size_t)i * mb, mb, APPLY_FUSED, s)) return -1;
  return 0;
}

int rl_ppo_set_world(rl_ppo* p, int32_t world_size) {
  if (!p) return fail("null argument");
  if (world_size < 1) return fail("rl_ppo_set_world: world_size " + std::to_string(world_size) + " must be >= 1");
  if (p->world) return fail("rl_ppo_set_world: the world of this learner is already set (it is set once, before the first mini-batch)");
  if (p->started) return fail("rl_ppo_set_world: refused after the first mini-batch - the replicas of a world start together; create a new learner");
  p->world = world_size;  // (no device work: the wire is the gradient buffer, the divisor a kernel argument)
  return 0;
}

int rl_ppo_wire(rl_ppo* p, float** dev, int64_t* count) {
  if (!p || !dev || !count) return fail("null argument");
  *dev = p->grads;
  *count = p->n_params + 1;
  return 0;
}

int rl_ppo_update_begin(rl_ppo* p, void* stream) {
  if (!p) return fail("null argument");
  if (p->local_pending) return fail("rl_ppo_update_begin: an rl_ppo_minibatch_local waits for its rl_ppo_minibatch_apply");
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  return reset_statistics(p, (hipStream_t)stream);
}

int rl_ppo_minibatch_local(rl_ppo* p, const rl_ppo_batch* batch, const int64_t* idx_dev, int32_t n_idx, void* stream) {
  if (enter(p, batch, idx_dev, n_idx, "n_idx", "rl_ppo_minibatch_local: the previous mini-batch waits for its rl_ppo_minibatch_apply")) return -1;
  if (minibatch(p, batch, idx_dev, n_idx, APPLY_LOCAL, (hipStream_t)stream)) return -1;
  p->local_pending = true;
  return 0;
}

int rl_ppo_minibatch_apply(rl_ppo* p, void* stream) {
  if (!p) return fail("null argument");
  if (!p->local_pending) return fail("rl_ppo_minibatch_apply: no rl_ppo_minibatch_local precedes it (the wire holds no gradient of this mini-batch)");
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ppo_world_apply_kernel, dim3(1), dim3(64), 0, s, p->grads + p->n_params, (float)std::max(p->world, 1), p->st,
                     p->hp.schedule == RL_PPO_SCHEDULE_ADAPTIVE ? 1 : 0, p->hp.desired_kl);
  optimiser_step(p, s);
  p->local_pending = false;
  return check_launch();
}

int rl_ppo_set_flat(rl_ppo* p, int32_t which, const float* src_dev, void* stream) {
  if (!p || !src_dev) return fail("null argument");
  if (which != 2 && which != 3) return fail("rl_ppo_set_flat: which must be 2 or 3 (the Adam moments; parameters go through rl_ppo_set_parameters)");
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  const hipError_t e = hipMemcpyAsync(which == 2 ? p->m1 : p->m2, src_dev, (size_t)p->n_params * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail(hipGetErrorString(e));
}

int rl_ppo_get_optimizer(rl_ppo* p, double* lr, int64_t* step, void* stream) {
  if (!p || !lr || !step) return fail("null argument");
  DevState st{};
  if (read_state(p, stream, &st, "optimiser state")) return -1;
  *lr = st.lr;
  *step = (int64_t)st.step;
  return 0;
}

int rl_ppo_set_optimizer(rl_ppo* p, double lr, int64_t step, void* stream) {
  if (!p) return fail("null argument");
  if (!std::isfinite(lr) || !(lr > 0.0)) return fail("rl_ppo_set_optimizer: the learning rate must be finite and > 0");
  if (step < 0) return fail("rl_ppo_set_optimizer: the step counter must be >= 0");
  if (hipSetDevice(p->device) != hipSuccess) return fail("hipSetDevice failed");
  hipLaunchKernelGGL(ppo_set_optimizer_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, p->st, lr, (long long)step);
  return check_launch();
}

namespace {
int read_stats(rl_ppo* p, double* out, int n_out, void* stream) {
  DevState st{};
  if (read_state(p, stream, &st, "statistics")) return -1;
  const double n = st.n_minibatches > 0 ? (double)st.n_minibatches : 1.0;
  out[0] = st.acc[0] / n; out[1] = st.acc[1] / n; out[2] = st.acc[2] / n; out[3] = st.acc[3] / n;
  out[4] = st.lr; out[5] = st.grad_norm; out[6] = (double)st.n_minibatches; out[7] = (double)st.step;
  if (n_out > 8) out[8] = st.mirror_acc / n;
  return 0;
}
}  // namespace

int rl_ppo_stats(rl_ppo* p, double* out, void* stream) {
  if (!p || !out) return fail("null argument");
  return read_stats(p, out, 8, stream);
}

int rl_ppo_stats_ex(rl_ppo* p, double* out, int32_t n_out, void* stream) {
  if (!p || !out) return fail("null argument");
  if (n_out != RL_PPO_STATS_EX) return fail("rl_ppo_stats_ex: n_out must be " + std::to_string(RL_PPO_STATS_EX));
  return read_stats(p, out, n_out, stream);
}

}  // extern "C"

// the distillation learner (include/rl_distill.h): the same translation unit, so that it launches THESE kernels - nothing is instantiated twice
#include "learner/rl_distill.inl"

// the recurrent PPO learner (include/rl_bptt.h): the same translation unit again; the step kernels of back-propagation through time are its own
#include "learner/rl_bptt.inl"

// the recurrent distillation learner (include/rl_distill_bptt.h): behind both, since it launches the distillation learner's head and the recurrent
// learner's step kernels
#include "learner/rl_distill_bptt.inl"

// the update of random network distillation (include/rl_rnd_learner.h): a new sequence of the kernels above and of the distillation learner's head
#include "learner/rl_rnd.inl"
