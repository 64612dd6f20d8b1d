// rl_lstm.hip - one step of a single-layer LSTM over all envs for gfx950 (MI355X): the memory in front of the actor's and the
// critic's MLP of a recurrent policy (RslRlRNNModelCfg(rnn_type="lstm", rnn_hidden_dim=256)), inside the captured collection loop.
// C-ABI: include/rl_lstm.h.
//
// Mapping: a workgroup (8 wavefronts) owns 32 rows (two 16-row tiles).  The rows' operand [x | h~] (h~: the state after the row's
// reset) sits in LDS in the fragment-major order of rl_policy.hip; the contraction over K = in_dim + hidden runs on the matrix cores
// in exact fp32 (v_mfma_f32_16x16x4_f32: D[16x16] += A[16x4] B[4x16], a k-ordered fmaf chain).  A wavefront owns 16 HIDDEN UNITS at a
// time and accumulates their four gates side by side (4 gates x 2 row tiles = 8 independent accumulators), so the gate epilogue
// (sigmoid, tanh, the new c and h, the state record) runs on the accumulator registers: z never leaves the wavefront unless
// gates_out asks for it.  The weights are pre-arranged as [k block][hidden tile][gate][lane][4 k-steps]: one global_load_dwordx4
// per gate and k block, reused for both row tiles.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/rl_lstm.h"

namespace {

constexpr int MT = 16;     // rows of an MFMA tile
constexpr int RT = 2;      // row tiles per workgroup
constexpr int WAVES = 8;   // wavefronts per workgroup
constexpr int KSTEP = 16;  // k block: four k-steps of the 16x16x4 MFMA per ds_read_b128 / global_load_dwordx4

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct LstmCell {
  const float* W;     // fragment-major image [KBx + KBh][HT][4 gates][64 lanes][4 k-steps]
  const float* bias;  // [4 gates][16 HT]: b_ih + b_hh, zero in the padding
  int D, H;           // input width, hidden width
  int KBx, KBh, HT;   // 16-deep k blocks of x and of h, 16-wide tiles of hidden units
};

struct LstmArgs {
  LstmCell cell;
  const float *x, *h, *c;
  float *h_saved, *c_saved, *h_out, *c_out, *gates;
};

// LDS operand tile, "fragment-major" (rl_policy.hip lds_index): lane (row = lane & 15, ak = lane >> 4) reads the four k-steps of a
// 16-deep k block (k = 16 kb + 4 s + ak) as one aligned ds_read_b128
__device__ inline int lds_index(int row, int k) { return ((((k >> 4) * 4 + (k & 3)) * 16 + row) << 2) + ((k >> 2) & 3); }

// 1 / (1 + e^-v): e^-v overflows to +inf for v < -88.7 and the quotient is then exactly 0; it underflows to 0 for v > 103 and the
// quotient is exactly 1.  No (e^v) / (1 + e^v) form: that one is inf / inf.
__device__ inline float sigmoidf_(float v) { return 1.0f / (1.0f + expf(-v)); }

__global__ __launch_bounds__(64 * WAVES) void lstm_step_kernel(LstmArgs qa, LstmArgs qb, const uint8_t* __restrict__ reset, int n_rows, int pair) {
  extern __shared__ float4 smem4[];  // RT tiles of [16 rows][16 (KBx + KBh)] floats
  float* tile = reinterpret_cast<float*>(smem4);
  const bool second = pair && (blockIdx.x & 1);
  const int rowtile = pair ? blockIdx.x >> 1 : blockIdx.x;
  // (field by field: a select between the two argument blocks as a whole would copy one into private memory)
  const int D = second ? qb.cell.D : qa.cell.D, H = second ? qb.cell.H : qa.cell.H, KBx = second ? qb.cell.KBx : qa.cell.KBx;
  const int KB = KBx + (second ? qb.cell.KBh : qa.cell.KBh), HT = second ? qb.cell.HT : qa.cell.HT;
  const float* __restrict__ W = second ? qb.cell.W : qa.cell.W;
  const float* __restrict__ bias = second ? qb.cell.bias : qa.cell.bias;
  const float* __restrict__ x = second ? qb.x : qa.x;
  const float* __restrict__ h = second ? qb.h : qa.h;
  const float* __restrict__ c = second ? qb.c : qa.c;
  float* __restrict__ h_saved = second ? qb.h_saved : qa.h_saved;
  float* __restrict__ c_saved = second ? qb.c_saved : qa.c_saved;
  float* __restrict__ h_out = second ? qb.h_out : qa.h_out;
  float* __restrict__ c_out = second ? qb.c_out : qa.c_out;
  float* __restrict__ gates = second ? qb.gates : qa.gates;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row0 = rowtile * (RT * MT);
  const int KX = KBx * KSTEP, KT = KB * KSTEP;
  // [x | h~] of the workgroup's rows -> LDS (zero fill of the k padding and of rows past the end); the state record of h on the way
  for (int r = wave; r < RT * MT; r += WAVES) {
    const int row = row0 + r;
    const bool live = row < n_rows;
    const bool rs = live && reset != nullptr && reset[row] != 0;
    float* __restrict__ dst = tile + (r >> 4) * (MT * KT);
    for (int k = lane; k < KT; k += 64) {
      float v = 0.f;
      if (k < KX) {
        if (live && k < D) v = x[(size_t)row * D + k];
      } else {
        const int j = k - KX;
        if (live && j < H) {
          const float old = h[(size_t)row * H + j];
          v = rs ? 0.f : old;
          if (h_saved) h_saved[(size_t)row * H + j] = v;
        }
      }
      dst[lds_index(r & 15, k)] = v;
    }
  }
  __syncthreads();
  typedef const f32x4 __attribute__((address_space(1))) * GlobalV4;
  const f32x4* xa = reinterpret_cast<const f32x4*>(tile) + lane;  // + kb * 64 + rt * (4 KT)
  const int col = lane & 15, rbase = (lane >> 4) * 4;
  for (int ht = wave; ht < HT; ht += WAVES) {  // (wavefront-uniform)
    f32x4 acc[RT][4];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[rt][g] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto load_b = [&](int kb, f32x4 (&b)[4]) {
      const int kc = kb < KB ? kb : KB - 1;  // clamped: the tail re-reads the last block instead of branching
      const float* base = W + ((size_t)(kc * HT + ht) * 4) * 256 + lane * 4;
#pragma unroll
      for (int g = 0; g < 4; ++g) b[g] = *(GlobalV4)(uintptr_t)(base + g * 256);
    };
    f32x4 b[4], bn[4];
    load_b(0, bn);
    for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
      for (int g = 0; g < 4; ++g) b[g] = bn[g];
      load_b(kb + 1, bn);  // the next block's weights are in flight under this block's MFMAs
      f32x4 a[RT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) a[rt] = xa[kb * 64 + rt * (4 * KT)];
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) acc[rt][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rt][s], b[g][s], acc[rt][g], 0, 0, 0);
    }
    // epilogue: D[row = (lane >> 4) * 4 + reg][unit = lane & 15] of every gate -> the cell update of (row, unit)
    const int j = ht * MT + col;
    if (j < H) {
      float bg[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) bg[g] = bias[g * (HT * MT) + j];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = row0 + rt * MT + rbase + r;
          if (row >= n_rows) continue;
          const float zi = acc[rt][0][r] + bg[0], zf = acc[rt][1][r] + bg[1], zg = acc[rt][2][r] + bg[2], zo = acc[rt][3][r] + bg[3];
          const bool rs = reset != nullptr && reset[row] != 0;
          const size_t o = (size_t)row * H + j;
          const float cold = c[o];
          const float ct = rs ? 0.f : cold;
          const float cn = sigmoidf_(zf) * ct + sigmoidf_(zi) * tanhf(zg);
          const float hn = sigmoidf_(zo) * tanhf(cn);
          if (c_saved) c_saved[o] = ct;
          c_out[o] = cn;
          h_out[o] = hn;
          if (gates) {
            float* __restrict__ gz = gates + (size_t)row * (4 * H) + j;
            gz[0] = zi; gz[H] = zf; gz[2 * H] = zg; gz[3 * H] = zo;
          }
        }
    }
  }
}

// nn.LSTM's four tensors (DEVICE copies) -> the two images the step kernel reads; every element of both images is written by the thread
// that owns its index, padding included
__global__ __launch_bounds__(256) void lstm_repack_kernel(const float* __restrict__ w_ih, const float* __restrict__ w_hh, const float* __restrict__ b_ih,
                                                          const float* __restrict__ b_hh, int D, int H, int KBx, int KBh, int HT, float* __restrict__ Wf,
                                                          float* __restrict__ bp) {
  const size_t nf = (size_t)(KBx + KBh) * HT * 4 * 256, nb = (size_t)4 * HT * MT;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < nf + nb; e += (size_t)gridDim.x * 256) {
    if (e < nf) {
      const int s = (int)(e & 3), ln = (int)((e >> 2) & 63), g = (int)((e >> 8) & 3), ht = (int)((e >> 10) % HT), kb = (int)((e >> 10) / HT);
      const int n = ht * MT + (ln & 15);
      float v = 0.f;
      if (n < H) {
        if (kb < KBx) {
          const int k = kb * KSTEP + 4 * s + (ln >> 4);
          if (k < D) v = w_ih[(size_t)(g * H + n) * D + k];
        } else {
          const int k = (kb - KBx) * KSTEP + 4 * s + (ln >> 4);
          if (k < H) v = w_hh[(size_t)(g * H + n) * H + k];
        }
      }
      Wf[e] = v;
    } else {
      const int q = (int)(e - nf), g = q / (HT * MT), n = q % (HT * MT);
      bp[q] = n < H ? b_ih[g * H + n] + b_hh[g * H + n] : 0.f;
    }
  }
}

std::string& err() {
  static thread_local std::string e;
  return e;
}
int fail(const std::string& m) {
  err() = m;
  return -1;
}

}  // namespace

struct rl_lstm {
  LstmCell cell;
  int device = 0;
  std::vector<void*> allocs;
};

namespace {

size_t lds_bytes(const rl_lstm* l) { return (size_t)RT * MT * (l->cell.KBx + l->cell.KBh) * KSTEP * sizeof(float); }

int repack(rl_lstm* l, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, hipStream_t stream) {
  const LstmCell& q = l->cell;
  const size_t total = (size_t)(q.KBx + q.KBh) * q.HT * 4 * 256 + (size_t)4 * q.HT * MT;
  hipLaunchKernelGGL(lstm_repack_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 1024)), dim3(256), 0, stream, w_ih, w_hh, b_ih, b_hh, q.D, q.H,
                     q.KBx, q.KBh, q.HT, const_cast<float*>(q.W), const_cast<float*>(q.bias));
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(hipGetErrorString(e));
}

bool overlap(const float* p, const float* q, size_t n) { return p && q && p < q + n && q < p + n; }

int check_args(const char* who, const rl_lstm* l, const LstmArgs& a, int n_rows) {
  if (!a.x || !a.h || !a.c || !a.h_out || !a.c_out) return fail(std::string(who) + ": null x / h / c / h_out / c_out");
  const size_t n = (size_t)n_rows * l->cell.H;
  const float* ins[2] = {a.h, a.c};
  const float* outs[4] = {a.h_out, a.c_out, a.h_saved, a.c_saved};
  for (const float* i : ins)
    for (const float* o : outs)
      if (overlap(i, o, n)) return fail(std::string(who) + ": an output aliases the input state h / c (a workgroup reads rows while another writes them): ping-pong two buffers");
  return 0;
}

int launch(rl_lstm* a, const LstmArgs& qa, rl_lstm* b, const LstmArgs& qb, const uint8_t* reset, int n_rows, void* stream) {
  if (hipSetDevice(a->device) != hipSuccess) return fail("hipSetDevice failed");
  const size_t lds = std::max(lds_bytes(a), b ? lds_bytes(b) : (size_t)0);
  static size_t configured[64] = {};  // the LDS opt-in belongs to the (kernel, device) pair
  if (lds > 64 * 1024 && lds > configured[a->device & 63]) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&lstm_step_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return fail("cannot reserve the LDS of the LSTM step kernel");
    configured[a->device & 63] = lds;
  }
  const int tiles = (n_rows + RT * MT - 1) / (RT * MT);
  hipLaunchKernelGGL(lstm_step_kernel, dim3(b ? 2 * tiles : tiles), dim3(64 * WAVES), lds, (hipStream_t)stream, qa, qb, reset, n_rows, b ? 1 : 0);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(hipGetErrorString(e));
}

}  // namespace

extern "C" {

int rl_lstm_create(int32_t in_dim, int32_t hidden, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int32_t device,
                   rl_lstm** out) {
  if (!w_ih || !w_hh || !b_ih || !b_hh || !out) return fail("null argument");
  if (in_dim < 1 || in_dim > RL_LSTM_MAX_WIDTH || hidden < 1 || hidden > RL_LSTM_MAX_WIDTH)
    return fail("in_dim / hidden out of range (1.." + std::to_string(RL_LSTM_MAX_WIDTH) + ")");
  if (hipSetDevice(device) != hipSuccess) return fail("hipSetDevice failed");
  rl_lstm* l = new rl_lstm();
  l->device = device;
  LstmCell& q = l->cell;
  q.D = in_dim; q.H = hidden;
  q.KBx = (in_dim + KSTEP - 1) / KSTEP; q.KBh = (hidden + KSTEP - 1) / KSTEP; q.HT = (hidden + MT - 1) / MT;
  const size_t nw = (size_t)(q.KBx + q.KBh) * q.HT * 4 * 256, nb = (size_t)4 * q.HT * MT;
  const size_t n_in[4] = {(size_t)4 * hidden * in_dim, (size_t)4 * hidden * hidden, (size_t)4 * hidden, (size_t)4 * hidden};
  const float* host[4] = {w_ih, w_hh, b_ih, b_hh};
  void *dW = nullptr, *db = nullptr, *tmp[4] = {};
  bool ok = hipMalloc(&dW, nw * 4) == hipSuccess && hipMalloc(&db, nb * 4) == hipSuccess;
  if (ok) { l->allocs.push_back(dW); l->allocs.push_back(db); }
  q.W = (const float*)dW; q.bias = (const float*)db;
  // the host tensors go through the device re-layout of rl_lstm_set_weights_device: one definition of the images
  for (int i = 0; ok && i < 4; ++i) ok = hipMalloc(&tmp[i], n_in[i] * 4) == hipSuccess && hipMemcpy(tmp[i], host[i], n_in[i] * 4, hipMemcpyHostToDevice) == hipSuccess;
  int rc = ok ? repack(l, (const float*)tmp[0], (const float*)tmp[1], (const float*)tmp[2], (const float*)tmp[3], nullptr) : fail("device allocation / upload failed");
  if (rc == 0 && hipStreamSynchronize(nullptr) != hipSuccess) rc = fail("the weight re-layout failed");
  for (void* p : tmp)
    if (p) (void)hipFree(p);
  if (rc != 0) {
    rl_lstm_destroy(l);
    return -1;
  }
  *out = l;
  return 0;
}

int rl_lstm_set_weights_device(rl_lstm* l, const float* w_ih_dev, const float* w_hh_dev, const float* b_ih_dev, const float* b_hh_dev, void* stream) {
  if (!l || !w_ih_dev || !w_hh_dev || !b_ih_dev || !b_hh_dev) return fail("null argument");
  if (hipSetDevice(l->device) != hipSuccess) return fail("hipSetDevice failed");
  return repack(l, w_ih_dev, w_hh_dev, b_ih_dev, b_hh_dev, (hipStream_t)stream);
}

int rl_lstm_step(rl_lstm* l, const float* x, const uint8_t* reset_u8, const float* h, const float* c, float* h_saved, float* c_saved, float* h_out,
                 float* c_out, float* gates_out, int32_t n_rows, void* stream) {
  if (!l) return fail("null argument");
  if (n_rows < 0) return fail("n_rows < 0");
  LstmArgs q{l->cell, x, h, c, h_saved, c_saved, h_out, c_out, gates_out};
  if (check_args("rl_lstm_step", l, q, n_rows)) return -1;
  if (n_rows == 0) return 0;
  return launch(l, q, nullptr, q, reset_u8, n_rows, stream);
}

int rl_lstm_step_pair(rl_lstm* a, const float* xa, const float* ha, const float* ca, float* ha_saved, float* ca_saved, float* ha_out, float* ca_out,
                      float* gates_a_out, rl_lstm* b, const float* xb, const float* hb, const float* cb, float* hb_saved, float* cb_saved, float* hb_out,
                      float* cb_out, float* gates_b_out, const uint8_t* reset_u8, int32_t n_rows, void* stream) {
  if (!a || !b) return fail("null argument");
  if (a->device != b->device) return fail("rl_lstm_step_pair: the two cells live on different devices");
  if (n_rows < 0) return fail("n_rows < 0");
  LstmArgs qa{a->cell, xa, ha, ca, ha_saved, ca_saved, ha_out, ca_out, gates_a_out};
  LstmArgs qb{b->cell, xb, hb, cb, hb_saved, cb_saved, hb_out, cb_out, gates_b_out};
  if (check_args("rl_lstm_step_pair", a, qa, n_rows) || check_args("rl_lstm_step_pair", b, qb, n_rows)) return -1;
  if (n_rows == 0) return 0;
  return launch(a, qa, b, qb, reset_u8, n_rows, stream);
}

int32_t rl_lstm_in_dim(const rl_lstm* l) { return l ? l->cell.D : -1; }
int32_t rl_lstm_hidden(const rl_lstm* l) { return l ? l->cell.H : -1; }

int rl_lstm_destroy(rl_lstm* l) {
  if (!l) return 0;
  (void)hipSetDevice(l->device);
  for (void* p : l->allocs) (void)hipFree(p);
  delete l;
  return 0;
}

const char* rl_lstm_last_error(void) { return err().c_str(); }

}  // extern "C"
