// rl_obsnorm.hip - empirical observation normalisation for gfx950 (MI355X): running column statistics of an observation group and
// y = (x - mean) / (std + eps).  C-ABI and the rule: include/rl_obsnorm.h (the definition is robot_lab_amd.ppo.EmpiricalNormalization).
//
//   update   grid (tiles of 64 rows, chunks of 64 columns, handles): a workgroup is 64 column lanes x 4 row groups, so that a wavefront
//            reads 64 consecutive floats of a row.  Two passes over the 16 values a thread keeps in registers, accumulated in fp64: the
//            tile's column sum -> mean, then sum (x - mean)^2 = M2 (never sum x^2 - (sum x)^2).  One (sum, mean, M2) per column and tile goes to the handle's
//            scratch; the workgroup that draws the last ticket combines all tiles in tile order (Chan et al.) in fp64 and applies the rule to the fp32 state.
//            (64-row tiles: 20.4 us for the A1 pair - 45 + 235 columns - at 4096 rows, 256-row tiles 27.3 us: profiles/obs_normalization.txt)
//   apply    a flat grid-stride stream.
// Built with -ffp-contract=off: apply's subtract / add / divide are three separate fp32 roundings, as in torch and numpy.
#include <hip/hip_runtime.h>

#include <math.h>
#include <cmath>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <vector>

#include "../../include/rl_obsnorm.h"

#pragma clang fp contract(off)

struct rl_obsnorm {
  int dim = 0, max_rows = 0, max_tiles = 0, device = 0;
  float eps = 0.f;
  float* state = nullptr;      // mean [dim] | var [dim] | std [dim]
  long long* count = nullptr;  // int64
  unsigned* ticket = nullptr;  // 0 between launches: the last workgroup rearms it
  double* partial = nullptr;   // [max_tiles][3][dim]: column sum, mean, M2 of a tile
};

namespace {

constexpr int BLOCK = 256;
constexpr int TILE_ROWS = 64, LANES = 64, GROUPS = BLOCK / LANES, ROWS_PER_THREAD = TILE_ROWS / GROUPS;

thread_local std::string g_err;
std::atomic<int64_t> g_launches{0};
int fail(const std::string& m) {
  g_err = m;
  return -1;
}
#define HIP_OK(x)                                                                  \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess) return fail(std::string(#x ": ") + hipGetErrorString(e_)); \
  } while (0)

struct Norm {  // one handle's side of a launch
  const float* x;
  float* y;
  float *mean, *var, *std;
  long long* count;
  unsigned* ticket;
  double* partial;
  int dim;
  float eps;
};

struct UpdateArgs {
  Norm d[2];
  int n_rows, tiles;
};

struct ApplyArgs {
  Norm d[2];
  long long n_rows;
};

__global__ __launch_bounds__(BLOCK) void update_kernel(UpdateArgs a) {
  const Norm& d = a.d[blockIdx.z];
  const int dim = d.dim, chunks = (dim + LANES - 1) / LANES;
  if ((int)blockIdx.y >= chunks) return;  // (a pair's narrower handle: whole workgroups leave, they hold no ticket)
  __shared__ double sh[BLOCK + 1];        // the one LDS object: 4 x 64 partial sums and, in [BLOCK], "this workgroup is the last"
  const int tid = threadIdx.x, lane = tid & (LANES - 1), grp = tid / LANES;
  const int tile = blockIdx.x, col = blockIdx.y * LANES + lane;
  const int row0 = tile * TILE_ROWS, nt = min(TILE_ROWS, a.n_rows - row0);
  const bool live = col < dim;
  float v[ROWS_PER_THREAD];
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < ROWS_PER_THREAD; ++i) {
    const int r = grp + i * GROUPS;
    v[i] = live && r < nt ? d.x[(size_t)(row0 + r) * dim + col] : 0.f;
  }
#pragma unroll
  for (int i = 0; i < ROWS_PER_THREAD; ++i) s += (double)v[i];  // (rows past the tile's end add 0)
  sh[tid] = s;
  __syncthreads();
  const double sum = ((sh[lane] + sh[LANES + lane]) + sh[2 * LANES + lane]) + sh[3 * LANES + lane];
  const double mean = sum / (double)nt;
  __syncthreads();
  double q = 0.0;
#pragma unroll
  for (int i = 0; i < ROWS_PER_THREAD; ++i) {
    const double e = (double)v[i] - mean;
    if (grp + i * GROUPS < nt) q += e * e;
  }
  sh[tid] = q;
  __syncthreads();
  if (grp == 0 && live) {
    double* p = d.partial + (size_t)tile * 3 * dim;
    p[col] = sum;
    p[dim + col] = mean;
    p[2 * dim + col] = ((sh[lane] + sh[LANES + lane]) + sh[2 * LANES + lane]) + sh[3 * LANES + lane];
  }
  // publish the tile, draw a ticket: every wavefront drains its stores, one lane releases at agent scope (the partials may sit in another
  // XCD's L2 than the merging workgroup's) and only then adds to the ticket
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned t = __hip_atomic_fetch_add(d.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = t == (unsigned)(a.tiles * chunks) - 1u;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    sh[BLOCK] = last ? 1.0 : 0.0;
  }
  __syncthreads();
  if (sh[BLOCK] == 0.0) return;
  // the last workgroup: Chan's merge in tile order, then the rule
  const long long count = *d.count + (long long)a.n_rows;  // (read by every thread before thread 0 writes it, below the barrier)
  const float rate = (float)a.n_rows / (float)count;
  for (int c = tid; c < dim; c += BLOCK) {
    // Chan, Golub and LeVeque's combination of all tiles at once, each pass in tile order: the batch mean from the tile sums (a mean that is
    // exactly 0 comes out as 0), then M2 = sum_t (M2_t + n_t (mean_t - mean)^2) - no division inside either loop and no load that waits for one
    const double n = (double)a.n_rows;
    const double* p = d.partial + c;
    const size_t tile_stride = (size_t)3 * dim;
    double S = 0.0;
#pragma unroll 16
    for (int t = 0; t < a.tiles; ++t) S += p[t * tile_stride];
    const double mean_x = S / n;
    double M2 = 0.0;
#pragma unroll 16
    for (int t = 0; t < a.tiles; ++t) {
      const double nb = (double)min(TILE_ROWS, a.n_rows - t * TILE_ROWS), e = p[t * tile_stride + dim] - mean_x;
      M2 += p[t * tile_stride + 2 * dim] + nb * (e * e);
    }
    // the rule on the fp32 state, evaluated in fp64 and rounded to fp32 once per entry (the rate alone is the rule's one fp32 division)
    const double var_x = M2 / n;
    const double mean_old = (double)d.mean[c], var_old = (double)d.var[c];
    const double delta = mean_x - mean_old;
    const double mean_upd = mean_old + (double)rate * delta;
    const float mean_new = (float)mean_upd;
    const float var_new = (float)(var_old + (double)rate * ((var_x - var_old) + delta * (mean_x - mean_upd)));
    d.mean[c] = mean_new;
    d.var[c] = var_new;
    d.std[c] = sqrtf(var_new);
  }
  __syncthreads();
  if (tid == 0) {
    *d.count = count;
    __hip_atomic_store(d.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(BLOCK) void apply_kernel(ApplyArgs a) {
  const Norm& d = a.d[blockIdx.y];
  const size_t total = (size_t)a.n_rows * d.dim, stride = (size_t)gridDim.x * BLOCK;
  for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < total; i += stride) {
    const int c = (int)(i % (size_t)d.dim);
    d.y[i] = (d.x[i] - d.mean[c]) / (d.std[c] + d.eps);
  }
}

__global__ void count_kernel(long long* p, long long v) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *p = v;
}

Norm side(rl_obsnorm* h, const float* x, float* y) {
  Norm d;
  d.x = x; d.y = y; d.mean = h->state; d.var = h->state + h->dim; d.std = h->state + 2 * h->dim;
  d.count = h->count; d.ticket = h->ticket; d.partial = h->partial; d.dim = h->dim; d.eps = h->eps;
  return d;
}

int update(rl_obsnorm* a, const float* xa, rl_obsnorm* b, const float* xb, int32_t n_rows, void* stream) {
  if (!a || !xa || (b && !xb)) return fail("NULL argument");
  if (n_rows < 0) return fail("n_rows is negative");
  if (n_rows > a->max_rows || (b && n_rows > b->max_rows)) return fail("n_rows above the max_rows the handle was created with");
  if (b && (b == a || b->device != a->device)) return fail("a pair needs two different handles on one device");
  if (n_rows == 0) return 0;
  HIP_OK(hipSetDevice(a->device));
  UpdateArgs u;
  u.d[0] = side(a, xa, nullptr);
  u.d[1] = b ? side(b, xb, nullptr) : u.d[0];
  u.n_rows = n_rows;
  u.tiles = (n_rows + TILE_ROWS - 1) / TILE_ROWS;
  const int chunks = (std::max(a->dim, b ? b->dim : 0) + LANES - 1) / LANES;
  hipLaunchKernelGGL(update_kernel, dim3(u.tiles, chunks, b ? 2 : 1), dim3(BLOCK), 0, (hipStream_t)stream, u);
  HIP_OK(hipGetLastError());
  ++g_launches;
  return 0;
}

int apply(rl_obsnorm* a, const float* xa, float* ya, rl_obsnorm* b, const float* xb, float* yb, int64_t n_rows, void* stream) {
  if (!a || !xa || !ya || (b && (!xb || !yb))) return fail("NULL argument");
  if (n_rows < 0) return fail("n_rows is negative");
  if (b && b->device != a->device) return fail("a pair needs two handles on one device");
  if (n_rows > (int64_t)1 << 40) return fail("n_rows too large");
  if (n_rows == 0) return 0;
  HIP_OK(hipSetDevice(a->device));
  ApplyArgs p;
  p.d[0] = side(a, xa, ya);
  p.d[1] = b ? side(b, xb, yb) : p.d[0];
  p.n_rows = n_rows;
  const size_t total = (size_t)n_rows * std::max(a->dim, b ? b->dim : 0);
  const int blocks = (int)std::min<size_t>((total + BLOCK - 1) / BLOCK, 2048);
  hipLaunchKernelGGL(apply_kernel, dim3(blocks, b ? 2 : 1), dim3(BLOCK), 0, (hipStream_t)stream, p);
  HIP_OK(hipGetLastError());
  ++g_launches;
  return 0;
}

}  // namespace

extern "C" {

const char* rl_obsnorm_last_error(void) { return g_err.c_str(); }
int64_t rl_obsnorm_launch_count(void) { return g_launches.load(); }
int32_t rl_obsnorm_dim(const rl_obsnorm* h) { return h ? h->dim : 0; }

int rl_obsnorm_create(int32_t dim, float eps, int32_t max_rows, int32_t device, rl_obsnorm** out) {
  if (!out) return fail("out is NULL");
  if (dim < 1 || dim > RL_OBSNORM_MAX_DIM) return fail("dim must be 1 .. " + std::to_string(RL_OBSNORM_MAX_DIM) + ", got " + std::to_string(dim));
  if (!(eps >= 0.f) || !std::isfinite(eps)) return fail("eps must be finite and >= 0");
  if (max_rows < 1) return fail("max_rows must be >= 1");
  HIP_OK(hipSetDevice(device));
  rl_obsnorm* h = new rl_obsnorm();
  h->dim = dim; h->eps = eps; h->max_rows = max_rows; h->device = device;
  h->max_tiles = (max_rows + TILE_ROWS - 1) / TILE_ROWS;
  std::vector<float> init(3 * (size_t)dim, 1.f);  // mean 0, var 1, std 1
  std::fill(init.begin(), init.begin() + dim, 0.f);
  const size_t bytes = init.size() * sizeof(float);
  if (hipMalloc(&h->state, bytes) != hipSuccess || hipMalloc(&h->count, sizeof(long long)) != hipSuccess ||
      hipMalloc(&h->ticket, sizeof(unsigned)) != hipSuccess || hipMalloc(&h->partial, (size_t)h->max_tiles * 3 * dim * sizeof(double)) != hipSuccess ||
      hipMemcpy(h->state, init.data(), bytes, hipMemcpyHostToDevice) != hipSuccess || hipMemset(h->count, 0, sizeof(long long)) != hipSuccess ||
      hipMemset(h->ticket, 0, sizeof(unsigned)) != hipSuccess) {
    rl_obsnorm_destroy(h);
    return fail("hipMalloc of the normaliser's state failed");
  }
  HIP_OK(hipDeviceSynchronize());  // the memsets ran on the null stream; callers launch on non-blocking streams
  *out = h;
  return 0;
}

int rl_obsnorm_destroy(rl_obsnorm* h) {
  if (!h) return 0;
  if (h->state) (void)hipFree(h->state);
  if (h->count) (void)hipFree(h->count);
  if (h->ticket) (void)hipFree(h->ticket);
  if (h->partial) (void)hipFree(h->partial);
  delete h;
  return 0;
}

int rl_obsnorm_update(rl_obsnorm* h, const float* x_dev, int32_t n_rows, void* stream) { return update(h, x_dev, nullptr, nullptr, n_rows, stream); }

int rl_obsnorm_update_pair(rl_obsnorm* a, const float* xa_dev, rl_obsnorm* b, const float* xb_dev, int32_t n_rows, void* stream) {
  if (!b) return fail("NULL argument");
  return update(a, xa_dev, b, xb_dev, n_rows, stream);
}

int rl_obsnorm_apply(rl_obsnorm* h, const float* x_dev, float* y_dev, int64_t n_rows, void* stream) {
  return apply(h, x_dev, y_dev, nullptr, nullptr, nullptr, n_rows, stream);
}

int rl_obsnorm_apply_pair(rl_obsnorm* a, const float* xa_dev, float* ya_dev, rl_obsnorm* b, const float* xb_dev, float* yb_dev, int64_t n_rows,
                          void* stream) {
  if (!b) return fail("NULL argument");
  return apply(a, xa_dev, ya_dev, b, xb_dev, yb_dev, n_rows, stream);
}

int rl_obsnorm_get_state(rl_obsnorm* h, float* mean_dev, float* var_dev, float* std_dev, int64_t* count, void* stream) {
  if (!h) return fail("NULL argument");
  HIP_OK(hipSetDevice(h->device));
  float* dst[3] = {mean_dev, var_dev, std_dev};
  for (int i = 0; i < 3; ++i)
    if (dst[i]) HIP_OK(hipMemcpyAsync(dst[i], h->state + (size_t)i * h->dim, h->dim * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  long long c = 0;
  if (count) HIP_OK(hipMemcpyAsync(&c, h->count, sizeof(c), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  if (count) *count = c;
  return 0;
}

int rl_obsnorm_set_state(rl_obsnorm* h, const float* mean_dev, const float* var_dev, const float* std_dev, int64_t count, void* stream) {
  if (!h) return fail("NULL argument");
  if (count < 0) return fail("count is negative");
  HIP_OK(hipSetDevice(h->device));
  const float* src[3] = {mean_dev, var_dev, std_dev};
  for (int i = 0; i < 3; ++i)
    if (src[i]) HIP_OK(hipMemcpyAsync(h->state + (size_t)i * h->dim, src[i], h->dim * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  hipLaunchKernelGGL(count_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, h->count, (long long)count);
  HIP_OK(hipGetLastError());
  return 0;
}

int rl_obsnorm_state_pointers(rl_obsnorm* h, float** mean, float** var, float** std, int64_t** count) {
  if (!h) return fail("NULL argument");
  if (mean) *mean = h->state;
  if (var) *var = h->state + h->dim;
  if (std) *std = h->state + 2 * h->dim;
  if (count) *count = reinterpret_cast<int64_t*>(h->count);
  return 0;
}

}  // extern "C"
