// env_history.h - observation history (include/rl_env.h rl_env_set_obs_history): the per-element rule of the history launch, written
// ONCE for the HIP kernel (csrc/rl_env_history.hip) and for the host loop the CPU lane emulator runs (csrc/rl_env_host.h), and the
// column table both read.  No step kernel includes this file.
//
// A group's history row is term-major: term k with frame width d_k and history length H_k owns max(H_k, 1) * d_k columns - its
// frames, oldest first, newest last (H_k = 0: the current frame only).  A launch that wrote a frame into the step kernel's ring slot
// t % 2 is followed by ONE history launch that builds history slot t % 2 from that frame and history slot (t - 1) % 2:
//     out[e][c] = frame[e][col[c].frame]   if env e was reset by the launch, or column c is a newest slot (col[c].prev < 0)
//               = prev[e][col[c].prev]     otherwise: the same term, one frame later
// Nothing moves in place, every pointer repeats with period 2 (the capture protocol of rl_env_graph_* holds as it is), rows N..Npad
// are never written.  The element type is a template parameter: the fp64 build of the emulator (tests/emu/make_f64.py) uses this file as it is.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RL_HIST_FN __host__ __device__ inline
#else
#define RL_HIST_FN inline
#endif

namespace rl {

constexpr int MAX_OBS_HISTORY = 32;  // = RL_MAX_OBS_HISTORY (include/rl_env.h)

struct HistCol {
  int32_t frame;  // column of the frame row this column takes when its env was reset or it is a newest slot
  int32_t prev;   // column of the previous history slot it takes otherwise; -1: a newest slot
};

template <class R>
struct HistGroupT {
  const R* frame;       // [Npad][frame_dim]: what the launch before wrote
  const R* prev;        // [Npad][hist_dim]: history slot (t - 1) % 2
  R* out;               // [Npad][hist_dim]: history slot t % 2
  const HistCol* cols;  // [hist_dim]
  int32_t frame_dim, hist_dim;  // hist_dim 0: the group keeps no history
};

template <class R>
struct HistArgsT {
  HistGroupT<R> g[2];       // policy, critic
  uint32_t n0, total;       // elements of the policy group (N * hist_dim), of both groups
  // env e was reset by the launch:  reset_all | r0[e] | r1[e]   (step: terminated, time_out; reset(env_ids): the mask, NULL)
  const uint8_t *r0, *r1;
  int32_t reset_all;
};

// element i of the flattened [N][hist_dim] row spaces, the policy group's first
template <class R>
RL_HIST_FN void history_element(const HistArgsT<R>& A, uint32_t i) {
  const int grp = i >= A.n0 ? 1 : 0;
  const HistGroupT<R>& G = A.g[grp];
  const uint32_t li = i - (grp ? A.n0 : 0u), hd = (uint32_t)G.hist_dim;
  const uint32_t e = li / hd, c = li - e * hd;
  const HistCol col = G.cols[c];
  bool reset = A.reset_all != 0;
  if (A.r0) reset = reset || A.r0[e] != 0;
  if (A.r1) reset = reset || A.r1[e] != 0;
  const R v = (reset || col.prev < 0) ? G.frame[(size_t)e * (uint32_t)G.frame_dim + (uint32_t)col.frame] : G.prev[(size_t)e * hd + (uint32_t)col.prev];
  G.out[(size_t)e * hd + c] = v;
}

// the column table of a group: term k has width dims[k] and history length hist[k]; returns hist_dim (cols may be NULL: the width only)
inline int32_t history_columns(const int32_t* dims, const int32_t* hist, int32_t n_terms, HistCol* cols) {
  int32_t off = 0, foff = 0;
  for (int32_t k = 0; k < n_terms; ++k) {
    const int32_t d = dims[k], H = hist[k] > 1 ? hist[k] : 1;
    for (int32_t s = 0; s < H; ++s)
      for (int32_t j = 0; j < d; ++j)
        if (cols) cols[off + s * d + j] = HistCol{foff + j, s == H - 1 ? -1 : off + (s + 1) * d + j};
    off += H * d;
    foff += d;
  }
  return off;
}

}  // namespace rl
