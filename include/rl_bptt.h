/* rl_bptt.h - C-ABI of the HIP-native recurrent PPO learner (csrc/learner/rl_bptt.inl, compiled into librl_ppo_hip.so next to the PPO and the
 * distillation learner): back-propagation through time.
 *
 * Replaces `alg.update()` of rsl_rl's `OnPolicyRunner.learn` for the reference's `rsl_rl_recurrent_cfg_entry_point` tasks: a single-layer LSTM
 * (`RslRlRNNModelCfg(rnn_type="lstm", rnn_hidden_dim=256, rnn_num_layers=1)`) in front of the actor's and the critic's ELU MLP.  The update
 * RULE is defined by robot_lab_amd/recurrent.py (`RecurrentPPO.update`, `Memory.forward`, `ActorCriticRecurrent.unroll`); this library
 * evaluates the same rule on fp32 master parameters, gradients and Adam moments in flat device buffers.
 *
 * The rule, over a filled storage of T steps x N envs.  A mini-batch (block) is n = N / num_mini_batches envs, contiguous and in order, over
 * all T steps; the remainder envs are left out; no shuffle.  Per block and network (actor memory on observations, critic memory on
 * privileged_observations) the recurrence starts from the saved state of step 0 (h0, c0 - stale across the epochs, no gradient), the input
 * state of step t >= 1 is zeroed where dones[t - 1] is set (a select: a NaN in a reset row's old state does not travel; dones[T - 1] is not
 * read), z_t = W_ih x_t + b_ih + W_hh h~_{t-1} + b_hh with gates i, f, g, o, c_t = s(f) c~ + s(i) tanh(g), h_t = s(o) tanh(c_t).  The heads read
 * the T n rows h_t in [T][block] order; behind them everything is the PPO learner's mini-batch (include/rl_ppo.h): loss head with the
 * KL-adaptive learning-rate word, dX, dW, column sums, reduce, sum of squares, clip + Adam, floor of std.  No gradient crosses a done.
 *
 * Launches of one block, all on the caller's stream: the row index + the summed biases; the input half of the gates (one forward GEMM, both
 * networks); T forward steps (h~ W_hh^T on the matrix cores in exact fp32, the gate nonlinearities in the epilogue, both networks per
 * launch); the heads' forward, the PPO head, the heads' dX down to dL/dh; T backward steps (dz_{t+1} W_hh, the cell's backward in the
 * epilogue); the weight gradients of both memories and of the heads; the optimiser step.  Every reduction has a fixed order (no
 * floating-point atomics, no workgroup waits for another): the same state gives bit-identical parameters, moments and statistics.
 * Every buffer is allocated by rl_bptt_create: the entry points below only ENQUEUE.
 *
 * All `*_dev` pointers are DEVICE pointers.  Flat layout (parameters, gradients, Adam moments), the order of
 * `ActorCriticRecurrent.parameters()`: std[act]; memory_a weight_ih [4H][obs], weight_hh [4H][H], bias_ih [4H], bias_hh [4H]; memory_c alike
 * ([4H][critic obs] ...); per actor layer W[out][in], b[out]; the critic's layers alike.  bias_ih and bias_hh are two parameters with equal
 * gradients and their own Adam moments; both count in the gradient norm. */
#ifndef RL_BPTT_H
#define RL_BPTT_H

#include <stdint.h>

#include "rl_ppo.h" /* rl_ppo_hyper, the activation / schedule / std enums */

#ifdef __cplusplus
extern "C" {
#endif

#define RL_BPTT_MAX_LAYERS 8   /* = RL_PPO_MAX_LAYERS: layers of a head */
#define RL_BPTT_MAX_WIDTH 512  /* = RL_PPO_MAX_WIDTH = RL_LSTM_MAX_WIDTH: observation rows, the hidden state, the heads' layers */
#define RL_BPTT_STATS 8        /* entries of rl_bptt_stats */

/* the [T][N] views of a filled rollout storage (include/rl_rollout.h) and the saved states of step 0, fp32 unless said otherwise */
typedef struct rl_bptt_batch {
  const float *observations, *privileged_observations, *actions; /* [T][N][obs], [T][N][critic obs], [T][N][act] */
  const float *values, *returns, *advantages, *actions_log_prob; /* [T][N] */
  const float *mu, *sigma;                                       /* [T][N][act] */
  const uint8_t* dones;                                          /* [T][N] bytes, != 0: the step ended an episode */
  const float *h0_a, *c0_a, *h0_c, *c0_c;                        /* [N][H]: the state step 0 started from (its own reset applied) */
} rl_bptt_batch;

typedef struct rl_bptt rl_bptt;

/* hidden: H of both memories.  actor_dims / critic_dims: n_layers + 1 widths of the heads (H, hidden..., output); actor_dims[0] and
 * critic_dims[0] must equal `hidden`, the critic's output width 1.  T, num_envs: the storage every later call reads.  Parameters start at
 * zero (std at 1): call rl_bptt_set_parameters.  The arguments are checked BEFORE the device is touched; refused with a reason
 * (rl_bptt_last_error) and a null handle: widths (obs_dim, critic_obs_dim, hidden, the heads') outside 1..RL_BPTT_MAX_WIDTH, a layer count
 * outside 1..RL_BPTT_MAX_LAYERS, an activation other than ELU, std_type "log", the adaptive schedule without a positive desired_kl,
 * num_envs < num_mini_batches (no block of whole trajectories), T < 1, T x num_envs rows that do not fit 31 bits. */
int rl_bptt_create(int32_t obs_dim, int32_t critic_obs_dim, int32_t hidden, const int32_t* actor_dims, const int32_t* critic_dims, int32_t n_layers,
                   int32_t activation, const rl_ppo_hyper* hyper, int32_t T, int32_t num_envs, int32_t device, rl_bptt** out);
int rl_bptt_destroy(rl_bptt* p);
const char* rl_bptt_last_error(void);

int64_t rl_bptt_num_parameters(const rl_bptt* p);

/* lstm_a_dev / lstm_c_dev: nn.LSTM's four tensors of a memory (weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0); then nn.Linear images
 * ([out][in], [out]) per head layer + std[act].  Device pointers; stream-ordered device-to-device copies.  A null array / pointer skips that part. */
int rl_bptt_set_parameters(rl_bptt* p, const float* const* lstm_a_dev, const float* const* lstm_c_dev, const float* const* actor_w_dev,
                           const float* const* actor_b_dev, const float* const* critic_w_dev, const float* const* critic_b_dev, const float* std_dev,
                           void* stream);
int rl_bptt_get_parameters(rl_bptt* p, float* const* lstm_a_dev, float* const* lstm_c_dev, float* const* actor_w_dev, float* const* actor_b_dev,
                           float* const* critic_w_dev, float* const* critic_b_dev, float* std_dev, void* stream);
/* the addresses of the master parameters inside the flat buffer: lstm_a_dev[4] / lstm_c_dev[4] are what rl_lstm_set_weights_device reads, the
 * heads' what rl_mlp_set_weights_device reads - the push after an update stays on the device */
int rl_bptt_parameter_pointers(rl_bptt* p, const float** lstm_a_dev, const float** lstm_c_dev, const float** actor_w_dev, const float** actor_b_dev,
                               const float** critic_w_dev, const float** critic_b_dev, const float** std_dev);
/* which: 0 parameters, 1 gradients, 2 Adam first moment, 3 Adam second moment -> dst_dev[rl_bptt_num_parameters] */
int rl_bptt_get_flat(rl_bptt* p, int32_t which, float* dst_dev, void* stream);
/* which: 2 or 3 <- src_dev[rl_bptt_num_parameters] */
int rl_bptt_set_flat(rl_bptt* p, int32_t which, const float* src_dev, void* stream);
/* the learning-rate word and the Adam step counter.  get: waits for `stream`, one small copy.  set: stream-ordered; refused: a learning rate
 * that is not finite and > 0, a negative step. */
int rl_bptt_get_optimizer(rl_bptt* p, double* lr, int64_t* step, void* stream);
int rl_bptt_set_optimizer(rl_bptt* p, double lr, int64_t step, void* stream);

/* (for tests) recurrence + heads + loss head + backward through time for the block of envs lo .. lo + n - 1 (n = num_envs / num_mini_batches):
 * the gradient is left in the flat gradient buffer.  No optimiser step, no change of the learning rate or the statistics. */
int rl_bptt_block_grad(rl_bptt* p, const rl_bptt_batch* batch, int32_t lo, void* stream);
/* (for tests) recurrence + heads of the same block: mean_out_dev [T][n][act], value_out_dev [T][n] */
int rl_bptt_forward(rl_bptt* p, const rl_bptt_batch* batch, int32_t lo, float* mean_out_dev, float* value_out_dev, void* stream);

/* The whole RecurrentPPO.update: num_learning_epochs x num_mini_batches blocks, block i of every epoch the envs i n .. (i + 1) n - 1. */
int rl_bptt_update(rl_bptt* p, const rl_bptt_batch* batch, void* stream);

/* out[RL_BPTT_STATS]: mean value loss, mean surrogate loss, mean entropy, mean KL (0 unless adaptive), learning rate, last pre-clip gradient
 * norm, blocks in the last update, Adam step counter.  Waits for `stream`, one small copy. */
int rl_bptt_stats(rl_bptt* p, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
