/* rl_rnd_learner.h - C-ABI of the HIP-native update of random network distillation (csrc/learner/rl_rnd.inl, compiled into librl_ppo_hip.so next
 * to the PPO learner, whose kernels it launches).  The reward half lives in include/rl_rnd.h.
 *
 * THE RULE is robot_lab_amd/rnd.py (`update_minibatch` inside `PPO.update`; rsl_rl 3.0.1 restated): per mini-batch of the PPO update, on the
 * same rows idx of the same permutation, L = mean over the n K entries of (predictor(s) - target(s))^2 with s the (already normalised) state
 * rows and the target held constant, then one step of a SEPARATE Adam (torch.optim.Adam's defaults, a learning rate nobody moves, NO gradient
 * clipping) on the predictor only.  This library evaluates it on fp32 master parameters, gradients and Adam moments in flat device buffers:
 * both networks forward through the PPO learner's exact-fp32 GEMMs (the rows gathered in the first layer's operand fetch), the MSE head and its
 * finish kernel are the distillation learner's (gradient 2 (p - t) / (n K) per entry; the loss summed in fp64 in a fixed order), dX and dW run
 * for the predictor, then the column sums, the reduce, the sum of squares and the Adam kernel with a clip coefficient of exactly 1
 * (max_norm = +inf: min(inf / (norm + 1e-6), 1) is 1 for every finite norm).  The target's parameters are read and never written.
 * Every reduction has a fixed order (no floating-point atomics): the same state and permutation give bit-identical parameters.
 * rl_rnd_update only ENQUEUES on the caller's stream; every buffer is allocated by rl_rnd_create.
 *
 * The state rows are given NORMALISED: with state normalisation the caller runs rl_obsnorm_apply (include/rl_obsnorm.h) over the stored rows
 * into a scratch matrix once per update, with the statistics as the collection left them.
 *
 * All `*_dev` pointers are DEVICE pointers.  Flat layout (parameters, gradients, Adam moments): per predictor layer W[out][in], b[out] - the
 * order of `predictor.parameters()`. */
#ifndef RL_RND_LEARNER_H
#define RL_RND_LEARNER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RL_RND_MAX_LAYERS 8  /* = RL_PPO_MAX_LAYERS */
#define RL_RND_MAX_WIDTH 512 /* = RL_PPO_MAX_WIDTH */
#define RL_RND_STATS 4       /* entries of rl_rnd_stats */

enum rl_rnd_activation { RL_RND_ACT_ELU = 0, RL_RND_ACT_RELU = 1, RL_RND_ACT_TANH = 2 }; /* only ELU is implemented; others are refused */

typedef struct rl_rnd_hyper {
  double learning_rate;
  int32_t num_learning_epochs, num_mini_batches;
} rl_rnd_hyper;

typedef struct rl_rnd rl_rnd;

/* predictor_dims / target_dims: n + 1 widths each (state, hidden..., outputs); input and output widths of the two networks must agree.
 * Parameters start at zero: call rl_rnd_set_parameters.  The arguments are checked BEFORE the device is touched; refused with a reason
 * (rl_rnd_last_error) and a null handle: an activation other than ELU, widths outside 1..RL_RND_MAX_WIDTH, a layer count outside
 * 1..RL_RND_MAX_LAYERS, networks whose ends differ, a learning rate that is not finite and positive, num_learning_epochs < 1,
 * num_mini_batches < 1, max_rows_per_minibatch < 1. */
int rl_rnd_create(const int32_t* predictor_dims, int32_t n_predictor_layers, const int32_t* target_dims, int32_t n_target_layers, int32_t activation,
                  const rl_rnd_hyper* hyper, int32_t max_rows_per_minibatch, int32_t device, rl_rnd** out);
int rl_rnd_destroy(rl_rnd* p);
const char* rl_rnd_last_error(void);

int64_t rl_rnd_num_parameters(const rl_rnd* p); /* of the predictor */

/* nn.Linear images ([out][in], [out]) per layer, device pointers; stream-ordered device-to-device copies.  A null array skips that part. */
int rl_rnd_set_parameters(rl_rnd* p, const float* const* predictor_w_dev, const float* const* predictor_b_dev, const float* const* target_w_dev,
                          const float* const* target_b_dev, void* stream);
int rl_rnd_get_parameters(rl_rnd* p, float* const* predictor_w_dev, float* const* predictor_b_dev, float* const* target_w_dev, float* const* target_b_dev,
                          void* stream);
/* the addresses of the predictor's master parameters inside the flat buffer (what rl_mlp_set_weights_device reads for a push without the host) */
int rl_rnd_parameter_pointers(rl_rnd* p, const float** predictor_w_dev, const float** predictor_b_dev);
/* which: 0 parameters, 1 gradients, 2 Adam first moment, 3 Adam second moment -> dst_dev[rl_rnd_num_parameters] */
int rl_rnd_get_flat(rl_rnd* p, int32_t which, float* dst_dev, void* stream);
/* which: 2 or 3 <- src_dev[rl_rnd_num_parameters] */
int rl_rnd_set_flat(rl_rnd* p, int32_t which, const float* src_dev, void* stream);
/* the learning-rate word and the Adam step counter.  get: waits for `stream`, one small copy.  set: stream-ordered; refused: a learning rate
 * that is not finite and > 0, a negative step. */
int rl_rnd_get_optimizer(rl_rnd* p, double* lr, int64_t* step, void* stream);
int rl_rnd_set_optimizer(rl_rnd* p, double lr, int64_t step, void* stream);

/* forward of both networks + head + backward of the predictor for the rows idx_dev[0 .. n_idx) (int64 row numbers into state_dev
 * [rows][state width]): the gradient of L is left in the flat gradient buffer.  No optimiser step, no statistics. */
int rl_rnd_minibatch_grad(rl_rnd* p, const float* state_dev, const int64_t* idx_dev, int32_t n_idx, void* stream);

/* The RND half of a whole PPO.update: num_learning_epochs x num_mini_batches mini-batches of n_rows / num_mini_batches rows, mini-batch i of
 * every epoch taking perm_dev[i * mb .. (i + 1) * mb) - the SAME perm_dev rl_ppo_update gets.  Enqueues only. */
int rl_rnd_update(rl_rnd* p, const float* state_dev, const int64_t* perm_dev, int32_t n_rows, void* stream);

/* out[RL_RND_STATS]: mean loss over the mini-batches of the last update, learning rate, mini-batches of the last update, Adam step counter.
 * Waits for `stream`, one small copy. */
int rl_rnd_stats(rl_rnd* p, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
