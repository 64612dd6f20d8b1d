/* rl_rnd.h - C-ABI of the intrinsic reward of random network distillation inside the collection loop (csrc/rl_rnd.hip -> librl_rnd_hip.so).
 *
 * THE RULE is robot_lab_amd/rnd.py (`RandomNetworkDistillation.collect_step`; rsl_rl 3.0.1 `modules/rnd.py` restated).  The two embeddings
 * target(s), predictor(s) [N][K] of a step come from ONE launch of the fused inference kernels (rl_mlp_forward_pair, include/rl_policy.h), the
 * state's and the reward's running statistics are rl_obsnorm handles (include/rl_obsnorm.h); this library owns what lies between them:
 *
 *   rows     r[n] = sqrt(sum_k (target[n][k] - predictor[n][k])^2), avg[n] = avg[n] gamma_r + r[n]
 *            The difference is one fp32 subtraction (the rule's); its squares (exact in fp64) are added in fp64 in a FIXED order: a row belongs
 *            to 16 neighbouring lanes, lane j adds the columns j, j + 16, j + 32, ... in ascending order, then the 16 sums are folded with the
 *            butterfly of strides 8, 4, 2, 1 (lane j takes lane j ^ stride: every lane holds the same bits).  The square root is the correctly
 *            rounded fp64 one, rounded once more to fp32: no approximate sqrt / rsq anywhere, so a difference (3 2^k, 0, .., 0, 4 2^k) gives
 *            5 2^k exactly.  avg: one fp32 multiplication and one fp32 addition, never fused.
 *   finish   r <- r / std if std > 0 (the std word of the reward's rl_obsnorm handle of dim 1, AFTER this step's update with avg; a null
 *            pointer: no reward normalisation), r <- r weight[t], slot[n] <- slot[n] + r: correctly rounded fp32 operations, never fused.
 *            slot is the reward slot of step t (rl_rollout_get_buffer(RL_RO_REWARDS) + t N), which the env kernel has filled with
 *            r_ext + gamma V on time-outs - so the sum is (r_ext + gamma V to) + r_int, the order the rule states.
 *            Every workgroup leaves the fp64 sums of its rows' r and new slot values in a partial of its own (step t, workgroup b);
 *            rl_rnd_reward_sums adds them in (t, b) order in one workgroup: no floating-point atomics, the same input gives the same bits.
 * Without reward normalisation rows + finish are ONE launch (rl_rnd_reward_step); with it the caller puts rl_obsnorm_update(avg) between
 * rl_rnd_reward_rows and rl_rnd_reward_finish.
 * The weights of an iteration are a [T] device vector: rl_rnd_reward_set_weights copies them stream-ordered, ahead of the (captured) loop; the
 * kernels of step t read entry t.  Nothing is allocated after create and every launch argument of a step is fixed, so a loop over the steps
 * can be stream-captured once and replayed.
 *
 * All array arguments are DEVICE pointers (fp32) unless they say HOST.  Arguments are checked before the device is touched; a refused call
 * returns -1, launches nothing and leaves its reason in rl_rnd_reward_last_error(). */
#ifndef RL_RND_H
#define RL_RND_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RL_RND_MAX_OUTPUTS 512 /* = RL_MLP_MAX_WIDTH: the widest embedding */

typedef struct rl_rnd_reward rl_rnd_reward;

/* num_envs >= 1 (N), num_outputs 1..RL_RND_MAX_OUTPUTS (K), num_steps >= 1 (T: the steps of an iteration), gamma_r finite in [0, 1].
 * avg starts at 0, the weights at 0. */
int rl_rnd_reward_create(int32_t num_envs, int32_t num_outputs, int32_t num_steps, float gamma_r, int32_t device, rl_rnd_reward** out);
int rl_rnd_reward_destroy(rl_rnd_reward* h);
const char* rl_rnd_reward_last_error(void);

/* weights_host: HOST array of num_steps finite floats, copied into the handle before the call returns and to the device stream-ordered. */
int rl_rnd_reward_set_weights(rl_rnd_reward* h, const float* weights_host, void* stream);

/* t in [0, num_steps).  rows: r and avg.  finish: see above; std_dev may be NULL.  step: both in one launch, without reward normalisation. */
int rl_rnd_reward_rows(rl_rnd_reward* h, const float* predictor_dev, const float* target_dev, void* stream);
int rl_rnd_reward_finish(rl_rnd_reward* h, int32_t t, const float* std_dev, float* reward_slot_dev, void* stream);
int rl_rnd_reward_step(rl_rnd_reward* h, const float* predictor_dev, const float* target_dev, int32_t t, float* reward_slot_dev, void* stream);

/* The handle's own buffers - r [N] (raw, of the last rows / step), avg [N], weights [T] - for a caller that views them in place; they live
 * until rl_rnd_reward_destroy.  Any of the three may be NULL. */
int rl_rnd_reward_pointers(rl_rnd_reward* h, float** r, float** avg, float** weights);
/* avg <- 0, stream-ordered (a new run) */
int rl_rnd_reward_reset(rl_rnd_reward* h, void* stream);

/* out[2] (HOST): the sums over the steps 0 .. n_steps - 1 of the last loop and all envs of the weighted intrinsic reward and of the slot values
 * after the addition.  One small launch, then waits for `stream`, one small copy. */
int rl_rnd_reward_sums(rl_rnd_reward* h, int32_t n_steps, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
