/* rl_obsnorm.h - C-ABI of the empirical observation normalisation: rsl_rl's running mean / variance of an observation group
 * and its application in front of a network (`actor_obs_normalization` / `critic_obs_normalization` of `RslRlPpoActorCriticCfg`,
 * which every agent cfg of the reference spells out, e.g. .../unitree_a1/agents/rsl_rl_ppo_cfg.py:15-22).
 *
 * THE RULE is `robot_lab_amd.ppo.EmpiricalNormalization` (torch code; rsl_rl/networks/normalization.py restated).  State per handle:
 * mean [dim], var [dim], std [dim] (fp32; zeros / ones / ones at creation) and count (int64, 0).
 *   apply:   y = (x - mean) / (std + eps)                               fp32, exactly these three operations
 *   update:  with the n rows of x:   count += n;  rate = (float)n / (float)count;
 *            mean_x, var_x = column mean and POPULATION variance of x;  delta = mean_x - mean;  mean += rate * delta;
 *            var += rate * (var_x - var + delta * (mean_x - mean));  std = sqrt(var)            (mean: the updated one)
 * mean_x / var_x are formed without the cancelling sum(x^2) - sum(x)^2: every 64-row tile gives a two-pass (mean, M2) per column,
 * accumulated in fp64; the last workgroup to arrive (an integer ticket behind an agent-scope release, no floating-point atomics, no
 * grid-wide synchronisation) combines the tiles IN TILE ORDER with Chan, Golub and LeVeque's formula in fp64 - the batch mean from the
 * tile sums, M2 = sum_t (M2_t + n_t (mean_t - mean)^2) - and evaluates the rule above on the fp32 state in fp64 (the rate is the rule's one
 * fp32 division), rounding mean and var to fp32 once; std = sqrtf(var).  The same input gives the same bits; nothing is allocated after
 * create and the row count is a launch argument, so every call below can be stream-captured.
 *
 * All array arguments are DEVICE pointers (fp32, row-major [n_rows][dim]); work is stream-ordered on `stream` (a hipStream_t, or NULL
 * for the default stream).  Arguments are checked before the device is touched; a refused call returns -1, launches nothing and leaves
 * its reason in rl_obsnorm_last_error(). */
#ifndef RL_OBSNORM_H
#define RL_OBSNORM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RL_OBSNORM_MAX_DIM 512 /* = RL_MLP_MAX_WIDTH: the widest input row of the networks behind it */

typedef struct rl_obsnorm rl_obsnorm;

/* dim 1 .. RL_OBSNORM_MAX_DIM; eps >= 0 (rsl_rl: 1e-2); max_rows >= 1: the largest n_rows rl_obsnorm_update will be given */
int rl_obsnorm_create(int32_t dim, float eps, int32_t max_rows, int32_t device, rl_obsnorm** out);
int rl_obsnorm_destroy(rl_obsnorm* h);

/* One launch.  n_rows == 0: nothing happens (and nothing is launched); n_rows > max_rows is refused. */
int rl_obsnorm_update(rl_obsnorm* h, const float* x_dev, int32_t n_rows, void* stream);
/* y = (x - mean) / (std + eps) with the state as the stream finds it (an update queued in front is seen).  Any n_rows >= 0, also
 * T * N of a stored batch; y_dev may equal x_dev. */
int rl_obsnorm_apply(rl_obsnorm* h, const float* x_dev, float* y_dev, int64_t n_rows, void* stream);

/* The same for two handles over the same row count in ONE launch each (the policy and the critic group of a rollout step); results
 * are bit-identical to two single calls.  Both handles live on one device. */
int rl_obsnorm_update_pair(rl_obsnorm* a, const float* xa_dev, rl_obsnorm* b, const float* xb_dev, int32_t n_rows, void* stream);
int rl_obsnorm_apply_pair(rl_obsnorm* a, const float* xa_dev, float* ya_dev, rl_obsnorm* b, const float* xb_dev, float* yb_dev, int64_t n_rows,
                          void* stream);

/* State: the three vectors go to / come from DEVICE arrays of dim floats (any of them may be NULL: skipped), the count by value.
 * set is stream-ordered; get waits for the stream (it returns the count to the host). */
int rl_obsnorm_get_state(rl_obsnorm* h, float* mean_dev, float* var_dev, float* std_dev, int64_t* count, void* stream);
int rl_obsnorm_set_state(rl_obsnorm* h, const float* mean_dev, const float* var_dev, const float* std_dev, int64_t count, void* stream);
/* The handle's own buffers (mean, var, std: dim floats each; count: one int64), for a caller that views them in place.  They live
 * until rl_obsnorm_destroy. */
int rl_obsnorm_state_pointers(rl_obsnorm* h, float** mean, float** var, float** std, int64_t** count);

int32_t rl_obsnorm_dim(const rl_obsnorm* h);
int64_t rl_obsnorm_launch_count(void); /* kernel launches this library has enqueued in this process (tests: a refusal launches nothing) */
const char* rl_obsnorm_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
