/* rl_lstm.h - C-ABI of the LSTM cell of a recurrent actor-critic's collection step.
 *
 * Replaces (reference call sites; the arithmetic itself lives in the third-party rsl_rl `Memory` / torch `nn.LSTM`):
 *   - `RslRlRNNModelCfg(rnn_type="lstm", rnn_hidden_dim=256, rnn_num_layers=1)` in front of the actor's and the critic's MLP, what the
 *     `rsl_rl_recurrent_cfg_entry_point` tasks train with: every `alg.act(obs)` of a rollout runs one cell step per network over all
 *     envs, and `Memory.reset(dones)` zeroes the state of the envs that ended.
 *
 * One step of a single-layer LSTM over n_rows independent rows in fp32 (exact-f32 MFMA, v_mfma_f32_16x16x4_f32, the gate
 * nonlinearities in the launch's epilogue), with the per-row reset and the state record of the rollout storage folded in.  All
 * pointers passed to rl_lstm_step are DEVICE pointers; weights are given once, on the host, in torch.nn.LSTM's layout.  No
 * floating-point atomics: the same input gives the same bits. */
#ifndef RL_LSTM_H
#define RL_LSTM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RL_LSTM_MAX_WIDTH 512 /* widest input row / hidden state */

typedef struct rl_lstm rl_lstm;

/* w_ih [4 hidden][in_dim], w_hh [4 hidden][hidden], b_ih / b_hh [4 hidden]: HOST pointers, nn.LSTM's `weight_ih_l0` ... layout, gate
 * order i, f, g, o.  1 <= in_dim, hidden <= RL_LSTM_MAX_WIDTH. */
int rl_lstm_create(int32_t in_dim, int32_t hidden, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                   int32_t device, rl_lstm** out);

/* New parameters for an existing cell from DEVICE copies of the same four tensors: the re-layout is a kernel on `stream` - no
 * device-wide wait, no host copy, capturable.  The images keep their addresses (a captured graph that launches the cell stays
 * valid) and are bit-identical to what rl_lstm_create makes of the same numbers.  Ordering against steps on OTHER streams is the
 * caller's.  The same contract as rl_mlp_set_weights_device (include/rl_policy.h). */
int rl_lstm_set_weights_device(rl_lstm* l, const float* w_ih_dev, const float* w_hh_dev, const float* b_ih_dev, const float* b_hh_dev,
                               void* stream);

/* One step over n_rows rows, stream-ordered:
 *     (h~, c~)[r] = reset_u8[r] != 0 ? (0, 0) : (h, c)[r]            (a select: NaN in a reset row's old state does not travel)
 *     z = W_ih x + W_hh h~ + (b_ih + b_hh)                            [n_rows][4 hidden], gate order i, f, g, o
 *     c' = sigmoid(z_f) c~ + sigmoid(z_i) tanh(z_g),   h' = sigmoid(z_o) tanh(c')
 * x [n_rows][in_dim]; h, c, h_out, c_out [n_rows][hidden]; reset_u8 [n_rows] or NULL (no row is reset).
 * h_saved / c_saved (each nullable, [n_rows][hidden]) receive (h~, c~), the state as the step saw it: the storage record.
 * gates_out (nullable, [n_rows][4 hidden]) receives z.  A NULL output costs no store and leaves the others bit-identical.
 * h_out / c_out must not be h / c (rows are read by other workgroups while theirs are written). */
int rl_lstm_step(rl_lstm* l, const float* x, const uint8_t* reset_u8, const float* h, const float* c, float* h_saved, float* c_saved,
                 float* h_out, float* c_out, float* gates_out, int32_t n_rows, void* stream);

/* Two cells over the same n_rows rows in ONE launch (the actor's and the critic's memory of a rollout step, one reset vector): the
 * results are bit-identical to two rl_lstm_step calls. */
int rl_lstm_step_pair(rl_lstm* a, const float* xa, const float* ha, const float* ca, float* ha_saved, float* ca_saved, float* ha_out,
                      float* ca_out, float* gates_a_out, rl_lstm* b, const float* xb, const float* hb, const float* cb, float* hb_saved,
                      float* cb_saved, float* hb_out, float* cb_out, float* gates_b_out, const uint8_t* reset_u8, int32_t n_rows,
                      void* stream);

int32_t rl_lstm_in_dim(const rl_lstm* l);
int32_t rl_lstm_hidden(const rl_lstm* l);
int rl_lstm_destroy(rl_lstm* l);
const char* rl_lstm_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
