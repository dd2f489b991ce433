/*
 * finenvs_amd_lstm_grad_streamed.h -- the gradient half of the one-output LSTM head at H = 256 / 512 / 1024 (same
 * library as finenvs_amd.h; the small sizes are finenvs_amd_lstm_grad.h).
 *
 * The reference trains its time-series agent with PPOAgentLSTM(hidden_dim=1024)
 * (examples/time_series/PPO_LSTM_training_SPY.py).  At H >= 256 fe_lstm_forward (finenvs_amd_ext.h) streams the
 * recurrent weights from L2, fragment-major; here is its backward on the same descriptors, for the same head as
 * fe_lstm_backward: one asset (A = 1), the env's W, the same six gradients in torch's layout (struct fe_lstm_grads).
 *
 * With p = w_out . h_W + b_out, y = act(p) as fe_lstm_forward returned it and g = d_outputs:
 *   out_activation 0 (tanh)   dp = g (1 - y^2)
 *   out_activation 2 (none)   dp = g
 *   d w_out = sum dp h_W,   d b_out = sum dp,   dh_W = w_out dp,
 * then the LSTM's backward through time.  Unlike the register-resident pass of H <= 128 this one is three large
 * contractions with the global workspace between them, run over the batch in chunks of
 * fe_lstm_streamed_grad_chunk_pairs pairs in ascending order:
 *   1. the recurrence recomputed with the forward's contraction and operation order; per (step, pair) the activated
 *      gates, c_t and [h_{t-1} | x_t | 1] go to the workspace (the "stash");
 *   2. the head, d w_out and d b_out summed in pair order;
 *   3. for t = W-1 .. 0: dz_t elementwise, then dh_{t-1} = W_hh^T dz_t on v_mfma_f32_32x32x2_f32;
 *   4. [dW_hh | dW_x | db] = dz^T [h_{t-1} | x_t | 1] on v_mfma_f32_32x32x2_f32, summed in blocks: one accumulator chain
 *      per 1024 (step, pair) columns, chain sums and K splits added in a fixed order;
 *   5. the sums written in torch's row order; the first chunk overwrites the six buffers, later chunks add.
 * No float atomics: the same inputs give the same bits on every device.  Python front end:
 * FusedLSTMHead(env, module, streamed=True) in finenvs_amd/lstm_head.py.  Conventions as in finenvs_amd.h.
 *
 * Errors (FE_ERR_ARG, message beginning "fe_lstm_backward_streamed:"), checked in this order before any pointer is
 * touched: null pointers or a null field of fe_lstm_grads or count < 0, out_activation 1 (clamp), null outputs with
 * out_activation 0, H outside {256, 512, 1024} (fe_lstm_backward runs 32, 64 and 128), an env with A != 1.  No host
 * synchronisation and no allocation in any call; count = 0 does nothing.
 */
#ifndef FINENVS_AMD_LSTM_GRAD_STREAMED_H
#define FINENVS_AMD_LSTM_GRAD_STREAMED_H

#include "finenvs_amd.h"
#include "finenvs_amd_ext.h"
#include "finenvs_amd_lstm_grad.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Pairs one pass of fe_lstm_backward_streamed works on (-1 for H outside {256, 512, 1024} or W < 1).  The rule: the
 * stash is W (6H + 32) floats per pair; the chunk is the largest multiple of 256 pairs whose stash is at most 2 GiB,
 * and at least 256 pairs.  A function of (H, W) alone -- never of the device -- so the chunk boundaries, and with them
 * the bits of the gradients, are the same everywhere.  H = 1024, W = 4: 21 504 pairs.
 */
int64_t fe_lstm_streamed_grad_chunk_pairs(int32_t H, int32_t W);

/*
 * Floats of the workspace fe_lstm_backward_streamed needs for `count` pairs of an env with window W (-1 for H outside
 * {256, 512, 1024}, W < 1 or count < 0).  Monotone in count; it grows with the batch, by W (6H + 32) + 3H floats per
 * pair in steps of 32 pairs, up to the chunk and is constant from count >= chunk_pairs on.  The rest -- W_hh^T and the
 * K-split sums of the weight contraction, at most 32 / 16 / 4 of them at H = 256 / 512 / 1024 -- is bounded.
 */
int64_t fe_lstm_streamed_grad_workspace_floats(int32_t H, int32_t W, int64_t count);

/*
 * The backward of fe_lstm_forward at H in {256, 512, 1024}: the arguments of fe_lstm_backward, with whh fragment-major
 * as fe_lstm_forward reads it at these sizes.  outputs (count) as fe_lstm_forward returned them (may be null with
 * out_activation 2), d_outputs (count) f32.  grads: the six parameter gradients, all fields required, each summed over
 * the batch and OVERWRITTEN.  workspace: fe_lstm_streamed_grad_workspace_floats(H, W, count) floats of device memory,
 * 16-byte aligned.  All launches go on `stream`: one weight transpose, then per chunk the recurrence, the head, two per
 * time step, the weight contraction and the final write.
 */
int fe_lstm_backward_streamed(fe_env *env, const float *logret_f32, const float *whh, const float *wx, const float *wout,
                              int32_t H, int32_t out_activation, const int64_t *obs_src, const double *obs_pos,
                              int64_t count, const float *outputs, const float *d_outputs, float *workspace,
                              const fe_lstm_grads *grads, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FINENVS_AMD_LSTM_GRAD_STREAMED_H */
