/*
 * finenvs_amd_lstm_grad.h -- the gradient half of the one-output LSTM head (same library as finenvs_amd.h).
 *
 * Two of the reference's gradient learners train the plain LSTMNetwork((5, H, 1), W, output_activation)
 * (networks/lstm.py:28-57: nn.LSTM(5, H) over the window, last_layer = Linear(H, 1) on the last hidden state, then
 * the output activation):
 *   PPO  ContinuousActorLSTM (PPO/continuous_actor.py:104-124, Tanh) under compute_actor_loss
 *        (continuous_actor.py:59-78), and CriticLSTM (PPO/critic.py:53-68, Identity) under compute_critic_loss
 *        (critic.py:26-32);
 *   TD3  ActorLSTM (TD3/actor.py:83-94, Tanh) under compute_loss (TD3/actor.py:50-56).
 * fe_lstm_forward (finenvs_amd_ext.h) evaluates that head on observation descriptors; here is its backward, on the
 * same descriptors: one asset (A = 1), H in {32, 64, 128}, the env's W.
 *
 * With p = w_out . h_W + b_out, y = act(p) as fe_lstm_forward returned it and g = d_outputs:
 *   out_activation 0 (tanh)   dp = g (1 - y^2)
 *   out_activation 2 (none)   dp = g
 *   d w_out = sum dp h_W,   d b_out = sum dp,   dh_W = w_out dp,
 * then the LSTM's backward through time on the matrix cores, the recurrence recomputed with the forward's contraction
 * and operation order.  The input has no learnt column, so no per-pair gradient leaves the kernel.  Python front end:
 * FusedLSTMHead in finenvs_amd/lstm_head.py.  Conventions as in finenvs_amd.h.
 *
 * Errors (FE_ERR_ARG, message naming the function): null pointers, a null field of fe_lstm_grads, count < 0,
 * out_activation 1 (clamp: an action bound, not a trainable output), null outputs with out_activation 0, H outside
 * {32, 64, 128} (the streamed-weight forward of H >= 256 has no register-resident recurrence to mirror: those sizes
 * are fe_lstm_backward_streamed of finenvs_amd_lstm_grad_streamed.h), an env with A != 1.  No host synchronisation and no allocation in any call; count = 0 does nothing.
 */
#ifndef FINENVS_AMD_LSTM_GRAD_H
#define FINENVS_AMD_LSTM_GRAD_H

#include "finenvs_amd.h"
#include "finenvs_amd_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Device pointers of the head's six parameter gradients, f32, in torch's row order and layout (the reduction applies
 * the inverse of lstm_row_order of finenvs_amd/rollout.py while it writes: the buffers are the parameters' .grad as
 * they stand).  Each gradient is summed over the batch and OVERWRITES its buffer (accumulation into .grad is the
 * caller's). */
typedef struct fe_lstm_grads {
    float *w_ih;  /* (4H, 5) d lstm.weight_ih_l0 */
    float *w_hh;  /* (4H, H) d lstm.weight_hh_l0 */
    float *b_ih;  /* (4H) d lstm.bias_ih_l0 */
    float *b_hh;  /* (4H) d lstm.bias_hh_l0 (equal to b_ih) */
    float *w_out; /* (H) d last_layer[0].weight */
    float *b_out; /* (1) d last_layer[0].bias */
} fe_lstm_grads;

/*
 * Floats of the workspace fe_lstm_backward needs for `count` pairs of an env with window W (-1 for H outside
 * {32, 64, 128}, W < 1 or count < 0).  Monotone in count and bounded in it: the transposed weights do not depend on
 * the batch, and the partial sums and the per-workgroup activation stash are sized by the resident workgroup count.
 * The per-pair term is 0 floats: beyond 32 * the resident workgroup count the size does not grow.
 */
int64_t fe_lstm_grad_workspace_floats(int32_t H, int32_t W, int64_t count);

/*
 * The backward of fe_lstm_forward on the same arguments (env, logret_f32, the packed weights whh, wx, wout, H,
 * out_activation, obs_src, obs_pos, count), given outputs (count) as fe_lstm_forward returned them (may be null with
 * out_activation 2) and the upstream gradient d_outputs (count) f32.  b_out is not an argument: the gradient does not
 * depend on it.  grads: the six parameter gradients (see fe_lstm_grads), all fields required.  workspace:
 * fe_lstm_grad_workspace_floats(H, W, count) floats of device memory, 16-byte aligned.  Every workgroup writes its own
 * partial sums and a second kernel adds them in a fixed order: no float atomics, the same inputs give the same bits.
 * Three launches on `stream` (weight transpose, backward, reduction).
 */
int fe_lstm_backward(fe_env *env, const float *logret_f32, const float *whh, const float *wx, const float *wout,
                     int32_t H, int32_t out_activation, const int64_t *obs_src, const double *obs_pos, int64_t count,
                     const float *outputs, const float *d_outputs, float *workspace, const fe_lstm_grads *grads,
                     void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FINENVS_AMD_LSTM_GRAD_H */
