/*
 * finenvs_amd_critic_streamed.h -- the twin LSTM critics of SAC and TD3 at H = 256 / 512 / 1024: values, Bellman
 * targets and the backward pass on observation descriptors (same library as finenvs_amd.h; the small sizes are
 * finenvs_amd_critic.h and finenvs_amd_critic_grad.h).
 *
 * The reference runs its off-policy LSTM agents at hidden_dim = 1024.  At these sizes the recurrent weights do not fit a
 * workgroup's registers: they stream from L2, fragment-major, as fe_lstm_forward (finenvs_amd_ext.h) reads them, and the
 * backward pass is the chunked one of finenvs_amd_lstm_grad_streamed.h with one more input -- the action, constant
 * over the window, in input slot 6 -- and one more gradient, dQ/da.  The stash row [h_{t-1} | x_t | 1 | action | 0 ...]
 * keeps its 32 input columns, so fe_lstm_streamed_grad_chunk_pairs(H, W) is the chunk here too.
 *
 * Every entry: H in {256, 512, 1024}; one asset (A = 1); weights an fe_critic_weights with whh FRAGMENT-MAJOR
 * ([row tile][k group][lane][4], lstm_fragment_major in finenvs_amd/rollout.py) and wx (4H, 8) in packed row order with
 * slot 5 = b_ih + b_hh and slot 6 = w_ih[:, 5].  The two critics run one after the other on `stream`.  No host
 * synchronisation and no allocation in any call; count = 0 does nothing.  Python front end:
 * FusedTwinCritic(env, c1, c2, streamed=True) in finenvs_amd/critic.py.  Conventions as in finenvs_amd.h.
 *
 * Errors (FE_ERR_ARG, message naming the function), checked before any pointer is touched: null pointers or count < 0,
 * log_probs without alpha, smooth_noise together with log_probs, H outside {256, 512, 1024} (the entries of
 * finenvs_amd_critic.h / finenvs_amd_critic_grad.h run 32, 64 and 128), an env with A != 1, a bad ring / head / size; in
 * fe_twin_q_backward_streamed a critic with dq but without its weights, or with neither its gradients nor d_actions.
 */
#ifndef FINENVS_AMD_CRITIC_STREAMED_H
#define FINENVS_AMD_CRITIC_STREAMED_H

#include "finenvs_amd.h"
#include "finenvs_amd_critic.h"
#include "finenvs_amd_critic_grad.h"
#include "finenvs_amd_lstm_grad_streamed.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fe_twin_q_forward at these sizes: the same arguments, the same meaning.  With w_ih[:, 5] = 0 a critic's value equals
 * fe_lstm_forward's (out_activation 2) on the same weights bit for bit. */
int fe_twin_q_forward_streamed(fe_env *env, const float *logret_f32, const fe_critic_weights *c1,
                               const fe_critic_weights *c2, int32_t H, const int64_t *obs_src, const double *obs_pos,
                               const float *actions, int64_t count, float *q1_out, float *q2_out, void *stream);

/* fe_twin_q_target at these sizes: the same arguments, the same meaning, the same epilogue kernel.  The next-state
 * descriptors come from the ring by logical index, TD3's smoothing is applied as the action is loaded; an index outside
 * [0, size) reads nothing of the ring, gives NaN in targets_out, q1_out and q2_out and counts in ring->errors[0]. */
int fe_twin_q_target_streamed(fe_env *env, const float *logret_f32, const fe_critic_weights *c1,
                              const fe_critic_weights *c2, int32_t H, const fe_replay_ring *ring, int64_t head,
                              int64_t size, const int64_t *indices, int64_t count, const float *next_actions,
                              const float *smooth_noise, float smooth_std, float smooth_clip, const float *log_probs,
                              const float *alpha, float gamma, float reward_scale, float *targets_out, float *q1_out,
                              float *q2_out, void *stream);

/* fe_twin_q_target_c (finenvs_amd_replay_cursor.h) at these sizes: head and size are read from the ring's cursor on the
 * device. */
int fe_twin_q_target_streamed_c(fe_env *env, const float *logret_f32, const fe_critic_weights *c1,
                                const fe_critic_weights *c2, int32_t H, const fe_replay_ring *ring, const int64_t *cursor,
                                const int64_t *indices, int64_t count, const float *next_actions,
                                const float *smooth_noise, float smooth_std, float smooth_clip, const float *log_probs,
                                const float *alpha, float gamma, float reward_scale, float *targets_out, float *q1_out,
                                float *q2_out, void *stream);

/*
 * Floats of the workspace fe_twin_q_backward_streamed needs for `count` pairs of an env with window W (-1 for H outside
 * {256, 512, 1024}, W < 1 or count < 0).  Monotone in count and constant from count >=
 * fe_lstm_streamed_grad_chunk_pairs(H, W) on: d_actions is written in place and needs nothing per pair.  The two
 * critics use the same workspace one after the other -- the stash of up to 2 GiB is not doubled -- so this is
 * fe_lstm_streamed_grad_workspace_floats(H, W, count).
 */
int64_t fe_twin_q_streamed_grad_workspace_floats(int32_t H, int32_t W, int64_t count);

/*
 * The backward of fe_twin_q_forward_streamed on the same arguments, given the upstream gradients dq1 / dq2 (count) f32.
 * The null-pointer rules are fe_twin_q_backward's: dq_c == null -- critic c does not run; grads_c == null with dq_c --
 * critic c is frozen, it contributes to d_actions (then required) only and its weight contraction and final write are
 * not launched.  Unlike fe_twin_q_backward the fe_critic_grads buffers are written in TORCH's row order and layout
 * (w_ih (4H, 6), w_hh (4H, H), b_ih = b_hh (4H), w_out (H), b_out (1)), each summed over the batch and overwritten: the
 * first chunk overwrites, later chunks add.  d_actions (count), or null: the sum over the W steps of w_ih[:, 5] . dz_t,
 * critic 1 first, then critic 2 added; zero if neither critic runs.  workspace:
 * fe_twin_q_streamed_grad_workspace_floats(H, W, count) floats of device memory, 16-byte aligned.  No float atomics:
 * the same inputs give the same bits.
 */
int fe_twin_q_backward_streamed(fe_env *env, const float *logret_f32, const fe_critic_weights *c1,
                                const fe_critic_weights *c2, int32_t H, const int64_t *obs_src, const double *obs_pos,
                                const float *actions, int64_t count, const float *dq1, const float *dq2,
                                float *workspace, const fe_critic_grads *grads1, const fe_critic_grads *grads2,
                                float *d_actions, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FINENVS_AMD_CRITIC_STREAMED_H */
