/*
 * finenvs_amd_sac_streamed.h -- the SAC LSTM actor at H = 256 / 512 / 1024: acting, the forward on observation
 * descriptors and the backward pass (same library as finenvs_amd.h; the small sizes are finenvs_amd_sac.h and
 * finenvs_amd_sac_grad.h).
 *
 * The reference's SAC agent is SACAgentLSTM(env_args, hidden_dim=1024) (its isaac_gym example SAC_LSTM_Isaac_Gym.py:16).
 * At these sizes the recurrent weights do not fit a workgroup's registers: they stream from L2, fragment-major, as
 * fe_env_rollout_lstm (finenvs_amd_ext.h) reads them there, and so does the last layer's weight, which finenvs_amd_sac.h
 * already stores fragment-major.  The head is the one of finenvs_amd_sac.h with the same operation order:
 *   z = W_l h_W + b_l (one accumulator chain from zero per 32-unit row tile, k groups ascending, b_l added afterwards),
 *   mu = w_mu . z + b_mu,  s = softplus(w_s . z + b_s) (from the bias, units ascending, fmaf),  u = mu + eps s,
 *   action = tanh(u),  log_prob = Normal(mu, s).log_prob(u) - log(1 - tanh(u)^2 + 1e-7).
 * The backward is the chunked pass of finenvs_amd_lstm_grad_streamed.h with the head of finenvs_amd_sac_grad.h (its
 * formulas, its operation order) between the recomputed recurrence and the loop over the time steps; the chunks are
 * fe_lstm_streamed_grad_chunk_pairs(H, W) pairs, the one-output head's boundaries.
 *
 * Every entry: H in {256, 512, 1024}; whh FRAGMENT-MAJOR ([row tile][k group][lane][4], lstm_fragment_major in
 * finenvs_amd/rollout.py), wx (4H, 8) in packed row order, wl / bl / wmu / wstd as in finenvs_amd_sac.h; the two output
 * biases bmu / bstd are (1) f32 each in DEVICE memory (the only form here: no copy to the host, as in the *_p entries
 * of finenvs_amd_optim.h).  Acting and the forward run any A the env has and the fused kernel at every count: there is
 * no split-by-time-step form (fe_env_rollout_lstm_split) for SAC, so below a few thousand pairs one CU walks the whole
 * matrix.  No host synchronisation and no allocation in any call.  Python front end: FusedSACRollout(env, actor,
 * streamed=True) in finenvs_amd/sac.py.  Conventions as in finenvs_amd.h.
 *
 * Errors (FE_ERR_ARG, message beginning with the function's name), checked in this order before any pointer is touched:
 * null pointers, K < 1 or count < 0 (and the argument pairings of the small entries); H outside {256, 512, 1024} (the
 * message names the entry of finenvs_amd_sac.h / finenvs_amd_sac_grad.h that runs 32, 64 and 128); in
 * fe_sac_backward_streamed an env with A != 1.
 */
#ifndef FINENVS_AMD_SAC_STREAMED_H
#define FINENVS_AMD_SAC_STREAMED_H

#include "finenvs_amd.h"
#include "finenvs_amd_sac.h"
#include "finenvs_amd_sac_grad.h"
#include "finenvs_amd_lstm_grad_streamed.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fe_env_rollout_sac at these sizes (SAC_agent.py:110-121, the loop agent.step -> env.step): the arguments of
 * fe_env_rollout_sac_p (finenvs_amd_optim.h), the same outputs, accounting and trajectory descriptors. */
int fe_env_rollout_sac_streamed(fe_env *env, const float *logret_f32, const float *whh, const float *wx, const float *wl,
                                const float *bl, const float *wmu, const float *bmu, const float *wstd, const float *bstd,
                                int32_t H, int32_t K, int64_t *obs_src, double *obs_pos, const float *noise,
                                float *actions_out, float *means_out, float *stds_out, double *rewards_out,
                                int32_t *dones_out, int64_t *states_src_out, double *states_pos_out, void *stream);

/* fe_sac_forward at these sizes (the no-grad actor half of SAC_agent.py:200-225, and SAC/actor.py:51-61): the arguments
 * of fe_sac_forward_p, the same meaning; count = 0 does nothing. */
int fe_sac_forward_streamed(fe_env *env, const float *logret_f32, const float *whh, const float *wx, const float *wl,
                            const float *bl, const float *wmu, const float *bmu, const float *wstd, const float *bstd,
                            int32_t H, const int64_t *obs_src, const double *obs_pos, int64_t count, const float *noise,
                            float *actions_out, float *log_probs_out, float *means_out, float *stds_out, void *stream);

/*
 * Floats of the workspace fe_sac_backward_streamed needs for `count` pairs of an env with window W (-1 for H outside
 * {256, 512, 1024}, W < 1 or count < 0).  Monotone in count and constant from count >=
 * fe_lstm_streamed_grad_chunk_pairs(H, W) on: fe_lstm_streamed_grad_workspace_floats(H, W, count) plus W_l^T, the split
 * sums of d W_l, the head's block sums and z and dz of one pass.
 */
int64_t fe_sac_streamed_grad_workspace_floats(int32_t H, int32_t W, int64_t count);

/*
 * The backward of fe_sac_forward_streamed (SAC/actor.py:63-81 descends through it) on the same arguments, given actions
 * and stds (count) as the forward returned them and the upstream gradients d_actions / d_log_probs (count) f32; either
 * may be null, not both.  One asset (A = 1).  Writes the ten gradients of fe_sac_grads (finenvs_amd_sac_grad.h) in
 * torch's row order and layout, each summed over the batch and overwritten: the first chunk overwrites, later chunks
 * add.  With d_log_probs null, W_l = I, b_l = 0 and w_std = 0 the LSTM's four tensors, w_mu and b_mu equal
 * fe_lstm_backward_streamed's (out_activation 0, w_out = w_mu) bit for bit.  bmu is accepted for symmetry; the gradient
 * does not depend on it.  workspace: fe_sac_streamed_grad_workspace_floats(H, W, count) floats of device memory,
 * 16-byte aligned.  count = 0 does nothing.  No float atomics: the same inputs give the same bits.
 */
int fe_sac_backward_streamed(fe_env *env, const float *logret_f32, const float *whh, const float *wx, const float *wl,
                             const float *bl, const float *wmu, const float *bmu, const float *wstd, const float *bstd,
                             int32_t H, const int64_t *obs_src, const double *obs_pos, int64_t count, const float *noise,
                             const float *actions, const float *stds, const float *d_actions, const float *d_log_probs,
                             float *workspace, const fe_sac_grads *grads, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FINENVS_AMD_SAC_STREAMED_H */
