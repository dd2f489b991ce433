/*
 * finenvs_amd_sac.h -- the SAC actor's head on the fused LSTM rollout (same library as finenvs_amd.h).
 *
 * The reference's SACAgentLSTM acts with finenvs/agents/SAC/actor.py:ActorLSTM: nn.LSTM(5, H) over the observation
 * window, Linear(H, H) on the last hidden state (LSTMNetwork duplicates the last size of the shape (5, H)), then
 * mu_layer and std_layer, both Linear(H, 1) here (one output per (env, asset) pair, like the other fused heads):
 *
 *   z = W_l h_W + b_l,   mu = w_mu . z + b_mu,   s = softplus(w_s . z + b_s)   (torch's rule: x > 20 ? x : log1p(exp(x)))
 *   with noise eps:  u = mu + eps * s,  action = tanh(u),
 *                    log_prob = Normal(mu, s).log_prob(u) - log(1 - tanh(u)^2 + 1e-7)
 *
 * The recurrence is fe_env_rollout_lstm's (register-resident weights, gate contractions on the matrix cores, the same
 * packed whh / wx), z another contraction on the matrix cores.  Python front end: finenvs_amd/sac.py.  Conventions as
 * in finenvs_amd.h.
 *
 * Weights (f32, device): whh (4H, H) and wx (4H, 8) packed as for fe_env_rollout_lstm; wl (H / 32, H / 8, 64, 4) the
 * last layer's weight fragment-major: element [t][g][r + 32 h][m] = W_l[32 t + r][8 g + 4 h + m]; bl, wmu, wstd (H).
 * H in {32, 64, 128}; anything else is refused (FE_ERR_ARG).
 */
#ifndef FINENVS_AMD_SAC_H
#define FINENVS_AMD_SAC_H

#include "finenvs_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * K env steps with the SAC actor in the kernel (SAC_agent.py:110-121, the loop agent.step -> env.step).  noise
 * (K, N, A) f32 standard normals or null.  With noise every env acts with tanh(u) except the env's evaluation env,
 * which acts on mu (an evaluate-mode env has none: there every env samples); without noise every env acts on mu.  The
 * env scales, rounds and clamps the action as env.step does.  Optional outputs (null = not written): actions_out,
 * means_out (mu), stds_out (s), each (K, N, A) f32; states_src_out (K + 1, N) / states_pos_out (K + 1, N, A) the
 * descriptors of the state every step's policy sees, plus the last one (go together).  Accounting, side effects and the
 * in/out descriptors obs_src / obs_pos as fe_env_rollout_lstm.
 */
int fe_env_rollout_sac(fe_env *env, const float *logret_f32, const float *whh, const float *wx, const float *wl,
                       const float *bl, const float *wmu, float bmu, const float *wstd, float bstd, int32_t H, int32_t K,
                       int64_t *obs_src, double *obs_pos, const float *noise, float *actions_out, float *means_out,
                       float *stds_out, double *rewards_out, int32_t *dones_out, int64_t *states_src_out,
                       double *states_pos_out, void *stream);

/*
 * The head on `count` observation descriptors (obs_src (count), obs_pos (count, A)) without stepping the env: the
 * no-grad actor half of SAC_agent.py:200-225 (compute_targets) on replayed states.  Outputs (count, A) f32, null = not
 * written: means_out (mu), stds_out (s) and, with noise (count, A), actions_out (tanh(u)) and log_probs_out.  Every
 * descriptor samples (there is no evaluation env here).  actions_out / log_probs_out without noise: FE_ERR_ARG.
 */
int fe_sac_forward(fe_env *env, const float *logret_f32, const float *whh, const float *wx, const float *wl, const float *bl,
                   const float *wmu, float bmu, const float *wstd, float bstd, int32_t H, const int64_t *obs_src,
                   const double *obs_pos, int64_t count, const float *noise, float *actions_out, float *log_probs_out,
                   float *means_out, float *stds_out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FINENVS_AMD_SAC_H */
