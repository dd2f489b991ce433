/*
 * finenvs_amd_critic.h -- the twin LSTM critics of SAC and TD3 and their Bellman targets (same library as finenvs_amd.h).
 *
 * The reference's off-policy agents value a (state, action) pair with CriticLSTM((5A + A, H, 1), W)
 * (finenvs/agents/SAC/critic.py, networks/lstm.py:28-57): nn.LSTM(5A + A, H) over [state row | action] -- the action
 * repeated over the W rows (agent_utils.py:5-14) -- and Linear(H, 1) + Identity on the last hidden state.  Here one
 * asset (A = 1): the critic is nn.LSTM(6, H), evaluated per observation descriptor on the register-resident recurrence of
 * fe_env_rollout_lstm (gate contractions on the matrix cores); the action takes input slot 6 of the packed wx.  For
 * A > 1 the reference's critic reads the whole env's window at once, which is not a per-(env, asset) pair network:
 * refused.  Python front end: finenvs_amd/critic.py.  Conventions as in finenvs_amd.h.
 *
 * Weights (f32, device): whh (4H, H) and wx (4H, 8) packed as for fe_env_rollout_lstm, with wx[:, 6] = the packed rows of
 * w_ih[:, 5] (the action's input weight); wout (H) and bout (1) the output layer.  H in {32, 64, 128}.
 *
 * Errors (FE_ERR_ARG, message naming the function): null pointers, count < 0, H outside {32, 64, 128}, an env with
 * A != 1, log_probs without alpha, smooth_noise together with log_probs; fe_twin_q_target also a bad ring / head / size.
 * No host synchronisation and no allocation in either call.
 */
#ifndef FINENVS_AMD_CRITIC_H
#define FINENVS_AMD_CRITIC_H

#include "finenvs_amd.h"
#include "finenvs_amd_replay.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fe_critic_weights {
    const float *whh;  /* (4H, H) packed row order */
    const float *wx;   /* (4H, 8): w_ih[:, 0..4] | b_ih + b_hh | w_ih[:, 5] | 0, packed row order */
    const float *wout; /* (H) */
    const float *bout; /* (1), device memory */
} fe_critic_weights;

/*
 * Both critics' values on `count` (state, action) pairs: obs_src (count) / obs_pos (count) observation descriptors, actions
 * (count) f32.  q1_out / q2_out (count) f32: Critic.forward(cat([states, actions repeated over W], dim=2)) of
 * SAC/critic.py:36-38 (compute_loss up to the loss), for critic 1 and critic 2.  Equal to the torch critic on the
 * rendered .float() observations within fp32 rounding.
 */
int fe_twin_q_forward(fe_env *env, const float *logret_f32, const fe_critic_weights *c1, const fe_critic_weights *c2,
                      int32_t H, const int64_t *obs_src, const double *obs_pos, const float *actions, int64_t count,
                      float *q1_out, float *q2_out, void *stream);

/*
 * The target critics' half of compute_targets on a replayed mini-batch, straight from the ring (fe_replay_sample's
 * slot map and out-of-range rule): for the `count` logical indices, the next-state descriptors of the ring, the next
 * actions next_actions (count) f32 (the actor's, computed by the caller on those descriptors), then
 *   SAC (log_probs != null; SAC_agent.py:200-227):
 *     y = r + gamma * (1 - d) * (min(q1, q2) + (-alpha * log_probs))
 *   TD3 (log_probs == null; TD3_agent.py:231-251, smooth_noise (count) standard normals or null):
 *     a = clamp(a + clamp(smooth_noise * smooth_std, -smooth_clip, smooth_clip), -1, 1) before the critics,
 *     y = r + gamma * (1 - d) * min(q1, q2)
 * with r = the ring's reward * reward_scale (1 = the reference) and d the ring's done, every operation one f32 rounding
 * in that order.  alpha (1) lives on the device.  targets_out, q1_out and q2_out (count) f32 (the critics' values are
 * written on the way).  An index outside [0, size) reads nothing of the ring: its outputs are NaN and it counts in
 * ring->errors[0].
 */
int fe_twin_q_target(fe_env *env, const float *logret_f32, const fe_critic_weights *c1, const fe_critic_weights *c2,
                     int32_t H, const fe_replay_ring *ring, int64_t head, int64_t size, const int64_t *indices,
                     int64_t count, const float *next_actions, const float *smooth_noise, float smooth_std,
                     float smooth_clip, const float *log_probs, const float *alpha, float gamma, float reward_scale,
                     float *targets_out, float *q1_out, float *q2_out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FINENVS_AMD_CRITIC_H */
