/*
 * finenvs_amd_critic_grad.h -- the gradient half of the twin LSTM critics (same library as finenvs_amd.h).
 *
 * The learner of the reference's off-policy agents differentiates its critics twice per update:
 *   - the critic loss, MSE(Q_c(s, a), y) per critic (SAC/critic.py:30-45 compute_loss and gradient_descent_step,
 *     TD3/critic.py:31-46), back to the critic's parameters;
 *   - the actor loss, through the critics to the action: -Q_1(s, mu(s)).mean() (TD3/actor.py compute_loss) or the
 *     SAC actor's min(Q_1, Q_2)(s, a~pi(s)) - alpha log pi (SAC actor loss), back to a = the actor's output.
 * Here both run on observation descriptors, as fe_twin_q_forward does (include/finenvs_amd_critic.h): one asset
 * (A = 1), nn.LSTM(6, H) over x_t = [4 log-returns of row t | position | action], H in {32, 64, 128}, the env's W.
 *
 * The forward: fe_twin_q_forward is the forward of this gradient.  fe_twin_q_backward recomputes its activations with
 * the same contraction and operation order (bit for bit the values fe_twin_q_forward returned), then runs the
 * backward pass through time on the matrix cores.  Python front end: FusedTwinCritic.q / critic_loss in
 * finenvs_amd/critic.py.  Conventions as in finenvs_amd.h.
 *
 * Errors (FE_ERR_ARG, message naming the function): null pointers, count < 0, H outside {32, 64, 128}, an env with
 * A != 1, a critic with dq but without its weights, or with neither its gradients nor d_actions.  No host
 * synchronisation and no allocation in any call; count = 0 does nothing.
 */
#ifndef FINENVS_AMD_CRITIC_GRAD_H
#define FINENVS_AMD_CRITIC_GRAD_H

#include "finenvs_amd.h"
#include "finenvs_amd_critic.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Device pointers of one critic's parameter gradients, f32, rows of the 4H-row tensors in the PACKED order of
 * fe_critic_weights (lstm_row_order in finenvs_amd/rollout.py: packed row R holds torch row gate * H + unit with
 * R = 32 mt + 8 b + 4 half + gate, unit = 8 mt + 4 half + b); columns in torch order.  Each gradient is summed over
 * the batch and OVERWRITES its buffer (accumulation into .grad is the caller's). */
typedef struct fe_critic_grads {
    float *w_ih;  /* (4H, 6) d lstm.weight_ih_l0 */
    float *w_hh;  /* (4H, H) d lstm.weight_hh_l0 */
    float *b_ih;  /* (4H) d lstm.bias_ih_l0 */
    float *b_hh;  /* (4H) d lstm.bias_hh_l0 (equal to b_ih) */
    float *w_out; /* (H) d last_layer[0].weight */
    float *b_out; /* (1) d last_layer[0].bias */
} fe_critic_grads;

/*
 * Floats of the workspace fe_twin_q_backward needs for `count` pairs of an env with window W (-1 for H outside
 * {32, 64, 128}, W < 1 or count < 0).  Bounded in count apart from 2 * count floats: the partial sums and the per-
 * workgroup activation stash are sized by the resident workgroup count, not by the batch.  Monotone in count.
 */
int64_t fe_twin_q_grad_workspace_floats(int32_t H, int32_t W, int64_t count);

/*
 * The backward of fe_twin_q_forward on the same arguments (env, logret_f32, c1, c2, H, obs_src, obs_pos, actions,
 * count; the env's W), given the upstream gradients dq1 / dq2 (count) f32 of q1 / q2 (SAC/critic.py:30-45 and
 * TD3/critic.py:31-46 for the critic loss; TD3/actor.py compute_loss and the SAC actor loss for d_actions):
 *   grads1 / grads2    the parameter gradients of critic 1 / 2, summed over the batch (see fe_critic_grads);
 *   d_actions (count)  sum over both critics and the W steps of w_ih[:, 5] . dz_t, or null (not computed).
 * dq1 == null: critic 1's half does not run (grads1 may be null and is not written), likewise dq2; TD3's actor loss
 * runs critic 1 only.  grads1 == null with dq1: critic 1's weights are frozen -- it adds to d_actions (then required)
 * and its weight-gradient contractions and reduction do not run; likewise grads2.  workspace:
 * fe_twin_q_grad_workspace_floats(H, W, count) floats of device memory.  Every workgroup writes its own partial sums
 * and a second kernel adds them in a fixed order: no float atomics, the same inputs give the same bits.  Three
 * launches on `stream`.
 */
int fe_twin_q_backward(fe_env *env, const float *logret_f32, const fe_critic_weights *c1, const fe_critic_weights *c2,
                       int32_t H, const int64_t *obs_src, const double *obs_pos, const float *actions, int64_t count,
                       const float *dq1, const float *dq2, float *workspace, const fe_critic_grads *grads1,
                       const fe_critic_grads *grads2, float *d_actions, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FINENVS_AMD_CRITIC_GRAD_H */
