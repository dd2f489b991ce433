/*
 * finenvs_amd_sac_grad.h -- the gradient half of the SAC LSTM actor (same library as finenvs_amd.h).
 *
 * The reference's SAC learner differentiates its actor once per update: Actor.compute_losses (SAC/actor.py:63-81)
 * samples actions and log-probabilities from the current policy on the mini-batch's states
 * (get_actions_and_log_probs, SAC/actor.py:51-61), takes min(Q_1, Q_2) of them and descends
 * -(q - alpha * log_prob).mean() back to the actor's parameters: nn.LSTM(5, H) over the window, last_layer =
 * Linear(H, H) on the last hidden state (networks/lstm.py:21-23, 28-57), mu_layer and std_layer = Linear(H, 1).
 * Here that backward runs on observation descriptors, as fe_sac_forward does (include/finenvs_amd_sac.h): one asset
 * (A = 1), H in {32, 64, 128}, the env's W.
 *
 * The forward: fe_sac_forward is the forward of this gradient,
 *   z = W_l h_W + b_l,  mu = w_mu . z + b_mu,  s = softplus(q), q = w_s . z + b_s,  u = mu + eps s,  a = tanh(u),
 *   log_prob = Normal(mu, s).log_prob(u) - log(1 - a^2 + 1e-7)                                (SAC/actor.py:51-61).
 * fe_sac_backward recomputes the recurrence with the same contraction and operation order, takes a and s as
 * fe_sac_forward returned them, and with ga = d_actions, gl = d_log_probs forms
 *   du = ga (1 - a^2) + gl 2 a (1 - a^2) / (1 - a^2 + 1e-7),   dmu = du,   ds = du eps - gl / s
 * (the Normal log-density's (u - mu) terms cancel between the u and the mu path and leave -gl / s on s),
 *   dq = ds sigmoid(q) (1 where q > 20, F.softplus's threshold),   dz = w_mu dmu + w_s dq,
 * then the last layer's and the LSTM's backward through time on the matrix cores.  Python front end:
 * FusedSACRollout.sample / actor_losses in finenvs_amd/sac.py.  Conventions as in finenvs_amd.h.
 *
 * Errors (FE_ERR_ARG, message naming the function): null pointers, a null field of fe_sac_grads, count < 0, both
 * upstream gradients null, H outside {32, 64, 128}, an env with A != 1 (the only fused consumer of the SAC actor loss
 * is the twin critic, which is A = 1).  No host synchronisation and no allocation in any call; count = 0 does nothing.
 */
#ifndef FINENVS_AMD_SAC_GRAD_H
#define FINENVS_AMD_SAC_GRAD_H

#include "finenvs_amd.h"
#include "finenvs_amd_sac.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Device pointers of the actor's ten parameter gradients, f32, in torch's row order and layout (the reduction applies
 * the inverse of lstm_row_order of finenvs_amd/rollout.py while it writes: the buffers are the parameters' .grad as
 * they stand).  Each gradient is summed over the batch and OVERWRITES its buffer (accumulation into .grad is the
 * caller's). */
typedef struct fe_sac_grads {
    float *w_ih;  /* (4H, 5) d lstm.weight_ih_l0 */
    float *w_hh;  /* (4H, H) d lstm.weight_hh_l0 */
    float *b_ih;  /* (4H) d lstm.bias_ih_l0 */
    float *b_hh;  /* (4H) d lstm.bias_hh_l0 (equal to b_ih) */
    float *w_l;   /* (H, H) d last_layer[0].weight, [out][in] */
    float *b_l;   /* (H) d last_layer[0].bias */
    float *w_mu;  /* (H) d mu_layer.weight */
    float *b_mu;  /* (1) d mu_layer.bias */
    float *w_std; /* (H) d std_layer.weight */
    float *b_std; /* (1) d std_layer.bias */
} fe_sac_grads;

/*
 * Floats of the workspace fe_sac_backward needs for `count` pairs of an env with window W (-1 for H outside
 * {32, 64, 128}, W < 1 or count < 0).  Monotone in count and bounded in it: the transposed weights do not depend on
 * the batch, and the partial sums and the per-workgroup activation stash are sized by the resident workgroup count.
 * The per-pair term is 0 floats (the actor's input has no learnt column, so no per-pair gradient leaves the kernel):
 * beyond 32 * the resident workgroup count the size does not grow.
 */
int64_t fe_sac_grad_workspace_floats(int32_t H, int32_t W, int64_t count);

/*
 * The backward of fe_sac_forward on the same arguments (env, logret_f32, the packed weights whh, wx, wl, bl, wmu, bmu,
 * wstd, bstd, H, obs_src, obs_pos, count, noise), given actions and stds (count) as fe_sac_forward returned them and
 * the upstream gradients d_actions / d_log_probs (count) f32 of its actions / log_probs outputs; either may be null
 * (an output nobody used), not both.  grads: the ten parameter gradients (see fe_sac_grads), all fields required.
 * bmu is accepted for symmetry with fe_sac_forward; the gradient does not depend on it.  workspace:
 * fe_sac_grad_workspace_floats(H, W, count) floats of device memory, 16-byte aligned.  Every workgroup writes its own
 * partial sums and a second kernel adds them in a fixed order: no float atomics, the same inputs give the same bits.
 * Three launches on `stream` (weight transposes, backward, reduction).
 */
int fe_sac_backward(fe_env *env, const float *logret_f32, const float *whh, const float *wx, const float *wl,
                    const float *bl, const float *wmu, float bmu, const float *wstd, float bstd, int32_t H,
                    const int64_t *obs_src, const double *obs_pos, int64_t count, const float *noise,
                    const float *actions, const float *stds, const float *d_actions, const float *d_log_probs,
                    float *workspace, const fe_sac_grads *grads, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FINENVS_AMD_SAC_GRAD_H */
