/*
 * finenvs_amd_mlp_critic.h -- the twin MLP critics Q(s, a) of TD3 and SAC on observation descriptors (same library as
 * finenvs_amd.h).
 *
 * The reference's MLP agents of the off-policy family train CriticMLP((5W + 1, H, H, 1)) (TD3/critic.py:49-64,
 * SAC/critic.py:48-58; TD3AgentMLP builds two of them and two targets with hidden_dims = (128, 128)): an
 * MLPNetwork on cat([states.float().flatten(1), actions], dim=1) (agent_utils.py:5-14 with 2-D states: concat_dim 1), so
 * the action is input column 5W.  Here, for one asset (A = 1), both hidden layers of width H in {32, 64, 128}, both with
 * the same activation (0 ELU alpha 1, 1 ReLU, 2 tanh), the output the identity:
 *   z1 = [the fmaf / MFMA chain of fe_mlp2_forward's first layer on network.0.weight[:, :5W], wpos, b1]
 *   z1 = fmaf(a, wact[h], z1)            wact = network.0.weight[:, 5W]: one more fmaf, after the chain
 *   a1 = act(z1);  z2 = b2 + W2 a1;  a2 = act(z2);  q = b3 + w3 . a2
 * With a = 0, or with wact = 0, q equals fe_mlp2_forward(out_activation 2) on the same weights bit for bit
 * (include/finenvs_amd_mlp2_head.h).  No observation is written to memory by any entry.  Python front end: MLPCritic and
 * FusedTwinMLPCritic in finenvs_amd/mlp_critic.py.  Conventions as in finenvs_amd.h.
 *
 * The weight image in LDS is the two-layer head's plus H floats for wact; the admission rule is fe_mlp2_*'s (the head's
 * image next to a rollout tile of 128 pairs must fit the 160 KiB LDS: FE_MLP2_MAX_WINDOW_*), so every (H, W) those
 * entries admit runs here too: at H = 128, W = 40 the image is 154 112 bytes.  The two H = 128 images do not fit one
 * workgroup together: the forward and target launches run critic c in the workgroups of blockIdx.y = c.
 *
 * Errors (FE_ERR_ARG, message naming the function): null pointers or a null struct field, H outside {32, 64, 128}, an
 * activation outside 0..2, count < 0, an env with A != 1, a window that does not fit ("does not fit"); for the backward
 * also a dq without its weights and a critic with neither its gradients nor d_actions.  No float atomics: every sum has a
 * fixed order that depends on (H, W, count) only, so the same inputs give the same bits.  No host synchronisation and
 * no allocation in any call; count = 0 does nothing; every launch goes on `stream` and can be captured into a graph.
 */
#ifndef FINENVS_AMD_MLP_CRITIC_H
#define FINENVS_AMD_MLP_CRITIC_H

#include "finenvs_amd.h"
#include "finenvs_amd_replay.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Pairs per split of the backward's two weight-gradient contractions (= FE_MLP2_GRAD_CHUNK_PAIRS). */
#define FE_MLPQ_GRAD_CHUNK_PAIRS 512

/* Device pointers of one critic (TD3/critic.py:49-64), f32. */
typedef struct fe_mlpq_weights {
    const float *w1t;  /* (H, 4W) as fe_mlp_pack writes it from a contiguous copy of network.0.weight[:, :5W] */
    const float *wpos; /* (H) as fe_mlp_pack writes it */
    const float *wact; /* (H) network.0.weight[:, 5W]: the action's input weight */
    const float *b1;   /* (H) network.0.bias */
    const float *w2;   /* (H, H) network.2.weight, row-major as torch holds it */
    const float *b2;   /* (H) network.2.bias */
    const float *w3;   /* (H) network.4.weight */
    const float *b3;   /* (1) network.4.bias */
} fe_mlpq_weights;

/* Device pointers of one critic's six parameter gradients, f32, in torch's layout.  Each gradient is summed over the
 * batch and OVERWRITES its buffer (accumulation into .grad is the caller's). */
typedef struct fe_mlpq_grads {
    float *w1; /* (H, 5W + 1) d network.0.weight: the position column written to every window row, the action's in column 5W */
    float *b1; /* (H) d network.0.bias */
    float *w2; /* (H, H) d network.2.weight */
    float *b2; /* (H) d network.2.bias */
    float *w3; /* (H) d network.4.weight */
    float *b3; /* (1) d network.4.bias */
} fe_mlpq_grads;

/*
 * Both critics on `count` (state, action) pairs (TD3/critic.py:55-64 forward, twice): obs_src (count) int64 / obs_pos
 * (count) f64 observation descriptors, actions (count) f32 -> q1_out, q2_out (count) f32.  The env's state is neither
 * read nor written; the env supplies W, A and the device.  One launch, critic c in blockIdx.y = c.
 */
int fe_twin_mlpq_forward(fe_env *env, const float *logret_f32, const fe_mlpq_weights *c1, const fe_mlpq_weights *c2,
                         int32_t H, int32_t activation, const int64_t *obs_src, const double *obs_pos,
                         const float *actions, int64_t count, float *q1_out, float *q2_out, void *stream);

/*
 * The Bellman targets of TD3Agent.compute_targets (TD3_agent.py:231-251) and SACAgent.compute_targets
 * (SAC_agent.py:200-227) with MLP critics, for the transitions `indices` (count, logical: slot (head - size + i) mod C)
 * of the ring: the argument list and semantics of fe_twin_q_target (include/finenvs_amd_critic.h).  The next states'
 * descriptors, the reward and the done flag come from the ring; next_actions (count) are the target actor's actions
 * there.  smooth_noise (count) non-null: TD3's smoothing a = clamp(a + clamp(noise * smooth_std, -smooth_clip,
 * smooth_clip), -1, 1) before the critics.  Then
 *   y = r reward_scale + (gamma (1 - d)) min(q1, q2)                            (log_probs null: TD3)
 *   y = r reward_scale + (gamma (1 - d)) (min(q1, q2) + (-alpha) log_probs)      (log_probs (count) and alpha (1): SAC)
 * one f32 rounding per operation, in that order.  q1_out / q2_out (count) receive the critics' values.  An index
 * outside [0, size) reads nothing of the ring: its outputs are NaN and it counts in ring->errors[0].  Two launches.
 * Also FE_ERR_ARG: log_probs without alpha, smooth_noise with log_probs, a head / size that describe no sample, a ring
 * of more than one asset.
 */
int fe_twin_mlpq_target(fe_env *env, const float *logret_f32, const fe_mlpq_weights *c1, const fe_mlpq_weights *c2,
                        int32_t H, int32_t activation, const fe_replay_ring *ring, int64_t head, int64_t size,
                        const int64_t *indices, int64_t count, const float *next_actions, const float *smooth_noise,
                        float smooth_std, float smooth_clip, const float *log_probs, const float *alpha, float gamma,
                        float reward_scale, float *targets_out, float *q1_out, float *q2_out, void *stream);

/* fe_twin_mlpq_target with head and size read on the device from the ring's cursor (an int64[4]: head, size, ...;
 * include/finenvs_amd_replay_cursor.h), as fe_twin_q_target_c: capturable across appends.  FE_ERR_ARG for a null cursor. */
int fe_twin_mlpq_target_c(fe_env *env, const float *logret_f32, const fe_mlpq_weights *c1, const fe_mlpq_weights *c2,
                          int32_t H, int32_t activation, const fe_replay_ring *ring, const int64_t *cursor,
                          const int64_t *indices, int64_t count, const float *next_actions, const float *smooth_noise,
                          float smooth_std, float smooth_clip, const float *log_probs, const float *alpha, float gamma,
                          float reward_scale, float *targets_out, float *q1_out, float *q2_out, void *stream);

/*
 * Floats of the workspace fe_twin_mlpq_backward needs for `count` pairs of an env with window W (-1 for H outside
 * {32, 64, 128}, W < 1 or count < 0; 0 for count = 0).  The two critics run one after the other and share it.  With
 *   blocks = ceil(count / 32),  splits = ceil(count / FE_MLPQ_GRAD_CHUNK_PAIRS),  F = 32 ceil((4W + 3) / 32),
 *   waves  = 4 min(ceil(blocks / 4), 512)
 * it is
 *   3 * 32 blocks H   +   splits H (F + H + 32)   +   waves (H + 4)
 * floats: three H-float rows per pair (dz1, a1, dz2), per split one H x F partial of [dW1t | d wpos | d wact | d b1] and
 * one H x (H + 32) partial of [dW2 | d b2], and one partial of d w3 / d b3 per wavefront of the first kernel.  (It
 * equals fe_mlp2_grad_workspace_floats(H, W, count): 4W + 2 is never a multiple of 32, so the action's column opens no
 * feature tile.)
 */
int64_t fe_twin_mlpq_grad_workspace_floats(int32_t H, int32_t W, int64_t count);

/*
 * The backward of fe_twin_mlpq_forward on the same arguments, given the upstream gradients dq1 / dq2 (count) f32 of
 * q1 / q2 (TD3/critic.py:31-46 compute_loss for the critic loss; TD3/actor.py compute_loss and the SAC actor loss for
 * d_actions):
 *   grads1 / grads2    the parameter gradients of critic 1 / 2, summed over the batch (see fe_mlpq_grads);
 *   d_actions (count)  critic 1's sum_h wact[h] dz1[n][h] plus critic 2's, in that order, or null (not computed).
 * dq1 == null: critic 1 does not run (grads1 may be null and is not written), likewise dq2; TD3's actor loss runs critic
 * 1 only.  grads1 == null with dq1: critic 1 is frozen -- it only adds to d_actions (then required) and its
 * weight-gradient contractions and reductions do not run; likewise grads2.
 * Per critic it is fe_mlp2_backward's sequence (include/finenvs_amd_mlp2_head.h) with the action: (1) both hidden layers
 * recomputed with the forward's contractions and the action term, a1, dz2 and per-wavefront partials of d w3 / d b3;
 * (2) da1 = W2^T dz2 on the matrix cores, dz1 = da1 * act'(z1) written, and dQ/da formed beside it: an in-lane partial
 * over the lane's units, then (half 0) + (half 1); (3) [dW2 | d b2] = dz2^T [a1 | 1]; (4) [dW1t | d wpos | d wact | d b1] =
 * dz1^T [X | pos | a | 1], split into chunks of FE_MLPQ_GRAD_CHUNK_PAIRS pairs; (5) its reduction into the (H, 5W + 1)
 * layout, which also adds the partials of d w3 / d b3; (6) the reduction of (3).  A frozen critic runs (1) and (2).
 * Every reduction adds blocked partials in index order in f64 and rounds once.  workspace:
 * fe_twin_mlpq_grad_workspace_floats(H, W, count) floats, 16-byte aligned.
 */
int fe_twin_mlpq_backward(fe_env *env, const float *logret_f32, const fe_mlpq_weights *c1, const fe_mlpq_weights *c2,
                          int32_t H, int32_t activation, const int64_t *obs_src, const double *obs_pos,
                          const float *actions, int64_t count, const float *dq1, const float *dq2, float *workspace,
                          const fe_mlpq_grads *grads1, const fe_mlpq_grads *grads2, float *d_actions, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FINENVS_AMD_MLP_CRITIC_H */
