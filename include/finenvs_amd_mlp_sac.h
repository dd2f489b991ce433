/*
 * finenvs_amd_mlp_sac.h -- the SAC MLP actor on observation descriptors (same library as finenvs_amd.h).
 *
 * The reference's SACAgentMLP (SAC/SAC_agent.py:244-279) acts with ActorMLP (SAC/actor.py:106-120):
 * MLPNetwork((5W, H, H), ELU, nn.Identity) -- so its second Linear has NO activation -- then mu_layer and std_layer,
 * both Linear(H, 1) here (one output per (env, asset) pair, like the other fused heads).  Per pair, x the flattened f32
 * window, H in {32, 64, 128}, act: 0 ELU (alpha 1), 1 ReLU, 2 tanh:
 *
 *   z1 = W1 x + b1        a1 = act(z1)          network.0, network.1
 *   z  = W2 a1 + b2       (Identity)            network.2, network.3
 *   mu = w_mu . z + b_mu  q = w_s . z + b_s     s = softplus(q)   (torch's rule: q > 20 ? q : log1p(exp(q)))
 *   with noise eps:  u = mu + eps s,  a = tanh(u),  log_prob = Normal(mu, s).log_prob(u) - log(1 - a^2 + 1e-7)
 *                                                                                          (SAC/actor.py:51-61)
 *
 * mu and q are affine in a1, so the H x H layer folds into two H-vectors and two constants per call:
 *
 *   v_mu = W2^T w_mu   c_mu = w_mu . b2 + b_mu      v_s = W2^T w_s   c_s = w_s . b2 + b_s
 *   mu = c_mu + v_mu . a1                           q = c_s + v_s . a1
 *
 * fe_mlp_sac_pack forms them on the device (every sum in f64 from the f32 parameters, index ascending, rounded once)
 * and every other entry evaluates the folded form with the one-layer head's own statements: mu equals fe_mlp_forward
 * (finenvs_amd_mlp_head.h, out_activation 2) on (w1t, wpos, b1, v_mu, c_mu) bit for bit, q likewise on (v_s, c_s).  The
 * actor therefore runs at the cost of the one-hidden-layer head.  Python front end: finenvs_amd/mlp_sac.py.
 * Conventions as in finenvs_amd.h.
 *
 * The weight image (W1^T, wpos, b1, v_mu, v_s, the constants) must fit the 160 KiB LDS next to the rollout's tile of
 * 128 pairs, in every entry: an env whose window is too long for a given H is refused ("does not fit") before any
 * pointer is touched.  With one asset the largest admitted window is
 *   H = 32: W <= 304      H = 64: W <= 144      H = 128: W <= 72
 * (FE_MLP_SAC_MAX_WINDOW_*: the one-layer head's limits; the twin MLP critics admit W <= 40 at H = 128).
 *
 * Errors (FE_ERR_ARG, message naming the function), in this order: null pointers and null fields of
 * fe_mlp_sac_weights / fe_mlp_sac_grads ("bad argument"); H outside {32, 64, 128}; activation outside 0..2; count < 0,
 * K < 1; states_src_out without states_pos_out or the reverse; actions_out / log_probs_out without noise; for
 * fe_mlp_sac_backward both upstream gradients null; a weight image that does not fit the LDS; for fe_mlp_sac_backward
 * an env with A != 1.
 * No host synchronisation and no allocation in any call; count = 0 does nothing; every launch goes on `stream` and can
 * be captured into a graph (no value is copied to the host: the biases are read on the device).
 */
#ifndef FINENVS_AMD_MLP_SAC_H
#define FINENVS_AMD_MLP_SAC_H

#include "finenvs_amd.h"
#include "finenvs_amd_mlp_head.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Pairs per split of the backward's weight-gradient contraction (= FE_MLP_GRAD_CHUNK_PAIRS). */
#define FE_MLP_SAC_GRAD_CHUNK_PAIRS 512
/* Workgroups (of four wavefronts) of the backward's first kernel at most. */
#define FE_MLP_SAC_GRAD_MAX_GROUPS 256

/* The largest window admitted per H for an env with one asset. */
#define FE_MLP_SAC_MAX_WINDOW_H32 304
#define FE_MLP_SAC_MAX_WINDOW_H64 144
#define FE_MLP_SAC_MAX_WINDOW_H128 72

/* Device pointers of the actor, f32.  The first seven are the parameters (the first layer packed); the last three are
 * what fe_mlp_sac_pack writes from them.  The rollout and the forward read w1t, wpos, b1, vmu, vstd and cfold only. */
typedef struct fe_mlp_sac_weights {
    const float *w1t;   /* (H, 4W) as fe_mlp_pack / fe_mlp_sac_pack writes it from network.0.weight */
    const float *wpos;  /* (H) likewise */
    const float *b1;    /* (H) network.0.bias */
    const float *w2;    /* (H, H) network.2.weight, row-major as torch holds it */
    const float *b2;    /* (H) network.2.bias */
    const float *wmu;   /* (H) mu_layer.weight */
    const float *bmu;   /* (1) mu_layer.bias */
    const float *wstd;  /* (H) std_layer.weight */
    const float *bstd;  /* (1) std_layer.bias */
    const float *vmu;   /* (H) W2^T w_mu */
    const float *vstd;  /* (H) W2^T w_s */
    const float *cfold; /* (2) c_mu, c_s */
} fe_mlp_sac_weights;

/* Device pointers of the eight parameter gradients, f32, in torch's layout.  Each gradient is summed over the batch and
 * OVERWRITES its buffer (accumulation into .grad is the caller's). */
typedef struct fe_mlp_sac_grads {
    float *w1;    /* (H, 5W) d network.0.weight */
    float *b1;    /* (H) d network.0.bias */
    float *w2;    /* (H, H) d network.2.weight */
    float *b2;    /* (H) d network.2.bias */
    float *w_mu;  /* (H) d mu_layer.weight */
    float *b_mu;  /* (1) d mu_layer.bias */
    float *w_std; /* (H) d std_layer.weight */
    float *b_std; /* (1) d std_layer.bias */
} fe_mlp_sac_grads;

/*
 * One launch: w1t / wpos from weight1 = network.0.weight (H, 5W) exactly as fe_mlp_pack writes them, and the fold
 * vmu, vstd (H each), cfold (2) from w2, b2, wmu, bmu, wstd, bstd (all on the device).  Refused: a null pointer, H
 * outside {32, 64, 128}, W < 1.
 */
int fe_mlp_sac_pack(const float *weight1, const float *w2, const float *b2, const float *wmu, const float *bmu,
                    const float *wstd, const float *bstd, int32_t H, int32_t W, float *w1t, float *wpos, float *vmu,
                    float *vstd, float *cfold, void *stream);

/*
 * K env steps with the actor in the kernel: the arguments and semantics of fe_env_rollout_sac (finenvs_amd_sac.h), any
 * A.  noise (K, N, A) f32 standard normals or null.  With noise every env acts with tanh(mu + eps s) except the
 * evaluation env of a training-mode env, which acts on mu; without noise every env acts on mu.  Optional outputs (null
 * = not written): actions_out, means_out (mu), stds_out (s), each (K, N, A) f32; states_src_out (K + 1, N) /
 * states_pos_out (K + 1, N, A) (go together).  Accounting, side effects and the in/out descriptors obs_src / obs_pos
 * as fe_env_rollout_mlp_sampled.
 */
int fe_env_rollout_mlp_sac(fe_env *env, const float *logret_f32, const fe_mlp_sac_weights *weights, int32_t H,
                           int32_t activation, int32_t K, int64_t *obs_src, double *obs_pos, const float *noise,
                           float *actions_out, float *means_out, float *stds_out, double *rewards_out,
                           int32_t *dones_out, int64_t *states_src_out, double *states_pos_out, void *stream);

/*
 * The head on `count` observation descriptors (obs_src (count), obs_pos (count, A)) without stepping the env: the
 * semantics of fe_sac_forward, any A.  Outputs (count, A) f32, null = not written: means_out (mu), stds_out (s) and,
 * with noise (count, A), actions_out (tanh(u)) and log_probs_out.  Every descriptor samples.  actions_out /
 * log_probs_out without noise: FE_ERR_ARG.
 */
int fe_mlp_sac_forward(fe_env *env, const float *logret_f32, const fe_mlp_sac_weights *weights, int32_t H,
                       int32_t activation, const int64_t *obs_src, const double *obs_pos, int64_t count,
                       const float *noise, float *actions_out, float *log_probs_out, float *means_out, float *stds_out,
                       void *stream);

/*
 * Floats of the workspace fe_mlp_sac_backward needs for `count` pairs of an env with window W (-1 for H outside
 * {32, 64, 128}, W < 1 or count < 0; 0 for count = 0).  With
 *   blocks = ceil(count / 32),  splits = ceil(count / FE_MLP_SAC_GRAD_CHUNK_PAIRS),  F = 32 ceil((4W + 2) / 32),
 *   waves  = 4 min(ceil(blocks / 4), FE_MLP_SAC_GRAD_MAX_GROUPS)
 * it is
 *   32 blocks H   +   splits H F   +   waves 2 (H + 4)
 * floats: ONE H-float row per pair (dz1; the two-layer head keeps three), one H x F partial product per split, and
 * one partial of [A_mu | S_mu | A_q | S_q] per wavefront of the first kernel.
 */
int64_t fe_mlp_sac_grad_workspace_floats(int32_t H, int32_t W, int64_t count);

/*
 * The backward of fe_mlp_sac_forward on the same arguments (A = 1), given noise, actions and stds (count) as
 * fe_mlp_sac_forward took / returned them and the upstream gradients d_actions / d_log_probs (count) f32 of its
 * actions / log_probs outputs; either may be null (an output nobody used), not both.  With ga = d_actions, gl =
 * d_log_probs, exactly as fe_sac_backward forms them (finenvs_amd_sac_grad.h):
 *   du = ga (1 - a^2) + gl 2 a (1 - a^2) / (1 - a^2 + 1e-7),  dmu = du,  ds = du eps - gl / s,
 *   dq = ds sigmoid(q) (1 where q > 20), q recomputed;
 * then the rank-two algebra of the fold:
 *   S_mu = sum dmu_n   S_q = sum dq_n   A_mu = sum dmu_n a1_n   A_q = sum dq_n a1_n        (H each)
 *   d b_mu = S_mu    d b_std = S_q
 *   d w_mu = W2 A_mu + b2 S_mu          d w_std = W2 A_q + b2 S_q
 *   d b2 = w_mu S_mu + w_s S_q          d W2 = w_mu A_mu^T + w_s A_q^T
 *   da1_n = v_mu dmu_n + v_s dq_n       dz1_n = da1_n * act'(z1_n)     d b1, d W1 from dz1 as fe_mlp_backward
 * (act' on the recomputed z1: ELU z > 0 ? 1 : exp(z), ReLU z > 0, tanh 1 - a1^2).  weights: as packed for the forward
 * (the fold must be current).  Three launches on `stream`: (1) a1 recomputed with the forward's contraction, dmu / dq
 * formed in-lane, dz1 and per-wavefront partials of [A_mu | S_mu | A_q | S_q] written to the workspace; (2)
 * fe_mlp_backward's weight-gradient kernel on dz1; (3) one reduction that finishes layer 1 and evaluates the O(H^2)
 * epilogue above: it adds blocked partials in index order in f64 and rounds every result once.  No float atomics: the
 * same inputs give the same bits.  workspace: fe_mlp_sac_grad_workspace_floats(H, W, count) floats, 16-byte aligned.
 */
int fe_mlp_sac_backward(fe_env *env, const float *logret_f32, const fe_mlp_sac_weights *weights, int32_t H,
                        int32_t activation, const int64_t *obs_src, const double *obs_pos, int64_t count,
                        const float *noise, const float *actions, const float *stds, const float *d_actions,
                        const float *d_log_probs, float *workspace, const fe_mlp_sac_grads *grads, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FINENVS_AMD_MLP_SAC_H */
