/*
 * finenvs_amd_mlp2_head.h -- the two-hidden-layer MLP head trained on observation descriptors (same library as
 * finenvs_amd.h).
 *
 * The reference's MLP agents default to hidden_dims = (128, 128): PPOAgentMLP and TD3AgentMLP build
 * MLPNetwork((5W, 128, 128, 1)) (networks/multilayer_perceptron.py).  This is that network with both hidden layers of
 * width H in {32, 64, 128}, per (env, asset) pair:
 *   z1 = W1^T flatten(states.float()) + b1     a1 = act(z1)     act: 0 ELU (alpha 1), 1 ReLU, 2 tanh, both layers alike
 *   z2 = W2 a1 + b2                            a2 = act(z2)     W2 = network.2.weight (H, H)
 *   p  = b3 + w3 . a2                          y  = out_act(p)  out_activation: 0 tanh, 1 clamp to [-1, 1], 2 none
 * The entries mirror finenvs_amd_mlp_head.h: the sampled K-step rollout, the head's value on any descriptors, and its
 * backward pass on the same descriptors.  No observation is written to memory by any of them.  The first layer and
 * the output layer are the one-layer head's, statement for statement (with W2 = I, b2 = 0 and ReLU every result equals
 * the one-layer entry's bit for bit); the H x H layer runs on v_mfma_f32_32x32x2_f32 straight from the first layer's
 * accumulators: lane (col, half) of a wavefront holds hidden unit 32t + 8b + 4 half + c of pair col, which is the
 * instruction's B operand, and the A operand is one 16-byte read of a row-padded image of W2 in LDS.  Python front end:
 * FusedMLP2Head in finenvs_amd/mlp2_head.py, FusedMLP2Rollout in finenvs_amd/rollout.py.  Conventions as in
 * finenvs_amd.h.
 *
 * Every weight is passed by device pointer, b3 included (one float).  The first layer comes packed as fe_mlp_pack
 * (finenvs_amd_mlp_head.h) writes it; W2, b2, w3 and b3 are read as torch holds them: nothing is packed for them.
 *
 * W1^T, W2 (rows padded to H + 4 floats) and the small vectors must fit the 160 KiB LDS next to the rollout's tile of
 * 128 pairs, in every entry: an env whose window is too long for a given H is refused ("does not fit") before any
 * pointer is touched.  With one asset the largest admitted window is
 *   H = 32: W <= 296      H = 64: W <= 128      H = 128: W <= 40
 * (FE_MLP2_MAX_WINDOW_*; the one-layer head admits W <= 72 at H = 128).  At H = 128 the W2 image alone is 66 KiB: one
 * workgroup per CU.
 *
 * Errors (FE_ERR_ARG, message naming the function): null pointers, a null field of fe_mlp2_weights / fe_mlp2_grads,
 * H outside {32, 64, 128}, activation outside 0..2, out_activation outside 0..2, count < 0, K < 1, states_src_out
 * without states_pos_out or the reverse, noise with a negative or NaN std, a weight image that does not fit the LDS;
 * for fe_mlp2_backward also out_activation 1 (clamp), null outputs with out_activation 0, and an env with A != 1.  No
 * host synchronisation and no allocation in any call; count = 0 does nothing; every launch goes on `stream` and can be
 * captured into a graph.
 */
#ifndef FINENVS_AMD_MLP2_HEAD_H
#define FINENVS_AMD_MLP2_HEAD_H

#include "finenvs_amd.h"
#include "finenvs_amd_mlp_head.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Pairs per split of the backward's two weight-gradient contractions (= FE_MLP_GRAD_CHUNK_PAIRS). */
#define FE_MLP2_GRAD_CHUNK_PAIRS 512

/* The largest window admitted per H for an env with one asset. */
#define FE_MLP2_MAX_WINDOW_H32 296
#define FE_MLP2_MAX_WINDOW_H64 128
#define FE_MLP2_MAX_WINDOW_H128 40

/* Device pointers of the head, f32. */
typedef struct fe_mlp2_weights {
    const float *w1t;  /* (H, 4W) as fe_mlp_pack writes it from network.0.weight */
    const float *wpos; /* (H) as fe_mlp_pack writes it */
    const float *b1;   /* (H) network.0.bias */
    const float *w2;   /* (H, H) network.2.weight, row-major as torch holds it */
    const float *b2;   /* (H) network.2.bias */
    const float *w3;   /* (H) network.4.weight */
    const float *b3;   /* (1) network.4.bias */
} fe_mlp2_weights;

/* Device pointers of the six parameter gradients, f32, in torch's layout.  Each gradient is summed over the batch and
 * OVERWRITES its buffer (accumulation into .grad is the caller's). */
typedef struct fe_mlp2_grads {
    float *w1; /* (H, 5W) d network.0.weight */
    float *b1; /* (H) d network.0.bias */
    float *w2; /* (H, H) d network.2.weight */
    float *b2; /* (H) d network.2.bias */
    float *w3; /* (H) d network.4.weight */
    float *b3; /* (1) d network.4.bias */
} fe_mlp2_grads;

/*
 * fe_env_rollout_mlp_sampled with the deeper network: mean = out_act(p); with noise (K, N*A) f32, action =
 * clamp(mean + std * noise, -1, 1) except for the evaluation env of a training-mode env, which acts on the mean;
 * without noise the action is the mean.  actions_out (K, N*A), means_out (K, N*A), rewards_out (K, N), dones_out (K, N);
 * states_src_out (K + 1, N) / states_pos_out (K + 1, N*A) receive the descriptor rows of the K + 1 states.  noise,
 * actions_out, means_out and the two states_*_out may be null.  Any A.
 */
int fe_env_rollout_mlp2_sampled(fe_env *env, const float *logret_f32, const fe_mlp2_weights *weights, int32_t H,
                                int32_t activation, int32_t out_activation, int32_t K, int64_t *obs_src, double *obs_pos,
                                const float *noise, float std, float *actions_out, float *means_out, double *rewards_out,
                                int32_t *dones_out, int64_t *states_src_out, double *states_pos_out, void *stream);

/*
 * The head on any `count` observation descriptors (obs_src (count) int64, obs_pos (count * A) f64): out (count * A)
 * f32.  The env's state is neither read nor written; the env supplies W, A and the device.
 */
int fe_mlp2_forward(fe_env *env, const float *logret_f32, const fe_mlp2_weights *weights, int32_t H, int32_t activation,
                    int32_t out_activation, const int64_t *obs_src, const double *obs_pos, int64_t count, float *out,
                    void *stream);

/*
 * Floats of the workspace fe_mlp2_backward needs for `count` pairs of an env with window W (-1 for H outside
 * {32, 64, 128}, W < 1 or count < 0; 0 for count = 0).  It grows with count: with
 *   blocks = ceil(count / 32),  splits = ceil(count / FE_MLP2_GRAD_CHUNK_PAIRS),  F = 32 ceil((4W + 2) / 32),
 *   waves  = 4 min(ceil(blocks / 4), 512)
 * it is
 *   3 * 32 blocks H   +   splits H (F + H + 32)   +   waves (H + 4)
 * floats: three H-float rows per pair (dz1, a1, dz2), per split of FE_MLP2_GRAD_CHUNK_PAIRS pairs one H x F partial of
 * the first layer's gradient and one H x (H + 32) partial of [dW2 | d b2], and one partial of d w3 / d b3 per wavefront
 * of the first kernel.
 */
int64_t fe_mlp2_grad_workspace_floats(int32_t H, int32_t W, int64_t count);

/*
 * The backward of fe_mlp2_forward on the same arguments (A = 1), given outputs (count) as fe_mlp2_forward returned
 * them (may be null with out_activation 2) and the upstream gradient d_outputs (count) f32.  With g = d_outputs:
 *   dp = g (1 - y^2) (tanh) or g (none);  d b3 = sum dp;  d w3[h] = sum dp a2[h];
 *   dz2[n][h] = dp_n w3[h] act'(z2[n][h]);  d b2 = sum_n dz2[n];  d W2 = sum_n dz2[n] a1[n]^T;
 *   da1 = W2^T dz2;  dz1 = da1 * act'(z1);  d b1, d W1 from dz1 as fe_mlp_backward forms them from dpre (the position
 *   column summed once and written to every window row).
 * act' of the second layer is taken on the recomputed z2 as in fe_mlp_backward (ELU: z > 0 ? 1 : exp(z)); act' of the
 * first layer on the stored a1: ReLU a > 0, tanh 1 - a^2, ELU a > 0 ? 1 : a + 1 (a = exp(z) - 1 there).
 * Six launches on `stream`: (1) both hidden layers recomputed with the forward's contractions, a1, dz2 and
 * per-wavefront partials of d w3 / d b3 written to the workspace; (2) da1 = W2^T dz2 per 32-pair block on the matrix
 * cores from an LDS image of W2^T, dz1 written; (3) [dW2 | d b2] = dz2^T [a1 | 1] on the matrix cores, split into chunks
 * of FE_MLP2_GRAD_CHUNK_PAIRS pairs; (4) fe_mlp_backward's weight-gradient kernel on dz1; (5) its reduction, which also
 * adds the partials of d w3 / d b3; (6) the reduction of (3).  Every reduction adds blocked partials in index order in
 * f64 and rounds once.  No float atomics: every sum has a fixed order that depends only on (H, W, count), so the same
 * inputs give the same bits.  workspace: fe_mlp2_grad_workspace_floats(H, W, count) floats, 16-byte aligned.
 */
int fe_mlp2_backward(fe_env *env, const float *logret_f32, const fe_mlp2_weights *weights, int32_t H, int32_t activation,
                     int32_t out_activation, const int64_t *obs_src, const double *obs_pos, int64_t count,
                     const float *outputs, const float *d_outputs, float *workspace, const fe_mlp2_grads *grads,
                     void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FINENVS_AMD_MLP2_HEAD_H */
