/*
 * finenvs_amd_mlp_head.h -- the MLP head trained on observation descriptors (same library as finenvs_amd.h).
 *
 * The reference ships every gradient learner in an MLP family next to the LSTM one: PPOAgentMLP
 * (PPO/PPO_agent.py:209-243) with ContinuousActorMLP (PPO/continuous_actor.py:81-101, Tanh) and CriticMLP
 * (PPO/critic.py:35-50, Identity), both MLPNetwork (networks/multilayer_perceptron.py).  With one hidden layer that
 * network is the head of fe_env_rollout_mlp (finenvs_amd_ext.h), per (env, asset) pair:
 *   p = b2 + w2 . act(W1^T flatten(states.float()) + b1)     act: 0 ELU, 1 ReLU, 2 tanh;  H in {32, 64, 128}
 *   y = out_act(p)                                           out_activation: 0 tanh, 1 clamp to [-1, 1], 2 none
 * Here are its training-time entries: the weights packed on the device, the sampled K-step rollout that fills a
 * trajectory chunk with state descriptors, the head's value on any descriptors, and its backward pass on the same
 * descriptors.  No observation is written to memory by any of them.  The first layer, forward and backward, runs on
 * v_mfma_f32_32x32x2_f32; the forward uses the contraction of fe_env_rollout_mlp in its k order, so p is that
 * rollout's p bit for bit.  The tanh output is the exact-operation tanh of fe_lstm_activations.  Python front end:
 * FusedMLPHead in finenvs_amd/mlp_head.py, FusedMLPRollout in finenvs_amd/rollout.py.  Conventions as in
 * finenvs_amd.h.
 *
 * Every weight is passed by device pointer, b2 included (one float): an optimizer step needs no copy to the host.
 * W1^T must fit the LDS next to the rollout's tile of 128 pairs, in every entry (the rule of fe_env_rollout_mlp at its
 * default tile): an env whose window is too long for a given H is refused.
 *
 * Errors (FE_ERR_ARG, message naming the function): null pointers, a null field of fe_mlp_weights / fe_mlp_grads,
 * H outside {32, 64, 128}, activation outside 0..2, out_activation outside 0..2, count < 0, K < 1, states_src_out
 * without states_pos_out or the reverse, noise with a negative or NaN std, W1^T that does not fit the LDS; for
 * fe_mlp_backward also out_activation 1 (clamp: an action bound, not a trainable output), null outputs with
 * out_activation 0, and an env with A != 1.  No host synchronisation and no allocation in any call; count = 0 does
 * nothing; every launch goes on `stream` and can be captured into a graph.
 */
#ifndef FINENVS_AMD_MLP_HEAD_H
#define FINENVS_AMD_MLP_HEAD_H

#include "finenvs_amd.h"
#include "finenvs_amd_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Pairs per split of the backward's weight-gradient contraction (see fe_mlp_grad_workspace_floats). */
#define FE_MLP_GRAD_CHUNK_PAIRS 512

/* Device pointers of the packed head, f32: what fe_mlp_pack writes, and the three small tensors as torch holds them. */
typedef struct fe_mlp_weights {
    const float *w1t;  /* (H, 4W) w1t[h][4j+c] = weight1[h][5j+c], c < 4 */
    const float *wpos; /* (H) sum over j of weight1[h][5j+4] */
    const float *b1;   /* (H) network.0.bias */
    const float *w2;   /* (H) network.2.weight */
    const float *b2;   /* (1) network.2.bias */
} fe_mlp_weights;

/* Device pointers of the head's four parameter gradients, f32, in torch's layout: the buffers are the parameters'
 * .grad as they stand.  Each gradient is summed over the batch and OVERWRITES its buffer (accumulation into .grad is
 * the caller's). */
typedef struct fe_mlp_grads {
    float *w1; /* (H, 5W) d network.0.weight */
    float *b1; /* (H) d network.0.bias */
    float *w2; /* (H) d network.2.weight */
    float *b2; /* (1) d network.2.bias */
} fe_mlp_grads;

/*
 * torch's Linear(5W, H).weight, weight1 (H, 5W) f32 on the device, as the kernels read it: w1t (H, 4W) and wpos (H),
 * wpos[h] the sequential f32 sum over j ascending of weight1[h][5j+4].  One launch, no copy to the host; the result
 * equals the host packing of FusedMLPRollout.set_weights bit for bit.
 */
int fe_mlp_pack(const float *weight1, int32_t H, int32_t W, float *w1t, float *wpos, void *stream);

/*
 * The K-step loop of fe_env_rollout_mlp as a training rollout (agent.step of PPO/PPO_agent.py:98-108; the semantics of
 * fe_env_rollout_lstm): mean = out_act(p); with noise (K, N*A) f32, action = clamp(mean + std * noise, -1, 1) -- one
 * f32 product, one f32 sum -- except for the evaluation env of a training-mode env, which acts on the mean; without
 * noise the action is the mean.  actions_out (K, N*A), means_out (K, N*A), rewards_out (K, N), dones_out (K, N);
 * states_src_out (K + 1, N) / states_pos_out (K + 1, N*A) receive the descriptor rows of the K + 1 states (row 0:
 * the state the first policy evaluation sees).  noise, actions_out, means_out and the two states_*_out may be null.
 * With noise = NULL and out_activation = 1 every output and the env's state equal fe_env_rollout_mlp's bit for bit.
 */
int fe_env_rollout_mlp_sampled(fe_env *env, const float *logret_f32, const fe_mlp_weights *weights, int32_t H,
                               int32_t activation, int32_t out_activation, int32_t K, int64_t *obs_src, double *obs_pos,
                               const float *noise, float std, float *actions_out, float *means_out, double *rewards_out,
                               int32_t *dones_out, int64_t *states_src_out, double *states_pos_out, void *stream);

/*
 * The head on any `count` observation descriptors (obs_src (count) int64, obs_pos (count * A) f64): out (count * A)
 * f32.  The env's state is neither read nor written; the env supplies W, A and the device.
 */
int fe_mlp_forward(fe_env *env, const float *logret_f32, const fe_mlp_weights *weights, int32_t H, int32_t activation,
                   int32_t out_activation, const int64_t *obs_src, const double *obs_pos, int64_t count, float *out,
                   void *stream);

/*
 * Floats of the workspace fe_mlp_backward needs for `count` pairs of an env with window W (-1 for H outside
 * {32, 64, 128}, W < 1 or count < 0; 0 for count = 0).  It GROWS with count -- unlike fe_lstm_grad_workspace_floats,
 * whose per-pair term is 0 --: with
 *   blocks = ceil(count / 32),  splits = ceil(count / FE_MLP_GRAD_CHUNK_PAIRS),  F = 32 ceil((4W + 2) / 32),
 *   waves  = 4 min(ceil(blocks / 4), 512)
 * it is
 *   32 blocks H   +   splits H F   +   waves (H + 4)
 * floats: the first-layer gradient dpre of every pair (H floats per pair), one H x F partial product per
 * split of FE_MLP_GRAD_CHUNK_PAIRS pairs, and one partial of d w2 / d b2 per wavefront of the first kernel.  The
 * per-pair term is H + H F / FE_MLP_GRAD_CHUNK_PAIRS floats.
 */
int64_t fe_mlp_grad_workspace_floats(int32_t H, int32_t W, int64_t count);

/*
 * The backward of fe_mlp_forward on the same arguments (A = 1), given outputs (count) as fe_mlp_forward returned them
 * (may be null with out_activation 2) and the upstream gradient d_outputs (count) f32.  With g = d_outputs:
 *   dp = g (1 - y^2) (tanh) or g (none);  d b2 = sum dp;  d w2[h] = sum dp act(pre[h]);
 *   dpre[n][h] = dp_n w2[h] act'(pre[n][h]),  act' on the forward's own value: ELU z > 0 ? 1 : exp(z) (the forward's
 *   v_exp_f32), ReLU z > 0 ? 1 : 0, tanh 1 - act^2;
 *   d b1[h] = sum_n dpre[n][h];  d W1[h][5j+c] = sum_n x[n][j][c] dpre[n][h] (c < 4);
 *   d W1[h][5j+4] = sum_n pos32_n dpre[n][h], the same for every j.
 * Three launches on `stream`: (1) the first layer recomputed with the forward's contraction, dp and dpre formed
 * in-lane, dpre and per-wavefront partials of d w2 / d b2 written to the workspace; (2) [dW1t | d wpos | d b1] =
 * dpre^T [X | pos | 1] on the matrix cores, X read straight from the f32 log-return table, split into chunks of
 * FE_MLP_GRAD_CHUNK_PAIRS pairs, each an accumulation from zero; (3) the splits and partials added in index order (in
 * f64, rounded once) and written in torch's layout.  No float atomics: every sum has a fixed order that depends only
 * on (H, W, count), so the same inputs give the same bits.  workspace: fe_mlp_grad_workspace_floats(H, W, count)
 * floats of device memory, 16-byte aligned.
 */
int fe_mlp_backward(fe_env *env, const float *logret_f32, const fe_mlp_weights *weights, int32_t H, int32_t activation,
                    int32_t out_activation, const int64_t *obs_src, const double *obs_pos, int64_t count,
                    const float *outputs, const float *d_outputs, float *workspace, const fe_mlp_grads *grads,
                    void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FINENVS_AMD_MLP_HEAD_H */
