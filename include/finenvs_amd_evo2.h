/*
 * finenvs_amd_evo2.h -- the evolution-strategies population with TWO hidden layers (same library as finenvs_amd.h).
 *
 * The reference's EvoAgent builds ParallelMLP(shape = (num_observations, *hidden_dims, num_actions)) with two hidden
 * layers by default (finenvs/agents/ES/evo_agent.py:17-37).  This header is finenvs_amd_evo.h's rollout for that shape:
 * the same population struct, members, noise streams, outputs and bookkeeping, with an H x H layer in the middle.  The
 * noise render (fe_evo_noise) and the gradient (fe_evo_gradient) of finenvs_amd_evo.h are generic in the parameter
 * count and serve this layout as they are, with P below.  Python front end: finenvs_amd/evo.py
 * (FusedPopulationMLP2Rollout).  Conventions as in finenvs_amd.h.
 *
 * Network (ParallelMLP with two hidden layers and its default tanh activations, parallel_mlp.py:45-65, 84-96):
 *   action = tanh(W3^T tanh(W2^T tanh(W1^T x + b1) + b2) + b3) + nu * xi,   x = (float) flatten(obs window), row 5j + c
 * theta (P floats, P = 5W*H + H*H + 3H + 1), in the reference's layer order:
 *   W1 (5W, H), b1 (H), W2 (H, H), b2 (H), W3 (H), b3      each row-major, (in, out);  H in {32, 64, 128}.
 * Every segment starts at a multiple of 4 floats.
 *
 * Members: as finenvs_amd_evo.h.  n_train = N - num_eval_envs (even, > 0), half = n_train / 2; env i < half uses
 * theta + s*z of pair p = i (s = +1), half <= i < n_train pair p = i - half (s = -1), i >= n_train theta itself and no
 * action noise: w_{i,j} = theta_j + s_i * fl(sigma * z_{g,p,j}) in f32.
 *
 * Noise: the streams are those of finenvs_amd_evo.h, unchanged.  z_{g,p,j} is word j % 4 of the f32 Box-Muller transform
 * of Philox4x32-10(key = seed, counter = (j / 4, p, g, 0x45565a00)), j indexing theta in the layout above; the action
 * noise xi of env n, asset a at step t of generation g is word a % 4 at counter (n, t, g, 0x45564100 | a / 4).
 *
 * Summation order (fixed; two launches give the same bits): per layer with a weight matrix, 64 / (H / 4) row groups each
 * sum their rows (group, group + 64 / (H / 4), ...) in ascending order with fused multiply-adds from +0, then a butterfly
 * over the row groups adds the partial sums, then the bias is added; the output layer sums four terms per lane and a
 * butterfly over the H / 4 lanes, as the one-hidden-layer kernel does.
 *
 * Limits: theta lives in the 160 KiB LDS, so H <= 128 (the reference's default 256 does not fit: its middle layer alone is
 * 256 KiB) and the window is bounded per H and A by fe_evo2_lds_bytes(W, A, H) <= 163840.  With one asset the largest
 * windows are W = 246 (H = 32), 112 (H = 64) and 35 (H = 128); with 100 assets 238, 108 and 33.
 */
#ifndef FINENVS_AMD_EVO2_H
#define FINENVS_AMD_EVO2_H

#include "finenvs_amd.h"
#include "finenvs_amd_evo.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * K steps of the population: fe_evo_rollout with the network above.  pop is finenvs_amd_evo.h's struct; pop->hidden is 32,
 * 64 or 128 and pop->theta holds P = fe_evo2_num_params(W, H) floats in the layout above.  Outputs, side effects and the
 * ordering rule are fe_evo_rollout's: steps of one generation must be issued in order and pop->step must count them;
 * run(32); run(32) equals run(64) bit for bit.  FE_ERR_ARG: null pointers, K < 1, H not 32 / 64 / 128, n_train odd / <= 0
 * / > N, an evaluate-mode env, redraw mode not 1, more than 128 assets, theta larger than the LDS ("... does not fit the
 * 160 KiB LDS"), unbound env.
 */
int fe_evo2_rollout(fe_env *env, const fe_evo_population *pop, int32_t K, float *actions_out, float *means_out,
                    double *rewards_out, int32_t *dones_out, void *stream);

/* P = 5W*H + H*H + 3H + 1, or -1 for W < 1 or H not 32 / 64 / 128. */
int64_t fe_evo2_num_params(int32_t W, int32_t H);

/*
 * Bytes of LDS a launch takes at window W, A assets and width H (theta, the tile's accounts and the per-wavefront
 * exchange buffer of the middle layer); the rollout refuses a shape above 160 KiB = 163840.  -1 for W < 1, A outside
 * [1, 128] or H not 32 / 64 / 128.
 */
int64_t fe_evo2_lds_bytes(int32_t W, int32_t A, int32_t H);

#ifdef __cplusplus
}
#endif

#endif /* FINENVS_AMD_EVO2_H */
