/*
 * finenvs_amd_evo2_streamed.h -- the two-hidden-layer evolution-strategies population with theta read through L2 (same
 * library as finenvs_amd.h).
 *
 * The reference's EvoAgent builds ParallelMLP with hidden_dims = (256, 256) by default (finenvs/agents/ES/evo_agent.py:17).
 * fe_evo2_rollout (finenvs_amd_evo2.h) copies theta into the 160 KiB LDS and stops at H = 128 and at a window per H.  The
 * entry below is the same rollout -- members, noise streams, outputs, bookkeeping and summation order -- with theta left
 * in global memory: every workgroup reads the same P floats (at most 256 KiB + 5W KiB), which live in L2.  It runs
 * H = 32 / 64 / 128 / 256 and its LDS does not grow with the window.  fe_evo_noise and fe_evo_gradient of
 * finenvs_amd_evo.h are generic in the parameter count and serve H = 256 as they are.  Python front end:
 * finenvs_amd/evo.py (FusedPopulationMLP2Rollout(..., streamed=True)).  Conventions as in finenvs_amd.h.
 *
 * Network and theta: those of finenvs_amd_evo2.h.
 *   action = tanh(W3^T tanh(W2^T tanh(W1^T x + b1) + b2) + b3) + nu * xi,   x = (float) flatten(obs window), row 5j + c
 *   theta (P floats, P = 5W*H + H*H + 3H + 1):  W1 (5W, H), b1 (H), W2 (H, H), b2 (H), W3 (H), b3, each row-major (in,
 *   out); every segment starts at a multiple of 4 floats.  Exactly P floats are read: no address at or beyond theta + P.
 *
 * Members: env i < half = n_train / 2 acts with theta + fl(sigma z_{g,p,.}) of pair p = i, half <= i < n_train with
 * theta - fl(sigma z_{g,p,.}) of p = i - half, i >= n_train with theta itself and no action noise.
 *
 * Noise: z_{g,p,j} is word j % 4 of the f32 Box-Muller transform of Philox4x32-10(key = seed, counter = (j / 4, p, g,
 * 0x45565a00)); the action noise xi of env n, asset a at step t is word a % 4 at counter (n, t, g, 0x45564100 | a / 4).
 *
 * Summation order (fixed; two launches give the same bits): per layer with a weight matrix, 64 / (H / 4) row groups each
 * sum their rows (group, group + 64 / (H / 4), ...) in ascending order with fused multiply-adds from +0, then a butterfly
 * over the row groups adds the partial sums, then the bias is added; at H = 256 there is one row group of all 64 lanes and
 * no butterfly.  The output layer sums four terms per lane and a butterfly over the H / 4 lanes.
 *
 * Wherever fe_evo2_rollout accepts the shape, the outputs and every side effect of this entry equal its bit for bit.
 *
 * Limits: H in {32, 64, 128, 256}; at most 128 assets; the window is bounded only by what the env accepts (1 <= W < the
 * bars of a day).
 */
#ifndef FINENVS_AMD_EVO2_STREAMED_H
#define FINENVS_AMD_EVO2_STREAMED_H

#include "finenvs_amd.h"
#include "finenvs_amd_evo.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * K steps of the population: fe_evo2_rollout with theta read from global memory.  pop is finenvs_amd_evo.h's struct;
 * pop->hidden is 32, 64, 128 or 256 and pop->theta holds P = fe_evo2_streamed_num_params(W, H) floats.  Outputs, side
 * effects and the ordering rule are fe_evo_rollout's.  FE_ERR_ARG: null pointers, K < 1, H not 32 / 64 / 128 / 256,
 * n_train odd / <= 0 / > N, an evaluate-mode env, redraw mode not 1, more than 128 assets; FE_ERR_STATE: unbound env.
 */
int fe_evo2_rollout_streamed(fe_env *env, const fe_evo_population *pop, int32_t K, float *actions_out, float *means_out,
                             double *rewards_out, int32_t *dones_out, void *stream);

/* P = 5W*H + H*H + 3H + 1, or -1 for W < 1 or H not 32 / 64 / 128 / 256. */
int64_t fe_evo2_streamed_num_params(int32_t W, int32_t H);

/*
 * Bytes of LDS a launch takes at A assets and width H (the tile's accounts and the per-wavefront exchange buffer of the
 * middle layer: about 8 KiB at H = 256); the same for every W.  -1 for W < 1, A outside [1, 128] or H not one of the four.
 */
int64_t fe_evo2_streamed_lds_bytes(int32_t W, int32_t A, int32_t H);

#ifdef __cplusplus
}
#endif

#endif /* FINENVS_AMD_EVO2_STREAMED_H */
