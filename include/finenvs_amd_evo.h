/*
 * finenvs_amd_evo.h -- the evolution-strategies population of the C ABI (same library as finenvs_amd.h).
 *
 * OpenAI-ES as the reference runs it (finenvs/agents/ES/evo_agent.py, finenvs/agents/networks/parallel_mlp.py) with the
 * per-env networks never materialised: every env of a training-mode env (redraw_mode 1) acts with its own perturbation
 * of one shared parameter vector, generated inside the rollout kernel from a counter-based normal stream, and the ES
 * gradient regenerates the same stream.  Python front end: finenvs_amd/evo.py.  Conventions as in finenvs_amd.h.
 *
 * Network (ParallelMLP with one hidden layer and its default tanh activations, parallel_mlp.py:45-65, 84-96):
 *   action = tanh(W2^T tanh(W1^T x + b1) + b2) + nu * xi,   x = (float) flatten(obs window of the asset), row 5j + c
 * theta (P floats, P = 5W*H + 2H + 1): W1 (5W, H), b1 (H), W2 (H), b2, each row-major; H in {32, 64}.
 *
 * Members: n_train = N - num_eval_envs (even, > 0), half = n_train / 2.  Env i < half uses theta + s*z of pair p = i
 * (s = +1), half <= i < n_train pair p = i - half (s = -1), i >= n_train theta itself and no action noise
 * (parallel_mlp.py:112-156): w_{i,j} = theta_j + s_i * fl(sigma * z_{g,p,j}) in f32.
 *
 * Noise: z_{g,p,j} = word j % 4 of the f32 Box-Muller transform of Philox4x32-10(key = seed, counter = (j / 4, p, g,
 * 0x45565a00)); the action noise xi of env n, asset a at step t of generation g (t counts from the generation's start) is
 * word a % 4 of the same transform at counter (n, t, g, 0x45564100 | a / 4).  fe_evo_noise renders z.
 */
#ifndef FINENVS_AMD_EVO_H
#define FINENVS_AMD_EVO_H

#include "finenvs_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fe_evo_population {
    int64_t num_train;          /* n_train = N - num_eval_envs: even, > 0, <= N */
    int32_t hidden;             /* H: 32 or 64 */
    int32_t max_episodes;       /* slots per env of episode_returns, >= 1 */
    float noise_std;            /* sigma */
    float action_noise_std;     /* nu (the reference's 0.01, parallel_mlp.py:95) */
    uint64_t seed;              /* key of the ES noise streams (independent of the env's redraw seed) */
    uint32_t generation;        /* g */
    uint32_t step;              /* steps of generation g run before this launch */
    const float *logret_f32;    /* (D, L, 4A) f32 copy of the env's log-return table */
    const float *theta;         /* (P) */
    int64_t *obs_src;           /* (N) in/out: descriptors of the observation the policy sees next (fe_env_describe) */
    double *obs_pos;            /* (N, A) in/out */
    float *returns;             /* (N) in/out: running return, f32(f64(ret) + reward) (evo_agent.py:103) */
    float *timesteps;           /* (N) in/out: running timestep count (evo_agent.py:93) */
    float *episode_returns;     /* (N, max_episodes): returns of the finished episodes, per env in finishing order */
    int32_t *episode_counts;    /* (N) */
    uint64_t *counters;         /* [0] += timesteps of every finished episode, [1] = 1 when a slot table overflowed */
    double *scratch_rewards;    /* (N): per-step rewards when rewards_out is null */
    int32_t *scratch_dones;     /* (N) */
} fe_evo_population;

/*
 * K steps of the population (the loop agent.step -> env.step -> agent.store of ES_MLP_Isaac_Gym.py, evo_agent.py:89-112,
 * with the per-step nonzero() / .item() host syncs gone).  Accounting and side effects as fe_env_rollout_mlp; a finished
 * episode of env n is appended to episode_returns[n] (or sets counters[1] when its slots are full) and its running
 * return / timesteps are zeroed.  Optional outputs (null = not written): actions_out (K, N, A) f32 (the action the env
 * took, unclamped), means_out (K, N, A) f32 (the same before the action noise), rewards_out (K, N) f64, dones_out (K, N)
 * int32.  Steps of one generation must be issued in order and pop->step must count them: run(32); run(32) equals run(64)
 * bit for bit.  FE_ERR_ARG: null pointers, K < 1, H not 32 / 64, n_train odd / <= 0 / > N, an evaluate-mode env, redraw
 * mode not 1, more than 128 assets, theta larger than the LDS, unbound env.
 */
int fe_evo_rollout(fe_env *env, const fe_evo_population *pop, int32_t K, float *actions_out, float *means_out,
                   double *rewards_out, int32_t *dones_out, void *stream);

/*
 * out[j] = sum_p diffed[p] * z_{g,p,j} for j < num_params, p < num_pairs, in f64 and in a fixed order (ascending pairs in
 * blocks of 64, then ascending blocks; no atomics): two calls give the same bits.  The ES gradient is
 * out / num_pairs - l2 * theta (parallel_mlp.py:176-220 with epsilon = sigma * z).  workspace: the number of doubles
 * fe_evo_gradient_workspace_doubles returns.  Runs on the current device.
 */
int64_t fe_evo_gradient_workspace_doubles(int64_t num_pairs, int64_t num_params);
int fe_evo_gradient(uint64_t seed, uint32_t generation, int64_t num_pairs, int64_t num_params, const float *diffed,
                    double *workspace, double *out, void *stream);

/*
 * out (count, num_params) f32: out[i][j] = z_{g, pairs[i], j} (the perturbation of parallel_mlp.py:127-138 divided by
 * sigma), as the rollout and the gradient generate it.  Runs on the current device.
 */
int fe_evo_noise(uint64_t seed, uint32_t generation, const int64_t *pairs, int64_t count, int64_t num_params, float *out,
                 void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FINENVS_AMD_EVO_H */
