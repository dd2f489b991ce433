// fe_evo.hip -- the fourth translation unit of libfinenvs_amd.so: the evolution-strategies population of
// include/finenvs_amd_evo.h (one hidden layer; the noise render and the gradient, generic in the parameter count) and
// include/finenvs_amd_evo2.h (two hidden layers).  The kernels are in fe_evo_kernels.h; fe_rollout_kernels.h, which it
// includes, brings fe_policy_table_kernel along, unused here as in the other small units.
//
// Shared with fe_env.hip, all host-side: the error buffer (FE_ERROR_BUFFER_ELSEWHERE), the cache of per-kernel LDS
// attributes, and what a K-step rollout takes from the env (hidden-visibility accessors at the end of fe_env.hip).
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <type_traits>

#include "finenvs_amd.h"
#include "finenvs_amd_evo.h"
#include "finenvs_amd_evo2.h"

#define FE_ERROR_BUFFER_ELSEWHERE 1
#include "fe_evo_kernels.h"
#include "fe_host_common.h"

extern "C" __attribute__((visibility("hidden"))) void fe_env_shape_internal(const fe_env *env, int32_t *W, int32_t *A, int *device);
extern "C" __attribute__((visibility("hidden"))) int fe_env_bound_internal(const fe_env *env);
extern "C" __attribute__((visibility("hidden"))) int fe_prepare_big_lds_internal(int device, const void *kern, size_t lds,
                                                                                 const char *who);
extern "C" __attribute__((visibility("hidden"))) int fe_env_mlp_rollout_internal(const fe_env *env, const char *who, void *params_out,
                                                                                 size_t params_bytes, int64_t *grid_out);

namespace {

// What tells the two rollout entries apart: the name, the depth and the hidden widths that depth has kernels for.
struct EvoEntry {
    const char *who;
    int layers;
    int32_t max_h;       // H = 32, 64, ... up to this
    const char *widths;  // as the refusal of another H spells them
};
constexpr EvoEntry kEvo1{"fe_evo_rollout", 1, 64, "32 or 64"};
constexpr EvoEntry kEvo2{"fe_evo2_rollout", 2, 128, "32, 64 or 128"};

bool evo_h_ok(const EvoEntry &e, int32_t H) { return (H == 32 || H == 64 || H == 128) && H <= e.max_h; }

// PB mirrored pairs per tile (2 PB envs): each wavefront evaluates whole pairs, every z element serves both signs
int evo_pairs_per_tile(int32_t A) {
    int PB = 128 / A;
    if (PB > 8) PB = 8;
    if (PB < 1) PB = 1;
    return PB;
}

// The kernel of an H the entry has accepted: the one-layer rollout has no H = 128 instantiation.
template <int LAYERS>
const void *evo_kernel(bool single, int32_t H) {
    return with_nt(H, [single](auto NT) {
        constexpr int HH = LAYERS == 1 && decltype(NT)::value == 4 ? 64 : 32 * decltype(NT)::value;
        if constexpr (LAYERS == 1)
            return single ? (const void *)fe_evo_rollout_kernel<true, HH> : (const void *)fe_evo_rollout_kernel<false, HH>;
        else
            return single ? (const void *)fe_evo2_rollout_kernel<true, HH> : (const void *)fe_evo2_rollout_kernel<false, HH>;
    });
}

int evo_rollout(const EvoEntry &e, fe_env *env, const fe_evo_population *pop, int32_t K, float *actions_out, float *means_out,
                double *rewards_out, int32_t *dones_out, void *stream) {
    const char *who = e.who;
    if (!env || !pop || K < 1 || !pop->logret_f32 || !pop->theta || !pop->obs_src || !pop->obs_pos || !pop->returns ||
        !pop->timesteps || !pop->episode_returns || !pop->episode_counts || !pop->counters || !pop->scratch_rewards ||
        !pop->scratch_dones)
        return fail(FE_ERR_ARG, "%s: bad argument", who);
    // the one-layer entry's own refusal of an unbound env; the two-layer entry's is the accessor's (FE_ERR_STATE)
    if (e.layers == 1 && !fe_env_bound_internal(env)) return fail(FE_ERR_ARG, "%s: env state not bound", who);
    Params p;
    int64_t grid = 0;
    if (int rc = fe_env_mlp_rollout_internal(env, who, &p, sizeof(p), &grid)) return rc;
    const int32_t H = pop->hidden;
    if (!evo_h_ok(e, H)) return fail(FE_ERR_ARG, "%s: H must be %s (got %d)", who, e.widths, (int)H);
    const int64_t nt = pop->num_train;
    if (nt <= 0 || nt % 2 != 0 || nt > p.N)
        return fail(FE_ERR_ARG, "%s: the %lld training envs must be positive, even and at most N = %lld "
                    "(mirrored sampling, parallel_mlp.py:24-27)", who, (long long)nt, (long long)p.N);
    if (pop->max_episodes < 1) return fail(FE_ERR_ARG, "%s: max_episodes must be >= 1", who);
    if (p.evaluate) return fail(FE_ERR_ARG, "%s: the population needs a training-mode env (evaluate = 0)", who);
    if (p.redraw_mode != 1) return fail(FE_ERR_ARG, "%s: the population needs redraw mode 1 (device redraws)", who);
    if (p.A > 128) return fail(FE_ERR_ARG, "%s: at most 128 assets per env (got %d)", who, (int)p.A);
    int32_t W = 0, A = 0;
    int device = 0;
    fe_env_shape_internal(env, &W, &A, &device);
    DeviceGuard guard(device);
    if (int rc = guard.status()) return rc;
    // one workgroup per tile (capped); the tile is fixed by the pair layout, so the accessor's tile and grid are replaced
    const int PB = evo_pairs_per_tile(p.A);
    const int64_t half = nt / 2;
    const int EB = 2 * PB;
    const int64_t pair_tiles = (half + PB - 1) / PB;
    const int64_t eval_tiles = (p.N - nt + EB - 1) / EB;
    p.EB = EB;
    p.num_tiles = pair_tiles + eval_tiles;
    const int64_t P = evo_num_params(e.layers, p.W, H);
    const size_t lds = evo_lds(e.layers, EB, p.A, P, H).total;
    if (lds > kMaxLds) {
        if (e.layers == 1)
            return fail(FE_ERR_ARG, "%s: theta (%lld floats) does not fit the 160 KiB LDS (%zu bytes needed)", who, (long long)P, lds);
        return fail(FE_ERR_ARG, "%s: theta (%lld floats: W1 (%d x %d), W2 (%d x %d)) does not fit the 160 KiB LDS (%zu bytes "
                    "needed)", who, (long long)P, 5 * p.W, (int)H, (int)H, (int)H, lds);
    }
    EvoArgs r;
    r.lr32 = pop->logret_f32; r.theta = pop->theta; r.obs_src = pop->obs_src; r.obs_pos = pop->obs_pos;
    r.ret = pop->returns; r.ts = pop->timesteps; r.ep_ret = pop->episode_returns; r.ep_cnt = pop->episode_counts;
    r.counters = reinterpret_cast<unsigned long long *>(pop->counters);
    r.actions_out = actions_out; r.means_out = means_out; r.rew_out = rewards_out; r.done_out = dones_out;
    r.rew_scratch = pop->scratch_rewards; r.done_scratch = pop->scratch_dones;
    r.n_train = nt; r.half = half; r.K = K; r.max_ep = pop->max_episodes; r.PB = PB; r.pair_tiles = (int32_t)pair_tiles;
    r.sigma = pop->noise_std; r.nu = pop->action_noise_std; r.seed = pop->seed; r.g = pop->generation; r.step0 = pop->step;
    const void *kern = e.layers == 1 ? evo_kernel<1>(p.A == 1, H) : evo_kernel<2>(p.A == 1, H);
    if (int rc = fe_prepare_big_lds_internal(device, kern, lds, who)) return rc;
    void *args[] = {&p, &r};
    const hipError_t he = hipLaunchKernel(kern, dim3((unsigned)capped_grid(p.num_tiles)), dim3(kBlock), args, lds, (hipStream_t)stream);
    return e.layers == 1 ? launched(who, he) : launched(who, "rollout", he);
}

}  // namespace

extern "C" {

int fe_evo_rollout(fe_env *env, const fe_evo_population *pop, int32_t K, float *actions_out, float *means_out,
                   double *rewards_out, int32_t *dones_out, void *stream) {
    return evo_rollout(kEvo1, env, pop, K, actions_out, means_out, rewards_out, dones_out, stream);
}

int fe_evo2_rollout(fe_env *env, const fe_evo_population *pop, int32_t K, float *actions_out, float *means_out,
                    double *rewards_out, int32_t *dones_out, void *stream) {
    return evo_rollout(kEvo2, env, pop, K, actions_out, means_out, rewards_out, dones_out, stream);
}

int64_t fe_evo2_num_params(int32_t W, int32_t H) {
    if (W < 1 || !evo_h_ok(kEvo2, H)) return -1;
    return evo_num_params(2, W, H);
}

int64_t fe_evo2_lds_bytes(int32_t W, int32_t A, int32_t H) {
    if (W < 1 || A < 1 || A > 128 || !evo_h_ok(kEvo2, H)) return -1;
    return (int64_t)evo_lds(2, 2 * evo_pairs_per_tile(A), A, evo_num_params(2, W, H), H).total;
}

int64_t fe_evo_gradient_workspace_doubles(int64_t num_pairs, int64_t num_params) {
    if (num_pairs < 1 || num_params < 1) return 0;
    return (num_pairs + kEvoGradPairs - 1) / kEvoGradPairs * num_params;
}

int fe_evo_gradient(uint64_t seed, uint32_t generation, int64_t num_pairs, int64_t num_params, const float *diffed,
                    double *workspace, double *out, void *stream) {
    if (!diffed || !workspace || !out || num_pairs < 1 || num_params < 1 || num_pairs > 0xffffffffll ||
        num_params > 4 * 0xffffffffll)
        return fail(FE_ERR_ARG, "fe_evo_gradient: bad argument");
    DeviceGuard guard(device_of(out));
    if (int rc = guard.status("fe_evo_gradient: out is not device memory")) return rc;
    const int64_t blocks = (num_pairs + kEvoGradPairs - 1) / kEvoGradPairs;
    const int64_t threads = blocks * ((num_params + 3) / 4);
    hipLaunchKernelGGL(fe_evo_gradient_partial_kernel, dim3((unsigned)((threads + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       (hipStream_t)stream, seed, generation, num_pairs, num_params, diffed, workspace);
    hipLaunchKernelGGL(fe_evo_gradient_reduce_kernel, dim3((unsigned)((num_params + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       (hipStream_t)stream, blocks, num_params, (const double *)workspace, out);
    return launched("fe_evo_gradient");
}

int fe_evo_noise(uint64_t seed, uint32_t generation, const int64_t *pairs, int64_t count, int64_t num_params, float *out,
                 void *stream) {
    if (!pairs || !out || count < 1 || num_params < 1 || num_params > 4 * 0xffffffffll)
        return fail(FE_ERR_ARG, "fe_evo_noise: bad argument");
    DeviceGuard guard(device_of(out));
    if (int rc = guard.status("fe_evo_noise: out is not device memory")) return rc;
    const int64_t threads = count * ((num_params + 3) / 4);
    hipLaunchKernelGGL(fe_evo_noise_kernel, dim3((unsigned)((threads + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       (hipStream_t)stream, seed, generation, pairs, count, num_params, out);
    return launched("fe_evo_noise");
}

}  // extern "C"
