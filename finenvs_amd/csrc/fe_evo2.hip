// fe_evo2.hip -- the fourth translation unit of libfinenvs_amd.so: the evolution-strategies population with two hidden
// layers of include/finenvs_amd_evo2.h (the K-step rollout; the noise render and the gradient are fe_env.hip's, generic in
// the parameter count).
//
// A unit of its own for fe_mlp_critic.hip's reason: the kernel sets of the other units are pinned by the committed resource
// tables.  The kernel is in fe_evo2_kernels.h; it calls the device functions of fe_evo_kernels.h as they stand.  Including
// that header emits its three non-template kernels again (fe_evo_gradient_partial_kernel, fe_evo_gradient_reduce_kernel,
// fe_evo_noise_kernel) and fe_rollout_kernels.h's fe_policy_table_kernel: all unused here.
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
#include "finenvs_amd_evo2.h"

#define FE_ERROR_BUFFER_ELSEWHERE 1
#include "fe_evo2_kernels.h"
#include "fe_host_common.h"

extern "C" __attribute__((visibility("hidden"))) void fe_env_shape_internal(const fe_env *env, int32_t *W, int32_t *A, int *device);
extern "C" __attribute__((visibility("hidden"))) int fe_prepare_big_lds_internal(int device, const void *kern, size_t lds,
                                                                                 const char *who);
extern "C" __attribute__((visibility("hidden"))) int fe_env_mlp_rollout_internal(const fe_env *env, const char *who, void *params_out,
                                                                                 size_t params_bytes, int64_t *grid_out);

namespace {

bool evo2_h_ok(int32_t H) { return H == 32 || H == 64 || H == 128; }

// PB mirrored pairs per tile (fe_evo_rollout's rule)
int evo2_pairs_per_tile(int32_t A) {
    int PB = 128 / A;
    if (PB > 8) PB = 8;
    if (PB < 1) PB = 1;
    return PB;
}

}  // namespace

extern "C" {

int64_t fe_evo2_num_params(int32_t W, int32_t H) {
    if (W < 1 || !evo2_h_ok(H)) return -1;
    return evo2_num_params(W, H);
}

int64_t fe_evo2_lds_bytes(int32_t W, int32_t A, int32_t H) {
    if (W < 1 || A < 1 || A > 128 || !evo2_h_ok(H)) return -1;
    return (int64_t)evo2_lds_bytes(2 * evo2_pairs_per_tile(A), A, W, H);
}

int fe_evo2_rollout(fe_env *env, const fe_evo_population *pop, int32_t K, float *actions_out, float *means_out,
                    double *rewards_out, int32_t *dones_out, void *stream) {
    static const char *who = "fe_evo2_rollout";
    if (!env || !pop || K < 1 || !pop->logret_f32 || !pop->theta || !pop->obs_src || !pop->obs_pos || !pop->returns ||
        !pop->timesteps || !pop->episode_returns || !pop->episode_counts || !pop->counters || !pop->scratch_rewards ||
        !pop->scratch_dones)
        return fail(FE_ERR_ARG, "%s: bad argument", who);
    Params p;
    int64_t grid = 0;
    if (int rc = fe_env_mlp_rollout_internal(env, who, &p, sizeof(p), &grid)) return rc;  // (refuses an unbound env)
    const int32_t H = pop->hidden;
    if (!evo2_h_ok(H)) return fail(FE_ERR_ARG, "%s: H must be 32, 64 or 128 (got %d)", who, (int)H);
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
    // a tile = PB mirrored pairs (2 PB envs), fixed by the pair layout: the accessor's tile and grid are replaced
    const int PB = evo2_pairs_per_tile(p.A);
    const int64_t half = nt / 2;
    const int EB = 2 * PB;
    const int64_t pair_tiles = (half + PB - 1) / PB;
    const int64_t eval_tiles = (p.N - nt + EB - 1) / EB;
    p.EB = EB;
    p.num_tiles = pair_tiles + eval_tiles;
    const size_t lds = evo2_lds_bytes(EB, p.A, p.W, H);
    if (lds > kMaxLds)
        return fail(FE_ERR_ARG, "%s: theta (%lld floats: W1 (%d x %d), W2 (%d x %d)) does not fit the 160 KiB LDS (%zu bytes "
                    "needed)", who, (long long)evo2_num_params(p.W, H), 5 * p.W, (int)H, (int)H, (int)H, lds);
    EvoArgs r;
    r.lr32 = pop->logret_f32; r.theta = pop->theta; r.obs_src = pop->obs_src; r.obs_pos = pop->obs_pos;
    r.ret = pop->returns; r.ts = pop->timesteps; r.ep_ret = pop->episode_returns; r.ep_cnt = pop->episode_counts;
    r.counters = reinterpret_cast<unsigned long long *>(pop->counters);
    r.actions_out = actions_out; r.means_out = means_out; r.rew_out = rewards_out; r.done_out = dones_out;
    r.rew_scratch = pop->scratch_rewards; r.done_scratch = pop->scratch_dones;
    r.n_train = nt; r.half = half; r.K = K; r.max_ep = pop->max_episodes; r.PB = PB; r.pair_tiles = (int32_t)pair_tiles;
    r.sigma = pop->noise_std; r.nu = pop->action_noise_std; r.seed = pop->seed; r.g = pop->generation; r.step0 = pop->step;
    const bool single = p.A == 1;
    const void *kern = with_nt(H, [single](auto NT) {
        constexpr int HH = 32 * decltype(NT)::value;
        return single ? (const void *)fe_evo2_rollout_kernel<true, HH> : (const void *)fe_evo2_rollout_kernel<false, HH>;
    });
    if (int rc = fe_prepare_big_lds_internal(device, kern, lds, who)) return rc;
    void *args[] = {&p, &r};
    return launched(who, "rollout",
                    hipLaunchKernel(kern, dim3((unsigned)capped_grid(p.num_tiles)), dim3(kBlock), args, lds, (hipStream_t)stream));
}

}  // extern "C"
