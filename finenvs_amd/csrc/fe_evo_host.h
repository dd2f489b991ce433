// fe_evo_host.h -- the host path of the ES population's rollout entries, shared by fe_evo.hip (fe_evo_rollout,
// fe_evo2_rollout: theta copied into the LDS) and fe_evo_streamed.hip (fe_evo2_rollout_streamed: theta read through L2).
// Included after fe_evo_kernels.h and fe_host_common.h.  Host code only.
#pragma once

extern "C" __attribute__((visibility("hidden"))) void fe_env_shape_internal(const fe_env *env, int32_t *W, int32_t *A, int *device);
extern "C" __attribute__((visibility("hidden"))) int fe_env_bound_internal(const fe_env *env);
extern "C" __attribute__((visibility("hidden"))) int fe_prepare_big_lds_internal(int device, const void *kern, size_t lds,
                                                                                 const char *who);
extern "C" __attribute__((visibility("hidden"))) int fe_env_mlp_rollout_internal(const fe_env *env, const char *who, void *params_out,
                                                                                 size_t params_bytes, int64_t *grid_out);

namespace {

// What tells the rollout entries apart: the name, the depth, the hidden widths that entry has kernels for, whether theta
// stays in global memory, and the kernel of an accepted H.
struct EvoEntry {
    const char *who;
    int layers;
    int32_t max_h;       // H = 32, 64, ... up to this
    const char *widths;  // as the refusal of another H spells them
    bool streamed;       // no LDS copy of theta: nothing of it to refuse
    const void *(*kernel)(bool single, int32_t H);
};

[[maybe_unused]] bool evo_h_ok(const EvoEntry &e, int32_t H) {
    return (H == 32 || H == 64 || H == 128 || H == 256) && H <= e.max_h;
}

// PB mirrored pairs per tile (2 PB envs): each wavefront evaluates whole pairs, every z element serves both signs
[[maybe_unused]] int evo_pairs_per_tile(int32_t A) {
    int PB = 128 / A;
    if (PB > 8) PB = 8;
    if (PB < 1) PB = 1;
    return PB;
}

// Bytes of LDS a launch of the entry takes (evo_lds with the tile of A assets; without theta when it is streamed)
[[maybe_unused]] size_t evo_launch_lds(const EvoEntry &e, int32_t W, int32_t A, int32_t H) {
    return evo_lds(e.layers, 2 * evo_pairs_per_tile(A), A, e.streamed ? 0 : evo_num_params(e.layers, W, H), H).total;
}

[[maybe_unused]] int evo_rollout(const EvoEntry &e, fe_env *env, const fe_evo_population *pop, int32_t K, float *actions_out,
                                 float *means_out, double *rewards_out, int32_t *dones_out, void *stream) {
    const char *who = e.who;
    if (!env || !pop || K < 1 || !pop->logret_f32 || !pop->theta || !pop->obs_src || !pop->obs_pos || !pop->returns ||
        !pop->timesteps || !pop->episode_returns || !pop->episode_counts || !pop->counters || !pop->scratch_rewards ||
        !pop->scratch_dones)
        return fail(FE_ERR_ARG, "%s: bad argument", who);
    // the one-layer entry's own refusal of an unbound env; the two-layer entries' is the accessor's (FE_ERR_STATE)
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
    const size_t lds = evo_launch_lds(e, p.W, p.A, H);
    if (!e.streamed && lds > kMaxLds) {
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
    const void *kern = e.kernel(p.A == 1, H);
    if (int rc = fe_prepare_big_lds_internal(device, kern, lds, who)) return rc;
    void *args[] = {&p, &r};
    const hipError_t he = hipLaunchKernel(kern, dim3((unsigned)capped_grid(p.num_tiles)), dim3(kBlock), args, lds, (hipStream_t)stream);
    return e.layers == 1 ? launched(who, he) : launched(who, "rollout", he);
}

}  // namespace
