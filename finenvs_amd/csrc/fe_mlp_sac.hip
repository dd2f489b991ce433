// fe_mlp_sac.hip -- the third translation unit of libfinenvs_amd.so: the SAC MLP actor of
// include/finenvs_amd_mlp_sac.h (fold / pack, sampled rollout, forward, backward).
//
// A unit of its own for fe_mlp_critic.hip's reason: the kernel sets of fe_env.hip and fe_mlp_critic.hip are pinned by the
// committed resource tables.  The kernels are in fe_mlp_sac_kernels.h; they call the device functions of
// fe_mlp_head_kernels.h as they stand.  Including that header emits its non-template kernels a third time
// (fe_policy_table_kernel, fe_mlp_pack_kernel, fe_mlp_grad_reduce_kernel: unused here) and instantiates
// fe_mlp_wgrad_kernel, which the backward launches on dz1.
//
// Shared with fe_env.hip, all host-side: the error buffer (FE_ERROR_BUFFER_ELSEWHERE), an env's shape, the cache of
// per-kernel LDS attributes, and what a K-step MLP rollout takes from the env (three hidden-visibility accessors at the
// end of fe_env.hip).
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <type_traits>

#include "finenvs_amd.h"
#include "finenvs_amd_mlp_sac.h"

#define FE_ERROR_BUFFER_ELSEWHERE 1
#include "fe_mlp_sac_kernels.h"
#include "fe_host_common.h"

extern "C" __attribute__((visibility("hidden"))) void fe_env_shape_internal(const fe_env *env, int32_t *W, int32_t *A, int *device);
extern "C" __attribute__((visibility("hidden"))) int fe_prepare_big_lds_internal(int device, const void *kern, size_t lds,
                                                                                 const char *who);
extern "C" __attribute__((visibility("hidden"))) int fe_env_mlp_rollout_internal(const fe_env *env, const char *who, void *params_out,
                                                                                 size_t params_bytes, int64_t *grid_out);

namespace {

static_assert(kMlpGradChunk == FE_MLP_SAC_GRAD_CHUNK_PAIRS, "the header's chunk is the weight-gradient kernel's");
static_assert(kMlpSacGradMaxGroups == FE_MLP_SAC_GRAD_MAX_GROUPS, "the header's group cap is the kernel's");

// f(std::bool_constant<SINGLE>, std::integral_constant<int, NT>)
template <class F>
auto with_single_nt(bool single, int32_t H, F &&f) {
    return single ? with_nt(H, [&](auto NT) { return f(std::true_type{}, NT); }) : with_nt(H, [&](auto NT) { return f(std::false_type{}, NT); });
}

bool weights_ok(const fe_mlp_sac_weights *w) {
    return w && w->w1t && w->wpos && w->b1 && w->w2 && w->b2 && w->wmu && w->bmu && w->wstd && w->bstd && w->vmu && w->vstd &&
           w->cfold;
}
bool grads_ok(const fe_mlp_sac_grads *g) { return g && g->w1 && g->b1 && g->w2 && g->b2 && g->w_mu && g->b_mu && g->w_std && g->b_std; }

int shape_checked(int32_t H, int32_t activation, const char *who) {
    if (H != 32 && H != 64 && H != 128) return fail(FE_ERR_ARG, "%s: H must be 32, 64 or 128 (got %d)", who, (int)H);
    if (activation < 0 || activation > 2) return fail(FE_ERR_ARG, "%s: activation must be 0 (ELU), 1 (ReLU) or 2 (tanh)", who);
    return FE_OK;
}

struct EnvShape { int32_t W, A; int device; };

// The admission rule of every entry: the image fits next to the rollout's default tile of 128 pairs.
int fits_checked(const fe_env *env, int32_t H, EnvShape &s, const char *who) {
    fe_env_shape_internal(env, &s.W, &s.A, &s.device);
    const int eb = 128 / s.A > 1 ? 128 / s.A : 1;
    const size_t lds = mlp_sac_lds_bytes(eb, s.A, s.W, H);
    if (lds > kMaxLds)
        return fail(FE_ERR_ARG, "%s: W1 (%d x %d) does not fit the 160 KiB LDS (%zu bytes needed)", who, (int)H, 4 * s.W, lds);
    return FE_OK;
}

MlpSacArgs sac_args(const float *logret_f32, const fe_mlp_sac_weights *w, int32_t activation) {
    MlpSacArgs r;
    memset(&r, 0, sizeof(r));
    r.lr32 = logret_f32; r.w1t = w->w1t; r.wpos = w->wpos; r.b1 = w->b1; r.vmu = w->vmu; r.vstd = w->vstd; r.cfold = w->cfold;
    r.act = activation; r.K = 1;
    return r;
}

// The backward's workspace, in floats from its start:
// [dz1 (32 blocks, H)][layer-1 partials (splits, H, FP)][[A_mu | S_mu | A_q | S_q] partials (waves, 2 (H + 4))].
// The exported size and the carve-up both read it.
struct SacGradLayout {
    int64_t blocks, splits, groups;
    int32_t FP;
    int64_t part, wpart, total;
};

SacGradLayout sac_grad_layout(int32_t H, int32_t W, int64_t count) {
    SacGradLayout l;
    l.blocks = (count + 31) / 32;
    l.splits = (count + kMlpGradChunk - 1) / kMlpGradChunk;
    l.groups = mlp_sac_grad_groups(l.blocks);
    l.FP = mlp_grad_fp(W);
    l.part = 32 * l.blocks * H;
    l.wpart = l.part + l.splits * H * l.FP;
    l.total = l.wpart + 4 * l.groups * 2 * (H + 4);
    return l;
}

}  // namespace

extern "C" {

int fe_mlp_sac_pack(const float *weight1, const float *w2, const float *b2, const float *wmu, const float *bmu,
                    const float *wstd, const float *bstd, int32_t H, int32_t W, float *w1t, float *wpos, float *vmu,
                    float *vstd, float *cfold, void *stream) {
    static const char *who = "fe_mlp_sac_pack";
    if (!weight1 || !w2 || !b2 || !wmu || !bmu || !wstd || !bstd || !w1t || !wpos || !vmu || !vstd || !cfold)
        return fail(FE_ERR_ARG, "%s: bad argument", who);
    if (H != 32 && H != 64 && H != 128) return fail(FE_ERR_ARG, "%s: H must be 32, 64 or 128 (got %d)", who, (int)H);
    if (W < 1) return fail(FE_ERR_ARG, "%s: W must be >= 1 (got %d)", who, (int)W);
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, weight1) != hipSuccess) {
        (void)hipGetLastError();
        return fail(FE_ERR_ARG, "%s: weight1 is not device memory", who);
    }
    DeviceGuard guard(attr.device);
    if (int rc = guard.status()) return rc;
    hipLaunchKernelGGL(fe_mlp_sac_pack_kernel, dim3(grid_for((int64_t)H * 4 * W + 3 * (int64_t)H + 2)), dim3(kBlock), 0,
                       (hipStream_t)stream, weight1, w2, b2, wmu, bmu, wstd, bstd, (int)H, (int)W, w1t, wpos, vmu, vstd, cfold);
    return launched(who, "pack", hipGetLastError());
}

int fe_env_rollout_mlp_sac(fe_env *env, const float *logret_f32, const fe_mlp_sac_weights *weights, int32_t H,
                           int32_t activation, int32_t K, int64_t *obs_src, double *obs_pos, const float *noise,
                           float *actions_out, float *means_out, float *stds_out, double *rewards_out,
                           int32_t *dones_out, int64_t *states_src_out, double *states_pos_out, void *stream) {
    static const char *who = "fe_env_rollout_mlp_sac";
    if (!env || !logret_f32 || !weights_ok(weights) || !obs_src || !obs_pos || !rewards_out || !dones_out)
        return fail(FE_ERR_ARG, "%s: bad argument", who);
    if (int rc = shape_checked(H, activation, who)) return rc;
    if (K < 1) return fail(FE_ERR_ARG, "%s: bad argument (K must be >= 1)", who);
    if ((states_src_out == nullptr) != (states_pos_out == nullptr))
        return fail(FE_ERR_ARG, "%s: states_src_out and states_pos_out go together", who);
    Params p;
    int64_t grid = 0;
    if (int rc = fe_env_mlp_rollout_internal(env, who, &p, sizeof(p), &grid)) return rc;
    EnvShape s;
    if (int rc = fits_checked(env, H, s, who)) return rc;
    DeviceGuard guard(s.device);
    if (int rc = guard.status()) return rc;
    MlpSacArgs r = sac_args(logret_f32, weights, activation);
    r.K = K; r.obs_src = obs_src; r.obs_pos = obs_pos; r.noise = noise; r.actions_out = actions_out; r.means_out = means_out;
    r.stds_out = stds_out; r.rew_out = rewards_out; r.done_out = dones_out; r.traj_src = states_src_out; r.traj_pos = states_pos_out;
    const size_t lds = mlp_sac_lds_bytes(p.EB, p.A, p.W, H);
    if (lds > kMaxLds)  // (a tile override larger than the default)
        return fail(FE_ERR_ARG, "%s: W1 (%d x %d) does not fit the 160 KiB LDS at this tile (%zu bytes needed)", who, (int)H, 4 * p.W, lds);
    const void *kern = with_single_nt(p.A == 1, H, [](auto S, auto NT) {
        return (const void *)fe_rollout_mlp_sac_kernel<decltype(S)::value, decltype(NT)::value>;
    });
    if (int rc = fe_prepare_big_lds_internal(s.device, kern, lds, who)) return rc;
    void *args[] = {&p, &r};
    return launched(who, "rollout", hipLaunchKernel(kern, dim3((unsigned)grid), dim3(kBlock), args, lds, (hipStream_t)stream));
}

int fe_mlp_sac_forward(fe_env *env, const float *logret_f32, const fe_mlp_sac_weights *weights, int32_t H,
                       int32_t activation, const int64_t *obs_src, const double *obs_pos, int64_t count,
                       const float *noise, float *actions_out, float *log_probs_out, float *means_out, float *stds_out,
                       void *stream) {
    static const char *who = "fe_mlp_sac_forward";
    if (!env || !logret_f32 || !weights_ok(weights) || !obs_src || !obs_pos) return fail(FE_ERR_ARG, "%s: bad argument", who);
    if (int rc = shape_checked(H, activation, who)) return rc;
    if (count < 0) return fail(FE_ERR_ARG, "%s: bad argument (count must be >= 0)", who);
    if (!noise && (actions_out || log_probs_out)) return fail(FE_ERR_ARG, "%s: actions_out / log_probs_out need noise", who);
    EnvShape s;
    if (int rc = fits_checked(env, H, s, who)) return rc;
    if (count == 0) return FE_OK;
    DeviceGuard guard(s.device);
    if (int rc = guard.status()) return rc;
    Params p;
    memset(&p, 0, sizeof(p));  // the kernel reads W and A only
    p.W = s.W; p.A = s.A;
    MlpSacArgs r = sac_args(logret_f32, weights, activation);
    r.obs_src = const_cast<int64_t *>(obs_src); r.obs_pos = const_cast<double *>(obs_pos);  // read only in this kernel
    r.noise = noise; r.actions_out = actions_out; r.logp_out = log_probs_out; r.means_out = means_out; r.stds_out = stds_out;
    r.count = count;
    const int64_t blocks = (count * s.A + 31) / 32;
    const int64_t grid = capped_grid((blocks + kBlock / 64 - 1) / (kBlock / 64));
    const size_t lds = mlp_sac_weight_lds_bytes(s.W, H);
    const void *kern = with_single_nt(s.A == 1, H, [](auto S, auto NT) {
        return (const void *)fe_mlp_sac_forward_kernel<decltype(S)::value, decltype(NT)::value>;
    });
    if (int rc = fe_prepare_big_lds_internal(s.device, kern, lds, who)) return rc;
    void *args[] = {&p, &r};
    return launched(who, "forward", hipLaunchKernel(kern, dim3((unsigned)grid), dim3(kBlock), args, lds, (hipStream_t)stream));
}

int64_t fe_mlp_sac_grad_workspace_floats(int32_t H, int32_t W, int64_t count) {
    if ((H != 32 && H != 64 && H != 128) || W < 1 || count < 0) return -1;
    return count == 0 ? 0 : sac_grad_layout(H, W, count).total;
}

int fe_mlp_sac_backward(fe_env *env, const float *logret_f32, const fe_mlp_sac_weights *weights, int32_t H,
                        int32_t activation, const int64_t *obs_src, const double *obs_pos, int64_t count,
                        const float *noise, const float *actions, const float *stds, const float *d_actions,
                        const float *d_log_probs, float *workspace, const fe_mlp_sac_grads *grads, void *stream) {
    static const char *who = "fe_mlp_sac_backward";
    if (!env || !logret_f32 || !weights_ok(weights) || !obs_src || !obs_pos || !noise || !actions || !stds || !workspace ||
        !grads_ok(grads))
        return fail(FE_ERR_ARG, "%s: bad argument", who);
    if (int rc = shape_checked(H, activation, who)) return rc;
    if (count < 0) return fail(FE_ERR_ARG, "%s: bad argument (count must be >= 0)", who);
    if (!d_actions && !d_log_probs) return fail(FE_ERR_ARG, "%s: d_actions and d_log_probs are both null: nothing to compute", who);
    EnvShape s;
    if (int rc = fits_checked(env, H, s, who)) return rc;
    if (s.A != 1)
        return fail(FE_ERR_ARG, "%s: the env has %d assets; the fused actor gradient runs A = 1 only (its consumer, the fused "
                    "twin critic, does)", who, (int)s.A);
    if (count == 0) return FE_OK;
    DeviceGuard guard(s.device);
    if (int rc = guard.status()) return rc;
    const hipStream_t st = (hipStream_t)stream;
    const int W = s.W;
    const SacGradLayout l = sac_grad_layout(H, W, count);
    MlpSacGradArgs ga;
    memset(&ga, 0, sizeof(ga));
    MlpGradArgs &g = ga.g;
    g.lr32 = logret_f32; g.w1t = weights->w1t; g.wpos = weights->wpos; g.b1 = weights->b1; g.w2 = weights->vmu;
    g.obs_src = obs_src; g.obs_pos = obs_pos;
    g.count = count; g.blocks = l.blocks; g.splits = l.splits; g.waves = 4 * l.groups;
    g.W = W; g.H = H; g.act = activation; g.out_act = 2; g.FP = l.FP;
    g.dpre = workspace; g.part = workspace + l.part; g.wpart = workspace + l.wpart;
    g.g_w1 = grads->w1; g.g_b1 = grads->b1;
    ga.vstd = weights->vstd; ga.cfold = weights->cfold;
    ga.w2h = weights->w2; ga.b2h = weights->b2; ga.wmu = weights->wmu; ga.wstd = weights->wstd;
    ga.noise = noise; ga.actions = actions; ga.stds = stds; ga.d_actions = d_actions; ga.d_logp = d_log_probs;
    ga.g_w2h = grads->w2; ga.g_b2h = grads->b2; ga.g_wmu = grads->w_mu; ga.g_bmu = grads->b_mu; ga.g_wstd = grads->w_std;
    ga.g_bstd = grads->b_std;
    const void *k1 = with_nt(H, [](auto NT) { return (const void *)fe_mlp_sac_grad_kernel<decltype(NT)::value>; });
    const void *k2 = with_nt(H, [](auto NT) { return (const void *)fe_mlp_wgrad_kernel<decltype(NT)::value>; });
    const size_t lds = mlp_sac_weight_lds_bytes(W, H);
    void *args[] = {&ga};
    // (1) a1 recomputed, the head's backward per pair: dz1 and the partials of [A_mu | S_mu | A_q | S_q]
    if (int rc = fe_prepare_big_lds_internal(s.device, k1, lds, who)) return rc;
    if (int rc = launched(who, "first layer", hipLaunchKernel(k1, dim3((unsigned)l.groups), dim3(kBlock), args, lds, st))) return rc;
    // (2) [dW1t | d wpos | d b1] partials from dz1
    void *args2[] = {&ga.g};
    const int64_t items = l.splits * (l.FP / 32);
    const int64_t grid2 = capped_grid((items + kBlock / 64 - 1) / (kBlock / 64));
    if (int rc = launched(who, "weight gradient", hipLaunchKernel(k2, dim3((unsigned)grid2), dim3(kBlock), args2, 0, st))) return rc;
    // (3) the reduction of (2) and the O(H^2) epilogue
    const int64_t work = (int64_t)H * (4 * W + 2) + (int64_t)H * H + 3 * (int64_t)H + 2;
    hipLaunchKernelGGL(fe_mlp_sac_grad_reduce_kernel, dim3(grid_for(work)), dim3(kBlock), 0, st, ga);
    return launched(who, "reduction", hipGetLastError());
}

}  // extern "C"
