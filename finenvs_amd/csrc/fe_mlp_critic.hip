// fe_mlp_critic.hip -- the second translation unit of libfinenvs_amd.so: the twin MLP critics Q(s, a) of
// include/finenvs_amd_mlp_critic.h (values, Bellman targets, backward).
//
// Why a unit of its own: fe_env.hip's device code object stays what it is when a network family is added here (its
// kernels' registers and occupancy are pinned by the committed resource tables).  The kernels of this unit are in
// fe_mlp_critic_kernels.h; they call the device functions of fe_mlp_head_kernels.h / fe_mlp2_head_kernels.h as they
// stand.  Including those headers emits their four non-template kernels (fe_policy_table_kernel, fe_mlp_pack_kernel,
// fe_mlp_grad_reduce_kernel, fe_mlp2_grad_reduce_kernel) a second time: the last is launched from here too, the
// others are unused.
//
// What the two units share, all host-side: the error buffer (fe_set_error is defined in fe_env.hip; this unit declares
// it -- FE_ERROR_BUFFER_ELSEWHERE -- so fe_last_error returns these entries' messages), an env's shape and the cache of
// per-kernel LDS attributes (two hidden-visibility accessors at the end of fe_env.hip).
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <type_traits>

#include "finenvs_amd.h"
#include "finenvs_amd_mlp_critic.h"

#define FE_ERROR_BUFFER_ELSEWHERE 1
#include "fe_mlp_critic_kernels.h"
#include "fe_host_common.h"

extern "C" __attribute__((visibility("hidden"))) void fe_env_shape_internal(const fe_env *env, int32_t *W, int32_t *A, int *device);
extern "C" __attribute__((visibility("hidden"))) int fe_prepare_big_lds_internal(int device, const void *kern, size_t lds,
                                                                                 const char *who);

namespace {

// (the launch helpers of fe_env.hip this unit needs are restated once for the small units, in fe_host_common.h)
bool weights_ok(const fe_mlpq_weights *w) { return w && w->w1t && w->wpos && w->wact && w->b1 && w->w2 && w->b2 && w->w3 && w->b3; }
bool grads_ok(const fe_mlpq_grads *g) { return g && g->w1 && g->b1 && g->w2 && g->b2 && g->w3 && g->b3; }

struct EnvShape { int32_t W, A; int device; };

// What every entry refuses about the network and the env, in `who`'s name; the admission rule of fe_mlp2_*: the
// two-layer head's image next to a rollout tile of 128 pairs fits the LDS (then this unit's image, H floats more
// than the head's bare image, fits as well -- checked all the same).
int mlpq_checked(const fe_env *env, int32_t H, int32_t activation, EnvShape &s, const char *who) {
    if (H != 32 && H != 64 && H != 128) return fail(FE_ERR_ARG, "%s: H must be 32, 64 or 128 (got %d)", who, (int)H);
    if (activation < 0 || activation > 2) return fail(FE_ERR_ARG, "%s: activation must be 0 (ELU), 1 (ReLU) or 2 (tanh)", who);
    fe_env_shape_internal(env, &s.W, &s.A, &s.device);
    if (s.A != 1)
        return fail(FE_ERR_ARG, "%s: the env has %d assets; the fused MLP critic runs A = 1 only (the reference's critic for "
                    "A > 1 takes the whole env's window and all its actions, not a per-(env, asset) pair)", who, (int)s.A);
    const size_t head = mlp2_lds_bytes(128, 1, s.W, H), image = mlpq_weight_lds_bytes(s.W, H);
    if (head > kMaxLds || image > kMaxLds)
        return fail(FE_ERR_ARG, "%s: W1 (%d x %d) and W2 (%d x %d) do not fit the 160 KiB LDS: the window does not fit (%zu bytes "
                    "needed)", who, (int)H, 4 * s.W, (int)H, (int)H, head > kMaxLds ? head : image);
    return FE_OK;
}

MlpqNet net_of(const fe_mlpq_weights *w, float *q_out) {
    return MlpqNet{w->w1t, w->wpos, w->wact, w->b1, w->w2, w->b2, w->w3, w->b3, q_out};
}

// The forward launch of both critics: blockIdx.y = critic, each looping over all 32-pair blocks.
int launch_forward(const EnvShape &s, MlpqArgs &r, int32_t H, const char *who, const char *what, void *stream) {
    const void *kern = with_nt(H, [](auto NT) { return (const void *)fe_mlpq_forward_kernel<decltype(NT)::value>; });
    const size_t lds = mlpq_weight_lds_bytes(s.W, H);
    if (int rc = fe_prepare_big_lds_internal(s.device, kern, lds, who)) return rc;
    const int64_t blocks = (r.count + 31) / 32;
    const int64_t grid = capped_grid((blocks + kBlock / 64 - 1) / (kBlock / 64));
    void *args[] = {&r};
    return launched(who, what, hipLaunchKernel(kern, dim3((unsigned)grid, 2), dim3(kBlock), args, lds, (hipStream_t)stream));
}

int target_impl(fe_env *env, const float *logret_f32, const fe_mlpq_weights *c1, const fe_mlpq_weights *c2, int32_t H,
                int32_t activation, const fe_replay_ring *ring, int64_t head, int64_t size, const int64_t *cursor,
                const int64_t *indices, int64_t count, const float *next_actions, const float *smooth_noise, float smooth_std,
                float smooth_clip, const float *log_probs, const float *alpha, float gamma, float reward_scale,
                float *targets_out, float *q1_out, float *q2_out, void *stream) {
    static const char *who = "fe_twin_mlpq_target";
    const bool ring_ok = ring && ring->capacity >= 1 && ring->num_assets >= 1 && ring->state_src && ring->state_pos &&
                         ring->next_src && ring->next_pos && ring->actions && ring->rewards && ring->dones && ring->errors;
    if (!env || !logret_f32 || !weights_ok(c1) || !weights_ok(c2) || !ring_ok || !indices || !next_actions || !targets_out ||
        !q1_out || !q2_out || count < 0)
        return fail(FE_ERR_ARG, "%s: bad argument", who);
    if (log_probs && !alpha) return fail(FE_ERR_ARG, "%s: log_probs (SAC) need alpha", who);
    if (smooth_noise && log_probs) return fail(FE_ERR_ARG, "%s: smooth_noise (TD3) and log_probs (SAC) are exclusive", who);
    EnvShape s;
    if (int rc = mlpq_checked(env, H, activation, s, who)) return rc;
    const int64_t C = ring->capacity;
    if (!cursor && (size < 1 || size > C || head < 0 || head >= C))
        return fail(FE_ERR_ARG, "%s: size %lld / head %lld do not describe a non-empty ring of %lld slots", who, (long long)size,
                    (long long)head, (long long)C);
    if (ring->num_assets != 1) return fail(FE_ERR_ARG, "%s: the ring holds %d assets, the env 1", who, (int)ring->num_assets);
    if (count == 0) return FE_OK;
    DeviceGuard guard(s.device);
    if (int rc = guard.status()) return rc;
    const int64_t start = cursor ? 0 : ((head - size) % C + C) % C;
    MlpqArgs r;
    memset(&r, 0, sizeof(r));
    r.lr32 = logret_f32; r.net[0] = net_of(c1, q1_out); r.net[1] = net_of(c2, q2_out);
    r.indices = indices; r.ring_src = ring->next_src; r.ring_pos = ring->next_pos; r.ring_C = C; r.start = start; r.size = size;
    r.cursor = cursor; r.actions = next_actions; r.smooth_noise = smooth_noise; r.smooth_std = smooth_std;
    r.smooth_clip = smooth_clip; r.count = count; r.W = s.W; r.act = activation;
    if (int rc = launch_forward(s, r, H, who, "critics", stream)) return rc;
    MlpqTargetArgs t;
    t.q1 = q1_out; t.q2 = q2_out; t.indices = indices; t.ring_rew = ring->rewards; t.ring_done = ring->dones;
    t.ring_C = C; t.start = start; t.size = size; t.count = count; t.log_probs = log_probs; t.alpha = alpha;
    t.gamma = gamma; t.reward_scale = reward_scale; t.targets = targets_out;
    t.errors = reinterpret_cast<unsigned long long *>(ring->errors);
    t.cursor = cursor;
    hipLaunchKernelGGL(fe_mlpq_target_kernel, dim3(grid_for(count)), dim3(kBlock), 0, (hipStream_t)stream, t);
    return launched(who, "epilogue", hipGetLastError());
}

// The backward's workspace, in floats from its start: fe_mlp2_backward's layout with the wider layer-1 partial
// [dz1 (32 blocks, H)][a1][dz2][layer-1 partials (splits, H, FP)][[dW2 | d b2] partials (splits, H, H + 32)]
// [output-layer partials (waves, H + 4)].  The exported size and the carve-up both read it.
struct MlpqGradLayout {
    int64_t blocks, splits, groups;
    int32_t FP;
    int64_t a1, dz2, part, part2, wpart, total;
};

int mlpq_grad_fp(int W) { return 32 * ((4 * W + 3 + 31) / 32); }

MlpqGradLayout mlpq_grad_layout(int32_t H, int32_t W, int64_t count) {
    MlpqGradLayout l;
    l.blocks = (count + 31) / 32;
    l.splits = (count + kMlpGradChunk - 1) / kMlpGradChunk;
    l.groups = mlp_grad_groups(l.blocks);
    l.FP = mlpq_grad_fp(W);
    const int64_t rows = 32 * l.blocks * H;
    l.a1 = rows;
    l.dz2 = 2 * rows;
    l.part = 3 * rows;
    l.part2 = l.part + l.splits * H * l.FP;
    l.wpart = l.part2 + l.splits * H * (H + 32);
    l.total = l.wpart + 4 * l.groups * (H + 4);
    return l;
}

}  // namespace

extern "C" {

int fe_twin_mlpq_forward(fe_env *env, const float *logret_f32, const fe_mlpq_weights *c1, const fe_mlpq_weights *c2,
                         int32_t H, int32_t activation, const int64_t *obs_src, const double *obs_pos,
                         const float *actions, int64_t count, float *q1_out, float *q2_out, void *stream) {
    static const char *who = "fe_twin_mlpq_forward";
    if (!env || !logret_f32 || !weights_ok(c1) || !weights_ok(c2) || !obs_src || !obs_pos || !actions || !q1_out || !q2_out ||
        count < 0)
        return fail(FE_ERR_ARG, "%s: bad argument", who);
    EnvShape s;
    if (int rc = mlpq_checked(env, H, activation, s, who)) return rc;
    if (count == 0) return FE_OK;
    DeviceGuard guard(s.device);
    if (int rc = guard.status()) return rc;
    MlpqArgs r;
    memset(&r, 0, sizeof(r));
    r.lr32 = logret_f32; r.net[0] = net_of(c1, q1_out); r.net[1] = net_of(c2, q2_out);
    r.obs_src = obs_src; r.obs_pos = obs_pos; r.actions = actions; r.count = count; r.W = s.W; r.act = activation;
    return launch_forward(s, r, H, who, "critics", stream);
}

int fe_twin_mlpq_target(fe_env *env, const float *logret_f32, const fe_mlpq_weights *c1, const fe_mlpq_weights *c2,
                        int32_t H, int32_t activation, const fe_replay_ring *ring, int64_t head, int64_t size,
                        const int64_t *indices, int64_t count, const float *next_actions, const float *smooth_noise,
                        float smooth_std, float smooth_clip, const float *log_probs, const float *alpha, float gamma,
                        float reward_scale, float *targets_out, float *q1_out, float *q2_out, void *stream) {
    return target_impl(env, logret_f32, c1, c2, H, activation, ring, head, size, nullptr, indices, count, next_actions,
                       smooth_noise, smooth_std, smooth_clip, log_probs, alpha, gamma, reward_scale, targets_out, q1_out,
                       q2_out, stream);
}

int fe_twin_mlpq_target_c(fe_env *env, const float *logret_f32, const fe_mlpq_weights *c1, const fe_mlpq_weights *c2,
                          int32_t H, int32_t activation, const fe_replay_ring *ring, const int64_t *cursor,
                          const int64_t *indices, int64_t count, const float *next_actions, const float *smooth_noise,
                          float smooth_std, float smooth_clip, const float *log_probs, const float *alpha, float gamma,
                          float reward_scale, float *targets_out, float *q1_out, float *q2_out, void *stream) {
    if (!cursor) return fail(FE_ERR_ARG, "fe_twin_mlpq_target_c: null cursor");
    return target_impl(env, logret_f32, c1, c2, H, activation, ring, 0, 0, cursor, indices, count, next_actions, smooth_noise,
                       smooth_std, smooth_clip, log_probs, alpha, gamma, reward_scale, targets_out, q1_out, q2_out, stream);
}

int64_t fe_twin_mlpq_grad_workspace_floats(int32_t H, int32_t W, int64_t count) {
    if ((H != 32 && H != 64 && H != 128) || W < 1 || count < 0) return -1;
    return count == 0 ? 0 : mlpq_grad_layout(H, W, count).total;
}

int fe_twin_mlpq_backward(fe_env *env, const float *logret_f32, const fe_mlpq_weights *c1, const fe_mlpq_weights *c2,
                          int32_t H, int32_t activation, const int64_t *obs_src, const double *obs_pos,
                          const float *actions, int64_t count, const float *dq1, const float *dq2, float *workspace,
                          const fe_mlpq_grads *grads1, const fe_mlpq_grads *grads2, float *d_actions, void *stream) {
    static const char *who = "fe_twin_mlpq_backward";
    if (!env || !logret_f32 || !obs_src || !obs_pos || !actions || !workspace || count < 0)
        return fail(FE_ERR_ARG, "%s: bad argument", who);
    const fe_mlpq_weights *c[2] = {c1, c2};
    const float *dq[2] = {dq1, dq2};
    const fe_mlpq_grads *grads[2] = {grads1, grads2};
    for (int i = 0; i < 2; ++i) {
        if (!dq[i]) continue;
        if (!weights_ok(c[i])) return fail(FE_ERR_ARG, "%s: dq%d is given without critic %d's weights", who, i + 1, i + 1);
        if (grads[i] && !grads_ok(grads[i])) return fail(FE_ERR_ARG, "%s: grads%d has a null field", who, i + 1);
        if (!grads[i] && !d_actions)
            return fail(FE_ERR_ARG, "%s: critic %d has neither its gradients nor d_actions: nothing to compute", who, i + 1);
    }
    EnvShape s;
    if (int rc = mlpq_checked(env, H, activation, s, who)) return rc;
    if (count == 0 || (!dq1 && !dq2)) return FE_OK;
    DeviceGuard guard(s.device);
    if (int rc = guard.status()) return rc;
    const hipStream_t st = (hipStream_t)stream;
    const int W = s.W;
    const MlpqGradLayout l = mlpq_grad_layout(H, W, count);
    const void *k1 = with_nt(H, [](auto NT) { return (const void *)fe_mlpq_grad_kernel<decltype(NT)::value>; });
    const void *k2 = with_nt(H, [](auto NT) { return (const void *)fe_mlpq_dgrad_kernel<decltype(NT)::value>; });
    const void *k3 = with_nt(H, [](auto NT) { return (const void *)fe_mlp2_wgrad2_kernel<decltype(NT)::value>; });
    const void *k4 = with_nt(H, [](auto NT) { return (const void *)fe_mlpq_wgrad_kernel<decltype(NT)::value>; });
    const size_t lds1 = mlpq_weight_lds_bytes(W, H);
    const size_t lds2 = ((size_t)H * mlp2_hp(H) + H) * 4;
    const int64_t wave_groups = capped_grid((l.blocks + kBlock / 64 - 1) / (kBlock / 64));
    bool accumulate = false;
    for (int i = 0; i < 2; ++i) {
        if (!dq[i]) continue;
        MlpqGradArgs ga;
        memset(&ga, 0, sizeof(ga));
        MlpGradArgs &g = ga.g2.g;
        g.lr32 = logret_f32; g.w1t = c[i]->w1t; g.wpos = c[i]->wpos; g.b1 = c[i]->b1; g.w2 = c[i]->w3;
        g.obs_src = obs_src; g.obs_pos = obs_pos; g.d_outputs = dq[i];
        g.count = count; g.blocks = l.blocks; g.splits = l.splits; g.waves = 4 * l.groups;
        g.W = W; g.H = H; g.act = activation; g.out_act = 2; g.FP = l.FP;
        g.dpre = workspace; g.part = workspace + l.part; g.wpart = workspace + l.wpart;
        ga.g2.a1 = workspace + l.a1; ga.g2.dz2 = workspace + l.dz2; ga.g2.part2 = workspace + l.part2;
        ga.g2.w2h = c[i]->w2; ga.g2.b2h = c[i]->b2;
        ga.wact = c[i]->wact; ga.actions = actions; ga.d_actions = d_actions; ga.accumulate = accumulate ? 1 : 0;
        if (grads[i]) {
            g.g_w1 = grads[i]->w1; g.g_b1 = grads[i]->b1; g.g_w2 = grads[i]->w3; g.g_b2 = grads[i]->b3;
            ga.g2.g_w2h = grads[i]->w2; ga.g2.g_b2h = grads[i]->b2;
        }
        void *args[] = {&ga};
        // (1) both hidden layers recomputed: a1, dz2, the partials of d w3 / d b3
        if (int rc = fe_prepare_big_lds_internal(s.device, k1, lds1, who)) return rc;
        if (int rc = launched(who, "hidden layers", hipLaunchKernel(k1, dim3((unsigned)l.groups), dim3(kBlock), args, lds1, st))) return rc;
        // (2) dz1 = (W2^T dz2) * act'(z1), dQ/da
        if (int rc = fe_prepare_big_lds_internal(s.device, k2, lds2, who)) return rc;
        if (int rc = launched(who, "W2^T dz2", hipLaunchKernel(k2, dim3((unsigned)wave_groups), dim3(kBlock), args, lds2, st))) return rc;
        if (d_actions) accumulate = true;
        if (!grads[i]) continue;  // frozen: no weight-gradient contraction, no reduction
        // (3) [dW2 | d b2] partials
        void *args2[] = {&ga.g2};
        const int64_t items3 = l.splits * (H / 32 + 1);
        const int64_t grid3 = capped_grid((items3 + kBlock / 64 - 1) / (kBlock / 64));
        if (int rc = launched(who, "dz2^T a1", hipLaunchKernel(k3, dim3((unsigned)grid3), dim3(kBlock), args2, 0, st))) return rc;
        // (4) [dW1t | d wpos | d wact | d b1] partials
        const int64_t items4 = l.splits * (l.FP / 32);
        const int64_t grid4 = capped_grid((items4 + kBlock / 64 - 1) / (kBlock / 64));
        if (int rc = launched(who, "first-layer weight gradient", hipLaunchKernel(k4, dim3((unsigned)grid4), dim3(kBlock), args, 0, st)))
            return rc;
        // (5) the reduction of (4) and of the output layer's partials, (6) the second hidden layer's
        hipLaunchKernelGGL(fe_mlpq_grad_reduce_kernel, dim3(grid_for((int64_t)H * (4 * W + 3) + H + 1)), dim3(kBlock), 0, st, g);
        if (int rc = launched(who, "reduction", hipGetLastError())) return rc;
        hipLaunchKernelGGL(fe_mlp2_grad_reduce_kernel, dim3(grid_for((int64_t)H * (H + 1))), dim3(kBlock), 0, st, ga.g2);
        if (int rc = launched(who, "W2 reduction", hipGetLastError())) return rc;
    }
    return FE_OK;
}

}  // extern "C"
