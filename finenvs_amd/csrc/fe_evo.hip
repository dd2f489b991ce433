// fe_evo.hip -- the fourth translation unit of libfinenvs_amd.so: the evolution-strategies population of
// include/finenvs_amd_evo.h (one hidden layer; the noise render and the gradient, generic in the parameter count) and
// include/finenvs_amd_evo2.h (two hidden layers).  The kernels are in fe_evo_kernels.h; fe_rollout_kernels.h, which it
// includes, brings fe_policy_table_kernel along, unused here as in the other small units.
//
// The rollout entries' host path is fe_evo_host.h, shared with fe_evo_streamed.hip.  Shared with fe_env.hip, all
// host-side: the error buffer (FE_ERROR_BUFFER_ELSEWHERE), the cache of per-kernel LDS attributes, and what a K-step
// rollout takes from the env (hidden-visibility accessors at the end of fe_env.hip).
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
#include "fe_evo_host.h"

namespace {

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

constexpr EvoEntry kEvo1{"fe_evo_rollout", 1, 64, "32 or 64", false, evo_kernel<1>};
constexpr EvoEntry kEvo2{"fe_evo2_rollout", 2, 128, "32, 64 or 128", false, evo_kernel<2>};

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
    return (int64_t)evo_launch_lds(kEvo2, W, A, H);
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
