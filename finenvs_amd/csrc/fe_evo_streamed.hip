// fe_evo_streamed.hip -- the fifth translation unit of libfinenvs_amd.so: the two-hidden-layer ES population with theta read
// through L2 instead of an LDS copy (include/finenvs_amd_evo2_streamed.h), which admits the reference's width H = 256 and
// any window.  The kernels are fe_evo_kernels.h's tile loop and policy with the streamed switch set; the host path is
// fe_evo_host.h, fe_evo.hip's.  The unit re-emits the non-template kernels of the headers it includes (the gradient and noise
// kernels, fe_policy_table_kernel), unused here; fe_evo.hip launches its own.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "finenvs_amd.h"
#include "finenvs_amd_evo.h"
#include "finenvs_amd_evo2_streamed.h"

#define FE_ERROR_BUFFER_ELSEWHERE 1
#include "fe_evo_kernels.h"
#include "fe_host_common.h"
#include "fe_evo_host.h"

namespace {

// fe_host_common.h's with_nt knows three widths; the fourth is dispatched here
template <bool SINGLE>
const void *evo_streamed_kernel_of(int32_t H) {
    switch (H) {
        case 32: return (const void *)fe_evo2_streamed_rollout_kernel<SINGLE, 32>;
        case 64: return (const void *)fe_evo2_streamed_rollout_kernel<SINGLE, 64>;
        case 128: return (const void *)fe_evo2_streamed_rollout_kernel<SINGLE, 128>;
        default: return (const void *)fe_evo2_streamed_rollout_kernel<SINGLE, 256>;
    }
}

const void *evo_streamed_kernel(bool single, int32_t H) {
    return single ? evo_streamed_kernel_of<true>(H) : evo_streamed_kernel_of<false>(H);
}

constexpr EvoEntry kEvo2Streamed{"fe_evo2_rollout_streamed", 2, 256, "32, 64, 128 or 256", true, evo_streamed_kernel};

}  // namespace

extern "C" {

int fe_evo2_rollout_streamed(fe_env *env, const fe_evo_population *pop, int32_t K, float *actions_out, float *means_out,
                             double *rewards_out, int32_t *dones_out, void *stream) {
    return evo_rollout(kEvo2Streamed, env, pop, K, actions_out, means_out, rewards_out, dones_out, stream);
}

int64_t fe_evo2_streamed_num_params(int32_t W, int32_t H) {
    if (W < 1 || !evo_h_ok(kEvo2Streamed, H)) return -1;
    return evo_num_params(2, W, H);
}

int64_t fe_evo2_streamed_lds_bytes(int32_t W, int32_t A, int32_t H) {
    if (W < 1 || A < 1 || A > 128 || !evo_h_ok(kEvo2Streamed, H)) return -1;
    return (int64_t)evo_launch_lds(kEvo2Streamed, W, A, H);
}

}  // extern "C"
