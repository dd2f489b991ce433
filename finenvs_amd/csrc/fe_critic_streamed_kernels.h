// fe_critic_streamed_kernels.h -- part of fe_env.hip (one translation unit; see the overview there): the twin LSTM
// critics of SAC and TD3 at H = 256 / 512 / 1024 on observation descriptors -- values, Bellman targets and the backward
// pass (include/finenvs_amd_critic_streamed.h).
#pragma once
#include "fe_device_common.h"
#include "fe_lstm_kernel.h"
#include "fe_critic_kernels.h"
#include "fe_lstm_grad_streamed_kernels.h"

namespace {

// ---- CriticLSTM((6, H, 1), W) with the recurrent weights streamed ----
// The network is the one-output head of fe_lstm_grad_streamed_kernels.h with one more input, the action, the same in
// every row of the window: it takes input slot 6 (wx[:, 6] = w_ih[:, 5], the convention of fe_critic_kernels.h), so the
// stash row [h_{t-1} | x_t | 1 | action | 0 ...] still has 32 input columns and the chunk rule does not change.  The
// elementwise dz, dh = W_hh^T dz, the weight transpose, the head and the weight contraction do not depend on the input
// width: the host launches fe_lstm_sgrad_{pack, head, dz, dh, wgrad}_kernel on the LstmSGradArgs below.  New here:
//   forward   fe_lstm_sgrad_forward_kernel's recurrence with xh = (pos, 1, action, 0); descriptors from given arrays or
//             from the replay ring by logical index, TD3's smoothing applied as the action is loaded.  STASH = true is
//             the backward's recompute; STASH = false writes nothing to the workspace and reduces h_W to q_c as
//             fe_rollout_lstm_big_kernel's accounting lane does (bout from the device);
//   da        d_actions[p] = sum_t sum_R wx[R, 6] dz[t, p, R] once the time loop has left dz_t in `gates`;
//   final     fe_lstm_sgrad_final_kernel for six input columns.
// The two critics run one after the other on the same stream, in the same workspace.
struct CriticSGradArgs {
    LstmSGradArgs g;            // what the shared kernels read; g.obs_src / g.obs_pos null when `indices` is given
    const float *actions;       // (cnt) the action in slot 6
    const float *bout;          // (1) on the device (STASH = false)
    float *q_out;               // (cnt) this critic's values (STASH = false)
    // descriptors by logical index of the replay ring (as CriticArgs'), or indices == null
    const int64_t *indices;
    const int64_t *ring_src;
    const double *ring_pos;
    int64_t ring_C, start, size;
    const int64_t *cursor;
    const float *smooth_noise;  // (cnt) standard normals or null: TD3's target smoothing
    float smooth_std, smooth_clip;
    float *da;                  // (cnt) d_actions of this chunk (fe_critic_sgrad_da_kernel)
    int32_t da_add;             // the second critic adds to what the first one wrote
};

__host__ __device__ inline size_t critic_sgrad_forward_lds_bytes(int H) {
    return 32 * 8 + 3 * 32 * 4 + (size_t)32 * (H + 4) * 4;  // src [32] | pos [32] | action [32] | valid [32] | h [32][H + 4]
}

// The tile loop of fe_lstm_sgrad_forward_kernel with the action slot; STASH = true is the backward's recompute.
template <int RTW, bool STASH>
__global__ __launch_bounds__(kLstmBlock, 2) void fe_critic_sgrad_forward_kernel(const CriticSGradArgs a) {
#define FE_LSTM_STREAM_ACTION 1
#include "fe_lstm_stream_sgrad_body.h"
#undef FE_LSTM_STREAM_ACTION
}

// the instantiation for H (host side)
template <bool STASH> const void *critic_sgrad_forward_kernel_for(int32_t H) {
    return H == 256 ? (const void *)fe_critic_sgrad_forward_kernel<4, STASH>
                    : (H == 512 ? (const void *)fe_critic_sgrad_forward_kernel<8, STASH>
                                : (const void *)fe_critic_sgrad_forward_kernel<16, STASH>);
}

// d_actions of one chunk: da[p] = sum_t sum_R wx[R, 6] dz[t, p, R] with dz_t in `gates` (packed row order, as wx).  One
// wavefront per pair: lane l adds its rows 4 l + 256 j .. + 3 in ascending (t, j) order, then the 64 lane sums are added
// in a fixed butterfly.  No float atomics; the first critic overwrites, the second adds.
__global__ __launch_bounds__(kBlock) void fe_critic_sgrad_da_kernel(const CriticSGradArgs a, int32_t H) {
    extern __shared__ __align__(16) unsigned char smem[];
    float *s_w = reinterpret_cast<float *>(smem);  // [4H] wx[:, 6]
    const LstmSGradArgs &g = a.g;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t G4 = 4 * H;
    for (int i = tid; i < G4; i += kBlock) s_w[i] = g.wx[(size_t)i * 8 + 6];
    __syncthreads();
    for (int64_t p = (int64_t)blockIdx.x * (kBlock / 64) + wave; p < g.cnt; p += (int64_t)gridDim.x * (kBlock / 64)) {
        float s = 0.0f;
        for (int t = 0; t < g.W; ++t) {
            const float *z = g.gates + ((int64_t)t * g.pp + p) * G4;
            for (int64_t R = 4 * lane; R < G4; R += 256) {
                const float4 zv = *reinterpret_cast<const float4 *>(z + R);
                const float4 wv = *reinterpret_cast<const float4 *>(s_w + R);
                s = fmaf(wv.x, zv.x, s);
                s = fmaf(wv.y, zv.y, s);
                s = fmaf(wv.z, zv.z, s);
                s = fmaf(wv.w, zv.w, s);
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
        if (lane == 0) a.da[p] = a.da_add ? a.da[p] + s : s;
    }
}

// lstm_sgrad_final for the critic's six input columns
__global__ __launch_bounds__(kBlock) void fe_critic_sgrad_final_kernel(const LstmSGradArgs g, int32_t H) {
    lstm_sgrad_final<6>(g, H);
}

}  // namespace
