// fe_critic_kernels.h -- part of fe_env.hip (one translation unit; see the overview there): the twin LSTM critics of
// SAC and TD3 on the register-resident recurrence, and their Bellman-target epilogue (include/finenvs_amd_critic.h).
#pragma once
#include "fe_device_common.h"
#include "fe_lstm_kernel.h"
#include "fe_replay_kernels.h"

namespace {

// ---- the reference's CriticLSTM((6, H, 1), W) per descriptor (finenvs/agents/SAC/critic.py, networks/lstm.py:28-57) ----
// nn.LSTM(6, H) over [state row | action] (agent_utils.py:5-14 repeats the action over the window), Linear(H, 1) +
// Identity on h_W.  The recurrence is fe_rollout_lstm_kernel's, included as source text (fe_lstm_rollout_body.h,
// FE_LSTM_CRITIC_HEAD): its K = 8 input slots are [logret row (4) | pos | 1 | 0 | 0] with wx = [w_ih (5) | b_ih + b_hh |
// 0 | 0]; the critic's sixth input, the same in every row, takes slot 6 -- wx[:, 6] = w_ih[:, 5], x[6] = the action --
// so the gate layout, the k order and the cell update are unchanged, and with w_ih[:, 5] = 0 a critic's value equals
// fe_lstm_forward's (out_activation 2) bit for bit.
// Both critics keep their recurrent weights in registers for the whole launch: at H = 128 one set is 128 VGPRs per lane,
// two do not fit, so the grid is split by critic -- blockIdx.y = c runs critic c over all tiles -- and each half writes
// its q_c.  A small second launch (fe_twin_q_target_kernel) takes the min and forms the target.
struct CriticNet {
    const float *whh, *wx, *wout;  // packed as for fe_env_rollout_lstm (wx slot 6 = the action's input weight)
    const float *bout;             // (1) on the device: no host round trip for a soft-updated bias
    float *q_out;                  // (count) this critic's values
};

struct CriticArgs {
    LstmArgs l;          // the recurrence's arguments (lr32, H, K = 1, forward_only); whh / wx / wout come from net[c]
    CriticNet net[2];
    // descriptors: l.obs_src (count) / l.obs_pos (count) given, or -- indices != null -- the next-state descriptors of the
    // replay ring's logical indices (fe_replay_sample's slot map: slot (start + i) mod C)
    const int64_t *indices;
    const int64_t *ring_src;
    const double *ring_pos;
    int64_t ring_C, start, size;
    const float *actions;       // (count) the action in slot 6
    const float *smooth_noise;  // (count) standard normals or null: TD3's target smoothing (TD3_agent.py:236-241)
    float smooth_std, smooth_clip;
    const int64_t *cursor;      // the ring's cursor or null: start / size are read from it (fe_twin_q_target_c)
};

__device__ __forceinline__ float clamp_pm(float x, float lo, float hi) {  // torch.clamp, NaN propagating
    return x < lo ? lo : (x > hi ? hi : x);
}

// Logical index k of the ring: its slot, or false (outside [0, size): nothing of the ring is read for it).
__device__ __forceinline__ bool ring_slot(int64_t k, int64_t start, int64_t size, int64_t C, int64_t &slot) {
    const bool ok = k >= 0 && k < size;
    slot = start + (ok ? k : 0);
    if (slot >= C) slot -= C;
    return ok;
}

// Descriptor and action of pair n (A = 1).  An out-of-range ring index reads window offset 0 and position 0 -- a valid
// window: its value is overwritten by NaN in critic_store.
__device__ __forceinline__ void critic_load_pair(const CriticArgs &cq, int64_t n, int64_t *src, double *pos, float *act) {
    if (cq.indices) {
        int64_t slot, start = cq.start, size = cq.size;
        ring_window(cq.cursor, cq.ring_C, start, size);
        const bool ok = ring_slot(cq.indices[n], start, size, cq.ring_C, slot);
        *src = ok ? cq.ring_src[slot] : 0;
        *pos = ok ? cq.ring_pos[slot] : 0.0;
    } else {
        *src = cq.l.obs_src[n];
        *pos = cq.l.obs_pos[n];
    }
    float a = cq.actions[n];
    if (cq.smooth_noise) {  // clamp(a + clamp(eps * std, -c, c), -1, 1), one f32 rounding per torch op
        const float dev = clamp_pm(__fmul_rn(cq.smooth_noise[n], cq.smooth_std), -cq.smooth_clip, cq.smooth_clip);
        a = clamp_pm(__fadd_rn(a, dev), -1.0f, 1.0f);
    }
    *act = a;
}

__device__ __forceinline__ void critic_store(const CriticArgs &cq, int64_t n, float q) {
    if (cq.indices) {
        const int64_t k = cq.indices[n];
        int64_t start = cq.start, size = cq.size;
        ring_window(cq.cursor, cq.ring_C, start, size);
        if (k < 0 || k >= size) q = __builtin_nanf("");
    }
    cq.net[blockIdx.y].q_out[n] = q;
}

template <int NT>
__global__ __launch_bounds__(kLstmBlock, (NT == 1 ? 4 : 2)) void fe_twin_q_kernel(const Params p, const CriticArgs cq) {
    constexpr bool SINGLE = true;
    LstmArgs r = cq.l;
    r.whh = cq.net[blockIdx.y].whh;
    r.wx = cq.net[blockIdx.y].wx;
    r.wout = cq.net[blockIdx.y].wout;
#define FE_LSTM_SAC_HEAD 0
#define FE_LSTM_CRITIC_HEAD 1
#include "fe_lstm_rollout_body.h"
#undef FE_LSTM_CRITIC_HEAD
#undef FE_LSTM_SAC_HEAD
}

// ---- the Bellman target (SAC_agent.py:200-227, TD3_agent.py:231-251), one lane per sample ----
// In the reference's operation order, every operation one f32 rounding (the file is compiled with -ffp-contract=off):
//   m = min(q1, q2) (NaN propagating, as torch.min / torch.minimum);  SAC: m = m + (-alpha) * logp  (A = 1: the mean
//   over the actions is logp itself);  y = r s + (gamma * (1 - d)) * m  with s = reward_scale (r s = r when s = 1).
// Rewards and dones come from the ring by logical index; an index outside [0, size) gives NaN and counts in errors[0].
struct TwinTargetArgs {
    const float *q1, *q2;
    const int64_t *indices;
    const float *ring_rew, *ring_done;
    int64_t ring_C, start, size, count;
    const float *log_probs;  // (count) or null (TD3)
    const float *alpha;      // (1), with log_probs
    float gamma, reward_scale;
    float *targets;
    unsigned long long *errors;
    const int64_t *cursor;  // as CriticArgs'
};

__global__ __launch_bounds__(kBlock) void fe_twin_q_target_kernel(const TwinTargetArgs t) {
    const float qnan = __builtin_nanf("");
    int64_t start = t.start, size = t.size;
    ring_window(t.cursor, t.ring_C, start, size);
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < t.count; i += (int64_t)gridDim.x * kBlock) {
        int64_t slot;
        const bool ok = ring_slot(t.indices[i], start, size, t.ring_C, slot);
        if (!ok) {
            atomicAdd(t.errors, 1ull);
            t.targets[i] = qnan;
            continue;
        }
        const float q1 = t.q1[i], q2 = t.q2[i];
        float m = (q1 != q1) ? q1 : ((q2 != q2) ? q2 : (q2 < q1 ? q2 : q1));
        if (t.log_probs) m = __fadd_rn(m, __fmul_rn(-*t.alpha, t.log_probs[i]));
        const float rew = __fmul_rn(t.ring_rew[slot], t.reward_scale);
        const float nd = __fmul_rn(t.gamma, __fsub_rn(1.0f, t.ring_done[slot]));
        t.targets[i] = __fadd_rn(rew, __fmul_rn(nd, m));
    }
}

}  // namespace
