// fe_mlp_critic_kernels.h -- part of fe_mlp_critic.hip (the library's second translation unit): the twin MLP critics
// Q(s, a) of TD3 and SAC on observation descriptors (include/finenvs_amd_mlp_critic.h): values, Bellman targets from the
// replay ring, backward.  The network is the two-hidden-layer head of fe_mlp2_head_kernels.h with one more input, the
// action in column 5W of network.0.weight: the first layer, the H x H layer and the output layer are that header's device
// functions called as they stand, and the action enters z1 by one fmaf after the first layer's chain.
#pragma once
#include "fe_mlp2_head_kernels.h"

namespace {

// One critic as the kernels read it: fe_mlpq_weights, and where its values go.
struct MlpqNet {
    const float *w1t, *wpos, *wact, *b1, *w2h, *b2h, *w3, *b3;
    float *q_out;  // (count); forward and target launches only
};

struct MlpqArgs {
    const float *lr32;
    MlpqNet net[2];  // blockIdx.y = critic
    // descriptors: obs_src / obs_pos (count) given, or -- indices != null -- the next-state descriptors of the replay
    // ring's logical indices (fe_replay_sample's slot map: slot (start + i) mod C)
    const int64_t *obs_src;
    const double *obs_pos;
    const int64_t *indices;
    const int64_t *ring_src;
    const double *ring_pos;
    int64_t ring_C, start, size;
    const int64_t *cursor;      // the ring's cursor or null: start / size are read from it (fe_twin_mlpq_target_c)
    const float *actions;       // (count)
    const float *smooth_noise;  // (count) standard normals or null: TD3's target smoothing (TD3_agent.py:236-241)
    float smooth_std, smooth_clip;
    int64_t count;
    int32_t W, act;
};

// LDS of the kernels that hold a critic's weight image: the two-layer head's, then wact (H)
__host__ __device__ inline size_t mlpq_weight_lds_bytes(int W, int H) { return mlp2_weight_lds_bytes(W, H) + (size_t)H * 4; }

// The ring's window, by value or from the cursor (int64 words: head, size), and a logical index's slot -- the rules of
// fe_twin_q_target (fe_replay_kernels.h ring_window, fe_critic_kernels.h ring_slot), restated for this unit.
__device__ __forceinline__ void mlpq_ring_window(const int64_t *__restrict__ cursor, int64_t C, int64_t &start, int64_t &size) {
    if (cursor) {
        size = cursor[1];
        start = cursor[0] - size;
        if (start < 0) start += C;
    }
}

__device__ __forceinline__ bool mlpq_ring_slot(int64_t k, int64_t start, int64_t size, int64_t C, int64_t &slot) {
    const bool ok = k >= 0 && k < size;
    slot = start + (ok ? k : 0);
    if (slot >= C) slot -= C;
    return ok;
}

__device__ __forceinline__ float mlpq_clamp(float x, float lo, float hi) {  // torch.clamp, NaN propagating
    return x < lo ? lo : (x > hi ? hi : x);
}

// z1 += a * wact: one fmaf per hidden unit after the first layer's chain (a = 0 or wact = 0 leaves every z1 as it was)
template <int NT>
__device__ __forceinline__ void mlpq_add_action(f32x16 (&acc)[NT], float a, const float *s_wact, int half) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int h = 32 * t + (rr & 3) + 8 * (rr >> 2) + 4 * half;
            acc[t][rr] = fmaf(a, s_wact[h], acc[t][rr]);
        }
}

// ---- fe_twin_mlpq_forward / fe_twin_mlpq_target: one wavefront per block of 32 pairs, grid-strided in x; critic
// blockIdx.y's weight image in LDS (two H = 128 images do not fit one workgroup) ----
template <int NT>
__global__ __launch_bounds__(kBlock, NT == 4 ? 1 : 2) void fe_mlpq_forward_kernel(const MlpqArgs r) {
    extern __shared__ __align__(16) unsigned char smem[];
    const MlpqNet &net = r.net[blockIdx.y];
    const int W = r.W;
    constexpr int H = 32 * NT;
    const int KP = mlp_kp(W);
    float *s_w1t = reinterpret_cast<float *>(smem);
    float *s_wpos = s_w1t + (size_t)H * KP;
    float *s_b1 = s_wpos + H;
    float *s_w3 = s_b1 + H;
    float *s_b2h = s_w3 + H;
    float *s_w2h = s_b2h + H;
    float *s_wact = s_w2h + (size_t)H * mlp2_hp(H);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, half = lane >> 5;
    mlp_head_load_weights(s_w1t, H, W, net.w1t, net.wpos, net.b1, net.w3, tid);
    for (int i = tid; i < H; i += kBlock) {
        s_b2h[i] = net.b2h[i];
        s_wact[i] = net.wact[i];
    }
    mlp2_load_w2<false>(s_w2h, H, net.w2h, tid);
    const float b3 = *net.b3;
    __syncthreads();
    int64_t start = r.start, size = r.size;
    if (r.indices) mlpq_ring_window(r.cursor, r.ring_C, start, size);
    const int64_t nblk = (r.count + 31) / 32;
    for (int64_t blk = (int64_t)blockIdx.x * (kBlock / 64) + wave; blk < nblk; blk += (int64_t)gridDim.x * (kBlock / 64)) {
        const int64_t q = blk * 32 + col;
        const int64_t qc = q < r.count ? q : r.count - 1;
        int64_t src;
        double pos;
        bool ok = true;
        if (r.indices) {  // an out-of-range index reads window offset 0 and position 0 -- a valid window; its value is NaN
            int64_t slot;
            ok = mlpq_ring_slot(r.indices[qc], start, size, r.ring_C, slot);
            src = ok ? r.ring_src[slot] : 0;
            pos = ok ? r.ring_pos[slot] : 0.0;
        } else {
            src = r.obs_src[qc];
            pos = r.obs_pos[qc];
        }
        float a = r.actions[qc];
        if (r.smooth_noise) {  // clamp(a + clamp(eps * std, -c, c), -1, 1), one f32 rounding per torch op
            const float dev = mlpq_clamp(__fmul_rn(r.smooth_noise[qc], r.smooth_std), -r.smooth_clip, r.smooth_clip);
            a = mlpq_clamp(__fadd_rn(a, dev), -1.0f, 1.0f);
        }
        f32x16 acc[NT], acc2[NT];
        mlp_head_first_layer<NT>(acc, r.lr32 + src, 4, (float)pos, W, s_w1t, s_wpos, s_b1, KP, lane);
        mlpq_add_action<NT>(acc, a, s_wact, half);
        mlp2_second_hidden_act<NT>(r.act, acc, acc2, s_w2h, s_b2h, lane);
        const float qv = mlp_head_p<NT>(acc2, r.act, s_w3, half, b3);
        if (half == 0 && q < r.count) net.q_out[q] = ok ? qv : __builtin_nanf("");
    }
}

// ---- the Bellman target (SAC_agent.py:200-227, TD3_agent.py:231-251), one lane per sample: fe_twin_q_target's
// epilogue, its operations in its order, every operation one f32 rounding ----
//   m = min(q1, q2) (NaN propagating);  SAC: m = m + (-alpha) * logp;  y = r s + (gamma * (1 - d)) * m
// Rewards and dones come from the ring by logical index; an index outside [0, size) gives NaN and counts in errors[0]
// (an integer atomic: no float sum depends on its order).
struct MlpqTargetArgs {
    const float *q1, *q2;
    const int64_t *indices;
    const float *ring_rew, *ring_done;
    int64_t ring_C, start, size, count;
    const float *log_probs;  // (count) or null (TD3)
    const float *alpha;      // (1), with log_probs
    float gamma, reward_scale;
    float *targets;
    unsigned long long *errors;
    const int64_t *cursor;
};

__global__ __launch_bounds__(kBlock) void fe_mlpq_target_kernel(const MlpqTargetArgs t) {
    const float qnan = __builtin_nanf("");
    int64_t start = t.start, size = t.size;
    mlpq_ring_window(t.cursor, t.ring_C, start, size);
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < t.count; i += (int64_t)gridDim.x * kBlock) {
        int64_t slot;
        const bool ok = mlpq_ring_slot(t.indices[i], start, size, t.ring_C, slot);
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

// ---- fe_twin_mlpq_backward, one critic at a time ----
// fe_mlp2_backward's argument block (g2.g.d_outputs = dq, out_act = 2; g2.g.FP = 32 ceil((4W + 3) / 32); g2.g.g_w1 is
// (H, 5W + 1)) and what the action adds.
struct MlpqGradArgs {
    Mlp2GradArgs g2;
    const float *wact;
    const float *actions;
    float *d_actions;    // (count) or null
    int32_t accumulate;  // d_actions already holds critic 1's value: this critic adds to it
};

// (a) fe_mlp2_grad_kernel with the action term in z1: both hidden layers recomputed, a1 stored, dz2 formed in-lane, the
// partials of d w3 and d b3 beside them
template <int NT>
__global__ __launch_bounds__(kBlock, NT == 4 ? 1 : 2) void fe_mlpq_grad_kernel(const MlpqGradArgs ga) {
    extern __shared__ __align__(16) unsigned char smem[];
    const Mlp2GradArgs &g2 = ga.g2;
    const MlpGradArgs &g = g2.g;
    constexpr int H = 32 * NT;
    const int W = g.W;
    const int KP = mlp_kp(W);
    float *s_w1t = reinterpret_cast<float *>(smem);
    float *s_wpos = s_w1t + (size_t)H * KP;
    float *s_b1 = s_wpos + H;
    float *s_w3 = s_b1 + H;
    float *s_b2h = s_w3 + H;
    float *s_w2h = s_b2h + H;
    float *s_wact = s_w2h + (size_t)H * mlp2_hp(H);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, half = lane >> 5;
    mlp_head_load_weights(s_w1t, H, W, g.w1t, g.wpos, g.b1, g.w2, tid);
    for (int i = tid; i < H; i += kBlock) {
        s_b2h[i] = g2.b2h[i];
        s_wact[i] = ga.wact[i];
    }
    mlp2_load_w2<false>(s_w2h, H, g2.w2h, tid);
    __syncthreads();
    float w3acc[NT][16];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) w3acc[t][rr] = 0.0f;
    float b3acc = 0.0f;
    const int64_t gw = (int64_t)blockIdx.x * (kBlock / 64) + wave;
    for (int64_t blk = gw; blk < g.blocks; blk += (int64_t)gridDim.x * (kBlock / 64)) {
        const int64_t q = blk * 32 + col;
        const int64_t qc = q < g.count ? q : g.count - 1;
        f32x16 acc[NT], acc2[NT];
        mlp_head_first_layer<NT, false>(acc, g.lr32 + g.obs_src[qc], 4, (float)g.obs_pos[qc], W, s_w1t, s_wpos, s_b1, KP, lane);
        mlpq_add_action<NT>(acc, ga.actions[qc], s_wact, half);
        mlp2_second_hidden_act<NT>(g.act, acc, acc2, s_w2h, s_b2h, lane);
        float *a1_row = g2.a1 + q * H;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int b = 0; b < 4; ++b)
                *reinterpret_cast<float4 *>(a1_row + 32 * t + 8 * b + 4 * half) =
                    make_float4(acc[t][4 * b], acc[t][4 * b + 1], acc[t][4 * b + 2], acc[t][4 * b + 3]);
        const float dp = q < g.count ? g.d_outputs[q] : 0.0f;
        if (half == 0) b3acc = b3acc + dp;
        float *dz2_row = g2.dz2 + q * H;
        if (g.act == 1) mlp_grad_block_tail<1, NT>(acc2, w3acc, s_w3, half, dp, q < g.count, dz2_row);
        else if (g.act == 2) mlp_grad_block_tail<2, NT>(acc2, w3acc, s_w3, half, dp, q < g.count, dz2_row);
        else mlp_grad_block_tail<0, NT>(acc2, w3acc, s_w3, half, dp, q < g.count, dz2_row);
    }
    // the 32 pairs of the wavefront's columns: a butterfly in a fixed order (every lane ends with the same sum)
#pragma unroll
    for (int m = 1; m < 32; m <<= 1) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) w3acc[t][rr] = w3acc[t][rr] + __shfl_xor(w3acc[t][rr], m, 64);
        b3acc = b3acc + __shfl_xor(b3acc, m, 64);
    }
    if (col == 0) {
        float *wp = g.wpart + gw * (H + 4);
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) wp[32 * t + (rr & 3) + 8 * (rr >> 2) + 4 * half] = w3acc[t][rr];
        if (half == 0) wp[H] = b3acc;
    }
}

// (b) fe_mlp2_dgrad_kernel -- da1 = W2^T dz2 per 32-pair block and wavefront, dz1 = da1 * act'(z1) -- and, where dz1 is
// formed, dQ/da = sum_h wact[h] dz1[h]: an in-lane partial over the lane's 16 NT units in unit order, then
// (half 0) + (half 1).  The LDS holds the W2^T image and wact.
template <int NT>
__global__ __launch_bounds__(kBlock, 2) void fe_mlpq_dgrad_kernel(const MlpqGradArgs ga) {
    extern __shared__ __align__(16) unsigned char smem[];
    const Mlp2GradArgs &g2 = ga.g2;
    const MlpGradArgs &g = g2.g;
    constexpr int H = 32 * NT, HP = H + 4;
    float *s_w2t = reinterpret_cast<float *>(smem);
    float *s_wact = s_w2t + (size_t)H * HP;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, half = lane >> 5;
    mlp2_load_w2<true>(s_w2t, H, g2.w2h, tid);
    for (int i = tid; i < H; i += kBlock) s_wact[i] = ga.wact[i];
    __syncthreads();
    const float *wrow = s_w2t + (size_t)col * HP + 4 * half;
    for (int64_t blk = (int64_t)blockIdx.x * (kBlock / 64) + wave; blk < g.blocks; blk += (int64_t)gridDim.x * (kBlock / 64)) {
        const int64_t q = blk * 32 + col;  // every row below 32 * blocks exists in the workspace
        const float *dz2_row = g2.dz2 + q * H + 4 * half;
        const float *a1_row = g2.a1 + q * H + 4 * half;
        float *dz1_row = g.dpre + q * H + 4 * half;
        f32x16 da[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) da[t][rr] = 0.0f;
#pragma unroll
        for (int t2 = 0; t2 < NT; ++t2)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const float4 d = *reinterpret_cast<const float4 *>(dz2_row + 32 * t2 + 8 * b);
                float4 wa[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) wa[t] = *reinterpret_cast<const float4 *>(wrow + (size_t)(32 * t) * HP + 32 * t2 + 8 * b);
                const float ds[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const float ws = c == 0 ? wa[t].x : (c == 1 ? wa[t].y : (c == 2 ? wa[t].z : wa[t].w));
                        da[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ws, ds[c], da[t], 0, 0, 0);
                    }
                // one (t2, b) step at a time, as in fe_mlp2_dgrad_kernel
                if constexpr (NT == 4) __builtin_amdgcn_sched_barrier(0);
            }
        float apart = 0.0f;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const float4 a = *reinterpret_cast<const float4 *>(a1_row + 32 * t + 8 * b);
                const float4 wv = *reinterpret_cast<const float4 *>(s_wact + 32 * t + 8 * b + 4 * half);
                const float4 dz = make_float4(da[t][4 * b] * mlp2_dact_of_a(g.act, a.x), da[t][4 * b + 1] * mlp2_dact_of_a(g.act, a.y),
                                              da[t][4 * b + 2] * mlp2_dact_of_a(g.act, a.z), da[t][4 * b + 3] * mlp2_dact_of_a(g.act, a.w));
                *reinterpret_cast<float4 *>(dz1_row + 32 * t + 8 * b) = dz;
                apart = fmaf(wv.x, dz.x, apart);
                apart = fmaf(wv.y, dz.y, apart);
                apart = fmaf(wv.z, dz.z, apart);
                apart = fmaf(wv.w, dz.w, apart);
                if constexpr (NT == 4) __builtin_amdgcn_sched_barrier(0);
            }
        if (ga.d_actions) {
            const float other = __shfl_xor(apart, 32, 64);
            const float tot = half == 0 ? apart + other : other + apart;  // always (half 0) + (half 1)
            if (half == 0 && q < g.count) ga.d_actions[q] = ga.accumulate ? ga.d_actions[q] + tot : tot;
        }
    }
}

// (c) fe_mlp_wgrad_kernel with one more column: [dW1t | d wpos | d wact | d b1] = dz1^T [X | pos | a | 1]
template <int NT>
__global__ __launch_bounds__(kBlock, 2) void fe_mlpq_wgrad_kernel(const MlpqGradArgs ga) {
    const MlpGradArgs &g = ga.g2.g;
    constexpr int H = 32 * NT;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, half = lane >> 5;
    const int FT = g.FP / 32;
    const int64_t CP = 32 * g.blocks;
    const int K4 = 4 * g.W;
    const int64_t items = g.splits * FT;
    for (int64_t item = (int64_t)blockIdx.x * (kBlock / 64) + wave; item < items; item += (int64_t)gridDim.x * (kBlock / 64)) {
        const int64_t split = item / FT;
        const int ft = (int)(item - split * FT);
        const int f = 32 * ft + col;
        const int fc = f < K4 ? f : 0;  // the table offset of a real feature; the three extra columns and the padding read none
        const int64_t n0 = split * kMlpGradChunk;
        const int64_t n1 = n0 + kMlpGradChunk < CP ? n0 + kMlpGradChunk : CP;
        f32x16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) acc[t][rr] = 0.0f;
        const float *arow = g.dpre + (int64_t)(4 * half) * H + col;
        for (int64_t nb = n0; nb < n1; nb += 8) {
            float wa[NT][4];
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int t = 0; t < NT; ++t) wa[t][m] = arow[(nb + m) * H + 32 * t];
            float xs[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int64_t n = nb + 4 * half + m;
                const int64_t nc = n < g.count ? n : g.count - 1;
                float v;
                if (f < K4) v = g.lr32[g.obs_src[nc] + fc];
                else if (f == K4) v = (float)g.obs_pos[nc];
                else if (f == K4 + 1) v = ga.actions[nc];
                else v = f == K4 + 2 ? 1.0f : 0.0f;
                xs[m] = n < g.count ? v : 0.0f;
            }
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[t][m], xs[m], acc[t], 0, 0, 0);
        }
        float *out = g.part + split * (int64_t)H * g.FP + f;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                const int h = 32 * t + (rr & 3) + 8 * (rr >> 2) + 4 * half;
                out[(int64_t)h * g.FP] = acc[t][rr];
            }
    }
}

// (d) the splits of (c) and the wavefronts' partials of (a) added in index order (f64, rounded once), written in torch's
// layout: network.0.weight's gradient is (H, 5W + 1), the position column written to every window row, the action's in
// column 5W
__global__ __launch_bounds__(kBlock) void fe_mlpq_grad_reduce_kernel(const MlpGradArgs g) {
    const int H = g.H, W = g.W, K4 = 4 * W, F = K4 + 3, LD = 5 * W + 1;
    const int64_t total = (int64_t)H * F + H + 1;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        if (i < (int64_t)H * F) {
            const int h = (int)(i / F), f = (int)(i - (int64_t)h * F);
            const float *src = g.part + (int64_t)h * g.FP + f;
            double s = 0.0;
            for (int64_t k = 0; k < g.splits; ++k) s += (double)src[k * (int64_t)H * g.FP];
            const float v = (float)s;
            float *row = g.g_w1 + (size_t)h * LD;
            if (f < K4) row[5 * (f >> 2) + (f & 3)] = v;
            else if (f == K4) {  // the position column is the same in every window row
                for (int j = 0; j < W; ++j) row[5 * j + 4] = v;
            } else if (f == K4 + 1) row[5 * W] = v;
            else g.g_b1[h] = v;
        } else {
            const int h = (int)(i - (int64_t)H * F);  // h == H: d b3
            double s = 0.0;
            for (int64_t k = 0; k < g.waves; ++k) s += (double)g.wpart[k * (H + 4) + h];
            if (h < H) g.g_w2[h] = (float)s;
            else g.g_b2[0] = (float)s;
        }
    }
}

}  // namespace
