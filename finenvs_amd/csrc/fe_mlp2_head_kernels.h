// fe_mlp2_head_kernels.h -- part of fe_env.hip (one translation unit; see the overview there): the two-hidden-layer MLP
// head (include/finenvs_amd_mlp2_head.h): sampled rollout, value on descriptors, backward.  The first layer, the output
// layer and the layer-1 weight gradient are those of fe_mlp_head_kernels.h (device functions and kernels called as they
// stand); new here are the H x H layer on the matrix cores, forward (W2 a1) and backward (W2^T dz2, dz2^T a1).
#pragma once
#include "fe_mlp_head_kernels.h"

namespace {

// The one-layer head's arguments (w2 / b2 there: the output layer, w3 / b3 here) and the second hidden layer's weights.
struct Mlp2HeadArgs {
    MlpHeadArgs h;
    const float *w2h;  // (H, H) network.2.weight as torch holds it
    const float *b2h;  // (H) network.2.bias
};

// row length of the W2 (or W2^T) image in LDS: 16 bytes of padding, so the 32 lanes of an A-operand read (one row each,
// float4) fall into different banks -- the rule of mlp_kp
__host__ __device__ inline int mlp2_hp(int H) { return H + 4; }
// what the second hidden layer adds to the one-layer head's weight image: b2 (H) and the padded W2 image
__host__ __device__ inline size_t mlp2_extra_lds_bytes(int H) { return ((size_t)H + (size_t)H * mlp2_hp(H)) * 4; }
__host__ __device__ inline size_t mlp2_lds_bytes(int EB, int A, int W, int H) { return mlp_lds_bytes(EB, A, W, H) + mlp2_extra_lds_bytes(H); }
__host__ __device__ inline size_t mlp2_weight_lds_bytes(int W, int H) { return mlp_head_weight_lds_bytes(W, H) + mlp2_extra_lds_bytes(H); }

// b2 and the image of W2 (TRANSPOSED = false: s[u2 * HP + u1] = W2[u2][u1]) or of W2^T (s[u1 * HP + u2] = W2[u2][u1])
template <bool TRANSPOSED>
__device__ __forceinline__ void mlp2_load_w2(float *s_w2h, int H, const float *w2h, int tid) {
    const int HP = mlp2_hp(H);
    for (int i = tid; i < H * H; i += kBlock) {
        const int r = i / H, c = i - r * H;
        s_w2h[TRANSPOSED ? c * HP + r : r * HP + c] = w2h[i];
    }
}

// The second hidden layer of the lane's pair.  acc holds z1 in the placement of mlp_head_first_layer -- lane (col, half)
// has unit 32t + 8b + 4 half + c of pair col in acc[t][4b + c] -- which is the B operand of v_mfma_f32_32x32x2_f32
// (B[k = half][j = col]) for the contraction pair (32t + 8b + c, 32t + 8b + 4 + c): a1 = act(z1) feeds the MFMAs from
// registers.  The A operand A[i = col][k = half] = W2[32 t2 + col][32t + 8b + 4 half + c] is one float4 of the image per
// (t, b, t2).  acc becomes a1 (in place), acc2 = z2 = b2 + W2 a1 in the same placement.
template <int ACT, int NT>
__device__ __forceinline__ void mlp2_second_hidden(f32x16 (&acc)[NT], f32x16 (&acc2)[NT], const float *s_w2h, const float *s_b2h,
                                                   int lane) {
    constexpr int HP = 32 * NT + 4;
    const int col = lane & 31, half = lane >> 5;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) acc2[t][rr] = s_b2h[32 * t + (rr & 3) + 8 * (rr >> 2) + 4 * half];
    const float *wrow = s_w2h + (size_t)col * HP + 4 * half;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            float4 wa[NT];
#pragma unroll
            for (int t2 = 0; t2 < NT; ++t2) wa[t2] = *reinterpret_cast<const float4 *>(wrow + (size_t)(32 * t2) * HP + 32 * t + 8 * b);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float a = mlp_act<ACT>(acc[t][4 * b + c]);
                acc[t][4 * b + c] = a;
#pragma unroll
                for (int t2 = 0; t2 < NT; ++t2) {
                    const float ws = c == 0 ? wa[t2].x : (c == 1 ? wa[t2].y : (c == 2 ? wa[t2].z : wa[t2].w));
                    acc2[t2] = __builtin_amdgcn_mfma_f32_32x32x2f32(ws, a, acc2[t2], 0, 0, 0);
                }
            }
        }
}

template <int NT>
__device__ __forceinline__ void mlp2_second_hidden_act(int act, f32x16 (&acc)[NT], f32x16 (&acc2)[NT], const float *s_w2h,
                                                       const float *s_b2h, int lane) {
    if (act == 1) mlp2_second_hidden<1, NT>(acc, acc2, s_w2h, s_b2h, lane);
    else if (act == 2) mlp2_second_hidden<2, NT>(acc, acc2, s_w2h, s_b2h, lane);
    else mlp2_second_hidden<0, NT>(acc, acc2, s_w2h, s_b2h, lane);
}

// p of the lane's pair: first layer, second hidden layer, then the output layer of the one-layer head on z2 (mlp_head_p:
// in-lane partial, (half 0) + (half 1), b3 +)
template <int NT>
__device__ __forceinline__ float mlp2_head_value(const float *xsrc, int64_t rstride, float pos32, int W, int act, const float *s_w1t,
                                                 const float *s_wpos, const float *s_b1, const float *s_w3, const float *s_b2h,
                                                 const float *s_w2h, int KP, int lane, float b3) {
    f32x16 acc[NT], acc2[NT];
    mlp_head_first_layer<NT>(acc, xsrc, rstride, pos32, W, s_w1t, s_wpos, s_b1, KP, lane);
    mlp2_second_hidden_act<NT>(act, acc, acc2, s_w2h, s_b2h, lane);
    return mlp_head_p<NT>(acc2, act, s_w3, lane >> 5, b3);
}

// the weight image of the forward kernels: the one-layer head's (W1t, wpos, b1, w3), then b2 and the W2 image
template <int NT>
__device__ __forceinline__ void mlp2_load_weights(float *s_w1t, int W, const MlpHeadArgs &h, const float *w2h, const float *b2h,
                                                  int tid) {
    constexpr int H = 32 * NT;
    mlp_head_load_weights(s_w1t, H, W, h.w1t, h.wpos, h.b1, h.w2, tid);
    float *s_b2h = s_w1t + (size_t)H * mlp_kp(W) + 3 * H;
    for (int i = tid; i < H; i += kBlock) s_b2h[i] = b2h[i];
    mlp2_load_w2<false>(s_b2h + H, H, w2h, tid);
}

// ---- fe_env_rollout_mlp2_sampled: fe_rollout_mlp_sampled_kernel's loop with the deeper policy ----
// At H = 128 the image (W2 alone: 66 KiB) leaves room for one workgroup per CU: that instantiation takes the registers
// of one wavefront per SIMD.
template <bool SINGLE, int NT>
__global__ __launch_bounds__(kBlock, NT == 4 ? 1 : 2) void fe_rollout_mlp2_sampled_kernel(const Params p, const Mlp2HeadArgs r2) {
    extern __shared__ __align__(16) unsigned char smem[];
    const MlpHeadArgs &r = r2.h;
    const int A = SINGLE ? 1 : p.A;
    const int EB = p.EB;
    const int S = EB * A;
    const int W = p.W;
    constexpr int H = 32 * NT;
    const TileLds l = carve_lds(smem, EB, S);
    size_t off = (size_t)EB * 8 + (size_t)S * 8 + (size_t)S * 8 + (size_t)S * 4 + (size_t)S * 4 + (size_t)EB * 4;
    off = (off + 7) & ~(size_t)7;
    int64_t *l_idx = reinterpret_cast<int64_t *>(smem + off);
    off += (size_t)EB * 8;
    float *s_act = reinterpret_cast<float *>(smem + off);
    off = (off + (size_t)S * 4 + 15) & ~(size_t)15;
    const int KP = mlp_kp(W);
    float *s_w1t = reinterpret_cast<float *>(smem + off);
    float *s_wpos = s_w1t + (size_t)H * KP;
    float *s_b1 = s_wpos + H;
    float *s_w3 = s_b1 + H;
    float *s_b2h = s_w3 + H;
    float *s_w2h = s_b2h + H;
    const int tid = threadIdx.x;
    const int e = SINGLE ? tid : (int)fdiv((uint32_t)tid, p.div_A);
    const int a = SINGLE ? 0 : tid - e * A;
    const int lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, half = lane >> 5;
    const int64_t NA = p.N * A;
    const int64_t rstride = 4 * (int64_t)A;
    mlp2_load_weights<NT>(s_w1t, W, r, r2.w2h, r2.b2h, tid);
    const float b3 = *r.b2;

    for (int64_t tile = blockIdx.x; tile < p.num_tiles; tile += gridDim.x) {
        const int64_t n0 = tile * EB;
        const int ebt = (p.N - n0) < (int64_t)EB ? (int)(p.N - n0) : EB;
        const bool active = e < ebt;
        const int64_t n = n0 + e;
        const int64_t sl = n * A + a;
        SleeveReg st = rollout_load_state(p, active, n, sl);
        if (active) {
            const double pos0 = r.obs_pos[sl];
            l.pos[e * A + a] = pos0;
            if (a == 0) l.src[e] = r.obs_src[n];
            if (r.traj_src) {  // row 0: the state the first policy evaluation sees
                r.traj_pos[sl] = pos0;
                if (a == 0) r.traj_src[n] = r.obs_src[n];
            }
        }
        __syncthreads();  // also covers the weight image on the first tile
        const int pairs = ebt * A;
        const int nblk = (pairs + 31) / 32;
        for (int k = 0; k < r.K; ++k) {
            // ---- policy: one wavefront per block of 32 pairs, the mean into s_act ----
            for (int blk = wave; blk < nblk; blk += kBlock / 64) {
                const int q = blk * 32 + col;
                const int qc = q < pairs ? q : pairs - 1;
                const int ee = SINGLE ? qc : (int)fdiv((uint32_t)qc, p.div_A);
                const int aa = SINGLE ? 0 : qc - ee * A;
                const float pv = mlp2_head_value<NT>(r.lr32 + l.src[ee] + 4 * aa, rstride, (float)l.pos[qc], W, r.act, s_w1t, s_wpos,
                                                     s_b1, s_w3, s_b2h, s_w2h, KP, lane, b3);
                const float mean = mlp_head_out(pv, r.out_act);
                if (half == 0 && q < pairs) s_act[q] = mean;
            }
            lds_barrier();
            float act = active ? s_act[e * A + a] : 0.0f;
            if (active) {
                const int64_t o = (int64_t)k * NA + sl;
                if (r.means_out) r.means_out[o] = act;
                if (r.noise && n != p.eval_env) {  // distribution.sample() clamped; the eval env keeps the mean
                    const float dev = r.std * r.noise[o];
                    const float smp = act + dev;
                    act = smp < -1.0f ? -1.0f : (smp > 1.0f ? 1.0f : smp);
                }
                if (r.actions_out) r.actions_out[o] = act;
            }
            account_keep<SINGLE>(p, l, l_idx, A, e, a, active, n, st, act, r.rew_out + (int64_t)k * p.N,
                                 r.done_out + (int64_t)k * p.N);
            if (active && r.traj_src) {  // row k + 1: the observation this step returns (own LDS entries: no barrier needed)
                r.traj_pos[(int64_t)(k + 1) * NA + sl] = l.pos[e * A + a];
                if (a == 0) r.traj_src[(int64_t)(k + 1) * p.N + n] = l.src[e];
            }
            lds_barrier();  // the new observation's descriptors are complete
        }
        rollout_store_state(p, active, a, n, sl, st);  // state and descriptors go back to HBM once per launch
        if (active) {
            r.obs_pos[sl] = l.pos[e * A + a];
            if (a == 0) r.obs_src[n] = l.src[e];
        }
        __syncthreads();
    }
}

// ---- fe_mlp2_forward: one wavefront per block of 32 descriptor pairs, grid-strided; the weight image in LDS ----
template <bool SINGLE, int NT>
__global__ __launch_bounds__(kBlock, NT == 4 ? 1 : 2) void fe_mlp2_forward_kernel(const Params p, const Mlp2HeadArgs r2) {
    extern __shared__ __align__(16) unsigned char smem[];
    const MlpHeadArgs &r = r2.h;
    const int A = SINGLE ? 1 : p.A;
    const int W = p.W;
    constexpr int H = 32 * NT;
    const int KP = mlp_kp(W);
    float *s_w1t = reinterpret_cast<float *>(smem);
    float *s_wpos = s_w1t + (size_t)H * KP;
    float *s_b1 = s_wpos + H;
    float *s_w3 = s_b1 + H;
    float *s_b2h = s_w3 + H;
    float *s_w2h = s_b2h + H;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, half = lane >> 5;
    mlp2_load_weights<NT>(s_w1t, W, r, r2.w2h, r2.b2h, tid);
    const float b3 = *r.b2;
    __syncthreads();
    const int64_t pairs = r.count * A;
    const int64_t nblk = (pairs + 31) / 32;
    for (int64_t blk = (int64_t)blockIdx.x * (kBlock / 64) + wave; blk < nblk; blk += (int64_t)gridDim.x * (kBlock / 64)) {
        const int64_t q = blk * 32 + col;
        const int64_t qc = q < pairs ? q : pairs - 1;
        const int64_t ee = SINGLE ? qc : qc / A;
        const int aa = SINGLE ? 0 : (int)(qc - ee * A);
        const float pv = mlp2_head_value<NT>(r.lr32 + r.obs_src[ee] + 4 * aa, 4 * (int64_t)A, (float)r.obs_pos[qc], W, r.act, s_w1t,
                                             s_wpos, s_b1, s_w3, s_b2h, s_w2h, KP, lane, b3);
        const float y = mlp_head_out(pv, r.out_act);
        if (half == 0 && q < pairs) r.actions_out[q] = y;
    }
}

// ---- fe_mlp2_backward ----
// The one-layer head's MlpGradArgs (dpre = dz1, w2 = w3, g_w2 / g_b2 = d w3 / d b3, wpart = their partials): what
// fe_mlp_wgrad_kernel and fe_mlp_grad_reduce_kernel read, launched as they stand for layer 1 and the output layer.
struct Mlp2GradArgs {
    MlpGradArgs g;
    const float *w2h, *b2h;
    float *a1;     // (CP, H) a1 = act(z1), CP = 32 * blocks
    float *dz2;    // (CP, H); pairs >= count hold zeros
    float *part2;  // (splits, H, H + 32): every split's [dz2^T a1 | dz2^T 1 | 31 unused columns]
    float *g_w2h, *g_b2h;
};

// (a) per 32-pair block and wavefront: both hidden layers recomputed, a1 stored, dp and dz2 formed in-lane
// (mlp_grad_block_tail on z2: dz2 rows and the partials of d w3); d b3's partial beside them
template <int NT>
__global__ __launch_bounds__(kBlock, NT == 4 ? 1 : 2) void fe_mlp2_grad_kernel(const Mlp2GradArgs g2) {
    extern __shared__ __align__(16) unsigned char smem[];
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
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, half = lane >> 5;
    mlp_head_load_weights(s_w1t, H, W, g.w1t, g.wpos, g.b1, g.w2, tid);
    for (int i = tid; i < H; i += kBlock) s_b2h[i] = g2.b2h[i];
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
        mlp2_second_hidden_act<NT>(g.act, acc, acc2, s_w2h, s_b2h, lane);
        float *a1_row = g2.a1 + q * H;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int b = 0; b < 4; ++b)
                *reinterpret_cast<float4 *>(a1_row + 32 * t + 8 * b + 4 * half) =
                    make_float4(acc[t][4 * b], acc[t][4 * b + 1], acc[t][4 * b + 2], acc[t][4 * b + 3]);
        float dp = 0.0f;
        if (q < g.count) {
            dp = g.d_outputs[q];
            if (g.out_act == 0) {
                const float y = g.outputs[q];
                dp = dp * (1.0f - y * y);
            }
        }
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

// act'(z1) from a1, the value the forward fed the second layer: ReLU a > 0, tanh 1 - a^2, ELU a > 0 ? 1 : a + 1
// (a = exp(z) - 1 there, and a > 0 exactly when z > 0)
__device__ __forceinline__ float mlp2_dact_of_a(int act, float a) {
    return act == 1 ? (a > 0.0f ? 1.0f : 0.0f) : (act == 2 ? 1.0f - a * a : (a > 0.0f ? 1.0f : a + 1.0f));
}

// (b) da1 = W2^T dz2 per 32-pair block and wavefront, dz1 = da1 * act'(z1).  A row of dz2 in the workspace is read in the
// B-operand placement (float4: units 32 t2 + 8b + 4 half + c), the A operand is a float4 of the W2^T image.
template <int NT>
__global__ __launch_bounds__(kBlock, 2) void fe_mlp2_dgrad_kernel(const Mlp2GradArgs g2) {
    extern __shared__ __align__(16) unsigned char smem[];
    const MlpGradArgs &g = g2.g;
    constexpr int H = 32 * NT, HP = H + 4;
    float *s_w2t = reinterpret_cast<float *>(smem);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, half = lane >> 5;
    mlp2_load_w2<true>(s_w2t, H, g2.w2h, tid);
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
                // one (t2, b) step at a time: left alone the scheduler hoists all 16 row reads of dz2 above the MFMAs, and
                // at H = 128 the register allocator then spills
                if constexpr (NT == 4) __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const float4 a = *reinterpret_cast<const float4 *>(a1_row + 32 * t + 8 * b);
                *reinterpret_cast<float4 *>(dz1_row + 32 * t + 8 * b) =
                    make_float4(da[t][4 * b] * mlp2_dact_of_a(g.act, a.x), da[t][4 * b + 1] * mlp2_dact_of_a(g.act, a.y),
                                da[t][4 * b + 2] * mlp2_dact_of_a(g.act, a.z), da[t][4 * b + 3] * mlp2_dact_of_a(g.act, a.w));
                if constexpr (NT == 4) __builtin_amdgcn_sched_barrier(0);
            }
    }
}

// (c) [dW2 | d b2] = dz2^T [a1 | 1]: one wavefront per (tile of 32 a1 units, or the ones column; split of kMlpGradChunk
// pairs), all H rows of dz2 -- the loop of fe_mlp_wgrad_kernel with a1 rows for the table reads.  The padding pairs of
// the last block hold dz2 = 0 and a finite a1.
template <int NT>
__global__ __launch_bounds__(kBlock, 2) void fe_mlp2_wgrad2_kernel(const Mlp2GradArgs g2) {
    const MlpGradArgs &g = g2.g;
    constexpr int H = 32 * NT, FP2 = H + 32, FT = NT + 1;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, half = lane >> 5;
    const int64_t CP = 32 * g.blocks;
    const int64_t items = g.splits * FT;
    for (int64_t item = (int64_t)blockIdx.x * (kBlock / 64) + wave; item < items; item += (int64_t)gridDim.x * (kBlock / 64)) {
        const int64_t split = item / FT;
        const int ft = (int)(item - split * FT);
        const int64_t n0 = split * kMlpGradChunk;
        const int64_t n1 = n0 + kMlpGradChunk < CP ? n0 + kMlpGradChunk : CP;
        f32x16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) acc[t][rr] = 0.0f;
        const float *arow = g2.dz2 + (int64_t)(4 * half) * H + col;
        const float *brow = g2.a1 + (int64_t)(4 * half) * H + (ft < NT ? 32 * ft + col : 0);
        const float one = col == 0 ? 1.0f : 0.0f;
        for (int64_t nb = n0; nb < n1; nb += 8) {
            float wa[NT][4];
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int t = 0; t < NT; ++t) wa[t][m] = arow[(nb + m) * H + 32 * t];
            float xs[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) xs[m] = ft < NT ? brow[(nb + m) * H] : one;
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[t][m], xs[m], acc[t], 0, 0, 0);
        }
        float *out = g2.part2 + split * (int64_t)H * FP2 + 32 * ft + col;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                const int h = 32 * t + (rr & 3) + 8 * (rr >> 2) + 4 * half;
                out[(int64_t)h * FP2] = acc[t][rr];
            }
    }
}

// (d) the splits of (c) added in index order (f64, rounded once): network.2.weight's and network.2.bias's gradients
__global__ __launch_bounds__(kBlock) void fe_mlp2_grad_reduce_kernel(const Mlp2GradArgs g2) {
    const int H = g2.g.H, FP2 = H + 32;
    const int64_t total = (int64_t)H * (H + 1);
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int h = (int)(i / (H + 1)), f = (int)(i - (int64_t)h * (H + 1));
        const float *src = g2.part2 + (int64_t)h * FP2 + f;
        double s = 0.0;
        for (int64_t k = 0; k < g2.g.splits; ++k) s += (double)src[k * (int64_t)H * FP2];
        if (f < H) g2.g_w2h[(size_t)h * H + f] = (float)s;
        else g2.g_b2h[h] = (float)s;
    }
}

}  // namespace
