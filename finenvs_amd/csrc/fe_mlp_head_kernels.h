// fe_mlp_head_kernels.h -- part of fe_env.hip (one translation unit; see the overview there): the MLP head's training
// entries (include/finenvs_amd_mlp_head.h): device packing, the sampled K-step rollout, the head's value on descriptors
// and its backward pass (first-layer recompute, weight-gradient GEMM on the matrix cores, deterministic reduction).
#pragma once
#include "fe_device_common.h"
#include "fe_rollout_kernels.h"
#include "fe_activations.h"

namespace {

struct MlpHeadArgs {
    const float *lr32;  // (D, L, 4A) f32 copy of the log-return table
    const float *w1t, *wpos, *b1, *w2, *b2;  // fe_mlp_weights
    int32_t H, act, out_act, K;  // act: 0 ELU, 1 ReLU, 2 tanh; out_act: 0 tanh, 1 clamp, 2 none
    int64_t *obs_src;   // rollout: the envs' descriptors, read and written; forward: `count` descriptors, read only
    double *obs_pos;
    const float *noise;  // (K, N*A) or null
    float std;
    float *actions_out;  // rollout: (K, N*A) or null; forward: out (count * A)
    float *means_out;    // (K, N*A) or null
    double *rew_out;
    int32_t *done_out;
    int64_t *traj_src;   // (K + 1, N) or null
    double *traj_pos;    // (K + 1, N*A) or null
    int64_t count;       // forward: descriptors
};

// LDS of the kernels that hold only the weight image (forward, backward): W1t, wpos, b1, w2
__host__ __device__ inline size_t mlp_head_weight_lds_bytes(int W, int H) { return ((size_t)H * mlp_kp(W) + 3 * (size_t)H) * 4; }

// the weight image of fe_rollout_mlp_kernel: W1t rows padded to KP with zeros, then wpos, b1, w2
__device__ __forceinline__ void mlp_head_load_weights(float *s_w1t, int H, int W, const float *w1t, const float *wpos,
                                                      const float *b1, const float *w2, int tid) {
    const int KP = mlp_kp(W), K4 = 4 * W;
    float *s_wpos = s_w1t + (size_t)H * KP, *s_b1 = s_wpos + H, *s_w2 = s_b1 + H;
    for (int i = tid; i < H * KP; i += kBlock) {
        const int h = i / KP, k = i - h * KP;
        s_w1t[i] = k < K4 ? w1t[(size_t)h * K4 + k] : 0.0f;
    }
    for (int i = tid; i < H; i += kBlock) {
        s_wpos[i] = wpos[i];
        s_b1[i] = b1[i];
        s_w2[i] = w2[i];
    }
}

// The first layer of mlp_policy_block for the pair whose window starts at xsrc (rows rstride floats apart), its
// statements restated (not factored out of it: the six fe_rollout_mlp_kernel instantiations keep their registers):
// acc[t][rr] = pre-activation of hidden unit 32t + (rr & 3) + 8 (rr >> 2) + 4 half of the lane's pair, the same fmaf
// chain in the same k order, hence the same bits.  PREFETCH = false loads a chunk's rows when it needs them instead of
// one chunk ahead (16 registers fewer: the backward at H = 128 keeps 64 more accumulators than the forward).
template <int NT, bool PREFETCH = true>
__device__ __forceinline__ void mlp_head_first_layer(f32x16 (&acc)[NT], const float *xsrc, int64_t rstride, float pos32,
                                                     int W, const float *s_w1t, const float *s_wpos, const float *s_b1,
                                                     int KP, int lane) {
    const int col = lane & 31, half = lane >> 5;
    const int ngroups = (4 * W + 7) / 8;  // two window rows per group
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            const int h = 32 * t + (rr & 3) + 8 * (rr >> 2) + 4 * half;
            acc[t][rr] = fmaf(pos32, s_wpos[h], s_b1[h]);
        }
    const float *wrow = s_w1t + (size_t)col * KP + 4 * half;
    // rows past the window re-read its last row: their W1t entries are zero padding (mlp_policy_block)
    auto load_x = [&](int g) {
        const int row = 2 * g + half;
        return *reinterpret_cast<const float4 *>(xsrc + (int64_t)(row < W ? row : W - 1) * rstride);
    };
    constexpr int CH = kMlpChunk;
    const int nchunks = (ngroups + CH - 1) / CH;
    float4 xc[CH], xn[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) xc[i] = load_x(i);
    for (int c = 0; c < nchunks; ++c) {
        if constexpr (PREFETCH) {
#pragma unroll
            for (int i = 0; i < CH; ++i) xn[i] = load_x((c + 1) * CH + i);
            if constexpr (NT == 4) __builtin_amdgcn_sched_barrier(0);
        } else if (c > 0) {
#pragma unroll
            for (int i = 0; i < CH; ++i) xc[i] = load_x(c * CH + i);
        }
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            float4 wa[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t)
                wa[t] = *reinterpret_cast<const float4 *>(wrow + (size_t)(32 * t) * KP + 8 * (c * CH + i));
            const float xs[4] = {xc[i].x, xc[i].y, xc[i].z, xc[i].w};
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const float ws = m == 0 ? wa[t].x : (m == 1 ? wa[t].y : (m == 2 ? wa[t].z : wa[t].w));
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(ws, xs[m], acc[t], 0, 0, 0);
                }
        }
        if constexpr (PREFETCH) {
#pragma unroll
            for (int i = 0; i < CH; ++i) xc[i] = xn[i];
        }
    }
}

// p = b2 + [half 0's units] + [half 1's units], mlp_policy_block's second layer (every lane of the pair gets it)
template <int NT>
__device__ __forceinline__ float mlp_head_p(const f32x16 (&acc)[NT], int act, const float *s_w2, int half, float b2) {
    float part;
    if (act == 1) part = mlp_second_layer<1, NT>(acc, s_w2, half);
    else if (act == 2) part = mlp_second_layer<2, NT>(acc, s_w2, half);
    else part = mlp_second_layer<0, NT>(acc, s_w2, half);
    const float other = __shfl_xor(part, 32, 64);
    const float tot = half == 0 ? part + other : other + part;  // always (half 0) + (half 1)
    return b2 + tot;
}

__device__ __forceinline__ float mlp_head_out(float p, int out_act) {
    return out_act == 0 ? lstm_tanh(p) : (out_act == 2 ? p : (p < -1.0f ? -1.0f : (p > 1.0f ? 1.0f : p)));
}

// ---- fe_mlp_pack ----
__global__ __launch_bounds__(kBlock) void fe_mlp_pack_kernel(const float *weight1, int H, int W, float *w1t, float *wpos) {
    const int K4 = 4 * W;
    const int64_t total = (int64_t)H * K4 + H;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        if (i < (int64_t)H * K4) {
            const int h = (int)(i / K4), k = (int)(i - (int64_t)h * K4);
            w1t[i] = weight1[(size_t)h * 5 * W + 5 * (k >> 2) + (k & 3)];
        } else {
            const int h = (int)(i - (int64_t)H * K4);
            float s = 0.0f;  // the host packing starts from zeros too
            for (int j = 0; j < W; ++j) s = s + weight1[(size_t)h * 5 * W + 5 * j + 4];
            wpos[h] = s;
        }
    }
}

// ---- fe_env_rollout_mlp_sampled: fe_rollout_mlp_kernel's loop with the training-rollout outputs ----
template <bool SINGLE, int NT>
__global__ __launch_bounds__(kBlock, 2) void fe_rollout_mlp_sampled_kernel(const Params p, const MlpHeadArgs r) {
    extern __shared__ __align__(16) unsigned char smem[];
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
    float *s_w2 = s_b1 + H;
    const int tid = threadIdx.x;
    const int e = SINGLE ? tid : (int)fdiv((uint32_t)tid, p.div_A);
    const int a = SINGLE ? 0 : tid - e * A;
    const int lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, half = lane >> 5;
    const int64_t NA = p.N * A;
    const int64_t rstride = 4 * (int64_t)A;
    mlp_head_load_weights(s_w1t, H, W, r.w1t, r.wpos, r.b1, r.w2, tid);
    const float b2 = *r.b2;

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
                f32x16 acc[NT];
                mlp_head_first_layer<NT>(acc, r.lr32 + l.src[ee] + 4 * aa, rstride, (float)l.pos[qc], W, s_w1t, s_wpos,
                                         s_b1, KP, lane);
                const float mean = mlp_head_out(mlp_head_p<NT>(acc, r.act, s_w2, half, b2), r.out_act);
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

// ---- fe_mlp_forward: one wavefront per block of 32 descriptor pairs, grid-strided; the weight image in LDS ----
template <bool SINGLE, int NT>
__global__ __launch_bounds__(kBlock, 2) void fe_mlp_forward_kernel(const Params p, const MlpHeadArgs r) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int A = SINGLE ? 1 : p.A;
    const int W = p.W;
    constexpr int H = 32 * NT;
    const int KP = mlp_kp(W);
    float *s_w1t = reinterpret_cast<float *>(smem);
    float *s_wpos = s_w1t + (size_t)H * KP;
    float *s_b1 = s_wpos + H;
    float *s_w2 = s_b1 + H;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, half = lane >> 5;
    mlp_head_load_weights(s_w1t, H, W, r.w1t, r.wpos, r.b1, r.w2, tid);
    const float b2 = *r.b2;
    __syncthreads();
    const int64_t pairs = r.count * A;
    const int64_t nblk = (pairs + 31) / 32;
    for (int64_t blk = (int64_t)blockIdx.x * (kBlock / 64) + wave; blk < nblk; blk += (int64_t)gridDim.x * (kBlock / 64)) {
        const int64_t q = blk * 32 + col;
        const int64_t qc = q < pairs ? q : pairs - 1;
        const int64_t ee = SINGLE ? qc : qc / A;
        const int aa = SINGLE ? 0 : (int)(qc - ee * A);
        f32x16 acc[NT];
        mlp_head_first_layer<NT>(acc, r.lr32 + r.obs_src[ee] + 4 * aa, 4 * (int64_t)A, (float)r.obs_pos[qc], W, s_w1t,
                                 s_wpos, s_b1, KP, lane);
        const float y = mlp_head_out(mlp_head_p<NT>(acc, r.act, s_w2, half, b2), r.out_act);
        if (half == 0 && q < pairs) r.actions_out[q] = y;
    }
}

// ---- fe_mlp_backward ----
constexpr int kMlpGradChunk = 512;      // FE_MLP_GRAD_CHUNK_PAIRS: pairs per split of the weight-gradient contraction
constexpr int kMlpGradMaxGroups = 512;  // workgroups of the first kernel at most: its partial count depends on `count` alone

struct MlpGradArgs {
    const float *lr32, *w1t, *wpos, *b1, *w2;
    const int64_t *obs_src;
    const double *obs_pos;
    const float *outputs, *d_outputs;
    float *dpre;    // (CP, H) dpre, CP = 32 * blocks; pairs >= count hold zeros
    float *part;    // (splits, H, FP) the splits' partial products, FP = 32 * feature tiles
    float *wpart;   // (waves, H + 4): every wavefront's partial of d w2 (H) and d b2 (1)
    float *g_w1, *g_b1, *g_w2, *g_b2;
    int64_t count, blocks, splits, waves;
    int32_t W, H, act, out_act, FP;
};

__host__ __device__ inline int mlp_grad_fp(int W) { return 32 * ((4 * W + 2 + 31) / 32); }
__host__ __device__ inline int64_t mlp_grad_groups(int64_t blocks) {
    const int64_t g = (blocks + 3) / 4;
    return g < kMlpGradMaxGroups ? g : kMlpGradMaxGroups;
}

// activation value and derivative on the forward's own value
template <int ACT>
__device__ __forceinline__ void mlp_act_grad(float z, float &a, float &d) {
    if constexpr (ACT == 1) {
        a = mlp_act<1>(z);
        d = z > 0.0f ? 1.0f : 0.0f;
    } else if constexpr (ACT == 2) {
        a = lstm_tanh(z);
        d = 1.0f - a * a;
    } else {
        const float ez = __expf(z);  // the forward's v_exp_f32
        a = z > 0.0f ? z : ez - 1.0f;
        d = z > 0.0f ? 1.0f : ez;
    }
}

// dpre of the lane's pair into its workspace row (four consecutive units per 16-byte store); d w2's in-lane partial
template <int ACT, int NT>
__device__ __forceinline__ void mlp_grad_block_tail(const f32x16 (&acc)[NT], float (&w2acc)[NT][16], const float *s_w2, int half,
                                                    float dp, bool valid, float *dpre_row) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int h0 = 32 * t + 8 * b + 4 * half;
            const float4 w2 = *reinterpret_cast<const float4 *>(s_w2 + h0);
            const float w2s[4] = {w2.x, w2.y, w2.z, w2.w};
            float o[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float a, d;
                mlp_act_grad<ACT>(acc[t][4 * b + c], a, d);
                w2acc[t][4 * b + c] = w2acc[t][4 * b + c] + (valid ? dp * a : 0.0f);
                o[c] = valid ? (dp * w2s[c]) * d : 0.0f;  // the padding pairs of the last block: zeros
            }
            *reinterpret_cast<float4 *>(dpre_row + h0) = make_float4(o[0], o[1], o[2], o[3]);
            // four units at a time: left alone the scheduler interleaves the activation chains of all 16 NT units, and at
            // H = 128 the register allocator then spills
            if constexpr (NT == 4) __builtin_amdgcn_sched_barrier(0);
        }
}

// (a) per 32-pair block and wavefront: the first layer recomputed, dp and dpre formed in-lane
template <int NT>
__global__ __launch_bounds__(kBlock, 2) void fe_mlp_grad_kernel(const MlpGradArgs g) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int H = 32 * NT;
    const int W = g.W;
    const int KP = mlp_kp(W);
    float *s_w1t = reinterpret_cast<float *>(smem);
    float *s_wpos = s_w1t + (size_t)H * KP;
    float *s_b1 = s_wpos + H;
    float *s_w2 = s_b1 + H;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, half = lane >> 5;
    mlp_head_load_weights(s_w1t, H, W, g.w1t, g.wpos, g.b1, g.w2, tid);
    __syncthreads();
    float w2acc[NT][16];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) w2acc[t][rr] = 0.0f;
    float b2acc = 0.0f;
    const int64_t gw = (int64_t)blockIdx.x * (kBlock / 64) + wave;
    for (int64_t blk = gw; blk < g.blocks; blk += (int64_t)gridDim.x * (kBlock / 64)) {
        const int64_t q = blk * 32 + col;
        const int64_t qc = q < g.count ? q : g.count - 1;
        f32x16 acc[NT];
        mlp_head_first_layer<NT>(acc, g.lr32 + g.obs_src[qc], 4, (float)g.obs_pos[qc], W, s_w1t, s_wpos, s_b1, KP, lane);
        float dp = 0.0f;
        if (q < g.count) {
            dp = g.d_outputs[q];
            if (g.out_act == 0) {
                const float y = g.outputs[q];
                dp = dp * (1.0f - y * y);
            }
        }
        if (half == 0) b2acc = b2acc + dp;
        float *dpre_row = g.dpre + q * H;
        if (g.act == 1) mlp_grad_block_tail<1, NT>(acc, w2acc, s_w2, half, dp, q < g.count, dpre_row);
        else if (g.act == 2) mlp_grad_block_tail<2, NT>(acc, w2acc, s_w2, half, dp, q < g.count, dpre_row);
        else mlp_grad_block_tail<0, NT>(acc, w2acc, s_w2, half, dp, q < g.count, dpre_row);
    }
    // the 32 pairs of the wavefront's columns: a butterfly in a fixed order (every lane ends with the same sum)
#pragma unroll
    for (int m = 1; m < 32; m <<= 1) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) w2acc[t][rr] = w2acc[t][rr] + __shfl_xor(w2acc[t][rr], m, 64);
        b2acc = b2acc + __shfl_xor(b2acc, m, 64);
    }
    if (col == 0) {
        float *wp = g.wpart + gw * (H + 4);
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) wp[32 * t + (rr & 3) + 8 * (rr >> 2) + 4 * half] = w2acc[t][rr];
        if (half == 0) wp[H] = b2acc;
    }
}

// (b) [dW1t | d wpos | d b1] = dpre^T [X | pos | 1]: one wavefront per (feature tile of 32, split of kMlpGradChunk pairs),
// all H rows; the contraction index is the pair, 8 pairs per group (lane half 0: pairs 8g..8g+3, half 1: 8g+4..8g+7).
// A elements are rows of dpre (32 hidden units of one pair: 128 contiguous bytes), B elements come straight from the f32
// log-return table (a feature tile of one pair is 128 contiguous bytes too).
template <int NT>
__global__ __launch_bounds__(kBlock, 2) void fe_mlp_wgrad_kernel(const MlpGradArgs g) {
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
        const int fc = f < K4 ? f : 0;  // the table offset of a real feature; the two extra columns and the padding read none
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
                else v = f == K4 ? (float)g.obs_pos[nc] : (f == K4 + 1 ? 1.0f : 0.0f);
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

// (c) the splits and the wavefronts' partials added in index order (f64, rounded once), written in torch's layout
__global__ __launch_bounds__(kBlock) void fe_mlp_grad_reduce_kernel(const MlpGradArgs g) {
    const int H = g.H, W = g.W, K4 = 4 * W, F = K4 + 2;
    const int64_t total = (int64_t)H * F + H + 1;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        if (i < (int64_t)H * F) {
            const int h = (int)(i / F), f = (int)(i - (int64_t)h * F);
            const float *src = g.part + (int64_t)h * g.FP + f;
            double s = 0.0;
            for (int64_t k = 0; k < g.splits; ++k) s += (double)src[k * (int64_t)H * g.FP];
            const float v = (float)s;
            float *row = g.g_w1 + (size_t)h * 5 * W;
            if (f < K4) row[5 * (f >> 2) + (f & 3)] = v;
            else if (f == K4) {  // the position column is the same in every window row
                for (int j = 0; j < W; ++j) row[5 * j + 4] = v;
            } else g.g_b1[h] = v;
        } else {
            const int h = (int)(i - (int64_t)H * F);  // h == H: d b2
            double s = 0.0;
            for (int64_t k = 0; k < g.waves; ++k) s += (double)g.wpart[k * (H + 4) + h];
            if (h < H) g.g_w2[h] = (float)s;
            else g.g_b2[0] = (float)s;
        }
    }
}

}  // namespace
