// fe_sac_streamed_kernels.h -- part of fe_env.hip (one translation unit; see the overview there): the SAC LSTM actor at
// H = 256 / 512 / 1024 (include/finenvs_amd_sac_streamed.h): acting, the forward on descriptors and the backward pass.
#pragma once
#include "fe_device_common.h"
#include "fe_lstm_kernel.h"
#include "fe_lstm_grad_streamed_kernels.h"

namespace {

// ---- the SAC actor's head on the streamed recurrence (fe_lstm_big_rollout_body.h with FE_LSTM_SAC_HEAD 1) ----
// LDS: fe_rollout_lstm_big_kernel's, with w_mu in the slot of wout, then w_std, b_l and SacBigHeadLds (16-byte aligned: H
// is a multiple of 64): 145 KiB at H = 1024, one workgroup per CU as there.  W_l (fragment-major, H x H) streams from L2.
struct SacBigHeadLds {  // copied to LDS once per launch (see fe_lstm_big_rollout_body.h)
    float *stds_out, *logp_out;
    const float *wl;
    float bmu, bstd;
};

__host__ __device__ constexpr int sac_big_head_lds_offset(int H) { return 3 * H; }

__host__ __device__ inline size_t sac_big_lds_bytes(int EB, int A, int H) {
    size_t b = lstm_big_lds_bytes(EB, A, H);  // ... h (one buffer), w_mu in the slot of wout
    b += (size_t)(sac_big_head_lds_offset(H) - H) * 4 + sizeof(SacBigHeadLds);
    return (b + 15) & ~(size_t)15;
}

template <bool SINGLE, int RTW>
__global__ __launch_bounds__(kLstmBlock, 2) void fe_rollout_sac_big_kernel(const Params p, const SacArgs hd) {
    const LstmArgs &r = hd.l;
#define FE_LSTM_SAC_HEAD 1
#include "fe_lstm_big_rollout_body.h"
#undef FE_LSTM_SAC_HEAD
}

// ---- d(loss) / d(parameters) of ActorLSTM((5, H, 1), W) at these sizes (SAC/actor.py:44-61, networks/lstm.py:28-57) ----
// The chunked pass of fe_lstm_grad_streamed_kernels.h -- its recompute (which leaves h_W in g.hw and the stash), its
// per-step dz / dh kernels and its weight contraction, unchanged -- with the SAC head between the recompute and the loop
// over t, every stage a kernel of its own over the chunk's pp pairs with the launch boundary as the exchange:
//   z        z = W_l h_W + b_l on v_mfma_f32_32x32x2_f32 with the forward's chain: one accumulator from zero per 32-unit
//            row tile, k groups ascending from the fragment-major W_l, b_l added afterwards;
//   head     per pair from the forward's own a = actions[n] and s = stds[n], the formulas and the operation order of
//            fe_sac_grad_kernel (include/finenvs_amd_sac_grad.h): q = w_std . z + b_std recomputed, du, dmu, ds, dq,
//            dz = w_mu dmu + w_std dq; dc = 0; the sums of d w_mu, d b_mu, d w_std, d b_std and d b_l per 256-pair block
//            in pair order (fe_lstm_sgrad_head_kernel's scheme: [d w_mu | d b_mu] lie where it puts [d w_out | d b_out]);
//   dh       dh_W = W_l^T dz (W_l^T from fe_sac_sgrad_pack_kernel): input units on M, pairs on N, K = H in LDS slices;
//   wl       d W_l = dz^T h_W, an H x H output over K = pairs: chains of kLstmSGradChain K columns, the chain sums added
//            in order, the K splits (sac_sgrad_wl_splits, a function of H and the padded pairs) in order by the final kernel;
//   final    lstm_sgrad_final<5> for the LSTM's four tensors, w_mu and b_mu, then d W_l, d b_l, d w_std and d b_std in
//            split / block order; the first chunk overwrites, a later one adds.
// No float atomics: the bits depend on the inputs alone.
__host__ __device__ constexpr int64_t sac_sgrad_wl_splits(int H, int64_t padded) {
    const int64_t chains = (padded + kLstmSGradChain - 1) / kLstmSGradChain;
    const int64_t most = H == 256 ? 32 : (H == 512 ? 16 : 4);
    return chains < 1 ? 1 : (chains < most ? chains : most);
}
__host__ __device__ constexpr int64_t sac_sgrad_hpart_floats(int H) { return 2LL * H + 32; }  // [d w_std | d b_l | d b_std | pad]
// floats in front of the LSTM pass's workspace: W_l^T | split sums of d W_l | head block sums | z | the head's dz
__host__ __device__ constexpr int64_t sac_sgrad_extra_floats(int H, int64_t padded) {
    return (1 + sac_sgrad_wl_splits(H, padded)) * (int64_t)H * H + lstm_sgrad_head_blocks(padded) * sac_sgrad_hpart_floats(H) +
           2 * padded * H;
}

struct SacSGradArgs {
    LstmSGradArgs g;  // recurrence, stash and the LSTM's gradients; g.hpart = [d w_mu | d b_mu], g.g_wout / g.g_bout = d w_mu / d b_mu
    const float *wl, *bl, *wmu, *wstd, *bstd;              // as fe_sac_forward_streamed reads them; bstd (1) on the device
    const float *noise, *actions, *stds;                   // of this chunk: eps, and what the forward returned
    const float *d_actions, *d_log_probs;                  // of this chunk, either may be null
    float *wlt;      // (H, H) W_l^T: row = input unit
    float *lpart;    // (wl_splits, H, H) split sums of d W_l, torch's [out][in]
    float *hpart2;   // (head blocks, 2H + 32) block sums of [d w_std | d b_l | d b_std]
    float *z, *dzh;  // (pp, H) each: z, and d loss / d z
    int64_t wl_splits;
    float *g_wl, *g_bl, *g_wstd, *g_bstd;  // the final kernel's further outputs (fe_sac_grads)
};

// W_l^T (H, H) from the fragment-major wl, one thread per element
__global__ __launch_bounds__(kBlock) void fe_sac_sgrad_pack_kernel(const SacSGradArgs a, int32_t H) {
    const int64_t NG = H / 8, n = (int64_t)H * H;
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int64_t in = i / H, o = i - in * H;  // W_l[o][in]
        a.wlt[i] = a.wl[((((o >> 5) * NG + (in >> 3)) * 64) + (o & 31) + 32 * ((in >> 2) & 1)) * 4 + (in & 3)];
    }
}

// z = W_l h_W + b_l: workgroup (x, y) computes units 128 x .. 128 x + 127 (one 32-unit row tile per wavefront) of pairs
// 32 y .. 32 y + 31; the A fragments straight from the fragment-major W_l (one coalesced KiB per k group), h_W in K slices
// of 64 through LDS.  The forward's chain: from zero, k groups ascending, the bias afterwards.
__global__ __launch_bounds__(kBlock) void fe_sac_sgrad_z_kernel(const SacSGradArgs a, int32_t H) {
    constexpr int KS = kLstmSGradDhK, KP = kLstmSGradDhKP;
    __shared__ __align__(16) float s_b[32 * KP];  // [pair][k]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
    const int64_t NG = H / 8, zt = (int64_t)blockIdx.x * 4 + wave, p0 = (int64_t)blockIdx.y * 32;
    const float4 *wf = reinterpret_cast<const float4 *>(a.wl) + zt * NG * 64 + lane;
    const float *hb = a.g.hw + p0 * H;
    f32x16 acc;
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) acc[rr] = 0.0f;
    for (int64_t k0 = 0; k0 < H; k0 += KS) {
#pragma unroll
        for (int j = 0; j < 32 * KS / 4 / kBlock; ++j) {
            const int idx = j * kBlock + tid, r = idx / (KS / 4), c4 = idx % (KS / 4);
            *reinterpret_cast<float4 *>(s_b + r * KP + 4 * c4) = *reinterpret_cast<const float4 *>(hb + r * H + k0 + 4 * c4);
        }
        __syncthreads();
#pragma unroll
        for (int gg = 0; gg < KS / 8; ++gg) {
            const float4 wv = wf[(k0 / 8 + gg) * 64];
            const float4 hv = *reinterpret_cast<const float4 *>(s_b + col * KP + 8 * gg + 4 * half);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const float ws = m == 0 ? wv.x : (m == 1 ? wv.y : (m == 2 ? wv.z : wv.w));
                const float hs = m == 0 ? hv.x : (m == 1 ? hv.y : (m == 2 ? hv.z : hv.w));
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ws, hs, acc, 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // acc[4b + c] is unit 32 zt + 8 b + 4 half + c of pair p0 + col
    float *out = a.z + (p0 + col) * H;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int64_t u0 = 32 * zt + 8 * b + 4 * half;
        *reinterpret_cast<float4 *>(out + u0) = make_float4(acc[4 * b] + a.bl[u0], acc[4 * b + 1] + a.bl[u0 + 1],
                                                            acc[4 * b + 2] + a.bl[u0 + 2], acc[4 * b + 3] + a.bl[u0 + 3]);
    }
}

// The head's backward (SAC/actor.py:51-61 differentiated) for one 256-pair block per workgroup, one thread per pair: q
// in slabs of 32 units staged through LDS (the chain stays the pair's own: from b_std, units ascending, fmaf), then
// dmu and dq, the head's dz and dc = 0 for the block's pairs, and the block's sums in pair order.
__global__ __launch_bounds__(kBlock) void fe_sac_sgrad_head_kernel(const SacSGradArgs a, int32_t H) {
    __shared__ float s_z[256 * 33];  // [pair][unit of the slab], padded against bank conflicts
    __shared__ float s_dmu[256], s_dq[256];
    const LstmSGradArgs &g = a.g;
    const int tid = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * 256;
    const int np = g.pp - p0 < 256 ? (int)(g.pp - p0) : 256;
    const float *zb = a.z + p0 * H;
    float q = *a.bstd;
    for (int u0 = 0; u0 < H; u0 += 32) {
        for (int i = tid; i < np * 32; i += kBlock) s_z[(i >> 5) * 33 + (i & 31)] = zb[(int64_t)(i >> 5) * H + u0 + (i & 31)];
        __syncthreads();
        if (tid < np) {
#pragma unroll 4
            for (int u = 0; u < 32; ++u) q = fmaf(a.wstd[u0 + u], s_z[tid * 33 + u], q);
        }
        __syncthreads();
    }
    {
        const int64_t n = p0 + tid;
        float du = 0.0f, dq = 0.0f;
        if (n < g.cnt) {  // a pair past the end of the batch contributes zero
            const float av = a.actions[n], sv = a.stds[n], ev = a.noise[n];
            const float ga = a.d_actions ? a.d_actions[n] : 0.0f;
            const float om = 1.0f - av * av;
            float ds;
            if (a.d_log_probs) {
                const float gl = a.d_log_probs[n];
                du = ga * om + gl * (2.0f * av * om / (om + 1e-7f));
                ds = du * ev - gl / sv;
            } else {  // fe_lstm_sgrad_head_kernel's dp for tanh, to the bit
                du = ga * om;
                ds = du * ev;
            }
            const float sg = q > 20.0f ? 1.0f : 1.0f / (1.0f + expf(-q));  // d softplus (beta 1, threshold 20)
            dq = ds * sg;
        }
        s_dmu[tid] = du;
        s_dq[tid] = dq;
    }
    __syncthreads();
    for (int i = tid; i < np * H; i += kBlock) {
        const int p = i / H, u = i - p * H;
        a.dzh[p0 * H + i] = a.wmu[u] * s_dmu[p] + a.wstd[u] * s_dq[p];
        g.dc[p0 * H + i] = 0.0f;
    }
    for (int u = tid; u <= H; u += kBlock) {  // d w_mu, d w_std, d b_l of unit u; u = H: d b_mu, d b_std
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
        const float wm = u < H ? a.wmu[u] : 0.0f, ws = u < H ? a.wstd[u] : 0.0f;
        for (int p = 0; p < np; ++p) {
            const float zv = u < H ? zb[(int64_t)p * H + u] : 1.0f;
            a0 = fmaf(zv, s_dmu[p], a0);
            a1 = fmaf(zv, s_dq[p], a1);
            a2 += wm * s_dmu[p] + ws * s_dq[p];
        }
        g.hpart[(int64_t)blockIdx.x * (H + 32) + u] = a0;
        float *h2 = a.hpart2 + (int64_t)blockIdx.x * sac_sgrad_hpart_floats(H);
        if (u < H) {
            h2[u] = a1;
            h2[H + u] = a2;
        } else {
            h2[2 * H] = a1;
        }
    }
}

// dh_W = W_l^T dz: fe_lstm_sgrad_dh_kernel's tiling with K = H output units of the last layer.
__global__ __launch_bounds__(kBlock) void fe_sac_sgrad_dh_kernel(const SacSGradArgs a, int32_t H) {
    constexpr int KS = kLstmSGradDhK, KP = kLstmSGradDhKP, UT = kLstmSGradDhUnits;
    __shared__ __align__(16) float s_a[UT * KP];  // [input unit][k]
    __shared__ __align__(16) float s_b[32 * KP];  // [pair][k]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
    const int64_t u0 = (int64_t)blockIdx.x * UT, p0 = (int64_t)blockIdx.y * 32;
    const float *wa = a.wlt + u0 * H;
    const float *zb = a.dzh + p0 * H;
    f32x16 acc;
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) acc[rr] = 0.0f;
    for (int64_t k0 = 0; k0 < H; k0 += KS) {
#pragma unroll
        for (int j = 0; j < UT * KS / 4 / kBlock; ++j) {
            const int idx = j * kBlock + tid, r = idx / (KS / 4), c4 = idx % (KS / 4);
            *reinterpret_cast<float4 *>(s_a + r * KP + 4 * c4) = *reinterpret_cast<const float4 *>(wa + r * H + k0 + 4 * c4);
        }
#pragma unroll
        for (int j = 0; j < 32 * KS / 4 / kBlock; ++j) {
            const int idx = j * kBlock + tid, r = idx / (KS / 4), c4 = idx % (KS / 4);
            *reinterpret_cast<float4 *>(s_b + r * KP + 4 * c4) = *reinterpret_cast<const float4 *>(zb + r * H + k0 + 4 * c4);
        }
        __syncthreads();
#pragma unroll
        for (int gg = 0; gg < KS / 8; ++gg) {
            const float4 wv = *reinterpret_cast<const float4 *>(s_a + (32 * wave + col) * KP + 8 * gg + 4 * half);
            const float4 zv = *reinterpret_cast<const float4 *>(s_b + col * KP + 8 * gg + 4 * half);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const float ws = m == 0 ? wv.x : (m == 1 ? wv.y : (m == 2 ? wv.z : wv.w));
                const float zs = m == 0 ? zv.x : (m == 1 ? zv.y : (m == 2 ? zv.z : zv.w));
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ws, zs, acc, 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // acc[4b + j] is input unit u0 + 32 wave + 8 b + 4 half + j of pair p0 + col
    float *out = a.g.dh + (p0 + col) * H + u0 + 32 * wave + 4 * half;
#pragma unroll
    for (int b = 0; b < 4; ++b)
        *reinterpret_cast<float4 *>(out + 8 * b) = make_float4(acc[4 * b], acc[4 * b + 1], acc[4 * b + 2], acc[4 * b + 3]);
}

// d W_l = dz^T h_W over the chunk's pp pairs: fe_lstm_sgrad_wgrad_kernel's scheme.  Workgroup (x, y): output tile x = 256
// output units (two 32-row tiles per wavefront) x 32 input units, K split y; K in slices of 32 pairs copied to LDS as they
// lie, chains of kLstmSGradChain pairs from zero, the chain sums added in order.  A split past the last chain writes zeros.
__global__ __launch_bounds__(kBlock) void fe_sac_sgrad_wl_kernel(const SacSGradArgs a, int32_t H) {
    constexpr int RT = kLstmSGradWgRows, AP = kLstmSGradWgAP, SPC = kLstmSGradChain / 32;  // slices per chain
    __shared__ __align__(16) float s_a[32 * AP];  // [k][output unit]
    __shared__ __align__(16) float s_b[32 * 32];  // [k][input unit]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
    const int64_t NTN = H / 32;
    const int64_t R0 = (int64_t)(blockIdx.x / NTN) * RT, n0 = (int64_t)(blockIdx.x % NTN) * 32;
    const int64_t slices = a.g.pp / 32, chains = (slices + SPC - 1) / SPC;
    const int64_t per = (chains + a.wl_splits - 1) / a.wl_splits;
    const int64_t c_begin = (int64_t)blockIdx.y * per, c_end = c_begin + per < chains ? c_begin + per : chains;
    f32x16 sum[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) sum[i][rr] = 0.0f;
    for (int64_t c = c_begin; c < c_end; ++c) {
        f32x16 acc[2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) acc[i][rr] = 0.0f;
        const int64_t s_end = (c + 1) * SPC < slices ? (c + 1) * SPC : slices;
        for (int64_t s = c * SPC; s < s_end; ++s) {  // slice s: pairs 32 s .. 32 s + 31
            const float *za = a.dzh + 32 * s * H + R0;
            const float *vb = a.g.hw + 32 * s * H + n0;
#pragma unroll
            for (int j = 0; j < 32 * RT / 4 / kBlock; ++j) {
                const int idx = j * kBlock + tid, r = idx / (RT / 4), c4 = idx % (RT / 4);
                *reinterpret_cast<float4 *>(s_a + r * AP + 4 * c4) = *reinterpret_cast<const float4 *>(za + r * H + 4 * c4);
            }
            *reinterpret_cast<float4 *>(s_b + 4 * tid) = *reinterpret_cast<const float4 *>(vb + (tid >> 3) * H + 4 * (tid & 7));
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) {
                const int k = 2 * kk + half;
                const float vs = s_b[k * 32 + col];
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(s_a[k * AP + 64 * wave + 32 * i + col], vs, acc[i], 0, 0, 0);
            }
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) sum[i][rr] += acc[i][rr];
    }
    // sum[i][rr] is output unit R0 + 64 wave + 32 i + 8 (rr >> 2) + 4 half + (rr & 3), input unit n0 + col
    float *out = a.lpart + (int64_t)blockIdx.y * H * H + (R0 + 64 * wave + 4 * half) * H + n0 + col;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) out[(32 * i + 8 * (rr >> 2) + (rr & 3)) * H] = sum[i][rr];
}

// All ten tensors in torch's row order and layout: the LSTM's four, w_mu and b_mu as the head's final kernel writes its
// six, then d W_l in split order and d w_std, d b_l, d b_std in block order.
__global__ __launch_bounds__(kBlock) void fe_sac_sgrad_final_kernel(const SacSGradArgs a, int32_t H) {
    lstm_sgrad_final<5>(a.g, H);
    const int64_t stride = (int64_t)gridDim.x * kBlock, i0 = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    const int64_t HH = (int64_t)H * H, E = HH + 2 * H + 1, HP2 = sac_sgrad_hpart_floats(H);
    const int64_t blocks = lstm_sgrad_head_blocks(a.g.pp);
    const bool first = a.g.first != 0;
    for (int64_t e = i0; e < E; e += stride) {
        float s = 0.0f;
        float *o;
        if (e < HH) {
            for (int64_t k = 0; k < a.wl_splits; ++k) s += a.lpart[k * HH + e];
            o = a.g_wl + e;
        } else {
            const int64_t u = e - HH;
            for (int64_t k = 0; k < blocks; ++k) s += a.hpart2[k * HP2 + u];
            o = u < H ? a.g_wstd + u : (u < 2 * H ? a.g_bl + (u - H) : a.g_bstd);
        }
        *o = first ? s : *o + s;
    }
}

}  // namespace
