// fe_lstm_grad_streamed_kernels.h -- part of fe_env.hip (one translation unit; see the overview there): the backward pass
// of the one-output LSTM head at H = 256 / 512 / 1024 on observation descriptors
// (include/finenvs_amd_lstm_grad_streamed.h).
#pragma once
#include "fe_device_common.h"
#include "fe_lstm_kernel.h"

namespace {

// ---- d(loss) / d(parameters) of LSTMNetwork((5, H, 1), W, Tanh | Identity) with the recurrent weights streamed ----
// fe_lstm_grad_kernel keeps dz of a 32-pair tile in LDS and gives every workgroup a private 4H x (H + 32) partial: 525 KB
// and 17 MB at H = 1024.  At these sizes the pass is three large contractions, each a kernel of its own over a CHUNK of
// pairs (lstm_sgrad_chunk_pairs), with everything between them in the global workspace and the launch boundary as the
// exchange (the precedent: fe_env_rollout_lstm_split):
//   forward   fe_rollout_lstm_big_kernel's recurrence, forward only, one asset: the SAME contraction (fragment-major
//             W_hh streamed from L2 kLstmBigAhead k groups ahead, kLstmBigRI row tiles together, x then h in k-group
//             order, lstm_act2, the same cell update).  Per (t, pair): the activated gates in packed row order, c_t and
//             [h_{t-1} | x_t | 1 | 0 ...] (the vst row of fe_lstm_grad_kernel) into the workspace; h_W beside them;
//   head      dp = g (1 - y^2) | g;  dh_W = w_out dp;  d w_out, d b_out summed per 256-pair block in pair order;
//   backward  t = W-1 .. 0: an elementwise kernel forms dz_t over the gates of step t and updates dc in place, then
//             dh_{t-1} = W_hh^T dz_t on v_mfma_f32_32x32x2_f32 (units on M, pairs on N, K = 4H in 64-wide LDS slices);
//   weights   [dW_hh | dW_x | db] = dz^T [h_{t-1} | x_t | 1]: a 4H x (H + 32) output over K = pairs x W.  Every output
//             tile has one owner per K split; an MFMA chain runs over 1024 K columns, the chain sums are added in
//             order, and the splits are added in order by the final kernel;
//   final     the split sums in split order into torch's row order and layout (lstm_row_order undone while writing),
//             overwriting for the first chunk and adding for the later ones.
// No float atomics: the bits depend on the inputs alone (the chunk size and the split count are functions of H and W).
constexpr int kLstmSGradChunkUnit = 256;              // chunk_pairs is a multiple of this many pairs
constexpr int64_t kLstmSGradStashBytes = 1LL << 31;   // ... and the largest whose stash stays within 2 GiB
constexpr int kLstmSGradChain = 1024;                 // K columns of one MFMA chain of the weight contraction
constexpr int kLstmSGradWgRows = 256;                 // gate rows of one workgroup of the weight contraction
constexpr int kLstmSGradDhUnits = 128;                // hidden units of one workgroup of the dh contraction
constexpr int kLstmSGradDhK = 64;                     // K slice of the dh contraction
constexpr int kLstmSGradDhKP = kLstmSGradDhK + 4;     // its LDS row length: 16 bytes against bank conflicts
constexpr int kLstmSGradWgAP = kLstmSGradWgRows + 32; // LDS row length of the weight contraction's A slice

__host__ __device__ constexpr bool lstm_sgrad_hidden_ok(int H) { return H == 256 || H == 512 || H == 1024; }
// floats of the stash per pair: W x (4H gates | H c_t | H + 32 [h_{t-1} | x_t | 1 | 0 ...])
__host__ __device__ constexpr int64_t lstm_sgrad_pair_floats(int H, int W) { return (int64_t)W * (6LL * H + 32); }
__host__ __device__ constexpr int64_t lstm_sgrad_chunk_pairs(int H, int W) {
    const int64_t n = kLstmSGradStashBytes / (4 * lstm_sgrad_pair_floats(H, W)) / kLstmSGradChunkUnit;
    return (n < 1 ? 1 : n) * kLstmSGradChunkUnit;
}
// pairs one pass holds in the workspace: the chunk, or the whole batch rounded up to a 32-pair tile
__host__ __device__ constexpr int64_t lstm_sgrad_padded_pairs(int H, int W, int64_t count) {
    const int64_t chunk = lstm_sgrad_chunk_pairs(H, W);
    return count >= chunk ? chunk : (count + 31) / 32 * 32;
}
// K splits of the weight contraction: enough workgroups for the device at every H, never more than there are chains
__host__ __device__ constexpr int64_t lstm_sgrad_splits(int H, int W, int64_t padded) {
    const int64_t chains = (padded * W + kLstmSGradChain - 1) / kLstmSGradChain;
    const int64_t most = H == 256 ? 32 : (H == 512 ? 16 : 4);
    return chains < 1 ? 1 : (chains < most ? chains : most);
}
__host__ __device__ constexpr int64_t lstm_sgrad_wt_floats(int H) { return 4LL * H * H; }
__host__ __device__ constexpr int64_t lstm_sgrad_part_floats(int H) { return 4LL * H * (H + 32); }
__host__ __device__ constexpr int64_t lstm_sgrad_head_blocks(int64_t padded) { return (padded + 255) / 256; }
__host__ __device__ inline size_t lstm_sgrad_forward_lds_bytes(int H) {
    return 32 * 8 + 32 * 4 + (size_t)32 * (H + 4) * 4;  // src [32] | pos [32] | h [32][H + 4]
}

struct LstmSGradArgs {
    const float *lr32;
    const int64_t *obs_src;  // of this chunk
    const double *obs_pos;
    const float *whh, *wx, *wout;  // as fe_lstm_forward reads them (whh fragment-major)
    const float *outputs;          // (cnt) what fe_lstm_forward returned; null with out_act 2
    const float *d_outputs;        // (cnt) upstream gradient
    float *wt;      // (H, 4H) W_hh^T in packed gate-row order
    float *part;    // (splits, 4H, H + 32) split sums of [dW_hh | dW_x | db], packed row order
    float *hpart;   // (head blocks, H + 32) block sums of [d w_out | d b_out]
    float *gates;   // (W, pp, 4H) activated gates, packed row order; dz_t once the backward has passed step t
    float *cst;     // (W, pp, H) c_t
    float *vst;     // (W, pp, H + 32) [h_{t-1} | x_t | 1 | 0 ...]
    float *hw;      // (pp, H) h_W
    float *dh, *dc; // (pp, H) each
    int64_t cnt, pp;  // pairs of this chunk; rounded up to a 32-pair tile
    int64_t splits;
    int32_t W, out_act, t, first;  // t: the step of a backward launch; first: the final kernel overwrites (else adds)
    // fe_lstm_sgrad_final_kernel's outputs, torch row order and layout (include/finenvs_amd_lstm_grad.h)
    float *g_wih, *g_whh, *g_bih, *g_bhh, *g_wout, *g_bout;
};

// W_hh^T (H, 4H) from the fragment-major whh ([row tile][k group][lane = (row & 31) + 32 * k half][4]), one thread per
// element
__global__ __launch_bounds__(kBlock) void fe_lstm_sgrad_pack_kernel(const LstmSGradArgs g, int32_t H) {
    const int64_t G4 = 4 * H, NG = H / 8, n = lstm_sgrad_wt_floats(H);
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int64_t u = i / G4, R = i - u * G4;
        g.wt[i] = g.whh[(((R >> 5) * NG + (u >> 3)) * 64 + ((u >> 2) & 1) * 32 + (R & 31)) * 4 + (u & 3)];
    }
}

// The recurrence of fe_rollout_lstm_big_kernel (forward only, A = 1) with its activations written out: the tile loop it
// shares with fe_critic_sgrad_forward_kernel, without the action slot.
template <int RTW>
__global__ __launch_bounds__(kLstmBlock, 2) void fe_lstm_sgrad_forward_kernel(const LstmSGradArgs g) {
#define FE_LSTM_STREAM_ACTION 0
#include "fe_lstm_stream_sgrad_body.h"
#undef FE_LSTM_STREAM_ACTION
}

// The head's backward (networks/lstm.py:55-56 differentiated) for one 256-pair block per workgroup: dh_W = w_out dp and
// dc = 0 for the block's pairs, and the block's sums of d w_out = dp h_W and d b_out = dp in pair order.
__global__ __launch_bounds__(kBlock) void fe_lstm_sgrad_head_kernel(const LstmSGradArgs g, int32_t H) {
    __shared__ float s_dp[256];
    const int tid = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * 256;
    const int np = g.pp - p0 < 256 ? (int)(g.pp - p0) : 256;
    {
        const int64_t n = p0 + tid;
        float dp = 0.0f;
        if (n < g.cnt) {  // a pair past the end of the batch contributes zero
            dp = g.d_outputs[n];
            if (g.out_act == 0) {
                const float y = g.outputs[n];
                dp = dp * (1.0f - y * y);
            }
        }
        s_dp[tid] = dp;
    }
    __syncthreads();
    for (int i = tid; i < np * H; i += kBlock) {
        const int p = i / H, u = i - p * H;
        g.dh[p0 * H + i] = g.wout[u] * s_dp[p];
        g.dc[p0 * H + i] = 0.0f;
    }
    const float *hw = g.hw + p0 * H;
    for (int u = tid; u <= H; u += kBlock) {  // d w_out of unit u; u = H: d b_out
        float a0 = 0.0f;
        for (int p = 0; p < np; ++p) a0 = fmaf(u < H ? hw[(int64_t)p * H + u] : 1.0f, s_dp[p], a0);
        g.hpart[(int64_t)blockIdx.x * (H + 32) + u] = a0;
    }
}

// dz_t from dh_t, dc, the gates, c_t and c_{t-1} (the formulas of fe_lstm_grad_kernel), written over the gates of step t;
// dc updated in place.  One thread per (pair, four units 8 mt + 4 half + b): their gates are the float4 at packed rows
// 32 mt + 8 b + 4 half.
__global__ __launch_bounds__(kBlock) void fe_lstm_sgrad_dz_kernel(const LstmSGradArgs g, int32_t H) {
    const int64_t Q = H / 4, n = g.pp * Q, G4 = 4 * H;
    const int t = g.t;
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int64_t p = i / Q, q = i - p * Q, mt = q >> 1, half = q & 1;
        const int64_t row = (int64_t)t * g.pp + p;
        float *gr = g.gates + row * G4 + 32 * mt + 4 * half;
        const float4 c4 = *reinterpret_cast<const float4 *>(g.cst + row * H + 4 * q);
        const float4 cp4 = t > 0 ? *reinterpret_cast<const float4 *>(g.cst + (row - g.pp) * H + 4 * q)
                                 : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const float4 dh4 = *reinterpret_cast<const float4 *>(g.dh + p * H + 4 * q);
        float4 dc4 = *reinterpret_cast<float4 *>(g.dc + p * H + 4 * q);
        const float cc[4] = {c4.x, c4.y, c4.z, c4.w}, cp[4] = {cp4.x, cp4.y, cp4.z, cp4.w};
        const float dh[4] = {dh4.x, dh4.y, dh4.z, dh4.w};
        float dc[4] = {dc4.x, dc4.y, dc4.z, dc4.w};
#pragma unroll
        for (int b = 0; b < 4; b += 2) {
            const v2f tc = lstm_act2<true, true>((v2f){cc[b], cc[b + 1]});
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) {
                const int u = b + bb;
                const float tcu = bb == 0 ? tc.x : tc.y;
                const float4 gt = *reinterpret_cast<const float4 *>(gr + 8 * u);
                const float ig = gt.x, fg = gt.y, gg = gt.z, og = gt.w;
                const float dcc = dc[u] + dh[u] * og * (1.0f - tcu * tcu);
                *reinterpret_cast<float4 *>(gr + 8 * u) =
                    make_float4(dcc * gg * ig * (1.0f - ig), dcc * cp[u] * fg * (1.0f - fg), dcc * ig * (1.0f - gg * gg),
                                dh[u] * tcu * og * (1.0f - og));
                dc[u] = dcc * fg;
            }
        }
        *reinterpret_cast<float4 *>(g.dc + p * H + 4 * q) = make_float4(dc[0], dc[1], dc[2], dc[3]);
    }
}

// dh_{t-1} = W_hh^T dz_t: workgroup (x, y) computes units 128 x .. 128 x + 127 (one 32-unit tile per wavefront) of pairs
// 32 y .. 32 y + 31, K = 4H packed gate rows in slices of 64 staged through LDS (32 pairs x 4H floats alone are 512 KB at
// H = 1024).  One accumulator chain in k order per output tile.
__global__ __launch_bounds__(kBlock) void fe_lstm_sgrad_dh_kernel(const LstmSGradArgs g, int32_t H) {
    constexpr int KS = kLstmSGradDhK, KP = kLstmSGradDhKP, UT = kLstmSGradDhUnits;
    __shared__ __align__(16) float s_a[UT * KP];  // [unit][k]
    __shared__ __align__(16) float s_b[32 * KP];  // [pair][k]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
    const int64_t G4 = 4 * H, u0 = (int64_t)blockIdx.x * UT, p0 = (int64_t)blockIdx.y * 32;
    const float *wa = g.wt + u0 * G4;
    const float *zb = g.gates + ((int64_t)g.t * g.pp + p0) * G4;
    f32x16 acc;
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) acc[rr] = 0.0f;
    for (int64_t k0 = 0; k0 < G4; k0 += KS) {
#pragma unroll
        for (int j = 0; j < UT * KS / 4 / kBlock; ++j) {
            const int idx = j * kBlock + tid, r = idx / (KS / 4), c4 = idx % (KS / 4);
            *reinterpret_cast<float4 *>(s_a + r * KP + 4 * c4) = *reinterpret_cast<const float4 *>(wa + r * G4 + k0 + 4 * c4);
        }
#pragma unroll
        for (int j = 0; j < 32 * KS / 4 / kBlock; ++j) {
            const int idx = j * kBlock + tid, r = idx / (KS / 4), c4 = idx % (KS / 4);
            *reinterpret_cast<float4 *>(s_b + r * KP + 4 * c4) = *reinterpret_cast<const float4 *>(zb + r * G4 + k0 + 4 * c4);
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
    // acc[4b + j] is unit u0 + 32 wave + 8 b + 4 half + j of pair p0 + col
    float *out = g.dh + (p0 + col) * H + u0 + 32 * wave + 4 * half;
#pragma unroll
    for (int b = 0; b < 4; ++b)
        *reinterpret_cast<float4 *>(out + 8 * b) = make_float4(acc[4 * b], acc[4 * b + 1], acc[4 * b + 2], acc[4 * b + 3]);
}

// [dW_hh | dW_x | db] = dz^T [h_{t-1} | x_t | 1 | 0 ...] over the chunk's pp x W (step, pair) columns.  Workgroup (x, y):
// output tile x = 256 packed gate rows (two 32-row tiles per wavefront) x 32 columns, K split y.  K runs in slices of 32
// (step, pair) rows -- both operands have K as their slow index, so a slice is copied to LDS as it lies -- and in chains
// of kLstmSGradChain columns: a chain is one MFMA accumulation from zero, the chain sums are added in order.  A single
// f32 chain over the whole of K would lose the accuracy a blocked GEMM keeps.
__global__ __launch_bounds__(kBlock) void fe_lstm_sgrad_wgrad_kernel(const LstmSGradArgs g, int32_t H) {
    constexpr int RT = kLstmSGradWgRows, AP = kLstmSGradWgAP, SPC = kLstmSGradChain / 32;  // slices per chain
    __shared__ __align__(16) float s_a[32 * AP];  // [k][gate row]
    __shared__ __align__(16) float s_b[32 * 32];  // [k][column]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
    const int64_t G4 = 4 * H, VN = H + 32, NTN = VN / 32;
    const int64_t R0 = (int64_t)(blockIdx.x / NTN) * RT, n0 = (int64_t)(blockIdx.x % NTN) * 32;
    const int64_t tiles = g.pp / 32, slices = tiles * g.W, chains = (slices + SPC - 1) / SPC;
    const int64_t per = (chains + g.splits - 1) / g.splits;
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
        for (int64_t s = c * SPC; s < s_end; ++s) {  // slice s: step s / tiles, pairs 32 (s % tiles) ..: rows 32 s .. of the stash
            const float *za = g.gates + 32 * s * G4 + R0;
            const float *vb = g.vst + 32 * s * VN + n0;
#pragma unroll
            for (int j = 0; j < 32 * RT / 4 / kBlock; ++j) {
                const int idx = j * kBlock + tid, r = idx / (RT / 4), c4 = idx % (RT / 4);
                *reinterpret_cast<float4 *>(s_a + r * AP + 4 * c4) = *reinterpret_cast<const float4 *>(za + r * G4 + 4 * c4);
            }
            *reinterpret_cast<float4 *>(s_b + 4 * tid) = *reinterpret_cast<const float4 *>(vb + (tid >> 3) * VN + 4 * (tid & 7));
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
    // sum[i][rr] is row R0 + 64 wave + 32 i + 8 (rr >> 2) + 4 half + (rr & 3), column n0 + col
    float *out = g.part + (int64_t)blockIdx.y * lstm_sgrad_part_floats(H) + (R0 + 64 * wave + 4 * half) * VN + n0 + col;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) out[(32 * i + 8 * (rr >> 2) + (rr & 3)) * VN] = sum[i][rr];
}

// The split sums added in split order (the head's block sums in block order) and written in torch's row order: packed
// gate row R = 32 mt + 8 b + 4 half + gate is row gate H + 8 mt + 4 half + b of the 4H-row tensors (lstm_row_order's
// inverse).  NX input columns (5: the head; 6: the critic): column n - H < 5 of a split sum is w_ih[row, n - H], column 5
// the bias, column 6 (the action's slot, NX = 6) w_ih[row, 5]; the rest of the input tile is skipped.  The first chunk
// overwrites the gradients, a later one adds to them.
template <int NX>
__device__ __forceinline__ void lstm_sgrad_final(const LstmSGradArgs &g, int32_t H) {
    const int64_t stride = (int64_t)gridDim.x * kBlock, i0 = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    const int64_t VN = H + 32, PV = lstm_sgrad_part_floats(H), E = PV + H + 1;
    const int64_t blocks = lstm_sgrad_head_blocks(g.pp);
    const bool first = g.first != 0;
    for (int64_t e = i0; e < E; e += stride) {
        float s = 0.0f;
        if (e < PV) {
            const int64_t R = e / VN, n = e - R * VN;
            if (n >= H + NX + 1) continue;  // the input tile's unused columns
            for (int64_t k = 0; k < g.splits; ++k) s += g.part[k * PV + e];
            const int64_t rho = R & 31, row = (rho & 3) * H + 8 * (R >> 5) + 4 * ((rho >> 2) & 1) + (rho >> 3);
            if (n < H) {
                float *o = g.g_whh + row * H + n;
                *o = first ? s : *o + s;
            } else if (NX == 6 ? n - H != 5 : n - H < 5) {  // (each width its own statements: the head's compile as before)
                float *o = g.g_wih + row * NX + (NX == 6 ? (n - H < 5 ? n - H : 5) : n - H);
                *o = first ? s : *o + s;
            } else {
                s = first ? s : g.g_bih[row] + s;
                g.g_bih[row] = s;
                g.g_bhh[row] = s;
            }
        } else {
            for (int64_t k = 0; k < blocks; ++k) s += g.hpart[k * VN + (e - PV)];
            float *o = e - PV < H ? g.g_wout + (e - PV) : g.g_bout;
            *o = first ? s : *o + s;
        }
    }
}

__global__ __launch_bounds__(kBlock) void fe_lstm_sgrad_final_kernel(const LstmSGradArgs g, int32_t H) {
    lstm_sgrad_final<5>(g, H);
}

}  // namespace
