// fe_lstm_grad_kernels.h -- part of fe_env.hip (one translation unit; see the overview there): the backward pass of the
// one-output LSTM head (PPO's actor and critic, TD3's actor) on observation descriptors
// (include/finenvs_amd_lstm_grad.h).
#pragma once
#include "fe_bptt_tile.h"

namespace {

// ---- d(loss) / d(parameters) of LSTMNetwork((5, H, 1), W, Tanh | Identity) (networks/lstm.py:28-57) ----
// The tile of fe_bptt_tile.h with a one-output head and a 5-wide input:
//   head      in-lane, one lane per pair, from the forward's own y = outputs[n] and g = d_outputs[n]:
//               dp = g (1 - y^2) (tanh) or g (none);   dh_W = w_out dp;   d w_out += dp h_W,  d b_out += dp;
//   backward  dh_{t-1} = W_hh^T dz_t only: the input has no learnt column, so dx_t is never formed.
// fe_lstm_grad_reduce_kernel writes the sums in torch's row order and layout (the inverse of lstm_row_order applied
// while writing).
constexpr int kLstmGradBlock = kBpttBlock;

// the resident workgroup count of fe_lstm_grad_kernel on an MI355X (256 CUs; at H = 128 the LDS admits one per CU)
__host__ __device__ constexpr int64_t lstm_grad_max_groups(int H) { return H == 128 ? 256 : 512; }
// [4H x (H + 32) LSTM tiles][d w_out (H) | d b_out | pad]
__host__ __device__ constexpr int64_t lstm_grad_part_floats(int H) { return 4LL * H * (H + 32) + H + 32; }
// W_hh^T (H, 4H)
__host__ __device__ constexpr int64_t lstm_grad_wt_floats(int H) { return 4LL * H * H; }
// LDS of one workgroup: 22 528 B at H = 32, 43 136 B at 64, 84 352 B at 128 (one workgroup per CU there)
__host__ __device__ inline size_t lstm_grad_lds_bytes(int H) {
    // dz [32][4H + 4] (holds the h double buffer before) | dh [32][H + 4] | w_out [H] | dp [32] | (pos, 1, 0, 0) [32] |
    // src [32]
    return (32 * (size_t)(4 * H + 4) + 32 * (size_t)(H + 4) + (size_t)H + 32 + 32 * 4) * 4 + 32 * 8;
}

struct LstmGradArgs {
    const float *lr32;
    const int64_t *obs_src;
    const double *obs_pos;
    const float *whh, *wx, *wout;  // as fe_lstm_forward reads them
    const float *outputs;          // (count) what fe_lstm_forward returned; null with out_act 2
    const float *d_outputs;        // (count) upstream gradient
    float *wt;     // (H, 4H) W_hh^T in packed gate-row order
    float *part;   // (groups, lstm_grad_part_floats(H))
    float *stash;  // (groups, bptt_stash_floats(H, W))
    int64_t count, num_tiles, groups;
    int32_t W, out_act;
    // fe_lstm_grad_reduce_kernel's outputs, torch row order and layout (include/finenvs_amd_lstm_grad.h)
    float *g_wih, *g_whh, *g_bih, *g_bhh, *g_wout, *g_bout;
};

// W_hh^T from the packed whh (one thread per element)
__global__ __launch_bounds__(kBlock) void fe_lstm_grad_pack_kernel(const LstmGradArgs g, int32_t H) {
    const int64_t G4 = 4 * H, n = lstm_grad_wt_floats(H);
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int64_t u = i / G4, R = i - u * G4;
        g.wt[i] = g.whh[R * H + u];
    }
}

template <int NT>
__global__ __launch_bounds__(kLstmGradBlock) void fe_lstm_grad_kernel(const LstmGradArgs g) {
    constexpr int H = 32 * NT, MPW = H / 32, G4 = 4 * H, ZT = H / 32;
    constexpr int HPF = H + 4, G4P = G4 + 4, VN = H + 32;
    constexpr int PV = 4 * H * VN;  // the head's vector in the partials
    static_assert(2 * 32 * HPF <= 32 * G4P, "the h double buffer shares the dz buffer");
    extern __shared__ __align__(16) unsigned char smem[];
    const int W = g.W;
    float *s_x = reinterpret_cast<float *>(smem);  // h double buffer [2][32][HPF]; dz_t [32][G4P]
    float *s_dh = s_x + 32 * G4P;                  // [32][HPF]: dh_t
    float *s_wout = s_dh + 32 * HPF;               // [H]
    float *s_dp = s_wout + H;                      // [32]: d loss / d p
    float4 *s_xh = reinterpret_cast<float4 *>(s_dp + 32);     // [32] (pos, 1, 0, 0)
    int64_t *s_src = reinterpret_cast<int64_t *>(s_xh + 32);  // [32]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
    float *part = g.part + blockIdx.x * lstm_grad_part_floats(H);
    float *stash = g.stash + blockIdx.x * bptt_stash_floats(H, W);
    float *vst = stash + (int64_t)W * 160 * H;  // [W][32][VN]: [h_{t-1} | x_t | 0] per pair
    for (int i = tid; i < H; i += kLstmGradBlock) s_wout[i] = g.wout[i];

    for (int64_t tile = blockIdx.x; tile < g.num_tiles; tile += gridDim.x) {
        const bool first = tile == (int64_t)blockIdx.x;  // the partials are written, then added to
        const int64_t n0 = tile * 32;
        const int pairs = g.count - n0 < 32 ? (int)(g.count - n0) : 32;
        if (tid < 32) {  // a pair past the batch computes on the last one's descriptor with a zero upstream gradient
            const int64_t n = n0 + (tid < pairs ? tid : pairs - 1);
            s_src[tid] = g.obs_src[n];
            s_xh[tid] = make_float4((float)g.obs_pos[n], 1.0f, 0.0f, 0.0f);
            float dp = 0.0f;
            if (tid < pairs) {
                dp = g.d_outputs[n];
                if (g.out_act == 0) {
                    const float y = g.outputs[n];
                    dp = dp * (1.0f - y * y);
                }
            }
            s_dp[tid] = dp;
        }
        __syncthreads();
        bptt_stash_inputs<H, false>(vst, g.lr32, s_src, s_xh, W, tid);

        // ---- forward: fe_lstm_forward's recurrence, the activations into the stash ----
        float cst[MPW][4];
#pragma unroll
        for (int i = 0; i < MPW; ++i)
#pragma unroll
            for (int b = 0; b < 4; ++b) cst[i][b] = 0.0f;
        const float *xsrc = g.lr32 + s_src[col];
        const float4 xhc = s_xh[col];
        for (int t = 0; t < W; ++t) {
            bptt_forward_step<H>(t, W, g.whh, g.wx, xsrc, xhc, s_x, stash, vst, cst, wave, lane, col, half);
            __syncthreads();  // h_t is complete
        }

        // ---- the head's backward (networks/lstm.py:55-56 differentiated): dh_W = w_out dp, d w_out, d b_out ----
        const float *hW = s_x + ((W - 1) & 1) * 32 * HPF;
        for (int i = tid; i < 32 * H; i += kLstmGradBlock) {
            const int p = i / H, u = i - p * H;
            s_dh[p * HPF + u] = s_wout[u] * s_dp[p];
        }
        for (int u = tid; u <= H; u += kLstmGradBlock) {  // d w_out of unit u; u = H: d b_out
            float a0 = 0.0f;
            for (int p = 0; p < 32; ++p) a0 = fmaf(u < H ? hW[p * HPF + u] : 1.0f, s_dp[p], a0);
            part[PV + u] = first ? a0 : part[PV + u] + a0;
        }
        __syncthreads();  // dh_W is complete; h_W is read (its buffer becomes dz_t)

        // ---- backward through time ----
        float dc[MPW][4];
#pragma unroll
        for (int i = 0; i < MPW; ++i)
#pragma unroll
            for (int b = 0; b < 4; ++b) dc[i][b] = 0.0f;
        for (int t = W - 1; t >= 0; --t) {
            bptt_dz_step<H, HPF>(t, s_dh, s_x, stash, dc, wave, lane, col, half);
            __syncthreads();  // dz_t is complete; dh_t and the gates of step t are read
            bptt_dz_to_stash<H>(t, s_x, stash, tid);
            // dh_{t-1} = W_hh^T dz_t: units on M, pairs on N, k = R (not needed before the first step)
            if (t > 0) bptt_wt_contract<G4, G4P, HPF>(g.wt, s_x, s_dh, ZT, wave, col, half);
            __syncthreads();  // dh_{t-1} is complete; dz_t is read
        }

        // ---- weight gradients: [dW_hh | dW_x] += dz [h | x]^T over the tile's 32 W (pair, step) columns ----
        bptt_weight_grads<H>(stash, vst, part, W, first, wave, lane, col, half);
        __syncthreads();  // the stash and LDS are free for the next tile
    }
}

// The partials of every workgroup summed in workgroup order, written in torch's row order: packed gate row
// R = 32 mt + 8 b + 4 half + gate is row gate H + 8 mt + 4 half + b of the 4H-row tensors (lstm_row_order's inverse).
__global__ __launch_bounds__(kBlock) void fe_lstm_grad_reduce_kernel(const LstmGradArgs g, int32_t H) {
    const int64_t stride = (int64_t)gridDim.x * kBlock, i0 = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    const int64_t PF = lstm_grad_part_floats(H), VN = H + 32, NTO = H / 32 + 1;
    const int64_t PV = 4LL * H * VN, E = PV + H + 1;
    for (int64_t e = i0; e < E; e += stride) {
        int64_t f = e, R = 0, n = 0;
        if (e < PV) {  // an element of a 32 x 32 accumulator tile: row R, column n of [dW_hh | dW_x]
            R = e / VN;
            n = e - R * VN;
            if (n >= H + 6) continue;  // the input tile's unused columns
            const int64_t mt = R >> 5, rr = R & 31, r = 4 * (rr >> 3) + (rr & 3), hh = (rr >> 2) & 1;
            f = ((mt * NTO + (n >> 5)) * 16 + r) * 64 + (n & 31) + 32 * hh;
        }
        float s = 0.0f;
        for (int64_t k = 0; k < g.groups; ++k) s += g.part[k * PF + f];
        if (e < PV) {
            const int64_t rho = R & 31, row = (rho & 3) * H + 8 * (R >> 5) + 4 * ((rho >> 2) & 1) + (rho >> 3);
            if (n < H) {
                g.g_whh[row * H + n] = s;
            } else if (n - H < 5) {
                g.g_wih[row * 5 + (n - H)] = s;
            } else {
                g.g_bih[row] = s;
                g.g_bhh[row] = s;
            }
        } else if (e - PV < H) {
            g.g_wout[e - PV] = s;
        } else {
            *g.g_bout = s;
        }
    }
}

}  // namespace
