// fe_critic_grad_kernels.h -- part of fe_env.hip (one translation unit; see the overview there): the backward pass
// through time of the twin LSTM critics on observation descriptors (include/finenvs_amd_critic_grad.h).
#pragma once
#include "fe_bptt_tile.h"

namespace {

// ---- d(loss) / d(parameters, action) of CriticLSTM((6, H, 1), W) (SAC/critic.py:30-45, TD3/critic.py:31-46) ----
// The tile of fe_bptt_tile.h, one critic per blockIdx.y, with a 6-wide input whose slot 6 is the action:
//   head      q = w_out . h_W + b_out: dh_W = w_out dq, d w_out += dq h_W, d b_out += dq;
//   backward  [dh_{t-1} | dx_t] = [W_hh | W_x]^T dz_t at every step (wt from fe_critic_grad_pack_kernel).  The action's
//             gradient of a pair is row 6 of dx summed over t (one lane per pair), per critic; the reduction
//             (fe_critic_grad_reduce_kernel, packed row order) adds the two critics'.
// A critic whose weights are frozen (g_whh null) forms no weight gradients.
constexpr int kCriticGradBlock = kBpttBlock;

// partial sums per critic: the resident workgroup count of fe_critic_grad_kernel on an MI355X (256 CUs; at H = 128
// the LDS admits one workgroup per CU, so 128 per critic half of the grid)
__host__ __device__ constexpr int64_t critic_grad_max_groups(int H) { return H == 128 ? 128 : 256; }
__host__ __device__ constexpr int64_t critic_grad_part_floats(int H) { return 4LL * H * (H + 32) + H + 32; }
__host__ __device__ constexpr int64_t critic_grad_wt_floats(int H) { return (int64_t)(H + 32) * 4 * H; }
__host__ __device__ inline size_t critic_grad_lds_bytes(int H) {
    const size_t hbuf = 2 * 32 * (size_t)(H + 4), dzb = 32 * (size_t)(4 * H + 4);
    return ((hbuf > dzb ? hbuf : dzb) + 32 * (size_t)(H + 36) + H + 32 + 32 * 4) * 4 + 32 * 8;
}

struct CriticGradNet {
    const float *whh, *wx, *wout;  // as fe_twin_q_kernel reads them (packed row order; wx slot 6 = the action's weight)
    const float *wt;               // (H + 32, 4H): rows u < H = whh^T, rows H + j = wx[:, j]^T (j < 8), then zeros
    const float *dq;               // (count) d(loss) / d(q) of this critic
    float *part;                   // (groups, critic_grad_part_floats(H)) partial sums
    float *stash;                  // (groups, bptt_stash_floats(H, W)) the current tile's activations
    float *da;                     // (count) this critic's d(loss) / d(action)
    // fe_critic_grad_reduce_kernel's outputs, packed row order (see include/finenvs_amd_critic_grad.h); all null: the
    // critic's weights are frozen, it contributes to the action's gradient only
    float *g_wih, *g_whh, *g_bih, *g_bhh, *g_wout, *g_bout;
};

struct CriticGradArgs {
    const float *lr32;
    const int64_t *obs_src;
    const double *obs_pos;
    const float *actions;
    int64_t count, num_tiles, groups;
    int32_t W, ncrit;   // ncrit: the critics that run (net[0 .. ncrit-1]; a critic without dq is left out)
    float *d_actions;   // (count) or null: da of net[0] (+ net[1])
    CriticGradNet net[2];
};

// wt of every running critic from its packed whh / wx (one thread per element)
__global__ __launch_bounds__(kBlock) void fe_critic_grad_pack_kernel(const CriticGradArgs g, int32_t H, float *wt0, float *wt1) {
    const CriticGradNet &c = g.net[blockIdx.y];
    float *wt = blockIdx.y == 0 ? wt0 : wt1;
    const int64_t n = critic_grad_wt_floats(H), G4 = 4 * H;
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int64_t row = i / G4, R = i - row * G4;
        wt[i] = row < H ? c.whh[R * H + row] : (row < H + 8 ? c.wx[R * 8 + (row - H)] : 0.0f);
    }
}

template <int NT>
__global__ __launch_bounds__(kCriticGradBlock) void fe_critic_grad_kernel(const CriticGradArgs g) {
    constexpr int H = 32 * NT, MPW = H / 32, G4 = 4 * H;
    constexpr int HPF = H + 4, G4P = G4 + 4, HX = H + 36, NTO = H / 32 + 1;
    extern __shared__ __align__(16) unsigned char smem[];
    const CriticGradNet &c = g.net[blockIdx.y];
    const int W = g.W;
    float *s_x = reinterpret_cast<float *>(smem);  // h double buffer [2][32][HPF] (forward), dz [32][G4P] (backward)
    constexpr int XF = (2 * 32 * HPF > 32 * G4P ? 2 * 32 * HPF : 32 * G4P);
    float *s_dhx = s_x + XF;                 // [32][HX]: dh_t (units) | dx_t (8 input slots) | 0
    float *s_wout = s_dhx + 32 * HX;         // [H]
    float *s_dq = s_wout + H;                // [32]
    float4 *s_xh = reinterpret_cast<float4 *>(s_dq + 32);  // [32] (pos, 1, action, 0)
    int64_t *s_src = reinterpret_cast<int64_t *>(s_xh + 32);  // [32]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
    float *part = c.part + blockIdx.x * critic_grad_part_floats(H);
    float *stash = c.stash + blockIdx.x * bptt_stash_floats(H, W);
    float *vst = stash + (int64_t)W * 160 * H;  // [W][32][VN]: [h_{t-1} | x_t | 0] per pair
    for (int i = tid; i < H; i += kCriticGradBlock) s_wout[i] = c.wout[i];

    for (int64_t tile = blockIdx.x; tile < g.num_tiles; tile += gridDim.x) {
        const bool first = tile == (int64_t)blockIdx.x;  // the partials are written, then added to
        const int64_t n0 = tile * 32;
        const int pairs = g.count - n0 < 32 ? (int)(g.count - n0) : 32;
        if (tid < 32) {  // a pair past the batch computes on the last one's descriptor (as the forward) with dq = 0
            const int64_t n = n0 + (tid < pairs ? tid : pairs - 1);
            s_src[tid] = g.obs_src[n];
            s_xh[tid] = make_float4((float)g.obs_pos[n], 1.0f, g.actions[n], 0.0f);
            s_dq[tid] = tid < pairs ? c.dq[n0 + tid] : 0.0f;
        }
        __syncthreads();
        bptt_stash_inputs<H, true>(vst, g.lr32, s_src, s_xh, W, tid);

        // ---- forward: fe_twin_q_kernel's recurrence, the activations into the stash ----
        float cst[MPW][4];
#pragma unroll
        for (int i = 0; i < MPW; ++i)
#pragma unroll
            for (int b = 0; b < 4; ++b) cst[i][b] = 0.0f;
        const float *xsrc = g.lr32 + s_src[col];
        const float4 xhc = s_xh[col];
        for (int t = 0; t < W; ++t) {
            bptt_forward_step<H>(t, W, c.whh, c.wx, xsrc, xhc, s_x, stash, vst, cst, wave, lane, col, half);
            __syncthreads();  // h_t is complete
        }

        // ---- the head: q = w_out . h_W + b_out ----
        const float *hW = s_x + ((W - 1) & 1) * 32 * HPF;
        for (int u = tid; c.g_whh && u <= H; u += kCriticGradBlock) {
            float s = 0.0f;
            for (int p = 0; p < 32; ++p) s = fmaf(s_dq[p], u < H ? hW[p * HPF + u] : 1.0f, s);
            part[4 * H * (H + 32) + u] = first ? s : part[4 * H * (H + 32) + u] + s;
        }
        for (int i = tid; i < 32 * H; i += kCriticGradBlock) s_dhx[(i / H) * HX + i % H] = s_dq[i / H] * s_wout[i % H];
        __syncthreads();  // dh_W is complete; h_W is read (its buffer becomes dz)

        // ---- backward through time ----
        float dc[MPW][4];
#pragma unroll
        for (int i = 0; i < MPW; ++i)
#pragma unroll
            for (int b = 0; b < 4; ++b) dc[i][b] = 0.0f;
        float da = 0.0f;
        for (int t = W - 1; t >= 0; --t) {
            bptt_dz_step<H, HX>(t, s_dhx, s_x, stash, dc, wave, lane, col, half);
            __syncthreads();  // dz_t is complete; dh_t and the gates of step t are read
            bptt_dz_to_stash<H>(t, s_x, stash, tid);
            // [dh_{t-1} | dx_t] = wt . dz_t: output rows (units, then input slots) on M, pairs on N, k = R
            bptt_wt_contract<G4, G4P, HX>(c.wt, s_x, s_dhx, NTO, wave, col, half);
            __syncthreads();  // dh_{t-1} and dx_t are complete; dz_t is read
            if (tid < 32) da += s_dhx[tid * HX + H + 6];
        }
        if (tid < pairs) c.da[n0 + tid] = da;

        // ---- weight gradients (none for a critic whose weights are frozen) ----
        if (c.g_whh) bptt_weight_grads<H>(stash, vst, part, W, first, wave, lane, col, half);
        __syncthreads();  // the stash and LDS are free for the next tile
    }
}

// The partials of every workgroup summed in workgroup order, written in packed row order; blockIdx.y = ncrit: the
// action gradient, critic 1's plus critic 2's.
__global__ __launch_bounds__(kBlock) void fe_critic_grad_reduce_kernel(const CriticGradArgs g, int32_t H) {
    const int64_t stride = (int64_t)gridDim.x * kBlock, i0 = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    if ((int)blockIdx.y == g.ncrit) {
        if (!g.d_actions) return;
        for (int64_t i = i0; i < g.count; i += stride)
            g.d_actions[i] = g.ncrit == 2 ? g.net[0].da[i] + g.net[1].da[i] : g.net[0].da[i];
        return;
    }
    const CriticGradNet &c = g.net[blockIdx.y];
    if (!c.g_whh) return;
    const int64_t PF = critic_grad_part_floats(H), VN = H + 32, NTO = H / 32 + 1, E = 4LL * H * VN + H + 1;
    for (int64_t e = i0; e < E; e += stride) {
        int64_t f = e, R = 0, n = 0;
        if (e < 4LL * H * VN) {
            R = e / VN;
            n = e - R * VN;
            const int64_t mt = R >> 5, rr = R & 31, r = 4 * (rr >> 3) + (rr & 3), hh = (rr >> 2) & 1;
            f = ((mt * NTO + (n >> 5)) * 16 + r) * 64 + (n & 31) + 32 * hh;
            if (n >= H + 7) continue;
        }
        float s = 0.0f;
        for (int64_t k = 0; k < g.groups; ++k) s += c.part[k * PF + f];
        if (e >= 4LL * H * VN) {
            const int64_t u = e - 4LL * H * VN;
            if (u < H) c.g_wout[u] = s;
            else *c.g_bout = s;
        } else if (n < H) {
            c.g_whh[R * H + n] = s;
        } else if (n - H < 5) {
            c.g_wih[R * 6 + (n - H)] = s;
        } else if (n - H == 5) {
            c.g_bih[R] = s;
            c.g_bhh[R] = s;
        } else {
            c.g_wih[R * 6 + 5] = s;
        }
    }
}

}  // namespace
