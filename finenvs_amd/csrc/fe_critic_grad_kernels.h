// fe_critic_grad_kernels.h -- part of fe_env.hip (one translation unit; see the overview there): the backward pass
// through time of the twin LSTM critics on observation descriptors (include/finenvs_amd_critic_grad.h).
#pragma once
#include "fe_device_common.h"
#include "fe_lstm_kernel.h"

namespace {

// ---- d(loss) / d(parameters, action) of CriticLSTM((6, H, 1), W) (SAC/critic.py:30-45, TD3/critic.py:31-46) ----
// One workgroup (4 wavefronts) runs one critic (blockIdx.y) over grid-strided 32-pair tiles.  Per tile:
//   forward   the recurrence of fe_twin_q_kernel recomputed with the SAME contraction: gate rows R (packed order) on
//             the M side of v_mfma_f32_32x32x2_f32, the 32 pairs on the N side, k order x (m = 0..3) then h (g, m),
//             the same activations and cell update -- so h_t, c_t are fe_twin_q_forward's bit for bit.  Wavefront w
//             owns gate-row tiles w, w + 4, ...; c stays in its registers; the activated gates and c_t go to the
//             workgroup's stash, h_t to LDS (next step's B operand) and to the stash (the weight gradient's B operand);
//   backward  t = W-1 .. 0, in-lane (the lane that computed a unit's gates holds them): dz_t = the four gate
//             pre-activation gradients from dh_t and the carried dc; dz_t goes to LDS as [pair][R] and to the stash
//             slot of step t (over the gates, after a barrier); then [dh_{t-1} | dx_t] = [W_hh | W_x]^T dz_t on the
//             matrix cores, A = the transposed weights (fe_critic_grad_pack_kernel), B = dz_t from LDS;
//   weights   [dW_hh | dW_x] += sum over (t, pair) of dz_t [h_{t-1} | x_t]^T, K = 32 W, A = dz_t, B = [h | x] from the
//             stash, one 32 x 32 output tile per wavefront at a time, added to the workgroup's partial sums.
// The partials (one set per workgroup, the grid bounded by the resident workgroup count) are summed in a fixed order by
// fe_critic_grad_reduce_kernel: no float atomics, the same inputs give the same bits.  The action's gradient of a pair
// is row 6 of dx summed over t (one lane per pair), per critic; the reduction adds the two critics'.
constexpr int kCriticGradBlock = 256;

// partial sums per critic: the resident workgroup count of fe_critic_grad_kernel on an MI355X (256 CUs; at H = 128
// the LDS admits one workgroup per CU, so 128 per critic half of the grid)
__host__ __device__ constexpr int64_t critic_grad_max_groups(int H) { return H == 128 ? 128 : 256; }
__host__ __device__ constexpr int64_t critic_grad_part_floats(int H) { return 4LL * H * (H + 32) + H + 32; }
__host__ __device__ constexpr int64_t critic_grad_stash_floats(int H, int W) {
    return (int64_t)W * (160LL * H + 32LL * (H + 32));
}
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
    float *stash;                  // (groups, critic_grad_stash_floats(H, W)) the current tile's activations
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
    constexpr int H = 32 * NT, MT = H / 8, MPW = MT / 4, NG = H / 8, G4 = 4 * H;
    constexpr int HPF = H + 4, G4P = G4 + 4, HX = H + 36, NTO = H / 32 + 1, VN = H + 32;
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
    float *stash = c.stash + blockIdx.x * critic_grad_stash_floats(H, W);
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
        for (int i = tid; i < W * 32 * 32; i += kCriticGradBlock) {  // x_t and h_{-1} = 0 into the stash
            const int t = i >> 10, p = (i >> 5) & 31, j = i & 31;
            const float4 xh = s_xh[p];
            float v = j < 4 ? g.lr32[s_src[p] + 4 * t + j] : (j == 4 ? xh.x : (j == 5 ? 1.0f : (j == 6 ? xh.z : 0.0f)));
            vst[((int64_t)t * 32 + p) * VN + H + j] = v;
        }
        for (int i = tid; i < 32 * H; i += kCriticGradBlock) vst[(i / H) * VN + i % H] = 0.0f;

        // ---- forward: fe_twin_q_kernel's recurrence, the activations into the stash ----
        float cst[MPW][4];
#pragma unroll
        for (int i = 0; i < MPW; ++i)
#pragma unroll
            for (int b = 0; b < 4; ++b) cst[i][b] = 0.0f;
        const float *xsrc = g.lr32 + s_src[col];
        const float4 xhc = s_xh[col];
        for (int t = 0; t < W; ++t) {
            const float *hprev = s_x + ((t + 1) & 1) * 32 * HPF;
            float *hnext = s_x + (t & 1) * 32 * HPF;
            float *slot = stash + (int64_t)t * 160 * H;
            const float4 xc = half == 0 ? *reinterpret_cast<const float4 *>(xsrc + 4 * t) : xhc;
#pragma unroll
            for (int i = 0; i < MPW; ++i) {
                const int mt = wave + 4 * i;
                const size_t R = (size_t)32 * mt + col;
                const float4 wxv = *reinterpret_cast<const float4 *>(c.wx + R * 8 + 4 * half);
                f32x16 acc;
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) acc[rr] = 0.0f;
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const float xs = m == 0 ? xc.x : (m == 1 ? xc.y : (m == 2 ? xc.z : xc.w));
                    const float ws = m == 0 ? wxv.x : (m == 1 ? wxv.y : (m == 2 ? wxv.z : wxv.w));
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ws, xs, acc, 0, 0, 0);
                }
                if (t > 0) {
#pragma unroll 4
                    for (int gg = 0; gg < NG; ++gg) {
                        const float4 wv = *reinterpret_cast<const float4 *>(c.whh + R * H + 8 * gg + 4 * half);
                        const float4 hb = *reinterpret_cast<const float4 *>(hprev + col * HPF + 8 * gg + 4 * half);
#pragma unroll
                        for (int m = 0; m < 4; ++m) {
                            const float ws = m == 0 ? wv.x : (m == 1 ? wv.y : (m == 2 ? wv.z : wv.w));
                            const float hs = m == 0 ? hb.x : (m == 1 ? hb.y : (m == 2 ? hb.z : hb.w));
                            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ws, hs, acc, 0, 0, 0);
                        }
                    }
                }
                // the cell update of fe_lstm_rollout_body.h: acc[4b + gate] is unit 8 mt + 4 half + b of pair col
                float hv[4], og[4];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const v2f sif = lstm_act2<false, false>((v2f){acc[4 * b + 0], acc[4 * b + 1]});
                    const v2f tgo = lstm_act2<true, false>((v2f){acc[4 * b + 2], acc[4 * b + 3]});
                    const float t1 = sif.y * cst[i][b];
                    const float t2 = sif.x * tgo.x;
                    cst[i][b] = t1 + t2;
                    og[b] = tgo.y;
                    float *gs = slot + (mt * 16 + 4 * b) * 64 + lane;
                    gs[0] = sif.x;
                    gs[64] = sif.y;
                    gs[128] = tgo.x;
                    gs[192] = tgo.y;
                    slot[128 * H + (mt * 4 + b) * 64 + lane] = cst[i][b];
                }
#pragma unroll
                for (int b = 0; b < 4; b += 2) {
                    const v2f tc = lstm_act2<true, true>((v2f){cst[i][b], cst[i][b + 1]});
                    hv[b] = og[b] * tc.x;
                    hv[b + 1] = og[b + 1] * tc.y;
                }
                const float4 h4 = make_float4(hv[0], hv[1], hv[2], hv[3]);
                *reinterpret_cast<float4 *>(hnext + col * HPF + 8 * mt + 4 * half) = h4;
                if (t + 1 < W) *reinterpret_cast<float4 *>(vst + ((int64_t)(t + 1) * 32 + col) * VN + 8 * mt + 4 * half) = h4;
            }
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
            float *slot = stash + (int64_t)t * 160 * H;
            const float *pslot = stash + (int64_t)(t - 1) * 160 * H;
#pragma unroll
            for (int i = 0; i < MPW; ++i) {
                const int mt = wave + 4 * i;
                const float4 dh4 = *reinterpret_cast<const float4 *>(s_dhx + col * HX + 8 * mt + 4 * half);
                const float dh[4] = {dh4.x, dh4.y, dh4.z, dh4.w};
                float cc[4], cp[4];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    cc[b] = slot[128 * H + (mt * 4 + b) * 64 + lane];
                    cp[b] = t > 0 ? pslot[128 * H + (mt * 4 + b) * 64 + lane] : 0.0f;
                }
#pragma unroll
                for (int b = 0; b < 4; b += 2) {
                    const v2f tc = lstm_act2<true, true>((v2f){cc[b], cc[b + 1]});
#pragma unroll
                    for (int bb = 0; bb < 2; ++bb) {
                        const int u = b + bb;
                        const float tcu = bb == 0 ? tc.x : tc.y;
                        const float *gs = slot + (mt * 16 + 4 * u) * 64 + lane;
                        const float ig = gs[0], fg = gs[64], gg = gs[128], og = gs[192];
                        const float dcc = dc[i][u] + dh[u] * og * (1.0f - tcu * tcu);
                        const float4 dz = make_float4(dcc * gg * ig * (1.0f - ig), dcc * cp[u] * fg * (1.0f - fg),
                                                      dcc * ig * (1.0f - gg * gg), dh[u] * tcu * og * (1.0f - og));
                        dc[i][u] = dcc * fg;
                        *reinterpret_cast<float4 *>(s_x + col * G4P + 32 * mt + 8 * u + 4 * half) = dz;
                    }
                }
            }
            __syncthreads();  // dz_t is complete; dh_t and the gates of step t are read
            for (int i = tid; i < 32 * G4 / 4; i += kCriticGradBlock) {  // dz_t to the stash, [pair][R], over the gates
                const int p = i / (G4 / 4), r4 = i - p * (G4 / 4);
                reinterpret_cast<float4 *>(slot)[i] = *reinterpret_cast<const float4 *>(s_x + p * G4P + 4 * r4);
            }
            // [dh_{t-1} | dx_t] = wt . dz_t: output rows (units, then input slots) on M, pairs on N, k = R
            for (int ut = wave; ut < NTO; ut += 4) {
                const float *wrow = c.wt + (size_t)(32 * ut + col) * G4 + 4 * half;
                const float *zrow = s_x + col * G4P + 4 * half;
                f32x16 acc;
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) acc[rr] = 0.0f;
#pragma unroll 4
                for (int gg = 0; gg < G4 / 8; ++gg) {
                    const float4 wv = *reinterpret_cast<const float4 *>(wrow + 8 * gg);
                    const float4 zb = *reinterpret_cast<const float4 *>(zrow + 8 * gg);
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        const float ws = m == 0 ? wv.x : (m == 1 ? wv.y : (m == 2 ? wv.z : wv.w));
                        const float zs = m == 0 ? zb.x : (m == 1 ? zb.y : (m == 2 ? zb.z : zb.w));
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ws, zs, acc, 0, 0, 0);
                    }
                }
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    *reinterpret_cast<float4 *>(s_dhx + col * HX + 32 * ut + 8 * b + 4 * half) =
                        make_float4(acc[4 * b], acc[4 * b + 1], acc[4 * b + 2], acc[4 * b + 3]);
            }
            __syncthreads();  // dh_{t-1} and dx_t are complete; dz_t is read
            if (tid < 32) da += s_dhx[tid * HX + H + 6];
        }
        if (tid < pairs) c.da[n0 + tid] = da;

        // ---- weight gradients: [dW_hh | dW_x] += dz [h | x]^T over the tile's 32 W (pair, step) columns ----
        for (int ot = wave; c.g_whh && ot < MT * NTO; ot += 4) {  // (none for a critic whose weights are frozen)
            const int mt = ot / NTO, nt = ot - mt * NTO;
            f32x16 acc;
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) acc[rr] = 0.0f;
            for (int t = 0; t < W; ++t) {
                const float *za = stash + (int64_t)t * 160 * H + 32 * mt + col;
                const float *vb = vst + (int64_t)t * 32 * VN + 32 * nt + col;
#pragma unroll
                for (int kk = 0; kk < 16; ++kk) {
                    const int p = 2 * kk + half;
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(za[p * G4], vb[p * VN], acc, 0, 0, 0);
                }
            }
            float *pt = part + ot * 1024 + lane;
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) pt[rr * 64] = first ? acc[rr] : pt[rr * 64] + acc[rr];
        }
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
