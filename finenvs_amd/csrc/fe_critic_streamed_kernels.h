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

template <int RTW, bool STASH>
__global__ __launch_bounds__(kLstmBlock, 2) void fe_critic_sgrad_forward_kernel(const CriticSGradArgs a) {
    constexpr int H = 64 * RTW, HP = H + 4, NG = H / 8, G4 = 4 * H, VN = H + 32;
    constexpr int RI = kLstmBigRI, AHEAD = kLstmBigAhead;
    static_assert(RTW % RI == 0 && (H / 8) % AHEAD == 0, "row tiles / k groups must come in whole groups");
    extern __shared__ __align__(16) unsigned char smem[];
    const LstmSGradArgs &g = a.g;
    int64_t *s_src = reinterpret_cast<int64_t *>(smem);      // [32]
    float *s_pos = reinterpret_cast<float *>(s_src + 32);    // [32]
    float *s_act = s_pos + 32;                               // [32]
    int *s_ok = reinterpret_cast<int *>(s_act + 32);         // [32] the ring index was in range
    float *s_h = s_act + 64;                                 // [32][HP]
    const int W = g.W;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
    const int mt0 = wave * RTW;  // this wavefront's row tiles: mt0 .. mt0 + RTW - 1
    const int64_t pp = g.pp, num_tiles = pp / 32;
    float4 wq[kLstmBigAhead][kLstmBigRI];  // weight fragments in flight (see the k loop)
    bool primed = false;

    for (int64_t tile = blockIdx.x; tile < num_tiles; tile += gridDim.x) {
        const int64_t n0 = tile * 32;
        const int pairs = g.cnt - n0 < 32 ? (int)(g.cnt - n0) : 32;
        if (tid < 32) {  // a pair past the batch computes on the last one's descriptor (its upstream gradient is zero)
            const int64_t n = n0 + (tid < pairs ? tid : pairs - 1);
            int64_t src;
            double pos;
            bool ok = true;
            if (a.indices) {  // an index outside [0, size) reads nothing of the ring: window offset 0, position 0
                int64_t slot, start = a.start, size = a.size;
                ring_window(a.cursor, a.ring_C, start, size);
                ok = ring_slot(a.indices[n], start, size, a.ring_C, slot);
                src = ok ? a.ring_src[slot] : 0;
                pos = ok ? a.ring_pos[slot] : 0.0;
            } else {
                src = g.obs_src[n];
                pos = g.obs_pos[n];
            }
            float act = a.actions[n];
            if (a.smooth_noise) {  // clamp(a + clamp(eps * std, -c, c), -1, 1), one f32 rounding per torch op
                const float dev = clamp_pm(__fmul_rn(a.smooth_noise[n], a.smooth_std), -a.smooth_clip, a.smooth_clip);
                act = clamp_pm(__fadd_rn(act, dev), -1.0f, 1.0f);
            }
            s_src[tid] = src;
            s_pos[tid] = (float)pos;
            s_act[tid] = act;
            s_ok[tid] = ok ? 1 : 0;
        }
        __syncthreads();
        if constexpr (STASH) {
            for (int i = tid; i < W * 32 * 32; i += kLstmBlock) {  // x_t into the stash
                const int t = i >> 10, p = (i >> 5) & 31, j = i & 31;
                const float v = j < 4 ? g.lr32[s_src[p] + 4 * t + j]
                                      : (j == 4 ? s_pos[p] : (j == 5 ? 1.0f : (j == 6 ? s_act[p] : 0.0f)));
                g.vst[((int64_t)t * pp + n0 + p) * VN + H + j] = v;
            }
            for (int i = tid; i < 32 * H; i += kLstmBlock) g.vst[(n0 + i / H) * VN + i % H] = 0.0f;  // h_{-1}
        }

        const float *xsrc = g.lr32 + s_src[col];
        const float4 xh = make_float4(s_pos[col], 1.0f, s_act[col], 0.0f);
        float4 xc = half == 0 ? *reinterpret_cast<const float4 *>(xsrc) : xh;
        float cst[RTW][4], hnew[RTW][4];
#pragma unroll
        for (int i = 0; i < RTW; ++i)
#pragma unroll
            for (int b = 0; b < 4; ++b) cst[i][b] = 0.0f;
        for (int t = 0; t < W; ++t) {
            const int tn = t + 1 < W ? t + 1 : t;
            const float4 xn = half == 0 ? *reinterpret_cast<const float4 *>(xsrc + 4 * tn) : xh;
            const float *hrow = s_h + (size_t)col * HP + 4 * half;
            const int64_t row = (int64_t)t * pp + n0 + col;  // this lane's (t, pair) row of the stash
            float *grow = nullptr, *crow = nullptr, *hout = nullptr;
            if constexpr (STASH) {
                grow = g.gates + row * G4 + 4 * half;
                crow = g.cst + row * H + 4 * half;
                // h_t is the h_{t-1} of step t + 1; the last one is h_W
                hout = (t + 1 < W ? g.vst + (row + pp) * VN : g.hw + (n0 + col) * (int64_t)H) + 4 * half;
            }
#pragma unroll 1
            for (int i0 = 0; i0 < RTW; i0 += RI) {
                f32x16 acc[RI];
#pragma unroll
                for (int i = 0; i < RI; ++i)
#pragma unroll
                    for (int rr = 0; rr < 16; ++rr) acc[i][rr] = 0.0f;
                // input part: four MFMAs per row tile
                float4 wxv[RI];
#pragma unroll
                for (int i = 0; i < RI; ++i)
                    wxv[i] = *reinterpret_cast<const float4 *>(g.wx + ((size_t)32 * (mt0 + i0 + i) + col) * 8 + 4 * half);
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int i = 0; i < RI; ++i) {
                        const float xs = m == 0 ? xc.x : (m == 1 ? xc.y : (m == 2 ? xc.z : xc.w));
                        const float ws = m == 0 ? wxv[i].x : (m == 1 ? wxv[i].y : (m == 2 ? wxv[i].z : wxv[i].w));
                        acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(ws, xs, acc[i], 0, 0, 0);
                    }
                if (t > 0) {
                    // fragment-major weights: one coalesced KiB per (row tile, k group), AHEAD groups in flight across row-tile
                    // groups, time steps and tiles (the matrix never changes)
                    const float4 *wbase = reinterpret_cast<const float4 *>(g.whh) + lane;
                    const float4 *wf[RI], *wfn[RI];
#pragma unroll
                    for (int i = 0; i < RI; ++i) {
                        wf[i] = wbase + ((size_t)(mt0 + i0 + i) * NG) * 64;
                        wfn[i] = wbase + ((size_t)(mt0 + (i0 + RI < RTW ? i0 + RI : 0) + i) * NG) * 64;
                    }
                    if (!primed) {
#pragma unroll
                        for (int d = 0; d < AHEAD; ++d)
#pragma unroll
                            for (int i = 0; i < RI; ++i) wq[d][i] = wf[i][(size_t)d * 64];
                        primed = true;
                    }
#pragma unroll 1  // a real loop: unrolled, its hoisted loads spill
                    for (int g0 = 0; g0 < NG; g0 += AHEAD) {
#pragma unroll
                        for (int d = 0; d < AHEAD; ++d) {
                            const int gg = g0 + d;
                            float4 wv[RI];
                            const int gn = gg + AHEAD;
#pragma unroll
                            for (int i = 0; i < RI; ++i) {
                                wv[i] = wq[d][i];
                                wq[d][i] = gn < NG ? wf[i][(size_t)gn * 64] : wfn[i][(size_t)(gn - NG) * 64];
                            }
                            const float4 hb = *reinterpret_cast<const float4 *>(hrow + 8 * gg);
#pragma unroll
                            for (int m = 0; m < 4; ++m) {
                                const float hs = m == 0 ? hb.x : (m == 1 ? hb.y : (m == 2 ? hb.z : hb.w));
#pragma unroll
                                for (int i = 0; i < RI; ++i) {
                                    const float ws = m == 0 ? wv[i].x : (m == 1 ? wv[i].y : (m == 2 ? wv[i].z : wv[i].w));
                                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(ws, hs, acc[i], 0, 0, 0);
                                }
                            }
                        }
                    }
                }
                // cell update, in-lane: acc[4b + gate] is unit 8 mt + 4 half + b of pair col.  STASH: the stash gets the gates,
                // c_t and h_t now; the LDS copy of h_t waits (in scratch) until everyone has read the old one
#pragma unroll
                for (int i = 0; i < RI; ++i) {
                    const int mt = mt0 + i0 + i;
                    float og[4];
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const v2f sif = lstm_act2<false, false>((v2f){acc[i][4 * b + 0], acc[i][4 * b + 1]});
                        const v2f tgo = lstm_act2<true, false>((v2f){acc[i][4 * b + 2], acc[i][4 * b + 3]});
                        const float t1 = sif.y * cst[i0 + i][b];
                        const float t2 = sif.x * tgo.x;
                        cst[i0 + i][b] = t1 + t2;
                        og[b] = tgo.y;
                        if constexpr (STASH)
                            *reinterpret_cast<float4 *>(grow + 32 * mt + 8 * b) = make_float4(sif.x, sif.y, tgo.x, tgo.y);
                    }
#pragma unroll
                    for (int b = 0; b < 4; b += 2) {
                        const v2f tc = lstm_act2<true, true>((v2f){cst[i0 + i][b], cst[i0 + i][b + 1]});
                        hnew[i0 + i][b] = og[b] * tc.x;
                        hnew[i0 + i][b + 1] = og[b + 1] * tc.y;
                    }
                    if constexpr (STASH) {
                        *reinterpret_cast<float4 *>(crow + 8 * mt) =
                            make_float4(cst[i0 + i][0], cst[i0 + i][1], cst[i0 + i][2], cst[i0 + i][3]);
                        *reinterpret_cast<float4 *>(hout + 8 * mt) =
                            make_float4(hnew[i0 + i][0], hnew[i0 + i][1], hnew[i0 + i][2], hnew[i0 + i][3]);
                    }
                }
            }
            lds_barrier();  // every wavefront has read h_{t-1}
#pragma unroll
            for (int i = 0; i < RTW; ++i)
                *reinterpret_cast<float4 *>(s_h + (size_t)col * HP + 8 * (mt0 + i) + 4 * half) =
                    make_float4(hnew[i][0], hnew[i][1], hnew[i][2], hnew[i][3]);
            xc = xn;
            lds_barrier();  // h_t is complete
        }
        if constexpr (!STASH) {
            // output layer: one lane per pair reduces its last hidden state, units ascending (fe_rollout_lstm_big_kernel's
            // chain); a ring index out of range gives NaN
            if (tid < pairs) {
                const float *hl = s_h + (size_t)tid * HP;
                float o = *a.bout;
#pragma unroll 8
                for (int u = 0; u < H; ++u) o = fmaf(g.wout[u], hl[u], o);
                a.q_out[n0 + tid] = s_ok[tid] ? o : __builtin_nanf("");
            }
        }
        __syncthreads();  // the descriptors and h are free for the next tile
    }
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

// fe_lstm_sgrad_final_kernel for the critic's six input columns: column n - H < 5 of a split sum is w_ih[row, n - H],
// column 5 the bias, column 6 (the action's slot) w_ih[row, 5]; the rest of the input tile is skipped.  Split sums in
// split order, head block sums in block order; the first chunk overwrites, a later one adds.
__global__ __launch_bounds__(kBlock) void fe_critic_sgrad_final_kernel(const LstmSGradArgs g, int32_t H) {
    const int64_t stride = (int64_t)gridDim.x * kBlock, i0 = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    const int64_t VN = H + 32, PV = lstm_sgrad_part_floats(H), E = PV + H + 1;
    const int64_t blocks = lstm_sgrad_head_blocks(g.pp);
    const bool first = g.first != 0;
    for (int64_t e = i0; e < E; e += stride) {
        float s = 0.0f;
        if (e < PV) {
            const int64_t R = e / VN, n = e - R * VN;
            if (n >= H + 7) continue;  // the input tile's unused columns
            for (int64_t k = 0; k < g.splits; ++k) s += g.part[k * PV + e];
            const int64_t rho = R & 31, row = (rho & 3) * H + 8 * (R >> 5) + 4 * ((rho >> 2) & 1) + (rho >> 3);
            if (n < H) {
                float *o = g.g_whh + row * H + n;
                *o = first ? s : *o + s;
            } else if (n - H != 5) {
                float *o = g.g_wih + row * 6 + (n - H < 5 ? n - H : 5);
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

}  // namespace
