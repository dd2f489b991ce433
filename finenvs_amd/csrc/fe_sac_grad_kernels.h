// fe_sac_grad_kernels.h -- part of fe_env.hip (one translation unit; see the overview there): the backward pass of the
// SAC LSTM actor's head and recurrence on observation descriptors (include/finenvs_amd_sac_grad.h).
#pragma once
#include "fe_bptt_tile.h"

namespace {

// ---- d(loss) / d(parameters) of ActorLSTM((5, H, 1), W) (SAC/actor.py:44-61, networks/lstm.py:28-57) ----
// The tile of fe_bptt_tile.h with the SAC head and a 5-wide input:
//   forward   after the recurrence, z = W_l h_W + b_l as the forward's head forms it (fragment-major W_l on the matrix
//             cores);
//   head      in-lane, one lane per pair, from the forward's own a = actions[n] and s = stds[n]:
//               du  = ga (1 - a^2) + gl 2 a (1 - a^2) / (1 - a^2 + 1e-7)        (ga = d actions, gl = d log_probs)
//               dmu = du,   ds = du eps - gl / s                 (the Normal's (u - mu) terms cancel analytically)
//               dq  = ds sigmoid(q), q = w_std . z + b_std recomputed (1 where q > 20: F.softplus's threshold)
//               dz  = w_mu dmu + w_std dq
//             the head's sums over the tile (d w_mu, d w_std, d b_mu, d b_std, d b_l) per unit in-lane; d W_l = dz h_W^T
//             and dh_W = W_l^T dz on the matrix cores (W_l^T from fe_sac_grad_pack_kernel, read through L2);
//   backward  dh_{t-1} = W_hh^T dz_t only: the actor's input has no learnt column, so dx_t is never formed.
// fe_sac_grad_reduce_kernel writes the sums in torch's row order and layout (the inverse of lstm_row_order applied while
// writing).
constexpr int kSacGradBlock = kBpttBlock;

// the resident workgroup count of fe_sac_grad_kernel on an MI355X (256 CUs; at H = 128 the LDS admits one per CU)
__host__ __device__ constexpr int64_t sac_grad_max_groups(int H) { return H == 128 ? 256 : 512; }
// [4H x (H + 32) LSTM tiles][H x H last layer tiles][d w_mu (H) | d w_std (H) | d b_l (H) | d b_mu | d b_std | pad]
__host__ __device__ constexpr int64_t sac_grad_part_floats(int H) { return 4LL * H * (H + 32) + (int64_t)H * H + 3 * H + 32; }
// W_hh^T (H, 4H), then W_l^T (H, H)
__host__ __device__ constexpr int64_t sac_grad_wt_floats(int H) { return 5LL * H * H; }
// LDS of one workgroup: 22 912 B at H = 32, 43 776 B at 64, 85 504 B at 128 (one workgroup per CU there)
__host__ __device__ inline size_t sac_grad_lds_bytes(int H) {
    // dz [32][4H + 4] (holds the h double buffer, z and the head's dz before) | dh [32][H + 4] | w_mu, w_std, b_l |
    // dmu, dq [32] each | (pos, 1, 0, 0) [32] | src [32]
    return (32 * (size_t)(4 * H + 4) + 32 * (size_t)(H + 4) + 3 * (size_t)H + 64 + 32 * 4) * 4 + 32 * 8;
}

struct SacGradArgs {
    const float *lr32;
    const int64_t *obs_src;
    const double *obs_pos;
    const float *whh, *wx, *wl, *bl, *wmu, *wstd;  // as fe_sac_forward reads them
    float bstd;
    const float *noise, *actions, *stds;           // (count): eps, and what fe_sac_forward returned
    const float *d_actions, *d_log_probs;          // (count) upstream gradients, either may be null
    float *wt;     // (H, 4H) W_hh^T in packed gate-row order, then (H, H) W_l^T (row = input unit)
    float *part;   // (groups, sac_grad_part_floats(H))
    float *stash;  // (groups, bptt_stash_floats(H, W))
    int64_t count, num_tiles, groups;
    int32_t W;
    // fe_sac_grad_reduce_kernel's outputs, torch row order and layout (include/finenvs_amd_sac_grad.h)
    float *g_wih, *g_whh, *g_bih, *g_bhh, *g_wl, *g_bl, *g_wmu, *g_bmu, *g_wstd, *g_bstd;
    const float *bstd_p;  // (1) on the device, or null: read instead of bstd (fe_sac_backward_p)
};

// W_hh^T and W_l^T from the packed whh and the fragment-major wl (one thread per element)
__global__ __launch_bounds__(kBlock) void fe_sac_grad_pack_kernel(const SacGradArgs g, int32_t H) {
    const int64_t G4 = 4 * H, n1 = G4 * H, n = sac_grad_wt_floats(H), NG = H / 8;
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        if (i < n1) {
            const int64_t u = i / G4, R = i - u * G4;
            g.wt[i] = g.whh[R * H + u];
        } else {
            const int64_t j = i - n1, in = j / H, o = j - in * H;  // W_l[o][in]
            g.wt[i] = g.wl[((((o >> 5) * NG + (in >> 3)) * 64) + (o & 31) + 32 * ((in >> 2) & 1)) * 4 + (in & 3)];
        }
    }
}

template <int NT>
__global__ __launch_bounds__(kSacGradBlock) void fe_sac_grad_kernel(const SacGradArgs g) {
    constexpr int H = 32 * NT, MT = H / 8, MPW = H / 32, NG = H / 8, G4 = 4 * H, ZT = H / 32;
    constexpr int HPF = H + 4, G4P = G4 + 4, NTO = H / 32 + 1, VN = H + 32;
    constexpr int PL = 4 * H * VN, PV = PL + H * H;  // the last layer's tiles / the head's vectors in the partials
    static_assert(3 * 32 * HPF <= 32 * G4P, "h double buffer, z and the head's dz share the dz buffer");
    extern __shared__ __align__(16) unsigned char smem[];
    const int W = g.W;
    float *s_x = reinterpret_cast<float *>(smem);  // h double buffer [2][32][HPF] + head dz [32][HPF]; dz_t [32][G4P]
    float *s_dzh = s_x + 2 * 32 * HPF;       // [32][HPF]: the head's dz (d loss / d z)
    float *s_dh = s_x + 32 * G4P;            // [32][HPF]: dh_t
    float *s_wmu = s_dh + 32 * HPF;          // [H], then w_std [H], b_l [H]
    float *s_wstd = s_wmu + H, *s_bl = s_wmu + 2 * H;
    float *s_dmu = s_wmu + 3 * H;            // [32], then dq [32]
    float *s_dq = s_dmu + 32;
    float4 *s_xh = reinterpret_cast<float4 *>(s_dq + 32);     // [32] (pos, 1, 0, 0)
    int64_t *s_src = reinterpret_cast<int64_t *>(s_xh + 32);  // [32]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
    float *part = g.part + blockIdx.x * sac_grad_part_floats(H);
    float *stash = g.stash + blockIdx.x * bptt_stash_floats(H, W);
    float *vst = stash + (int64_t)W * 160 * H;  // [W][32][VN]: [h_{t-1} | x_t | 0] per pair
    const float *wlt = g.wt + (size_t)G4 * H;
    for (int i = tid; i < H; i += kSacGradBlock) {
        s_wmu[i] = g.wmu[i];
        s_wstd[i] = g.wstd[i];
        s_bl[i] = g.bl[i];
    }

    for (int64_t tile = blockIdx.x; tile < g.num_tiles; tile += gridDim.x) {
        const bool first = tile == (int64_t)blockIdx.x;  // the partials are written, then added to
        const int64_t n0 = tile * 32;
        const int pairs = g.count - n0 < 32 ? (int)(g.count - n0) : 32;
        float ga = 0.0f, gl = 0.0f, av = 0.0f, sv = 1.0f, ev = 0.0f;  // the head's per-pair inputs (tid < 32)
        if (tid < 32) {  // a pair past the batch computes on the last one's descriptor with zero upstream gradients
            const int64_t n = n0 + (tid < pairs ? tid : pairs - 1);
            s_src[tid] = g.obs_src[n];
            s_xh[tid] = make_float4((float)g.obs_pos[n], 1.0f, 0.0f, 0.0f);
            av = g.actions[n];
            sv = g.stds[n];
            ev = g.noise[n];
            if (tid < pairs) {
                ga = g.d_actions ? g.d_actions[n] : 0.0f;
                gl = g.d_log_probs ? g.d_log_probs[n] : 0.0f;
            }
        }
        __syncthreads();
        bptt_stash_inputs<H, false>(vst, g.lr32, s_src, s_xh, W, tid);

        // ---- forward: fe_sac_forward's recurrence, the activations into the stash ----
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

        // ---- the head's forward: z = W_l h_W + b_l into the idle h buffer (fe_lstm_rollout_body.h, FE_LSTM_SAC_HEAD) ----
        const float *hW = s_x + ((W - 1) & 1) * 32 * HPF;
        float *zb = s_x + (W & 1) * 32 * HPF;
        if (wave < ZT) {
            const float4 *wf = reinterpret_cast<const float4 *>(g.wl) + (size_t)wave * NG * 64 + lane;
            const float *hrow = hW + col * HPF + 4 * half;
            f32x16 acc;
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) acc[rr] = 0.0f;
#pragma unroll 2
            for (int gg = 0; gg < NG; ++gg) {
                const float4 wv = wf[(size_t)gg * 64];
                const float4 hb = *reinterpret_cast<const float4 *>(hrow + 8 * gg);
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const float ws = m == 0 ? wv.x : (m == 1 ? wv.y : (m == 2 ? wv.z : wv.w));
                    const float hs = m == 0 ? hb.x : (m == 1 ? hb.y : (m == 2 ? hb.z : hb.w));
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ws, hs, acc, 0, 0, 0);
                }
            }
#pragma unroll
            for (int b = 0; b < 4; ++b) {  // acc[4b + c] is unit 32 wave + 8 b + 4 half + c of pair col
                const int u0 = 32 * wave + 8 * b + 4 * half;
                *reinterpret_cast<float4 *>(zb + col * HPF + u0) =
                    make_float4(acc[4 * b] + s_bl[u0], acc[4 * b + 1] + s_bl[u0 + 1], acc[4 * b + 2] + s_bl[u0 + 2],
                                acc[4 * b + 3] + s_bl[u0 + 3]);
            }
        }
        __syncthreads();  // z is complete

        // ---- the head's backward, one lane per pair (SAC/actor.py:51-61 differentiated) ----
        if (tid < 32) {
            const float *zr = zb + tid * HPF;
            float q = g.bstd_p ? *g.bstd_p : g.bstd;
#pragma unroll 4
            for (int u = 0; u < H; ++u) q = fmaf(s_wstd[u], zr[u], q);
            const float om = 1.0f - av * av;
            const float du = ga * om + gl * (2.0f * av * om / (om + 1e-7f));
            const float ds = du * ev - gl / sv;
            const float sg = q > 20.0f ? 1.0f : 1.0f / (1.0f + expf(-q));  // d softplus (beta 1, threshold 20)
            s_dmu[tid] = du;
            s_dq[tid] = ds * sg;
        }
        __syncthreads();  // dmu, dq are complete
        for (int i = tid; i < 32 * H; i += kSacGradBlock) {
            const int p = i / H, u = i - p * H;
            s_dzh[p * HPF + u] = s_wmu[u] * s_dmu[p] + s_wstd[u] * s_dq[p];
        }
        for (int u = tid; u <= H; u += kSacGradBlock) {  // d w_mu, d w_std, d b_l of unit u; u = H: d b_mu, d b_std
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
            for (int p = 0; p < 32; ++p) {
                const float zv = u < H ? zb[p * HPF + u] : 1.0f;
                a0 = fmaf(zv, s_dmu[p], a0);
                a1 = fmaf(zv, s_dq[p], a1);
                if (u < H) a2 += s_wmu[u] * s_dmu[p] + s_wstd[u] * s_dq[p];
            }
            float *pv = part + PV;
            if (u < H) {
                pv[u] = first ? a0 : pv[u] + a0;
                pv[H + u] = first ? a1 : pv[H + u] + a1;
                pv[2 * H + u] = first ? a2 : pv[2 * H + u] + a2;
            } else {
                pv[3 * H] = first ? a0 : pv[3 * H] + a0;
                pv[3 * H + 1] = first ? a1 : pv[3 * H + 1] + a1;
            }
        }
        __syncthreads();  // the head's dz is complete
        // d W_l += dz h_W^T (rows = output units on M, input units on N, k = the 32 pairs)
        for (int ot = wave; ot < ZT * ZT; ot += 4) {
            const int mt = ot / ZT, nt = ot - mt * ZT;
            const float *za = s_dzh + 32 * mt + col, *hb = hW + 32 * nt + col;
            f32x16 acc;
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) acc[rr] = 0.0f;
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) {
                const int p = 2 * kk + half;
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(za[p * HPF], hb[p * HPF], acc, 0, 0, 0);
            }
            float *pt = part + PL + ot * 1024 + lane;
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) pt[rr * 64] = first ? acc[rr] : pt[rr * 64] + acc[rr];
        }
        // dh_W = W_l^T dz: input units on M, pairs on N, k = output units
        bptt_wt_contract<H, HPF, HPF>(wlt, s_dzh, s_dh, ZT, wave, col, half);
        __syncthreads();  // dh_W is complete; h_W, z and the head's dz are read (their buffer becomes dz_t)

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
        // bptt_weight_grads (fe_bptt_tile.h) written out, statement for statement: called from the header it raised
        // this kernel's VGPRs at H = 64 to within one register of losing the second wave (NOTES.md, 2026-10-18)
        for (int ot = wave; ot < MT * NTO; ot += 4) {
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

// The partials of every workgroup summed in workgroup order, written in torch's row order: packed gate row
// R = 32 mt + 8 b + 4 half + gate is row gate H + 8 mt + 4 half + b of the 4H-row tensors (lstm_row_order's inverse).
__global__ __launch_bounds__(kBlock) void fe_sac_grad_reduce_kernel(const SacGradArgs g, int32_t H) {
    const int64_t stride = (int64_t)gridDim.x * kBlock, i0 = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    const int64_t PF = sac_grad_part_floats(H), VN = H + 32, NTO = H / 32 + 1, ZT = H / 32;
    const int64_t PL = 4LL * H * VN, PV = PL + (int64_t)H * H, E = PV + 3 * H + 2;
    for (int64_t e = i0; e < E; e += stride) {
        int64_t f = e, R = 0, n = 0;
        if (e < PV) {  // an element of a 32 x 32 accumulator tile: row R, column n of its matrix
            const bool lstm = e < PL;
            const int64_t k = lstm ? e : e - PL, cols = lstm ? VN : H;
            R = k / cols;
            n = k - R * cols;
            if (lstm && n >= H + 6) continue;  // the input tile's unused columns
            const int64_t mt = R >> 5, rr = R & 31, r = 4 * (rr >> 3) + (rr & 3), hh = (rr >> 2) & 1;
            f = (lstm ? 0 : PL) + ((mt * (lstm ? NTO : ZT) + (n >> 5)) * 16 + r) * 64 + (n & 31) + 32 * hh;
        }
        float s = 0.0f;
        for (int64_t k = 0; k < g.groups; ++k) s += g.part[k * PF + f];
        if (e < PL) {
            const int64_t rho = R & 31, row = (rho & 3) * H + 8 * (R >> 5) + 4 * ((rho >> 2) & 1) + (rho >> 3);
            if (n < H) {
                g.g_whh[row * H + n] = s;
            } else if (n - H < 5) {
                g.g_wih[row * 5 + (n - H)] = s;
            } else {
                g.g_bih[row] = s;
                g.g_bhh[row] = s;
            }
        } else if (e < PV) {
            g.g_wl[R * H + n] = s;
        } else {
            const int64_t u = e - PV;
            if (u < H) g.g_wmu[u] = s;
            else if (u < 2 * H) g.g_wstd[u - H] = s;
            else if (u < 3 * H) g.g_bl[u - 2 * H] = s;
            else if (u == 3 * H) *g.g_bmu = s;
            else *g.g_bstd = s;
        }
    }
}

}  // namespace
