// fe_bptt_tile.h -- part of fe_env.hip (one translation unit; see the overview there): the stages of one 32-pair
// backward-through-time tile that fe_lstm_grad_kernel, fe_critic_grad_kernel and fe_sac_grad_kernel share.
#pragma once
#include "fe_device_common.h"
#include "fe_lstm_kernel.h"

namespace {

// One workgroup (kBpttBlock threads, 4 wavefronts) runs grid-strided 32-pair tiles.  Per tile, in the order the kernels
// call the stages (every __syncthreads() is the kernel's own, between the calls):
//   inputs    bptt_stash_inputs: x_t = (4 log-returns, position, 1 for the bias, slot 6, 0 ...) of every step and
//             h_{-1} = 0 into the stash's [h_{t-1} | x_t] rows (the weight gradient's B operand);
//   forward   bptt_forward_step: the recurrence of the acting kernel recomputed with the SAME contraction: gate rows R
//             (packed order) on the M side of v_mfma_f32_32x32x2_f32, the 32 pairs on the N side, k order x (m = 0..3)
//             then h (g, m), lstm_act2 and the same cell update -- so h_t, c_t are the forward's bit for bit.
//             Wavefront w owns gate-row tiles w, w + 4, ...; c stays in its registers; the activated gates and c_t go
//             to the workgroup's stash, h_t to LDS (next step's B operand) and to the stash;
//   (head)    the kernel's own: dh_W into LDS, the head's sums into the partials;
//   backward  t = W-1 .. 0.  bptt_dz_step, in-lane (the lane that computed a unit's gates holds them): dz_t = the four
//             gate pre-activation gradients from dh_t and the carried dc, to LDS as [pair][R]; after a barrier
//             bptt_dz_to_stash copies dz_t over the gates of step t, and bptt_wt_contract forms dh_{t-1} (the critic:
//             [dh_{t-1} | dx_t]) = W^T dz_t on the matrix cores, A = the transposed weights from the kernel's pack
//             kernel (read through L2), B = dz_t from LDS;
//   weights   bptt_weight_grads: [dW_hh | dW_x] += sum over (t, pair) of dz_t [h_{t-1} | x_t]^T, K = 32 W, A = dz_t,
//             B = [h | x] from the stash, one 32 x 32 output tile per wavefront at a time, written to (first tile) or
//             added to the workgroup's partial sums.
// Every workgroup writes its own partials; the kernel's reduce kernel adds them in workgroup order: no float atomics,
// the same inputs give the same bits.
// LDS: s_x holds the h double buffer [2][32][H + 4] in the forward and dz_t [32][4H + 4] in the backward.
// In every stage: lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5.
constexpr int kBpttBlock = 256;

// The stash of one workgroup: per step, activated gates (128 H; dz_t over them in the backward) and c_t (32 H) in
// fragment order, then [W][32][H + 32]: [h_{t-1} | x_t | 0] per pair.
__host__ __device__ constexpr int64_t bptt_stash_floats(int H, int W) {
    return (int64_t)W * (160LL * H + 32LL * (H + 32));
}

// x_t and h_{-1} = 0 into the stash.  s_xh[p] = (position, 1, slot 6, 0).  SLOT6: x_t's slot 6 is s_xh[p].z (the critic's
// action); without it the slot is 0 and only .x is read (the two actors).  The actors do not go through the .z form,
// although their .z is 0: with it their entries measured about 1 us longer per call at H = 32, B = 256 (the arms `new`
// and `v_in` of the diagnostic run in profiles/grad_tile_body_ab.txt; why a prologue statement costs that was not found).
template <int H, bool SLOT6>
__device__ __forceinline__ void bptt_stash_inputs(float *vst, const float *lr32, const int64_t *s_src,
                                                  const float4 *s_xh, int W, int tid) {
    constexpr int VN = H + 32;
    for (int i = tid; i < W * 32 * 32; i += kBpttBlock) {
        const int t = i >> 10, p = (i >> 5) & 31, j = i & 31;
        float v;
        if constexpr (SLOT6) {
            const float4 xh = s_xh[p];
            v = j < 4 ? lr32[s_src[p] + 4 * t + j] : (j == 4 ? xh.x : (j == 5 ? 1.0f : (j == 6 ? xh.z : 0.0f)));
        } else {
            v = j < 4 ? lr32[s_src[p] + 4 * t + j] : (j == 4 ? s_xh[p].x : (j == 5 ? 1.0f : 0.0f));
        }
        vst[((int64_t)t * 32 + p) * VN + H + j] = v;
    }
    for (int i = tid; i < 32 * H; i += kBpttBlock) vst[(i / H) * VN + i % H] = 0.0f;
}

// Step t of the forward recurrence for the wavefront's H / 32 gate-row tiles.  xsrc = lr32 + s_src[col], xhc = s_xh[col].
template <int H>
__device__ __forceinline__ void bptt_forward_step(int t, int W, const float *whh, const float *wx, const float *xsrc,
                                                  const float4 xhc, float *s_x, float *stash, float *vst,
                                                  float (&cst)[H / 32][4], int wave, int lane, int col, int half) {
    constexpr int MT = H / 8, MPW = MT / 4, NG = H / 8, HPF = H + 4, VN = H + 32;
    const float *hprev = s_x + ((t + 1) & 1) * 32 * HPF;
    float *hnext = s_x + (t & 1) * 32 * HPF;
    float *slot = stash + (int64_t)t * 160 * H;
    const float4 xc = half == 0 ? *reinterpret_cast<const float4 *>(xsrc + 4 * t) : xhc;
#pragma unroll
    for (int i = 0; i < MPW; ++i) {
        const int mt = wave + 4 * i;
        const size_t R = (size_t)32 * mt + col;
        const float4 wxv = *reinterpret_cast<const float4 *>(wx + R * 8 + 4 * half);
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
                const float4 wv = *reinterpret_cast<const float4 *>(whh + R * H + 8 * gg + 4 * half);
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
}

// dz_t of the wavefront's units, in-lane, from dh_t (s_dh, rows of DHS floats) and the carried dc, into s_x as [pair][R].
template <int H, int DHS>
__device__ __forceinline__ void bptt_dz_step(int t, const float *s_dh, float *s_x, const float *stash,
                                             float (&dc)[H / 32][4], int wave, int lane, int col, int half) {
    constexpr int MT = H / 8, MPW = MT / 4, G4P = 4 * H + 4;
    const float *slot = stash + (int64_t)t * 160 * H;
    const float *pslot = stash + (int64_t)(t - 1) * 160 * H;
#pragma unroll
    for (int i = 0; i < MPW; ++i) {
        const int mt = wave + 4 * i;
        const float4 dh4 = *reinterpret_cast<const float4 *>(s_dh + col * DHS + 8 * mt + 4 * half);
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
}

// dz_t from LDS to the stash slot of step t, [pair][R], over the gates (which every lane has read: after a barrier)
template <int H>
__device__ __forceinline__ void bptt_dz_to_stash(int t, const float *s_x, float *stash, int tid) {
    constexpr int G4 = 4 * H, G4P = G4 + 4;
    float *slot = stash + (int64_t)t * 160 * H;
    for (int i = tid; i < 32 * G4 / 4; i += kBpttBlock) {
        const int p = i / (G4 / 4), r4 = i - p * (G4 / 4);
        reinterpret_cast<float4 *>(slot)[i] = *reinterpret_cast<const float4 *>(s_x + p * G4P + 4 * r4);
    }
}

// dst = wt . z for `tiles` 32-row output tiles: output rows on M (wt: [row][K]), pairs on N, k over z's K columns
// (z: rows of ZS floats, one per pair); dst: rows of DS floats, one per pair.
template <int K, int ZS, int DS>
__device__ __forceinline__ void bptt_wt_contract(const float *wt, const float *z, float *dst, int tiles, int wave,
                                                 int col, int half) {
    for (int ut = wave; ut < tiles; ut += 4) {
        const float *wrow = wt + (size_t)(32 * ut + col) * K + 4 * half;
        const float *zrow = z + col * ZS + 4 * half;
        f32x16 acc;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) acc[rr] = 0.0f;
#pragma unroll 4
        for (int gg = 0; gg < K / 8; ++gg) {
            const float4 wv = *reinterpret_cast<const float4 *>(wrow + 8 * gg);
            const float4 zv = *reinterpret_cast<const float4 *>(zrow + 8 * gg);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const float ws = m == 0 ? wv.x : (m == 1 ? wv.y : (m == 2 ? wv.z : wv.w));
                const float zs = m == 0 ? zv.x : (m == 1 ? zv.y : (m == 2 ? zv.z : zv.w));
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ws, zs, acc, 0, 0, 0);
            }
        }
#pragma unroll
        for (int b = 0; b < 4; ++b)
            *reinterpret_cast<float4 *>(dst + col * DS + 32 * ut + 8 * b + 4 * half) =
                make_float4(acc[4 * b], acc[4 * b + 1], acc[4 * b + 2], acc[4 * b + 3]);
    }
}

// [dW_hh | dW_x] += dz [h | x]^T over the tile's 32 W (pair, step) columns; `first`: the partials are written, else
// added to.  fe_sac_grad_kernel does not call this: it keeps the same statements written out (see there), so a change
// to this stage has to be made in both places.
template <int H>
__device__ __forceinline__ void bptt_weight_grads(const float *stash, const float *vst, float *part, int W, bool first,
                                                  int wave, int lane, int col, int half) {
    constexpr int MT = H / 8, G4 = 4 * H, NTO = H / 32 + 1, VN = H + 32;
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
}

}  // namespace
