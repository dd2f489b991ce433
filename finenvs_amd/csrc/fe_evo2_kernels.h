// fe_evo2_kernels.h -- part of fe_evo2.hip (the library's fourth translation unit): the evolution-strategies population
// with TWO hidden layers (H, H), the network shape the reference's EvoAgent defaults to (finenvs/agents/ES/evo_agent.py:17-37,
// finenvs/agents/networks/parallel_mlp.py; C ABI: include/finenvs_amd_evo2.h).  The noise streams, the argument block, the
// tile layout and the bookkeeping are fe_evo_kernels.h's, included as it stands; only the per-env policy differs.
//
// theta (P = 5W*H + H*H + 3H + 1 floats): W1 (5W, H), b1 (H), W2 (H, H), b2 (H), W3 (H), b3, each row-major (in, out).
// Every segment starts at a multiple of 4, so z_{g,p,j} stays word j % 4 of the counter (j / 4, p, g, 0x45565a00).
//
// Summation order (fixed: two launches give the same bits, and run(32); run(32) equals run(64)).  Lane l owns the outputs
// 4q..4q+3 (q = l % G, G = H / 4) of the rows rg, rg + R, ... (rg = l / G, R = 64 / G) of a layer's weight, in ascending
// order with fmaf from +0; then a butterfly over the row groups (xor G, 2G, ..., 32) completes the sums; then the bias is
// added as (acc + (b + e)).  That holds for the first layer (5W rows) and for the second (H rows).  The third layer is the
// one-layer kernel's second: four fmaf per lane in ascending i from +0, a butterfly over q (xor 1, 2, ..., G / 2), + b3.
#pragma once
#include "fe_evo_kernels.h"

namespace {

__host__ __device__ inline int64_t evo2_num_params(int W, int H) {
    return (int64_t)5 * W * H + (int64_t)H * H + 3 * (int64_t)H + 1;
}

// evo_lds_bytes plus the per-wave exchange buffer of the second layer: 2 H floats (members A and B) per wavefront.
__host__ __device__ inline size_t evo2_lds_bytes(int EB, int A, int W, int H) {
    return evo_lds_bytes(EB, A, evo2_num_params(W, H)) + (size_t)(kBlock / 64) * 2 * H * 4;
}

// Compiler-level ordering of one wavefront's LDS traffic: a wave issues its DS instructions in order and they complete in
// order, so what is needed is only that the compiler moves no LDS access across this point.  NOT a workgroup barrier: the
// waves of a tile run different trip counts of the unit loop when PB is 7 or 1.
__device__ __forceinline__ void evo2_wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The policy of one unit = two env slots of the tile, by one wavefront: evo_policy_unit's member layout and first layer,
// then the H x H layer by the same row loop with x = h1[row].  After the first layer's butterfly lane l holds h1[4q..4q+3];
// row i of the second layer needs h1[i] in every lane: the lanes of row group 0 write h1 to the wave's LDS buffer s_h
// (A at [0, H), B at [H, 2H)) and every lane reads the rows it owns.
template <bool SINGLE, int H>
__device__ __forceinline__ void evo2_policy_unit(const Params &p, const EvoArgs &r, const TileLds &l, float *s_act,
                                                 const float *s_theta, float *s_h, bool pair_tile, int64_t base, int u,
                                                 int k, int lane) {
    constexpr int G = H / 4, R = 64 / G;
    const int A = SINGLE ? 1 : p.A;
    const int R5 = 5 * p.W;
    const int PB = r.PB;
    int eA, eB;
    int64_t nA, nB, pair = 0;
    bool vA, vB;
    if (pair_tile) {
        pair = base + u;
        eA = u; eB = PB + u;
        nA = pair; nB = r.half + pair;
        vA = vB = pair < r.half;
    } else {
        eA = 2 * u; eB = 2 * u + 1;
        nA = base + eA; nB = base + eB;
        vA = nA < p.N; vB = nB < p.N;
    }
    if (!vA) return;          // wave-uniform
    if (!vB) eB = eA;         // (an eval tile's last odd env: computed twice, stored once)
    const int q = lane % G, rg = lane / G;
    const float sigma = r.sigma;
    const int64_t rstride = 4 * (int64_t)A;
    const int64_t NA = p.N * A;
    // Philox counters (float offset / 4) of b1, W2, b2, W3, b3
    const uint32_t qb1 = (uint32_t)R5 * G, qw2 = qb1 + G, qb2 = qw2 + (uint32_t)H * G, qw3 = qb2 + G, qb3 = qw3 + G;
    const float *tb1 = s_theta + (size_t)R5 * H;
    const float *tw2 = tb1 + H;
    const float *tb2 = tw2 + (size_t)H * H;
    const float *tw3 = tb2 + H;
    for (int a = 0; a < A; ++a) {
        const float *xa = r.lr32 + l.src[eA] + 4 * a;
        const float *xb = r.lr32 + l.src[eB] + 4 * a;
        const float posA = (float)l.pos[eA * A + a], posB = (float)l.pos[eB * A + a];
        float accA[4] = {0.0f, 0.0f, 0.0f, 0.0f}, accB[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int row = rg; row < R5; row += R) {
            const int jw = row / 5, c = row - 5 * jw;
            const float xA = c < 4 ? xa[jw * rstride + c] : posA;
            const float xB = c < 4 ? xb[jw * rstride + c] : posB;
            const float4 th = *reinterpret_cast<const float4 *>(s_theta + (size_t)row * H + 4 * q);
            if (pair_tile) {
                const float4 z = evo_z4(r.seed, r.g, pair, (uint32_t)row * G + q);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float e = sigma * f4get(z, i);
                    accA[i] = fmaf(xA, f4get(th, i) + e, accA[i]);
                    accB[i] = fmaf(xB, f4get(th, i) - e, accB[i]);
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    accA[i] = fmaf(xA, f4get(th, i), accA[i]);
                    accB[i] = fmaf(xB, f4get(th, i), accB[i]);
                }
            }
        }
#pragma unroll
        for (int m = G; m < 64; m <<= 1)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                accA[i] = accA[i] + __shfl_xor(accA[i], m, 64);
                accB[i] = accB[i] + __shfl_xor(accB[i], m, 64);
            }
        {  // h1 = tanh(acc + b1): every row group holds the same values; row group 0 publishes them to the wave
            const float4 b1 = *reinterpret_cast<const float4 *>(tb1 + 4 * q);
            float4 zb = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (pair_tile) zb = evo_z4(r.seed, r.g, pair, qb1 + q);
            float hA[4], hB[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float eb = sigma * f4get(zb, i);
                hA[i] = lstm_tanh(accA[i] + (f4get(b1, i) + eb));
                hB[i] = lstm_tanh(accB[i] + (f4get(b1, i) - eb));
            }
            evo2_wave_fence();  // the previous asset's (step's, unit's) reads of s_h are done
            if (rg == 0) {
                *reinterpret_cast<float4 *>(s_h + 4 * q) = make_float4(hA[0], hA[1], hA[2], hA[3]);
                *reinterpret_cast<float4 *>(s_h + H + 4 * q) = make_float4(hB[0], hB[1], hB[2], hB[3]);
            }
            evo2_wave_fence();  // h1 is in s_h before any lane reads it
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) accA[i] = accB[i] = 0.0f;
        for (int row = rg; row < H; row += R) {
            const float xA = s_h[row], xB = s_h[H + row];
            const float4 th = *reinterpret_cast<const float4 *>(tw2 + (size_t)row * H + 4 * q);
            if (pair_tile) {
                const float4 z = evo_z4(r.seed, r.g, pair, qw2 + (uint32_t)row * G + q);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float e = sigma * f4get(z, i);
                    accA[i] = fmaf(xA, f4get(th, i) + e, accA[i]);
                    accB[i] = fmaf(xB, f4get(th, i) - e, accB[i]);
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    accA[i] = fmaf(xA, f4get(th, i), accA[i]);
                    accB[i] = fmaf(xB, f4get(th, i), accB[i]);
                }
            }
        }
#pragma unroll
        for (int m = G; m < 64; m <<= 1)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                accA[i] = accA[i] + __shfl_xor(accA[i], m, 64);
                accB[i] = accB[i] + __shfl_xor(accB[i], m, 64);
            }
        const float4 b2 = *reinterpret_cast<const float4 *>(tb2 + 4 * q);
        const float4 w3 = *reinterpret_cast<const float4 *>(tw3 + 4 * q);
        float b3A = tw3[H], b3B = b3A;
        float4 zb = make_float4(0.0f, 0.0f, 0.0f, 0.0f), zw = zb;
        if (pair_tile) {
            zb = evo_z4(r.seed, r.g, pair, qb2 + q);
            zw = evo_z4(r.seed, r.g, pair, qw3 + q);
            const float e = sigma * evo_z4(r.seed, r.g, pair, qb3).x;
            b3A = b3A + e;
            b3B = b3B - e;
        }
        float partA = 0.0f, partB = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float eb = sigma * f4get(zb, i), ew = sigma * f4get(zw, i);
            const float hA = lstm_tanh(accA[i] + (f4get(b2, i) + eb));
            const float hB = lstm_tanh(accB[i] + (f4get(b2, i) - eb));
            partA = fmaf(f4get(w3, i) + ew, hA, partA);
            partB = fmaf(f4get(w3, i) - ew, hB, partB);
        }
#pragma unroll
        for (int m = 1; m < G; m <<= 1) {
            partA = partA + __shfl_xor(partA, m, 64);
            partB = partB + __shfl_xor(partB, m, 64);
        }
        const float outA = lstm_tanh(partA + b3A), outB = lstm_tanh(partB + b3B);
        float actA = outA, actB = outB;
        if (pair_tile && r.nu != 0.0f) {  // parallel_mlp.py:95,106-110: training members only
            const uint32_t step = r.step0 + (uint32_t)k;
            actA = outA + r.nu * evo_action_noise(r.seed, r.g, step, nA, a);
            actB = outB + r.nu * evo_action_noise(r.seed, r.g, step, nB, a);
        }
        if (lane == 0) {
            s_act[eA * A + a] = actA;
            if (r.means_out) r.means_out[(int64_t)k * NA + nA * A + a] = outA;
            if (vB) {
                s_act[eB * A + a] = actB;
                if (r.means_out) r.means_out[(int64_t)k * NA + nB * A + a] = outB;
            }
        }
    }
}

// fe_evo_rollout_kernel with the policy above: the same tiles (pair tiles of PB mirrored pairs, then eval tiles of EB = 2 PB
// envs), the same accounting, episode slots and counters.  LDS: [TileLds][redrawn days][actions][theta (P)][4 waves x 2H].
// At H = 128 theta is above half the LDS from W = 5 on, so one workgroup per CU is resident there whatever the registers allow.
template <bool SINGLE, int H>
__global__ __launch_bounds__(kBlock, 2) void fe_evo2_rollout_kernel(const Params p, const EvoArgs r) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int A = SINGLE ? 1 : p.A;
    const int EB = p.EB;
    const int S = EB * A;
    const TileLds l = carve_lds(smem, EB, S);
    size_t off = (size_t)EB * 8 + (size_t)S * 8 + (size_t)S * 8 + (size_t)S * 4 + (size_t)S * 4 + (size_t)EB * 4;
    off = (off + 7) & ~(size_t)7;
    int64_t *l_idx = reinterpret_cast<int64_t *>(smem + off);
    off += (size_t)EB * 8;
    float *s_act = reinterpret_cast<float *>(smem + off);
    off = (off + (size_t)S * 4 + 15) & ~(size_t)15;
    float *s_theta = reinterpret_cast<float *>(smem + off);
    const int64_t P = evo2_num_params(p.W, H);
    off = (off + (size_t)P * 4 + 15) & ~(size_t)15;
    const int tid = threadIdx.x;
    const int e = SINGLE ? tid : (int)fdiv((uint32_t)tid, p.div_A);
    const int a = SINGLE ? 0 : tid - e * A;
    const int lane = tid & 63, wave = tid >> 6;
    float *s_h = reinterpret_cast<float *>(smem + off) + (size_t)wave * 2 * H;
    const int64_t NA = p.N * A;
    const int PB = r.PB;
    for (int64_t i = tid; i < P; i += kBlock) s_theta[i] = r.theta[i];

    for (int64_t tile = blockIdx.x; tile < p.num_tiles; tile += gridDim.x) {
        const bool pair_tile = tile < r.pair_tiles;
        int64_t base, n;
        bool valid;
        if (pair_tile) {
            base = tile * PB;
            const int64_t np = r.half - base < PB ? r.half - base : PB;
            n = e < PB ? base + e : r.half + base + (e - PB);
            valid = (e < PB ? e : e - PB) < np;
        } else {
            base = r.n_train + (tile - r.pair_tiles) * EB;
            n = base + e;
            valid = n < p.N;
        }
        const bool active = e < EB && valid;
        if (!active) n = 0;
        const int64_t sl = n * A + a;
        SleeveReg st = rollout_load_state(p, active, n, sl);
        float ret = 0.0f, ts = 0.0f;
        if (active) {
            if (a == 0) {
                l.src[e] = r.obs_src[n];
                ret = r.ret[n];
                ts = r.ts[n];
            }
            l.pos[e * A + a] = r.obs_pos[sl];
        }
        __syncthreads();  // also covers theta on the first tile
        for (int k = 0; k < r.K; ++k) {
            for (int u = wave; u < PB; u += kBlock / 64)
                evo2_policy_unit<SINGLE, H>(p, r, l, s_act, s_theta, s_h, pair_tile, base, u, k, lane);
            lds_barrier();
            const float act = active ? s_act[e * A + a] : 0.0f;
            if (active && r.actions_out) r.actions_out[(int64_t)k * NA + sl] = act;
            double *rew = r.rew_out ? r.rew_out + (int64_t)k * p.N : r.rew_scratch;
            int32_t *done = r.done_out ? r.done_out + (int64_t)k * p.N : r.done_scratch;
            account_keep<SINGLE>(p, l, l_idx, A, e, a, active, n, st, act, rew, done);
            if (active && a == 0) {  // evo_agent.py:96-112 (current_returns is f32, the rewards f64)
                ret = (float)((double)ret + rew[n]);
                ts = ts + 1.0f;
                if (done[n]) {
                    const int32_t c = r.ep_cnt[n];
                    if (c < r.max_ep) {
                        r.ep_ret[n * r.max_ep + c] = ret;
                        r.ep_cnt[n] = c + 1;
                    } else {
                        r.counters[1] = 1ull;  // train() refuses: an episode would be lost
                    }
                    atomicAdd(&r.counters[0], (unsigned long long)ts);
                    ret = 0.0f;
                    ts = 0.0f;
                }
            }
            lds_barrier();  // the new observation's descriptors are complete
        }
        rollout_store_state(p, active, a, n, sl, st);
        if (active) {
            r.obs_pos[sl] = l.pos[e * A + a];
            if (a == 0) {
                r.obs_src[n] = l.src[e];
                r.ret[n] = ret;
                r.ts[n] = ts;
            }
        }
        __syncthreads();
    }
}

}  // namespace
