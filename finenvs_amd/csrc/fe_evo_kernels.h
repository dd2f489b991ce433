// fe_evo_kernels.h -- part of fe_evo.hip and fe_evo_streamed.hip (two translation units of the library, the second with
// theta read through L2, include/finenvs_amd_evo2_streamed.h): the evolution-strategies population -- a
// K-step rollout in which every env acts with ITS OWN perturbed perceptron of one hidden layer (H) or two (H, H), generated
// inside the kernel from a counter-based normal stream -- plus the gradient and noise-render kernels of the ES update
// (finenvs/agents/ES/evo_agent.py, finenvs/agents/networks/parallel_mlp.py; C ABI: include/finenvs_amd_evo.h and
// include/finenvs_amd_evo2.h).
//
// theta, each segment row-major (in, out): W1 (5W, H), b1 (H), [W2 (H, H), b2 (H),] Wo (H), bo.  Every segment starts at a
// multiple of 4 (H is one), so z_{g,p,j} is word j % 4 of the counter (j / 4, p, g, 0x45565a00) at either depth.
//
// Summation order (fixed: two launches give the same bits, and run(32); run(32) equals run(64)).  Lane l owns the outputs
// 4q..4q+3 (q = l % G, G = H / 4) of the rows rg, rg + R, ... (rg = l / G, R = 64 / G) of a hidden layer's weight, in
// ascending order with fmaf from +0; then a butterfly over the row groups (xor G, 2G, ..., 32) completes the sums; then the
// bias is added as (acc + (b + e)).  The output layer: four fmaf per lane in ascending i from +0, a butterfly over q (xor 1,
// 2, ..., G / 2), + bo.
#pragma once
#include "fe_device_common.h"
#include "fe_rollout_kernels.h"
#include "fe_activations.h"

namespace {

// Counter domains (word c3 of the Philox counter).  The redraw stream of redraw_mode 1 uses c2 = 0x46454e56, c3 = 0, so a
// non-zero c3 keeps both streams below apart from it and from each other.
constexpr uint32_t kEvoDomainZ = 0x45565a00u;    // "EVZ": parameter perturbations, counter (j / 4, pair, generation)
constexpr uint32_t kEvoDomainAct = 0x45564100u;  // "EVA" | asset / 4: action noise, counter (env, step, generation)
constexpr int kEvoGradPairs = 64;                // pairs per partial sum of the gradient's first pass

// Philox4x32-10 with all four output words (philox_u32 of fe_device_common.h returns the first only).
__device__ __forceinline__ uint4 evo_philox4(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        uint32_t n1 = (uint32_t)p1;
        uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return make_uint4(c0, c1, c2, c3);
}

// f32 Box-Muller on the four words: (w0, w1) -> normals 0, 1 and (w2, w3) -> normals 2, 3.  u = ((w >> 8) + 1) / 2^24 in
// (0, 1], the angle (w >> 8) / 2^24 in revolutions (what v_sin_f32 / v_cos_f32 take), ln u = ln 2 * log2 u (v_log_f32).
// This device function IS the definition of the stream: the host never restates it, tests read it through fe_evo_noise.
__device__ __forceinline__ float4 evo_normal4(uint4 w) {
    const float k = 5.9604644775390625e-8f;  // 2^-24
    const float u0 = (float)((w.x >> 8) + 1u) * k, t0 = (float)(w.y >> 8) * k;
    const float u1 = (float)((w.z >> 8) + 1u) * k, t1 = (float)(w.w >> 8) * k;
    const float r0 = __builtin_amdgcn_sqrtf(-1.38629436f * __builtin_amdgcn_logf(u0));
    const float r1 = __builtin_amdgcn_sqrtf(-1.38629436f * __builtin_amdgcn_logf(u1));
    return make_float4(r0 * __builtin_amdgcn_cosf(t0), r0 * __builtin_amdgcn_sinf(t0), r1 * __builtin_amdgcn_cosf(t1),
                       r1 * __builtin_amdgcn_sinf(t1));
}

// z_{g,p,4q..4q+3}
__device__ __forceinline__ float4 evo_z4(uint64_t seed, uint32_t g, int64_t pair, uint32_t q) {
    return evo_normal4(evo_philox4(seed, q, (uint32_t)pair, g, kEvoDomainZ));
}

__device__ __forceinline__ float evo_action_noise(uint64_t seed, uint32_t g, uint32_t step, int64_t n, int a) {
    const float4 v = evo_normal4(evo_philox4(seed, (uint32_t)n, step, g, kEvoDomainAct | (uint32_t)(a >> 2)));
    const int m = a & 3;
    return m == 0 ? v.x : (m == 1 ? v.y : (m == 2 ? v.z : v.w));
}

__device__ __forceinline__ float f4get(const float4 &v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : (i == 2 ? v.z : v.w)); }

struct EvoArgs {
    const float *lr32;   // (D, L, 4A) f32 copy of the log-return table
    const float *theta;  // (P) W1 (5W, H), b1 (H), W2 (H), b2, each row-major
    int64_t *obs_src;
    double *obs_pos;
    float *ret;          // (N) running return
    float *ts;           // (N) running timestep count
    float *ep_ret;       // (N, max_ep) finished episodes' returns
    int32_t *ep_cnt;     // (N)
    unsigned long long *counters;  // [0] timesteps of finished episodes, [1] slot-table overflow flag
    float *actions_out;  // (K, N, A) or null
    float *means_out;    // (K, N, A) or null: the network's output before the action noise
    double *rew_out;     // (K, N) or null (then rew_scratch (N) takes every step)
    int32_t *done_out;
    double *rew_scratch;
    int32_t *done_scratch;
    int64_t n_train, half;
    int32_t K, max_ep, PB, pair_tiles;
    float sigma, nu;
    uint64_t seed;
    uint32_t g, step0;
};

// Floats of theta with `layers` hidden layers: 5W*H + 2H + 1, and H*H + H more for the middle layer.
__host__ __device__ inline int64_t evo_num_params(int layers, int W, int H) {
    return (int64_t)5 * W * H + (layers - 1) * ((int64_t)H * H + H) + 2 * (int64_t)H + 1;
}

// Byte offsets of a tile's dynamic LDS behind TileLds (carve_lds, at 0) and their total: the redrawn day per env, the
// actions, theta (P floats) and, with two hidden layers only, the middle layer's exchange buffer: 2 H floats (members A
// and B) for each of the workgroup's wavefronts.  The kernel and the host's byte count both read this.
struct EvoLds {
    size_t idx, act, theta, xchg, total;
};

__host__ __device__ inline EvoLds evo_lds(int layers, int EB, int A, int64_t P, int H) {
    const size_t S = (size_t)EB * A;
    EvoLds o;
    o.idx = (size_t)EB * 8 + S * 8 + S * 8 + S * 4 + S * 4 + (size_t)EB * 4;  // TileLds
    o.idx = (o.idx + 7) & ~(size_t)7;
    o.act = o.idx + (size_t)EB * 8;
    o.theta = (o.act + S * 4 + 15) & ~(size_t)15;
    o.xchg = (o.theta + (size_t)P * 4 + 15) & ~(size_t)15;
    o.total = o.xchg + (layers == 2 ? (size_t)(kBlock / 64) * 2 * H * 4 : 0);
    return o;
}

// Compiler-level ordering of one wavefront's LDS traffic: a wave issues its DS instructions in order and they complete in
// order, so what is needed is only that the compiler moves no LDS access across this point.  NOT a workgroup barrier: the
// waves of a tile run different trip counts of the unit loop when PB is 7 or 1.
__device__ __forceinline__ void evo_wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The two members of unit u of a tile.  Pair tiles: slot u is env p (sign +1), slot PB + u env p + n_train/2 (sign -1) of
// the same pair p = base + u, so every z element is generated once and serves both signs.  Eval tiles: slots 2u, 2u + 1,
// both unperturbed; a last odd env is computed twice (eB = eA) and stored once (vB is false).
struct EvoMembers {
    int eA, eB;      // env slots of the tile
    int64_t nA, nB;  // env indices
    int64_t pair;
    bool vA, vB;
};

__device__ __forceinline__ EvoMembers evo_members(const Params &p, const EvoArgs &r, bool pair_tile, int64_t base, int u) {
    EvoMembers m;
    m.pair = 0;
    if (pair_tile) {
        m.pair = base + u;
        m.eA = u; m.eB = r.PB + u;
        m.nA = m.pair; m.nB = r.half + m.pair;
        m.vA = m.vB = m.pair < r.half;
    } else {
        m.eA = 2 * u; m.eB = 2 * u + 1;
        m.nA = base + m.eA; m.nB = base + m.eB;
        m.vA = m.nA < p.N; m.vB = m.nB < p.N;
    }
    if (!m.vB) m.eB = m.eA;
    return m;
}

// One hidden layer's sums for both members: acc[i] = sum over the lane's rows rg, rg + R, ... of x(row) * w[row][4q + i],
// the weight perturbed by +- sigma z on pair tiles (Philox counter q0 + row * G + q, q0 the segment's offset / 4), then
// the butterfly over the row groups.  x(row, xA, xB) gives the row's input of either member.
template <int H, class X>
__device__ __forceinline__ void evo_layer(const EvoArgs &r, bool pair_tile, int64_t pair, const float *w, uint32_t q0,
                                          int rows, int lane, X x, float (&accA)[4], float (&accB)[4]) {
    constexpr int G = H / 4, R = 64 / G;
    const int q = lane % G, rg = lane / G;
#pragma unroll
    for (int i = 0; i < 4; ++i) accA[i] = accB[i] = 0.0f;
    for (int row = rg; row < rows; row += R) {
        float xA, xB;
        x(row, xA, xB);
        const float4 th = *reinterpret_cast<const float4 *>(w + (size_t)row * H + 4 * q);
        if (pair_tile) {
            const float4 z = evo_z4(r.seed, r.g, pair, q0 + (uint32_t)row * G + q);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float e = r.sigma * f4get(z, i);
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
}

// h = tanh(acc + (b +- sigma z)) for the lane's four hidden units; qb is the Philox counter of b[0..3].
__device__ __forceinline__ void evo_hidden(const EvoArgs &r, bool pair_tile, int64_t pair, const float *b, uint32_t qb, int q,
                                           const float (&accA)[4], const float (&accB)[4], float (&hA)[4], float (&hB)[4]) {
    const float4 bq = *reinterpret_cast<const float4 *>(b + 4 * q);
    float4 zb = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (pair_tile) zb = evo_z4(r.seed, r.g, pair, qb + q);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float eb = r.sigma * f4get(zb, i);
        hA[i] = lstm_tanh(accA[i] + (f4get(bq, i) + eb));
        hB[i] = lstm_tanh(accB[i] + (f4get(bq, i) - eb));
    }
}

// The policy of one unit = two env slots of the tile (evo_members), by one wavefront.  Every row group holds the same
// hidden values after a layer's butterfly.  Row i of the middle layer needs h1[i] in every lane: the lanes of row group 0
// write h1 to the wave's LDS buffer s_h (A at [0, H), B at [H, 2H); null with one hidden layer) and every lane reads the
// rows it owns.  Assets are evaluated one after the other with the env's weights (z regenerated per asset).
// theta is read where it lives: the workgroup's LDS copy, or global memory (the streamed kernels).
template <bool SINGLE, int H, int LAYERS>
__device__ __forceinline__ void evo_policy_unit(const Params &p, const EvoArgs &r, const TileLds &l, float *s_act,
                                                const float *s_theta, float *s_h, bool pair_tile, int64_t base, int u,
                                                int k, int lane) {
    constexpr int G = H / 4;
    const int A = SINGLE ? 1 : p.A;
    const int R5 = 5 * p.W;
    const EvoMembers m = evo_members(p, r, pair_tile, base, u);
    if (!m.vA) return;  // wave-uniform
    const int q = lane % G;
    const int64_t rstride = 4 * (int64_t)A;
    const int64_t NA = p.N * A;
    for (int a = 0; a < A; ++a) {
        const float *xa = r.lr32 + l.src[m.eA] + 4 * a;
        const float *xb = r.lr32 + l.src[m.eB] + 4 * a;
        const float posA = (float)l.pos[m.eA * A + a], posB = (float)l.pos[m.eB * A + a];
        // the segment being read and the Philox counter of its first four floats advance together
        const float *t = s_theta;
        uint32_t qc = 0;
        float accA[4], accB[4], hA[4], hB[4];
        evo_layer<H>(r, pair_tile, m.pair, t, qc, R5, lane, [&](int row, float &xA, float &xB) {
            const int jw = row / 5, c = row - 5 * jw;
            xA = c < 4 ? xa[jw * rstride + c] : posA;
            xB = c < 4 ? xb[jw * rstride + c] : posB;
        }, accA, accB);
        t += (size_t)R5 * H; qc += (uint32_t)R5 * G;
        evo_hidden(r, pair_tile, m.pair, t, qc, q, accA, accB, hA, hB);
        t += H; qc += G;
        if constexpr (LAYERS == 2) {
            evo_wave_fence();  // the previous asset's (step's, unit's) reads of s_h are done
            if (lane < G) {    // row group 0
                *reinterpret_cast<float4 *>(s_h + 4 * q) = make_float4(hA[0], hA[1], hA[2], hA[3]);
                *reinterpret_cast<float4 *>(s_h + H + 4 * q) = make_float4(hB[0], hB[1], hB[2], hB[3]);
            }
            evo_wave_fence();  // h1 is in s_h before any lane reads it
            evo_layer<H>(r, pair_tile, m.pair, t, qc, H, lane, [&](int row, float &xA, float &xB) {
                xA = s_h[row];
                xB = s_h[H + row];
            }, accA, accB);
            t += (size_t)H * H; qc += (uint32_t)H * G;
            evo_hidden(r, pair_tile, m.pair, t, qc, q, accA, accB, hA, hB);
            t += H; qc += G;
        }
        // the output layer: t = Wo (H) with bo behind it, their counters qc + q and qc + G (word .x)
        const float4 wo = *reinterpret_cast<const float4 *>(t + 4 * q);
        float boA = t[H], boB = boA;
        float4 zw = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (pair_tile) {
            zw = evo_z4(r.seed, r.g, m.pair, qc + q);
            const float e = r.sigma * evo_z4(r.seed, r.g, m.pair, qc + G).x;
            boA = boA + e;
            boB = boB - e;
        }
        float partA = 0.0f, partB = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float ew = r.sigma * f4get(zw, i);
            partA = fmaf(f4get(wo, i) + ew, hA[i], partA);
            partB = fmaf(f4get(wo, i) - ew, hB[i], partB);
        }
#pragma unroll
        for (int s = 1; s < G; s <<= 1) {
            partA = partA + __shfl_xor(partA, s, 64);
            partB = partB + __shfl_xor(partB, s, 64);
        }
        const float outA = lstm_tanh(partA + boA), outB = lstm_tanh(partB + boB);
        float actA = outA, actB = outB;
        if (pair_tile && r.nu != 0.0f) {  // parallel_mlp.py:95,106-110: training members only
            const uint32_t step = r.step0 + (uint32_t)k;
            actA = outA + r.nu * evo_action_noise(r.seed, r.g, step, m.nA, a);
            actB = outB + r.nu * evo_action_noise(r.seed, r.g, step, m.nB, a);
        }
        if (lane == 0) {
            s_act[m.eA * A + a] = actA;
            if (r.means_out) r.means_out[(int64_t)k * NA + m.nA * A + a] = outA;
            if (m.vB) {
                s_act[m.eB * A + a] = actB;
                if (r.means_out) r.means_out[(int64_t)k * NA + m.nB * A + a] = outB;
            }
        }
    }
}

// K steps of the whole population per launch: the loop of fe_rollout_mlp_kernel (account state in registers, descriptors
// in LDS, account_keep), with the per-env policy above and EvoAgent.store's bookkeeping (evo_agent.py:96-112) where the
// done flag is known.  Tiles: pair tiles [0, pair_tiles) hold PB mirrored pairs (2 PB envs), the rest EB = 2 PB
// consecutive eval envs.  At two layers and H = 128 theta is above half the LDS from W = 5 on, so one workgroup per CU
// is resident there whatever the registers allow.
// STREAMED: theta stays in global memory (every workgroup reads the same <= 256 KiB + 5W KiB, which lives in L2) and the
// policy's row loads go there, one float4 per lane and row next to that row's Philox chain; the LDS then holds no theta
// (evo_lds with P = 0) and does not grow with W.  Loading the rows one or two trips ahead into registers was measured and
// is slower at every H (profiles/evo_streamed_bench.txt).
template <bool SINGLE, int H, int LAYERS, bool STREAMED = false>
__device__ __forceinline__ void evo_rollout_body(const Params &p, const EvoArgs &r) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int A = SINGLE ? 1 : p.A;
    const int EB = p.EB;
    const int S = EB * A;
    const int64_t P = STREAMED ? 0 : evo_num_params(LAYERS, p.W, H);
    const TileLds l = carve_lds(smem, EB, S);
    const EvoLds o = evo_lds(LAYERS, EB, A, P, H);
    int64_t *l_idx = reinterpret_cast<int64_t *>(smem + o.idx);
    float *s_act = reinterpret_cast<float *>(smem + o.act);
    const float *s_theta = r.theta;
    const int tid = threadIdx.x;
    const int e = SINGLE ? tid : (int)fdiv((uint32_t)tid, p.div_A);
    const int a = SINGLE ? 0 : tid - e * A;
    const int lane = tid & 63, wave = tid >> 6;
    float *s_h = nullptr;
    if constexpr (LAYERS == 2) s_h = reinterpret_cast<float *>(smem + o.xchg) + (size_t)wave * 2 * H;
    const int64_t NA = p.N * A;
    const int PB = r.PB;
    if constexpr (!STREAMED) {
        float *copy = reinterpret_cast<float *>(smem + o.theta);
        for (int64_t i = tid; i < P; i += kBlock) copy[i] = r.theta[i];
        s_theta = copy;
    }

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
                evo_policy_unit<SINGLE, H, LAYERS>(p, r, l, s_act, s_theta, s_h, pair_tile, base, u, k, lane);
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

// The entry points: one hidden layer (fe_evo_rollout, H = 32 / 64) and two (fe_evo2_rollout, H = 32 / 64 / 128).
template <bool SINGLE, int H>
__global__ __launch_bounds__(kBlock, 2) void fe_evo_rollout_kernel(const Params p, const EvoArgs r) {
    evo_rollout_body<SINGLE, H, 1>(p, r);
}

template <bool SINGLE, int H>
__global__ __launch_bounds__(kBlock, 2) void fe_evo2_rollout_kernel(const Params p, const EvoArgs r) {
    evo_rollout_body<SINGLE, H, 2>(p, r);
}

// The streamed two-layer entry (fe_evo2_rollout_streamed, H = 32 / 64 / 128 / 256; include/finenvs_amd_evo2_streamed.h):
// fe_evo2_rollout_kernel with theta read through L2.  Instantiated by fe_evo_streamed.hip only.
template <bool SINGLE, int H>
__global__ __launch_bounds__(kBlock, 2) void fe_evo2_streamed_rollout_kernel(const Params p, const EvoArgs r) {
    evo_rollout_body<SINGLE, H, 2, true>(p, r);
}

// First pass of the gradient: partial[b][j] = sum over the pairs of block b (ascending) of diffed[p] * z_{g,p,j}, in f64.
// One thread per (block, Philox counter q = j / 4).
__global__ __launch_bounds__(kBlock) void fe_evo_gradient_partial_kernel(uint64_t seed, uint32_t g, int64_t num_pairs,
                                                                         int64_t P, const float *diffed, double *partial) {
    const int64_t nq = (P + 3) / 4;
    const int64_t blocks = (num_pairs + kEvoGradPairs - 1) / kEvoGradPairs;
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= nq * blocks) return;
    const int64_t b = t / nq, q = t - b * nq;
    const int64_t p0 = b * kEvoGradPairs;
    const int64_t p1 = p0 + kEvoGradPairs < num_pairs ? p0 + kEvoGradPairs : num_pairs;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t pp = p0; pp < p1; ++pp) {
        const float4 z = evo_z4(seed, g, pp, (uint32_t)q);
        const double d = (double)diffed[pp];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = fma(d, (double)f4get(z, i), acc[i]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (4 * q + i < P) partial[b * P + 4 * q + i] = acc[i];
}

// Second pass: out[j] = sum over the blocks (ascending) of partial[b][j].
__global__ __launch_bounds__(kBlock) void fe_evo_gradient_reduce_kernel(int64_t blocks, int64_t P, const double *partial,
                                                                        double *out) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= P) return;
    double acc = 0.0;
    for (int64_t b = 0; b < blocks; ++b) acc += partial[b * P + j];
    out[j] = acc;
}

// out[i][j] = z_{g, pairs[i], j} for j < P: the noise as the rollout and the gradient see it.
__global__ __launch_bounds__(kBlock) void fe_evo_noise_kernel(uint64_t seed, uint32_t g, const int64_t *pairs, int64_t count,
                                                              int64_t P, float *out) {
    const int64_t nq = (P + 3) / 4;
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= nq * count) return;
    const int64_t i = t / nq, q = t - i * nq;
    const float4 z = evo_z4(seed, g, pairs[i], (uint32_t)q);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (4 * q + k < P) out[i * P + 4 * q + k] = f4get(z, k);
}

}  // namespace
