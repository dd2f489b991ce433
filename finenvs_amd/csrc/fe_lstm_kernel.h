// fe_lstm_kernel.h -- part of fe_env.hip (one translation unit; see the overview there): K-step fused rollout with the reference's LSTM actor on MFMA, and its exact-operation sigmoid / tanh.
#pragma once
#include "fe_device_common.h"
#include "fe_rollout_kernels.h"
#include "fe_activations.h"

namespace {

// ---- f2, LSTM head: the actor of the reference's own time-series scripts, on the matrix cores ----
// finenvs/agents/networks/lstm.py:28-57 -- nn.LSTM(5, H, batch_first) from a zero state over the W rows of the
// observation, Linear(H, 1) on the last hidden state, Tanh (continuous_actor.py:104-126) -- evaluated on
// states.float() per (env, asset) pair; examples/time_series/PPO_LSTM_testing_SPY.py:43-52 is the loop this fuses.
// Per time step the gates are a (4H) x (H + 8) x (pairs) contraction, G^T = [Whh | Wx] . [h_{t-1} ; x_t]^T:
//   * gate rows on the M side of v_mfma_f32_32x32x2_f32, 32 (env, asset) pairs on the N side; the rows are packed by
//     the host so that an accumulator lane holds all four gates of four hidden units of ITS pair (row
//     R = 32 mt + 8 b + 4 half + gate <-> unit 8 mt + 4 half + b): the cell update is in-lane, c_t never leaves
//     the registers, and h_t goes to LDS as one 16-byte store per lane -- already in the [pair][unit] layout the next
//     step's B operand reads with one ds_read_b128 per four MFMAs;
//   * the recurrent weights stay in REGISTERS for the whole launch: Whh for H = 128 is 256 KiB, more than the LDS,
//     but split over the 8 wavefronts of a 512-thread workgroup it is 128 VGPRs per lane (2 wavefronts per SIMD,
//     256 VGPRs each); every wavefront owns MPW row tiles and runs all the workgroup's 32-pair column tiles;
//   * the input part (K = 8: four log-returns | position, 1 for the bias, 0, 0) is four more MFMAs per tile;
//   * the f32 MFMA is an fmaf chain in k order, and sigmoid / tanh are built from rintf, fmaf, ldexpf and IEEE
//     division only (lstm_exp_nonpos), so the test-side CPU restatement (fo_policy_lstm) reproduces every
//     action BIT FOR BIT; against torch's own nn.LSTM the actions agree to ~1e-7.
// One barrier per time step (h double-buffered in LDS); the last hidden state is reduced by the pair's accounting lane.
constexpr int kLstmBlock = 512;
// large-H kernel: row tiles run together (independent accumulator chains per B fragment) / k groups of weight
// fragments in flight; split kernel: k groups of h in flight (profiles/r02_microbench/lstm_*.txt)
constexpr int kLstmBigRI = 4;
constexpr int kLstmBigAhead = 2;
constexpr int kLstmSplitAhead = 16;

struct LstmArgs {
    const float *lr32;  // (D, L, 4A) f32 copy of the log-return table
    const float *whh;   // (4H, H) f32, packed row order
    const float *wx;    // (4H, 8) f32, packed row order: w_ih[0..3], w_ih[4], b_ih + b_hh, 0, 0
    const float *wout;  // (H)
    float bout;
    int32_t H, out_act, K;  // out_act: 0 tanh (the reference's actor), 1 clamp to [-1, 1], 2 none (a critic's value)
    int64_t *obs_src;
    double *obs_pos;
    float *actions_out;
    double *rew_out;
    int32_t *done_out;
    // training rollouts (PPO_agent.py:98-108): actions = clamp(mean + std * noise, -1, 1), the eval env acts on the mean
    const float *noise;  // (K, N*A) standard normal draws, or null: act on the mean
    float std;
    float *means_out;    // (K, N*A) or null
    int64_t *traj_src;   // (K + 1, N) or null: descriptors of the state the policy sees at every step (+ the last one)
    double *traj_pos;    // (K + 1, N*A)
    int32_t forward_only;  // fe_lstm_forward: evaluate the head on p.N given descriptors, no env step (K = 1, actions_out = the outputs)
    const float *bout_p = nullptr;  // (1) on the device, or null: the output bias of the *_p entries, read instead of bout
};

template <int NT> struct LstmGeom {
    static constexpr int H = 32 * NT;
    static constexpr int MT = H / 8;                        // 32-row gate tiles
    static constexpr int MPW = MT >= 8 ? MT / 8 : 1;        // row tiles per wavefront
    static constexpr int NSPLIT = MT >= 8 ? 1 : 8 / MT;     // wavefronts sharing a row tile split the column tiles
    static constexpr int SP = NT == 4 ? 64 : 128;           // (env, asset) pairs per workgroup tile
    static constexpr int MAXNT = SP / 32 / NSPLIT;          // column tiles per wavefront
    static constexpr int HP = H + 4;                        // LDS row length of h: 16 bytes against bank conflicts
};

__host__ __device__ inline size_t lstm_lds_bytes(int EB, int A, int H, int SP) {
    size_t S = (size_t)EB * A;
    size_t b = (size_t)EB * 8 + S * 8 + S * 8 + S * 4 + S * 4 + (size_t)EB * 4;  // TileLds
    b = (b + 7) & ~(size_t)7;
    b += (size_t)EB * 8;  // redrawn day per env
    b = (b + 15) & ~(size_t)15;
    b += 2 * (size_t)SP * (H + 4) * 4;  // h, double-buffered
    b += (size_t)H * 4;                 // wout
    return (b + 15) & ~(size_t)15;
}

__global__ __launch_bounds__(kBlock) void fe_lstm_activations_kernel(const float *x, float *sig, float *tnh, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const v2f v = lstm_act2<false, true>((v2f){x[i], x[i]});
        sig[i] = v.x;
        tnh[i] = v.y;
    }
}

// ---- the SAC actor's head on the same recurrence (finenvs/agents/SAC/actor.py:ActorLSTM, shape (5, H, 1)) ----
// LSTMNetwork duplicates the last size, so h_W goes through Linear(H, H) (Identity activation) before mu_layer and
// std_layer (both Linear(H, 1) per pair): z = W_l h_W + b_l, mu = w_mu . z + b_mu, s = softplus(w_s . z + b_s).
// z is one more (H) x (H) x (pairs) contraction on v_mfma_f32_32x32x2_f32 with the gates' operand layout: W_l rows in
// torch order on the M side (H / 32 row tiles), the workgroup's 32-pair column tiles on the N side, h_W from LDS as the
// B operand; wavefront w owns row tile w % (H / 32) of column tile w / (H / 32) (H = 32: four of the eight wavefronts
// work), one accumulator chain over the H / 8 k groups.  z lands in the idle half of the h double buffer (h_{W-1},
// read by nobody after the last time step's barrier) and the pair's accounting lane reduces it as the LSTM head does.
// W_l (fragment-major, [row tile][k group][lane][4]) lives in LDS at H = 32 (4 KiB; two workgroups per CU still fit)
// and H = 128 (64 KiB; the kernel runs one workgroup per CU and has that much LDS free); at H = 64 two workgroups per
// CU take 151 of the 160 KiB, so there the A fragments stream from L2 (16 KiB, shared by every workgroup).
struct SacArgs {
    LstmArgs l;         // recurrence, descriptors and env outputs; l.means_out = mu, l.wout / l.bout / l.out_act unused
    const float *wl;    // (H / 32, H / 8, 64, 4) f32: last_layer weight, fragment-major
    const float *bl;    // (H) last_layer bias
    const float *wmu;   // (H) mu_layer weight
    const float *wstd;  // (H) std_layer weight
    float bmu, bstd;
    float *stds_out;    // (K, N*A) or null: softplus(std_layer(z))
    float *logp_out;    // forward only, with noise: (N*A) log_prob of tanh(u), or null
    const float *bmu_p = nullptr, *bstd_p = nullptr;  // (1) each on the device, or null: read instead of bmu / bstd (*_p entries)
};

template <int NT> constexpr bool sac_wl_in_lds() { return NT != 2; }

struct SacHeadLds {  // copied to LDS once per launch (see the kernel)
    float *stds_out, *logp_out;
    float bmu, bstd;
};

// in floats from w_mu: w_mu, w_std, b_l, W_l (if in LDS), then SacHeadLds (16-byte aligned: H is a multiple of 32)
__host__ __device__ constexpr int sac_head_lds_offset(int H) { return 3 * H + (H != 64 ? H * H : 0); }

__host__ __device__ inline size_t sac_lds_bytes(int EB, int A, int H, int SP) {
    size_t b = lstm_lds_bytes(EB, A, H, SP);  // ... h double buffer, w_mu in the slot of wout
    b += (size_t)(sac_head_lds_offset(H) - H) * 4 + sizeof(SacHeadLds);
    return (b + 15) & ~(size_t)15;
}

template <bool SINGLE, int NT>
__global__ __launch_bounds__(kLstmBlock, (NT == 1 ? 4 : 2)) void fe_rollout_lstm_kernel(const Params p, const LstmArgs r) {
#define FE_LSTM_SAC_HEAD 0
#include "fe_lstm_rollout_body.h"
#undef FE_LSTM_SAC_HEAD
}

template <bool SINGLE, int NT>
__global__ __launch_bounds__(kLstmBlock, (NT == 1 ? 4 : 2)) void fe_rollout_sac_kernel(const Params p, const SacArgs hd) {
    const LstmArgs &r = hd.l;
#define FE_LSTM_SAC_HEAD 1
#include "fe_lstm_rollout_body.h"
#undef FE_LSTM_SAC_HEAD
}

// ---- the same head for H = 256, 512, 1024 (the reference example trains hidden_dim = 1024): weights from L2 ----
// Whh no longer fits a workgroup's registers (4 MiB / 16 MiB), so it is STREAMED: the host stores it fragment-major --
// [row tile mt][k group g][lane][4], one contiguous KiB per (mt, g), exactly the A fragment of four MFMAs -- and every
// wavefront loads its fragments with coalesced 16-byte loads two k groups (32 MFMAs) ahead of their use, continuously; the XCD's 4 MiB L2 (and the
// Infinity Cache behind it) serves the 32 CUs that sweep the same matrix.  Per workgroup ONE 32-pair column tile
// (H = 1024: h alone is 128 KiB of LDS, single-buffered: a wavefront keeps its new h values in registers until every
// wavefront has finished reading the old ones -- two barriers per time step); each of the 8 wavefronts owns
// RTW = H / 64 row tiles and runs them four at a time (four independent accumulator chains sharing the B fragment;
// measured against two: +6 % at H = 256, +2 % at H = 1024, tools/fused_bench.py with FUSED_LIB).
// c_t and the pending h_t live in per-lane scratch (RTW x 4 floats each, touched once per row tile).  Same k order, same activations, same cell update as the register-
// resident kernel: the same oracle function pins it bit for bit.
__host__ __device__ inline size_t lstm_big_lds_bytes(int EB, int A, int H) {
    size_t S = (size_t)EB * A;
    size_t b = (size_t)EB * 8 + S * 8 + S * 8 + S * 4 + S * 4 + (size_t)EB * 4;  // TileLds
    b = (b + 7) & ~(size_t)7;
    b += (size_t)EB * 8;  // redrawn day per env
    b = (b + 15) & ~(size_t)15;
    b += (size_t)32 * (H + 4) * 4;  // h, one buffer
    b += (size_t)H * 4;             // wout
    return (b + 15) & ~(size_t)15;
}

template <bool SINGLE, int RTW>
__global__ __launch_bounds__(kLstmBlock, 2) void fe_rollout_lstm_big_kernel(const Params p, const LstmArgs r) {
#define FE_LSTM_SAC_HEAD 0
#include "fe_lstm_big_rollout_body.h"
#undef FE_LSTM_SAC_HEAD
}

// ---- large H at SMALL env counts: one launch per time step, the row tiles spread over the whole GPU ----
// The fused kernels keep a tile on one CU for a whole env step; at H = 1024 that CU walks 128 row tiles (1.8 ms per step
// however few envs there are).  Below a few thousand pairs the step is better cut the other way: one launch per LSTM
// time step in which workgroup (mt, y) computes gate-row tile mt for four 32-pair column tiles (one per wavefront), with
// h_{t-1}, h_t and c_t in global memory -- FRAGMENT-MAJOR, [column tile][k group][lane][4]: the float4 a lane of row
// tile mt produces (units 8 mt + 4 half + b of its pair) IS the B fragment of k group g = mt of the next time step, so
// both sides are one coalesced KiB per wavefront -- and the launch boundary is the exchange of h.  A last launch per env
// step reduces h_W to the action and runs the accounting (one lane per sleeve).  Same k order, same activations, same
// cell update: the same oracle function, bit for bit.  The floor is the accumulator chain itself: H/2 + 4 DEPENDENT MFMAs
// per time step at 64 cycles each (measured in round 2 with a dependent-MFMA probe, NOTES.md) = 15 us at H = 1024; the launch reaches 25 - 30 us: its L2 is
// cold, so the row tile's weights are staged through LDS by the whole workgroup and h arrives 16 k groups ahead.
struct LstmSplitArgs {
    LstmArgs a;          // weights (whh fragment-major), descriptors, outputs of step k (pointers already offset)
    float *hbuf;         // [2][CT][H/8][64][4] f32: h, double-buffered by time-step parity
    float *cbuf;         // [CT][H/8][64][4] f32
    int32_t t;           // time step of this launch (gates kernel)
    int32_t k;           // env step of this launch (finish kernel: row k + 1 of the trajectory)
    int64_t pairs;       // N * A
};

// PER float4s per lane, all loads in flight before the first LDS write
template <int PER>
__device__ __forceinline__ void lstm_stage_weights(const float4 *src, float4 *dst, int tid) {
    float4 v[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) v[j] = src[j * kBlock + tid];
#pragma unroll
    for (int j = 0; j < PER; ++j) dst[j * kBlock + tid] = v[j];
}

template <bool SINGLE>
__global__ __launch_bounds__(kBlock) void fe_lstm_split_gates_kernel(const Params p, const LstmSplitArgs s) {
    extern __shared__ __align__(16) unsigned char smem[];
    const LstmArgs &r = s.a;
    const int A = SINGLE ? 1 : p.A;
    const int H = r.H, NG = H / 8, t = s.t;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, half = lane >> 5;
    const int mt = blockIdx.x;
    const int64_t ct = (int64_t)blockIdx.y * (kBlock / 64) + wave;
    const int64_t CT = (s.pairs + 31) / 32;
    // Every launch starts with a cold L2: everything this wavefront needs first goes out FIRST -- its row of x, the input
    // weights, the first AHEAD k groups of h -- and then the whole workgroup fetches the row tile's recurrent weights (H/8
    // KiB, fragment-major; Infinity Cache / HBM at ~1.5 us) ONCE into LDS with all its loads in flight together (up to 32 per
    // lane), instead of each wavefront trickling them in a few KiB ahead of its accumulator chain.
    const bool valid = ct < CT;
    const int64_t ctc = valid ? ct : CT - 1;
    const int64_t q = ctc * 32 + col;
    const int64_t qc = q < s.pairs ? q : s.pairs - 1;
    const int64_t n = SINGLE ? qc : qc / A;
    const int aa = SINGLE ? 0 : (int)(qc - n * A);
    // B fragment of the input part: the row's four log-returns | position, 1, 0, 0
    float4 xv;
    if (half == 0) xv = *reinterpret_cast<const float4 *>(r.lr32 + r.obs_src[n] + 4 * aa + (int64_t)t * 4 * A);
    else xv = make_float4((float)r.obs_pos[qc], 1.0f, 0.0f, 0.0f);
    const float4 wxv = *reinterpret_cast<const float4 *>(r.wx + ((size_t)32 * mt + col) * 8 + 4 * half);
    const size_t frag = (size_t)CT * NG * 64;  // float4s per h buffer
    float4 *hnext = reinterpret_cast<float4 *>(s.hbuf) + (size_t)(t & 1) * frag;
    const float4 *hprev = reinterpret_cast<const float4 *>(s.hbuf) + (size_t)((t + 1) & 1) * frag + ((size_t)ctc * NG) * 64 + lane;
    constexpr int AHEAD = kLstmSplitAhead;  // k groups of h in flight (h was written by the previous launch: also cold)
    float4 hq[AHEAD];
    if (t > 0) {
#pragma unroll
        for (int d = 0; d < AHEAD; ++d) hq[d] = hprev[(size_t)d * 64];
    }
    float4 *s_w = reinterpret_cast<float4 *>(smem);  // [NG][64]
    if (t > 0) {
        const float4 *wsrc = reinterpret_cast<const float4 *>(r.whh) + ((size_t)mt * NG) * 64;
        const int per = NG * 64 / kBlock;  // float4s per lane: 8 (H = 256), 16, 32 (H = 1024)
        if (per == 32) lstm_stage_weights<32>(wsrc, s_w, tid);
        else if (per == 16) lstm_stage_weights<16>(wsrc, s_w, tid);
        else lstm_stage_weights<8>(wsrc, s_w, tid);
    }
    __syncthreads();
    if (!valid) return;  // (no further barriers)
    f32x16 acc;
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) acc[rr] = 0.0f;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const float xs = m == 0 ? xv.x : (m == 1 ? xv.y : (m == 2 ? xv.z : xv.w));
        const float ws = m == 0 ? wxv.x : (m == 1 ? wxv.y : (m == 2 ? wxv.z : wxv.w));
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ws, xs, acc, 0, 0, 0);
    }
    if (t > 0) {
        float4 wnext = s_w[lane];  // the A fragment is read from LDS one k group ahead of its MFMAs (a dependent MFMA can
                                   // issue every 64 cycles, measured in round 2, NOTES.md: nothing may wait in between)
#pragma unroll 1
        for (int g0 = 0; g0 < NG; g0 += AHEAD) {
#pragma unroll
            for (int d = 0; d < AHEAD; ++d) {
                const float4 hb = hq[d];
                const int gn = g0 + d + AHEAD < NG ? g0 + d + AHEAD : NG - 1;  // (the last loads are redundant, in range)
                hq[d] = hprev[(size_t)gn * 64];
                const float4 wv = wnext;
                wnext = s_w[(g0 + d + 1 < NG ? g0 + d + 1 : NG - 1) * 64 + lane];
                // keep the refill load HERE, AHEAD groups before its use: left alone, the scheduler sinks it to ~3 groups ahead
                // (and splits it into dword loads), which the cold h cannot cover
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const float hs = m == 0 ? hb.x : (m == 1 ? hb.y : (m == 2 ? hb.z : hb.w));
                    const float ws = m == 0 ? wv.x : (m == 1 ? wv.y : (m == 2 ? wv.z : wv.w));
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ws, hs, acc, 0, 0, 0);
                }
            }
        }
    }
    // cell update, in-lane: acc[4b + gate] belongs to unit 8 mt + 4 half + b of pair col
    float4 *cptr = reinterpret_cast<float4 *>(s.cbuf) + ((size_t)ct * NG + mt) * 64 + lane;
    const float4 cold = t > 0 ? *cptr : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float co[4] = {cold.x, cold.y, cold.z, cold.w};
    float cn[4], og[4], hv[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const v2f sif = lstm_act2<false, false>((v2f){acc[4 * b + 0], acc[4 * b + 1]});
        const v2f tgo = lstm_act2<true, false>((v2f){acc[4 * b + 2], acc[4 * b + 3]});
        const float t1 = sif.y * co[b];
        const float t2 = sif.x * tgo.x;
        cn[b] = t1 + t2;
        og[b] = tgo.y;
    }
#pragma unroll
    for (int b = 0; b < 4; b += 2) {
        const v2f tc = lstm_act2<true, true>((v2f){cn[b], cn[b + 1]});
        hv[b] = og[b] * tc.x;
        hv[b + 1] = og[b + 1] * tc.y;
    }
    *cptr = make_float4(cn[0], cn[1], cn[2], cn[3]);
    hnext[((size_t)ct * NG + mt) * 64 + lane] = make_float4(hv[0], hv[1], hv[2], hv[3]);
}

// output layer + accounting of one env step (the tail of fe_rollout_lstm_kernel's step loop as its own launch)
template <bool SINGLE>
__global__ __launch_bounds__(kBlock) void fe_lstm_split_finish_kernel(const Params p, const LstmSplitArgs s) {
    extern __shared__ __align__(16) unsigned char smem[];
    const LstmArgs &r = s.a;
    const int A = SINGLE ? 1 : p.A;
    const int EB = p.EB;
    const int S = EB * A;
    const int H = r.H, NG = H / 8;
    const TileLds l = carve_lds(smem, EB, S);
    size_t off = (size_t)EB * 8 + (size_t)S * 8 + (size_t)S * 8 + (size_t)S * 4 + (size_t)S * 4 + (size_t)EB * 4;
    off = (off + 7) & ~(size_t)7;
    int64_t *l_idx = reinterpret_cast<int64_t *>(smem + off);
    off = (off + (size_t)EB * 8 + 15) & ~(size_t)15;
    float4 *s_hq = reinterpret_cast<float4 *>(smem + off);  // [EB * A][2 NG]
    const int tid = threadIdx.x;
    const int e = SINGLE ? tid : (int)fdiv((uint32_t)tid, p.div_A);
    const int a = SINGLE ? 0 : tid - e * A;
    const int64_t NA = p.N * A;
    const int64_t CT = (s.pairs + 31) / 32;
    const float *hW = s.hbuf + (size_t)((p.W - 1) & 1) * CT * NG * 64 * 4;
    for (int64_t tile = blockIdx.x; tile < p.num_tiles; tile += gridDim.x) {
        const int64_t n0 = tile * EB;
        const int ebt = (p.N - n0) < (int64_t)EB ? (int)(p.N - n0) : EB;
        const bool active = e < ebt;
        const int64_t n = n0 + e;
        const int64_t sl = n * A + a;
        SleeveReg st = rollout_load_state(p, active && !r.forward_only, n, sl);
        // h_W of the tile's pairs -> LDS, the whole workgroup loading (the launch starts with a cold L2: a lane walking its
        // own 4 KiB alone would pay ~0.3 us per dependent-latency step): [pair][2 NG] float4, units ascending per pair
        {
            const int tp = ebt * A;  // pairs of this tile: sl0 .. sl0 + tp - 1
            const int64_t sl0 = n0 * A;
            const int per = 2 * NG;  // float4s per pair
            for (int i = tid; i < tp * per; i += kBlock) {
                const int pq = i / per, j = i - pq * per;       // pair, (g, half) = (j >> 1, j & 1)
                const int64_t qg = sl0 + pq;
                s_hq[i] = reinterpret_cast<const float4 *>(hW)[(((size_t)(qg >> 5) * NG + (j >> 1)) * 64 + (qg & 31) + 32 * (j & 1))];
            }
            __syncthreads();
        }
        float act = 0.0f;
        if (active) {
            if (s.k == 0 && r.traj_src) {  // row 0: the state the first policy evaluation saw
                r.traj_pos[sl] = r.obs_pos[sl];
                if (a == 0) r.traj_src[n] = r.obs_src[n];
            }
            const float4 *hp = s_hq + (size_t)(e * A + a) * (2 * NG);  // this pair's h_W, units ascending (staged above)
            float o = r.bout_p ? *r.bout_p : r.bout;
#pragma unroll 4
            for (int g = 0; g < NG; ++g) {  // units 8g + 4 half + c
                const float4 h0 = hp[2 * g], h1 = hp[2 * g + 1];
                const float *w = r.wout + 8 * g;
                o = fmaf(w[0], h0.x, o); o = fmaf(w[1], h0.y, o); o = fmaf(w[2], h0.z, o); o = fmaf(w[3], h0.w, o);
                o = fmaf(w[4], h1.x, o); o = fmaf(w[5], h1.y, o); o = fmaf(w[6], h1.z, o); o = fmaf(w[7], h1.w, o);
            }
            act = r.out_act == 0 ? lstm_tanh(o) : (r.out_act == 2 ? o : (o < -1.0f ? -1.0f : (o > 1.0f ? 1.0f : o)));
            if (r.means_out) r.means_out[sl] = act;
            if (r.noise && n != p.eval_env) {
                const float dev = r.std * r.noise[sl];
                const float smp = act + dev;
                act = smp < -1.0f ? -1.0f : (smp > 1.0f ? 1.0f : smp);
            }
            if (r.actions_out) r.actions_out[sl] = act;
        }
        if (!r.forward_only) {  // (uniform)
            account_keep<SINGLE>(p, l, l_idx, A, e, a, active, n, st, act, r.rew_out, r.done_out);
            rollout_store_state(p, active, a, n, sl, st);
            if (active) {
                r.obs_pos[sl] = l.pos[e * A + a];
                if (a == 0) r.obs_src[n] = l.src[e];
                if (r.traj_src) {
                    r.traj_pos[(int64_t)(s.k + 1) * NA + sl] = l.pos[e * A + a];
                    if (a == 0) r.traj_src[(int64_t)(s.k + 1) * p.N + n] = l.src[e];
                }
            }
        }
        __syncthreads();  // s_hq and the accounting scratch are reused by the next tile
    }
}

}  // namespace
