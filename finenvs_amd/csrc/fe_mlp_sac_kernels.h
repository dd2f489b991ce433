// fe_mlp_sac_kernels.h -- part of fe_mlp_sac.hip (the library's third translation unit): the SAC MLP actor on
// observation descriptors (include/finenvs_amd_mlp_sac.h).
//
// The actor's second Linear has no activation, and mu_layer / std_layer are linear in its output, so
//   mu = c_mu + v_mu . a1,  q = c_s + v_s . a1,  a1 = act(W1 x + b1)
// with v = W2^T w and c = w . b2 + b (fe_mlp_sac_pack_kernel, sums in f64, rounded once).  Every row is therefore the
// one-layer head's: mlp_head_first_layer and mlp_head_p of fe_mlp_head_kernels.h as they stand, called twice on the
// same accumulators (the activations are pure functions of them; the compiler evaluates them once).  The backward
// keeps the rank-two form: per pair only dmu and dq enter the first layer (dz1 = (v_mu dmu + v_s dq) act'(z1)), and the
// H x H layer's gradients are an O(H^2) epilogue on the four batch sums [A_mu | S_mu | A_q | S_q].
#pragma once
#include "fe_mlp_head_kernels.h"

namespace {

struct MlpSacArgs {
    const float *lr32;  // (D, L, 4A) f32 copy of the log-return table
    const float *w1t, *wpos, *b1;  // the first layer as fe_mlp_pack writes it
    const float *vmu, *vstd;       // (H) each: the folded head
    const float *cfold;            // (2): c_mu, c_s
    int32_t act, K;
    int64_t *obs_src;   // rollout: the envs' descriptors, read and written; forward: `count` descriptors, read only
    double *obs_pos;
    const float *noise;  // rollout: (K, N*A) or null; forward: (count * A) or null
    float *actions_out, *logp_out, *means_out, *stds_out;  // each may be null
    double *rew_out;
    int32_t *done_out;
    int64_t *traj_src;   // (K + 1, N) or null
    double *traj_pos;    // (K + 1, N*A) or null
    int64_t count;       // forward: descriptors
};

// what the image holds beyond the one-layer head's [W1t | wpos | b1 | w2 = v_mu]: v_s and the two constants (padded to 16 B)
__host__ __device__ inline size_t mlp_sac_extra_lds_bytes(int H) { return ((size_t)H + 4) * 4; }
__host__ __device__ inline size_t mlp_sac_lds_bytes(int EB, int A, int W, int H) {
    return mlp_lds_bytes(EB, A, W, H) + mlp_sac_extra_lds_bytes(H);
}
__host__ __device__ inline size_t mlp_sac_weight_lds_bytes(int W, int H) {
    return mlp_head_weight_lds_bytes(W, H) + mlp_sac_extra_lds_bytes(H);
}

// the image at s_w1t: the head's own, then v_s and [c_mu, c_s]
__device__ __forceinline__ void mlp_sac_load_weights(float *s_w1t, int H, int W, const float *w1t, const float *wpos,
                                                     const float *b1, const float *vmu, const float *vstd,
                                                     const float *cfold, int tid) {
    mlp_head_load_weights(s_w1t, H, W, w1t, wpos, b1, vmu, tid);
    float *s_vs = s_w1t + (size_t)H * mlp_kp(W) + 3 * H;
    for (int i = tid; i < H; i += kBlock) s_vs[i] = vstd[i];
    if (tid < 2) s_vs[H + tid] = cfold[tid];
}

// F.softplus (beta 1, threshold 20), the LSTM actor's statement
__device__ __forceinline__ float mlp_sac_softplus(float q) { return q > 20.0f ? q : log1pf(expf(q)); }

// Normal(mu, sd).log_prob(u) - log(1 - tanh(u)^2 + 1e-7) (SAC/actor.py:51-61), the LSTM actor's statements
__device__ __forceinline__ float mlp_sac_log_prob(float u, float mu, float sd, float act) {
    const float d = u - mu;
    const float lp = -(d * d) / (2.0f * (sd * sd)) - logf(sd) - 0.918938533204672742f;
    return lp - logf((1.0f - act * act) + 1e-7f);
}

// ---- fe_mlp_sac_pack: the first layer as fe_mlp_pack_kernel packs it, and the fold ----
__global__ __launch_bounds__(kBlock) void fe_mlp_sac_pack_kernel(const float *weight1, const float *w2, const float *b2,
                                                                 const float *wmu, const float *bmu, const float *wstd,
                                                                 const float *bstd, int H, int W, float *w1t, float *wpos,
                                                                 float *vmu, float *vstd, float *cfold) {
    const int K4 = 4 * W;
    const int64_t n1 = (int64_t)H * K4, total = n1 + 3 * (int64_t)H + 2;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        if (i < n1) {
            const int h = (int)(i / K4), k = (int)(i - (int64_t)h * K4);
            w1t[i] = weight1[(size_t)h * 5 * W + 5 * (k >> 2) + (k & 3)];
        } else if (i < n1 + H) {
            const int h = (int)(i - n1);
            float s = 0.0f;  // fe_mlp_pack_kernel's sequential f32 sum
            for (int j = 0; j < W; ++j) s = s + weight1[(size_t)h * 5 * W + 5 * j + 4];
            wpos[h] = s;
        } else if (i < n1 + 3 * (int64_t)H) {  // v[j] = sum_i W2[i][j] w[i], i ascending, f64, rounded once
            const int j = (int)(i - n1 - H);
            const float *w = j < H ? wmu : wstd;
            const int c = j < H ? j : j - H;
            double s = 0.0;
            for (int r = 0; r < H; ++r) s += (double)w2[(size_t)r * H + c] * (double)w[r];
            (j < H ? vmu : vstd)[c] = (float)s;
        } else {  // c = sum_i w[i] b2[i] + b
            const int which = (int)(i - n1 - 3 * (int64_t)H);
            const float *w = which == 0 ? wmu : wstd;
            double s = 0.0;
            for (int r = 0; r < H; ++r) s += (double)w[r] * (double)b2[r];
            s += (double)(which == 0 ? bmu[0] : bstd[0]);
            cfold[which] = (float)s;
        }
    }
}

// ---- fe_env_rollout_mlp_sac: fe_rollout_mlp_sampled_kernel's loop; the wavefront that evaluates a 32-pair block
// samples there, writes mu and s itself and leaves only the action in s_act ----
template <bool SINGLE, int NT>
__global__ __launch_bounds__(kBlock, 2) void fe_rollout_mlp_sac_kernel(const Params p, const MlpSacArgs r) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int A = SINGLE ? 1 : p.A;
    const int EB = p.EB;
    const int S = EB * A;
    const int W = p.W;
    constexpr int H = 32 * NT;
    const TileLds l = carve_lds(smem, EB, S);
    size_t off = (size_t)EB * 8 + (size_t)S * 8 + (size_t)S * 8 + (size_t)S * 4 + (size_t)S * 4 + (size_t)EB * 4;
    off = (off + 7) & ~(size_t)7;
    int64_t *l_idx = reinterpret_cast<int64_t *>(smem + off);
    off += (size_t)EB * 8;
    float *s_act = reinterpret_cast<float *>(smem + off);
    off = (off + (size_t)S * 4 + 15) & ~(size_t)15;
    const int KP = mlp_kp(W);
    float *s_w1t = reinterpret_cast<float *>(smem + off);
    float *s_wpos = s_w1t + (size_t)H * KP;
    float *s_b1 = s_wpos + H;
    float *s_vmu = s_b1 + H;
    float *s_vs = s_vmu + H;
    const int tid = threadIdx.x;
    const int e = SINGLE ? tid : (int)fdiv((uint32_t)tid, p.div_A);
    const int a = SINGLE ? 0 : tid - e * A;
    const int lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, half = lane >> 5;
    const int64_t NA = p.N * A;
    const int64_t rstride = 4 * (int64_t)A;
    mlp_sac_load_weights(s_w1t, H, W, r.w1t, r.wpos, r.b1, r.vmu, r.vstd, r.cfold, tid);

    for (int64_t tile = blockIdx.x; tile < p.num_tiles; tile += gridDim.x) {
        const int64_t n0 = tile * EB;
        const int ebt = (p.N - n0) < (int64_t)EB ? (int)(p.N - n0) : EB;
        const bool active = e < ebt;
        const int64_t n = n0 + e;
        const int64_t sl = n * A + a;
        SleeveReg st = rollout_load_state(p, active, n, sl);
        if (active) {
            const double pos0 = r.obs_pos[sl];
            l.pos[e * A + a] = pos0;
            if (a == 0) l.src[e] = r.obs_src[n];
            if (r.traj_src) {  // row 0: the state the first policy evaluation sees
                r.traj_pos[sl] = pos0;
                if (a == 0) r.traj_src[n] = r.obs_src[n];
            }
        }
        __syncthreads();  // also covers the weight image on the first tile
        const float cmu = s_vs[H], cs = s_vs[H + 1];
        const int pairs = ebt * A;
        const int nblk = (pairs + 31) / 32;
        for (int k = 0; k < r.K; ++k) {
            // ---- policy: one wavefront per block of 32 pairs; mu, s and the action leave from here ----
            for (int blk = wave; blk < nblk; blk += kBlock / 64) {
                const int q = blk * 32 + col;
                const int qc = q < pairs ? q : pairs - 1;
                const int ee = SINGLE ? qc : (int)fdiv((uint32_t)qc, p.div_A);
                const int aa = SINGLE ? 0 : qc - ee * A;
                f32x16 acc[NT];
                mlp_head_first_layer<NT>(acc, r.lr32 + l.src[ee] + 4 * aa, rstride, (float)l.pos[qc], W, s_w1t, s_wpos,
                                         s_b1, KP, lane);
                const float mu = mlp_head_p<NT>(acc, r.act, s_vmu, half, cmu);
                const float sd = mlp_sac_softplus(mlp_head_p<NT>(acc, r.act, s_vs, half, cs));
                const int64_t o = (int64_t)k * NA + (n0 + ee) * A + aa;
                float av = mu;  // the eval env, and every env without noise, acts on the un-squashed mean
                if (r.noise && n0 + ee != p.eval_env) av = lstm_tanh(mu + r.noise[o] * sd);  // Normal.rsample: loc + eps * scale
                if (half == 0 && q < pairs) {
                    s_act[q] = av;
                    if (r.means_out) r.means_out[o] = mu;
                    if (r.stds_out) r.stds_out[o] = sd;
                    if (r.actions_out) r.actions_out[o] = av;
                }
            }
            lds_barrier();
            const float act = active ? s_act[e * A + a] : 0.0f;
            account_keep<SINGLE>(p, l, l_idx, A, e, a, active, n, st, act, r.rew_out + (int64_t)k * p.N,
                                 r.done_out + (int64_t)k * p.N);
            if (active && r.traj_src) {  // row k + 1: the observation this step returns (own LDS entries: no barrier needed)
                r.traj_pos[(int64_t)(k + 1) * NA + sl] = l.pos[e * A + a];
                if (a == 0) r.traj_src[(int64_t)(k + 1) * p.N + n] = l.src[e];
            }
            lds_barrier();  // the new observation's descriptors are complete
        }
        rollout_store_state(p, active, a, n, sl, st);  // state and descriptors go back to HBM once per launch
        if (active) {
            r.obs_pos[sl] = l.pos[e * A + a];
            if (a == 0) r.obs_src[n] = l.src[e];
        }
        __syncthreads();
    }
}

// ---- fe_mlp_sac_forward: one wavefront per block of 32 descriptor pairs, grid-strided; the weight image in LDS ----
template <bool SINGLE, int NT>
__global__ __launch_bounds__(kBlock, 2) void fe_mlp_sac_forward_kernel(const Params p, const MlpSacArgs r) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int A = SINGLE ? 1 : p.A;
    const int W = p.W;
    constexpr int H = 32 * NT;
    const int KP = mlp_kp(W);
    float *s_w1t = reinterpret_cast<float *>(smem);
    float *s_wpos = s_w1t + (size_t)H * KP;
    float *s_b1 = s_wpos + H;
    float *s_vmu = s_b1 + H;
    float *s_vs = s_vmu + H;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, half = lane >> 5;
    mlp_sac_load_weights(s_w1t, H, W, r.w1t, r.wpos, r.b1, r.vmu, r.vstd, r.cfold, tid);
    __syncthreads();
    const float cmu = s_vs[H], cs = s_vs[H + 1];
    const int64_t pairs = r.count * A;
    const int64_t nblk = (pairs + 31) / 32;
    for (int64_t blk = (int64_t)blockIdx.x * (kBlock / 64) + wave; blk < nblk; blk += (int64_t)gridDim.x * (kBlock / 64)) {
        const int64_t q = blk * 32 + col;
        const int64_t qc = q < pairs ? q : pairs - 1;
        const int64_t ee = SINGLE ? qc : qc / A;
        const int aa = SINGLE ? 0 : (int)(qc - ee * A);
        f32x16 acc[NT];
        mlp_head_first_layer<NT>(acc, r.lr32 + r.obs_src[ee] + 4 * aa, 4 * (int64_t)A, (float)r.obs_pos[qc], W, s_w1t,
                                 s_wpos, s_b1, KP, lane);
        const float mu = mlp_head_p<NT>(acc, r.act, s_vmu, half, cmu);
        const float sd = mlp_sac_softplus(mlp_head_p<NT>(acc, r.act, s_vs, half, cs));
        if (half == 0 && q < pairs) {
            if (r.means_out) r.means_out[q] = mu;
            if (r.stds_out) r.stds_out[q] = sd;
            if (r.noise) {  // every descriptor samples: there is no evaluation env here
                const float u = mu + r.noise[q] * sd;
                const float av = lstm_tanh(u);
                if (r.actions_out) r.actions_out[q] = av;
                if (r.logp_out) r.logp_out[q] = mlp_sac_log_prob(u, mu, sd, av);
            }
        }
    }
}

// ---- fe_mlp_sac_backward ----
constexpr int kMlpSacGradMaxGroups = 256;  // workgroups of the first kernel at most: one per CU of an MI355X

struct MlpSacGradArgs {
    MlpGradArgs g;  // what fe_mlp_wgrad_kernel reads; here w2 = v_mu, wpart rows are 2 (H + 4) floats wide
    const float *vstd, *cfold;            // the rest of the folded head
    const float *w2h, *b2h, *wmu, *wstd;  // (H, H), (H), (H), (H) as torch holds them: the epilogue's operands
    const float *noise, *actions, *stds;  // (count): eps, and what fe_mlp_sac_forward returned
    const float *d_actions, *d_logp;      // (count) upstream gradients, either may be null
    float *g_w2h, *g_b2h, *g_wmu, *g_bmu, *g_wstd, *g_bstd;
};

__host__ __device__ inline int64_t mlp_sac_grad_groups(int64_t blocks) {
    const int64_t g = (blocks + 3) / 4;
    return g < kMlpSacGradMaxGroups ? g : kMlpSacGradMaxGroups;
}

// dz1 of the lane's pair into its workspace row (four consecutive units per 16-byte store); the in-lane partials of
// A_mu = sum dmu a1 and A_q = sum dq a1
template <int ACT, int NT>
__device__ __forceinline__ void mlp_sac_grad_block_tail(const f32x16 (&acc)[NT], float (&amu)[NT][16], float (&aq)[NT][16],
                                                        const float *s_vmu, const float *s_vs, int half, float dmu, float dq,
                                                        bool valid, float *dz_row) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int h0 = 32 * t + 8 * b + 4 * half;
            const float4 vm = *reinterpret_cast<const float4 *>(s_vmu + h0);
            const float4 vs = *reinterpret_cast<const float4 *>(s_vs + h0);
            const float vms[4] = {vm.x, vm.y, vm.z, vm.w}, vss[4] = {vs.x, vs.y, vs.z, vs.w};
            float o[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float a, d;
                mlp_act_grad<ACT>(acc[t][4 * b + c], a, d);
                amu[t][4 * b + c] = amu[t][4 * b + c] + (valid ? dmu * a : 0.0f);
                aq[t][4 * b + c] = aq[t][4 * b + c] + (valid ? dq * a : 0.0f);
                o[c] = valid ? (vms[c] * dmu + vss[c] * dq) * d : 0.0f;  // the padding pairs of the last block: zeros
            }
            *reinterpret_cast<float4 *>(dz_row + h0) = make_float4(o[0], o[1], o[2], o[3]);
            // four units at a time (mlp_grad_block_tail); with two accumulator sets H = 64 needs it too, or it spills
            if constexpr (NT >= 2) __builtin_amdgcn_sched_barrier(0);
        }
}

// (a) per 32-pair block and wavefront: the first layer recomputed, the head's backward per pair, dz1 written
template <int NT>
__global__ __launch_bounds__(kBlock, (NT == 4 ? 1 : 2)) void fe_mlp_sac_grad_kernel(const MlpSacGradArgs ga) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int H = 32 * NT;
    const MlpGradArgs &g = ga.g;
    const int W = g.W;
    const int KP = mlp_kp(W);
    float *s_w1t = reinterpret_cast<float *>(smem);
    float *s_wpos = s_w1t + (size_t)H * KP;
    float *s_b1 = s_wpos + H;
    float *s_vmu = s_b1 + H;
    float *s_vs = s_vmu + H;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, half = lane >> 5;
    mlp_sac_load_weights(s_w1t, H, W, g.w1t, g.wpos, g.b1, g.w2, ga.vstd, ga.cfold, tid);
    __syncthreads();
    const float cs = s_vs[H + 1];
    float amu[NT][16], aq[NT][16];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) amu[t][rr] = aq[t][rr] = 0.0f;
    float smu = 0.0f, sq = 0.0f;
    const int64_t gw = (int64_t)blockIdx.x * (kBlock / 64) + wave;
    for (int64_t blk = gw; blk < g.blocks; blk += (int64_t)gridDim.x * (kBlock / 64)) {
        const int64_t q = blk * 32 + col;
        const int64_t qc = q < g.count ? q : g.count - 1;
        f32x16 acc[NT];
        mlp_head_first_layer<NT, NT != 4>(acc, g.lr32 + g.obs_src[qc], 4, (float)g.obs_pos[qc], W, s_w1t, s_wpos, s_b1, KP, lane);
        const float qv = mlp_head_p<NT>(acc, g.act, s_vs, half, cs);  // the forward's pre-softplus std, the same bits
        float dmu = 0.0f, dq = 0.0f;
        if (q < g.count) {  // SAC/actor.py:51-61 differentiated, fe_sac_grad_kernel's statements
            const float av = ga.actions[q], sv = ga.stds[q], ev = ga.noise[q];
            const float gav = ga.d_actions ? ga.d_actions[q] : 0.0f, gl = ga.d_logp ? ga.d_logp[q] : 0.0f;
            const float om = 1.0f - av * av;
            const float du = gav * om + gl * (2.0f * av * om / (om + 1e-7f));
            const float ds = du * ev - gl / sv;
            const float sg = qv > 20.0f ? 1.0f : 1.0f / (1.0f + expf(-qv));  // d softplus (beta 1, threshold 20)
            dmu = du;
            dq = ds * sg;
        }
        if (half == 0) {
            smu = smu + dmu;
            sq = sq + dq;
        }
        float *dz_row = g.dpre + q * H;
        if (g.act == 1) mlp_sac_grad_block_tail<1, NT>(acc, amu, aq, s_vmu, s_vs, half, dmu, dq, q < g.count, dz_row);
        else if (g.act == 2) mlp_sac_grad_block_tail<2, NT>(acc, amu, aq, s_vmu, s_vs, half, dmu, dq, q < g.count, dz_row);
        else mlp_sac_grad_block_tail<0, NT>(acc, amu, aq, s_vmu, s_vs, half, dmu, dq, q < g.count, dz_row);
    }
    // the 32 pairs of the wavefront's columns: a butterfly in a fixed order (every lane ends with the same sum)
#pragma unroll
    for (int m = 1; m < 32; m <<= 1) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                amu[t][rr] = amu[t][rr] + __shfl_xor(amu[t][rr], m, 64);
                aq[t][rr] = aq[t][rr] + __shfl_xor(aq[t][rr], m, 64);
            }
        smu = smu + __shfl_xor(smu, m, 64);
        sq = sq + __shfl_xor(sq, m, 64);
    }
    if (col == 0) {  // the wavefront's row of the partials: [A_mu (H) | S_mu | 3 unused | A_q (H) | S_q | 3 unused]
        float *wp = g.wpart + gw * (2 * (H + 4));
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                const int h = 32 * t + (rr & 3) + 8 * (rr >> 2) + 4 * half;
                wp[h] = amu[t][rr];
                wp[H + 4 + h] = aq[t][rr];
            }
        if (half == 0) {
            wp[H] = smu;
            wp[2 * H + 4] = sq;
        }
    }
}

// (c) fe_mlp_grad_reduce_kernel's layer-1 half, and the epilogue: every workgroup first adds the wavefronts' partials
// of [A_mu | S_mu | A_q | S_q] in index order (f64) into LDS, then its threads form their elements of the H x H layer's
// and the two output layers' gradients from those sums in f64 and round once.
__global__ __launch_bounds__(kBlock) void fe_mlp_sac_grad_reduce_kernel(const MlpSacGradArgs ga) {
    __shared__ double s_sum[2 * (128 + 4)];
    const MlpGradArgs &g = ga.g;
    const int H = g.H, W = g.W, K4 = 4 * W, F = K4 + 2, PW = 2 * (H + 4);
    for (int v = threadIdx.x; v < PW; v += kBlock) {
        const int h = v < H + 4 ? v : v - (H + 4);
        double s = 0.0;
        if (h <= H)  // the three unused floats of either half are never read
            for (int64_t k = 0; k < g.waves; ++k) s += (double)g.wpart[k * PW + v];
        s_sum[v] = s;
    }
    __syncthreads();
    const double *A_mu = s_sum, *A_q = s_sum + H + 4;
    const double S_mu = s_sum[H], S_q = s_sum[2 * H + 4];
    const int64_t n1 = (int64_t)H * F, n2 = n1 + (int64_t)H * H, total = n2 + 3 * (int64_t)H + 2;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        if (i < n1) {  // the first layer: the splits added in index order
            const int h = (int)(i / F), f = (int)(i - (int64_t)h * F);
            const float *src = g.part + (int64_t)h * g.FP + f;
            double s = 0.0;
            for (int64_t k = 0; k < g.splits; ++k) s += (double)src[k * (int64_t)H * g.FP];
            const float v = (float)s;
            float *row = g.g_w1 + (size_t)h * 5 * W;
            if (f < K4) row[5 * (f >> 2) + (f & 3)] = v;
            else if (f == K4) {  // the position column is the same in every window row
                for (int j = 0; j < W; ++j) row[5 * j + 4] = v;
            } else g.g_b1[h] = v;
        } else if (i < n2) {  // d W2 = w_mu A_mu^T + w_s A_q^T
            const int r = (int)((i - n1) / H), c = (int)((i - n1) - (int64_t)r * H);
            ga.g_w2h[i - n1] = (float)((double)ga.wmu[r] * A_mu[c] + (double)ga.wstd[r] * A_q[c]);
        } else if (i < n2 + H) {  // d b2 = w_mu S_mu + w_s S_q
            const int r = (int)(i - n2);
            ga.g_b2h[r] = (float)((double)ga.wmu[r] * S_mu + (double)ga.wstd[r] * S_q);
        } else if (i < n2 + 3 * (int64_t)H) {  // d w = W2 A + b2 S
            const int r0 = (int)(i - n2 - H);
            const bool is_mu = r0 < H;
            const int r = is_mu ? r0 : r0 - H;
            const double *Av = is_mu ? A_mu : A_q;
            double s = 0.0;
            for (int c = 0; c < H; ++c) s += (double)ga.w2h[(size_t)r * H + c] * Av[c];
            s += (double)ga.b2h[r] * (is_mu ? S_mu : S_q);
            (is_mu ? ga.g_wmu : ga.g_wstd)[r] = (float)s;
        } else {
            if (i == n2 + 3 * (int64_t)H) ga.g_bmu[0] = (float)S_mu;
            else ga.g_bstd[0] = (float)S_q;
        }
    }
}

}  // namespace
