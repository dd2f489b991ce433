// fe_lstm_big_rollout_body.h -- part of fe_env.hip (one translation unit; see the overview there): the body of the LSTM
// rollout at H = 256 / 512 / 1024 with the recurrent weights streamed from L2, included INSIDE
// fe_rollout_lstm_big_kernel (FE_LSTM_SAC_HEAD 0: tanh / clamp / value head, fe_lstm_kernel.h) and
// fe_rollout_sac_big_kernel (FE_LSTM_SAC_HEAD 1: the SAC actor's head, fe_sac_streamed_kernels.h).  Shared as source
// text, as fe_lstm_rollout_body.h is by the register-resident kernels and for the same reason: a function around the body
// moves scratch and spills in exactly this kernel (fe_lstm_stream_tile.h, NOTES.md).  Expects p (Params), r (LstmArgs),
// SINGLE, RTW and, with the SAC head, hd (SacArgs).
//
// The SAC head after the last time step (z = W_l h_W + b_l, then mu_layer / std_layer per pair, fe_lstm_kernel.h): h is
// single-buffered here, so there is no idle half to put z into.  Wavefront w computes the RTW / 4 row tiles
// (32 units each) w RTW / 4 .. of z from the LDS copy of h_W with W_l's fragments from L2 ([row tile][k group][lane][4],
// as pack_sac_weights stores them) -- one accumulator chain from zero per tile, k groups ascending, b_l added afterwards:
// the register-resident kernel's order -- keeps them in registers (c_t and the pending h_t are dead by then), passes a
// barrier, writes z over h_W and passes another; the pair's accounting lane then reduces z exactly as that kernel does.
    constexpr int H = 64 * RTW, HP = H + 4, SP = 32;
    extern __shared__ __align__(16) unsigned char smem[];
    const int A = SINGLE ? 1 : p.A;
    const int EB = p.EB;
    const int S = EB * A;
    const int W = p.W;
    const TileLds l = carve_lds(smem, EB, S);
    size_t off = (size_t)EB * 8 + (size_t)S * 8 + (size_t)S * 8 + (size_t)S * 4 + (size_t)S * 4 + (size_t)EB * 4;
    off = (off + 7) & ~(size_t)7;
    int64_t *l_idx = reinterpret_cast<int64_t *>(smem + off);
    off = (off + (size_t)EB * 8 + 15) & ~(size_t)15;
    float *s_h = reinterpret_cast<float *>(smem + off);  // [SP][HP]
    float *s_wout = s_h + (size_t)SP * HP;  // SAC: w_mu, then w_std, b_l and SacBigHeadLds
    const int tid = threadIdx.x;
    const int e = SINGLE ? tid : (int)fdiv((uint32_t)tid, p.div_A);
    const int a = SINGLE ? 0 : tid - e * A;
    const int lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, half = lane >> 5;
    const int64_t NA = p.N * A;
    const int64_t rstride = 4 * (int64_t)A;
    const int mt0 = wave * RTW;  // this wavefront's row tiles: mt0 .. mt0 + RTW - 1
    float4 wq[kLstmBigAhead][kLstmBigRI];  // weight fragments in flight (fe_lstm_stream_tile.h)
    bool primed = false;
    constexpr bool STASH = false;  // nothing goes to a workspace: the rows fe_lstm_stream_tile.h would write are null
    float *const grow = nullptr, *const crow = nullptr, *const hout = nullptr;
#if FE_LSTM_SAC_HEAD
    for (int i = tid; i < H; i += kLstmBlock) {
        s_wout[i] = hd.wmu[i];
        s_wout[H + i] = hd.wstd[i];
        s_wout[2 * H + i] = hd.bl[i];
    }
    // the head's scalars and pointers (W_l's among them) wait in LDS: as kernel arguments they would occupy SGPRs for the
    // whole launch, and the recurrence has none to spare (its SGPR spills cost VGPRs)
    if (tid == 0) *reinterpret_cast<SacBigHeadLds *>(s_wout + sac_big_head_lds_offset(H)) = {hd.stds_out, hd.logp_out, hd.wl, hd.bmu_p ? *hd.bmu_p : hd.bmu, hd.bstd_p ? *hd.bstd_p : hd.bstd};
#else
    for (int i = tid; i < H; i += kLstmBlock) s_wout[i] = r.wout[i];
#endif

    for (int64_t tile = blockIdx.x; tile < p.num_tiles; tile += gridDim.x) {
        const int64_t n0 = tile * EB;
        const int ebt = (p.N - n0) < (int64_t)EB ? (int)(p.N - n0) : EB;
        const bool active = e < ebt;
#if FE_LSTM_SAC_HEAD
        // (e is widened here, per tile: hoisted out of the tile loop its 64-bit copy is the one value this kernel spills)
        int et = e;
        asm volatile("" : "+v"(et));
        const int64_t n = n0 + et;
#else
        const int64_t n = n0 + e;
#endif
        const int64_t sl = n * A + a;
        SleeveReg st = rollout_load_state(p, active && !r.forward_only, n, sl);
        if (active) {
            const double pos0 = r.obs_pos[sl];
            l.pos[e * A + a] = pos0;
            if (a == 0) l.src[e] = r.obs_src[n];
            if (r.traj_src) {
                r.traj_pos[sl] = pos0;
                if (a == 0) r.traj_src[n] = r.obs_src[n];
            }
        }
        __syncthreads();  // also covers s_wout on the first tile
        const int pairs = ebt * A;
        for (int k = 0; k < r.K; ++k) {
            const int qc = col < pairs ? col : pairs - 1;
            const int ee = SINGLE ? qc : (int)fdiv((uint32_t)qc, p.div_A);
            const int aa = SINGLE ? 0 : qc - ee * A;
            const float *xsrc = r.lr32 + l.src[ee] + 4 * aa;
            const float4 xh = make_float4((float)l.pos[qc], 1.0f, 0.0f, 0.0f);
            float4 xc = half == 0 ? *reinterpret_cast<const float4 *>(xsrc) : xh;
            float cst[RTW][4], hnew[RTW][4];
#pragma unroll
            for (int i = 0; i < RTW; ++i)
#pragma unroll
                for (int b = 0; b < 4; ++b) cst[i][b] = 0.0f;
            for (int t = 0; t < W; ++t) {
                const int tn = t + 1 < W ? t + 1 : t;
                const float4 xn = half == 0 ? *reinterpret_cast<const float4 *>(xsrc + (int64_t)tn * rstride) : xh;
                const float *hrow = s_h + (size_t)col * HP + 4 * half;
                // a real loop over this wavefront's row-tile groups: c_t and the pending h_t (RTW x 4 floats each per lane,
                // touched once per 1040 MFMAs) are indexed dynamically, i.e. live in per-lane scratch, not in VGPRs
#define FE_LSTM_STREAM_ARGS r
#pragma unroll 1
                for (int i0 = 0; i0 < RTW; i0 += kLstmBigRI) {
#include "fe_lstm_stream_tile.h"
                }
#undef FE_LSTM_STREAM_ARGS
                lds_barrier();  // every wavefront has read h_{t-1}
#pragma unroll
                for (int i = 0; i < RTW; ++i)
                    *reinterpret_cast<float4 *>(s_h + (size_t)col * HP + 8 * (mt0 + i) + 4 * half) =
                        make_float4(hnew[i][0], hnew[i][1], hnew[i][2], hnew[i][3]);
                xc = xn;
                lds_barrier();  // h_t is complete
            }
            float act = 0.0f;
#if FE_LSTM_SAC_HEAD
            {
                // ---- SAC head: z = W_l h_W + b_l on the matrix cores, this wavefront's ZT row tiles together ----
                constexpr int ZT = RTW / 4, NGZ = H / 8;
                // the addresses below are loop-invariant: hoisted out of the step loop they would hold VGPRs through the
                // whole recurrence (and spill), so they derive from a thread index the compiler cannot see through
                int ztid = tid;
                asm volatile("" : "+v"(ztid));
                const int zl = ztid & 63, zcol = zl & 31, zhalf = zl >> 5, zt0 = (ztid >> 6) * ZT;  // (zt0 wavefront-uniform)
                const float4 *wlf = reinterpret_cast<const float4 *>(reinterpret_cast<const SacBigHeadLds *>(s_wout + sac_big_head_lds_offset(H))->wl) +
                                    ((size_t)zt0 * NGZ) * 64 + zl;
                const float *hrow = s_h + (size_t)zcol * HP + 4 * zhalf;
                f32x16 zacc[ZT];
#pragma unroll
                for (int i = 0; i < ZT; ++i)
#pragma unroll
                    for (int rr = 0; rr < 16; ++rr) zacc[i][rr] = 0.0f;
                float4 wv[ZT];
#pragma unroll
                for (int i = 0; i < ZT; ++i) wv[i] = wlf[(size_t)i * NGZ * 64];
#pragma unroll 2
                for (int g = 0; g < NGZ; ++g) {
                    const int gn = g + 1 < NGZ ? g + 1 : g;  // the next k group's fragments, one group ahead of their use
                    float4 wn[ZT];
#pragma unroll
                    for (int i = 0; i < ZT; ++i) wn[i] = wlf[((size_t)i * NGZ + gn) * 64];
                    const float4 hb = *reinterpret_cast<const float4 *>(hrow + 8 * g);
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        const float hs = m == 0 ? hb.x : (m == 1 ? hb.y : (m == 2 ? hb.z : hb.w));
#pragma unroll
                        for (int i = 0; i < ZT; ++i) {
                            const float ws = m == 0 ? wv[i].x : (m == 1 ? wv[i].y : (m == 2 ? wv[i].z : wv[i].w));
                            zacc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(ws, hs, zacc[i], 0, 0, 0);
                        }
                    }
#pragma unroll
                    for (int i = 0; i < ZT; ++i) wv[i] = wn[i];
                }
                lds_barrier();  // every wavefront has read h_W
                // zacc[i][4b + c] is unit 32 (zt0 + i) + 8 b + 4 half + c of pair col
                const float *s_bl = s_wout + 2 * H;
#pragma unroll
                for (int i = 0; i < ZT; ++i)
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int u0 = 32 * (zt0 + i) + 8 * b + 4 * zhalf;
                        float zv[4];
#pragma unroll
                        for (int c = 0; c < 4; ++c) zv[c] = zacc[i][4 * b + c] + s_bl[u0 + c];
                        *reinterpret_cast<float4 *>(s_h + (size_t)zcol * HP + u0) = make_float4(zv[0], zv[1], zv[2], zv[3]);
                    }
                lds_barrier();  // z is complete
                if (active) {
                    int zp = e * A + a;
                    asm volatile("" : "+v"(zp));  // (as above: the row address is not to be hoisted out of the step loop)
                    const float *zr = s_h + (size_t)zp * HP;
                    const float *s_wstd = s_wout + H;
                    const SacBigHeadLds hs = *reinterpret_cast<const SacBigHeadLds *>(s_wout + sac_big_head_lds_offset(H));
                    float mu = hs.bmu, q = hs.bstd;
#pragma unroll 4
                    for (int u = 0; u < H; ++u) {
                        mu = fmaf(s_wout[u], zr[u], mu);
                        q = fmaf(s_wstd[u], zr[u], q);
                    }
                    const float sd = q > 20.0f ? q : log1pf(expf(q));  // F.softplus (beta 1, threshold 20)
                    const int64_t o = (int64_t)k * NA + sl;
                    if (r.means_out) r.means_out[o] = mu;
                    if (hs.stds_out) hs.stds_out[o] = sd;
                    act = mu;  // the eval env, and every env without noise, acts on the un-squashed mean (SAC_agent.py:110-121)
                    if (r.noise && n != p.eval_env) {
                        const float u = mu + r.noise[o] * sd;  // Normal.rsample: loc + eps * scale
                        act = lstm_tanh(u);
                        if (hs.logp_out) {  // Normal.log_prob(u) - log(1 - tanh(u)^2 + 1e-7) (SAC/actor.py:51-61)
                            const float d = u - mu;
                            const float lp = -(d * d) / (2.0f * (sd * sd)) - logf(sd) - 0.918938533204672742f;
                            hs.logp_out[o] = lp - logf((1.0f - act * act) + 1e-7f);
                        }
                    }
                    if (r.actions_out) r.actions_out[o] = act;
                }
            }
#else
            // ---- output layer: the pair's accounting lane reduces its last hidden state ----
            if (active) {
                const float *hl = s_h + (size_t)(e * A + a) * HP;
                float o = r.bout_p ? *r.bout_p : r.bout;
#pragma unroll 8
                for (int u = 0; u < H; ++u) o = fmaf(s_wout[u], hl[u], o);
                act = r.out_act == 0 ? lstm_tanh(o) : (r.out_act == 2 ? o : (o < -1.0f ? -1.0f : (o > 1.0f ? 1.0f : o)));
                if (r.means_out) r.means_out[(int64_t)k * NA + sl] = act;
                if (r.noise && n != p.eval_env) {
                    const float dev = r.std * r.noise[(int64_t)k * NA + sl];
                    const float smp = act + dev;
                    act = smp < -1.0f ? -1.0f : (smp > 1.0f ? 1.0f : smp);
                }
                if (r.actions_out) r.actions_out[(int64_t)k * NA + sl] = act;
            }
#endif
            if (!r.forward_only) {  // (uniform)
                account_keep<SINGLE>(p, l, l_idx, A, e, a, active, n, st, act, r.rew_out + (int64_t)k * p.N,
                                     r.done_out + (int64_t)k * p.N);
                if (active && r.traj_src) {
                    r.traj_pos[(int64_t)(k + 1) * NA + sl] = l.pos[e * A + a];
                    if (a == 0) r.traj_src[(int64_t)(k + 1) * p.N + n] = l.src[e];
                }
            }
            lds_barrier();  // the new observation's descriptors are complete; everyone is done with h_W (and z)
        }
        if (!r.forward_only) {
            rollout_store_state(p, active, a, n, sl, st);
            if (active) {
                r.obs_pos[sl] = l.pos[e * A + a];
                if (a == 0) r.obs_src[n] = l.src[e];
            }
        }
        __syncthreads();
    }
