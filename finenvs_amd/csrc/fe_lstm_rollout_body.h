// fe_lstm_rollout_body.h -- part of fe_env.hip (one translation unit; see the overview there): the body of the
// register-resident LSTM rollout, included INSIDE fe_rollout_lstm_kernel (FE_LSTM_SAC_HEAD 0: tanh / clamp / value head),
// fe_rollout_sac_kernel (FE_LSTM_SAC_HEAD 1: the SAC actor's head), see fe_lstm_kernel.h, and fe_twin_q_kernel
// (FE_LSTM_CRITIC_HEAD 1: a twin critic's value on given descriptors and actions, see fe_critic_kernels.h; it also
// defines FE_LSTM_SAC_HEAD 0).  Shared as source text
// rather than as an inlined device function: a function boundary around the body -- its arguments taken by reference or
// by value -- changes how the kernel reads its argument block, and with it the register allocation of the LSTM kernels
// (their VGPR / scratch figures in tools/resource_usage.py moved either way).  Expects p (Params), r (LstmArgs),
// SINGLE, NT and, with the SAC head, hd (SacArgs), with the critic head, cq (CriticArgs).
    using G = LstmGeom<NT>;
    constexpr int H = G::H, HP = G::HP, MPW = G::MPW, NSPLIT = G::NSPLIT, MAXNT = G::MAXNT, NG = H / 8;
    constexpr int JB = MPW == 1 ? 2 : 1;  // column tiles processed together
    static_assert(MAXNT % JB == 0, "column tiles per wavefront must come in whole groups");
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
    float *s_h = reinterpret_cast<float *>(smem + off);  // [2][SP][HP]
    float *s_wout = s_h + 2 * (size_t)G::SP * HP;  // SAC: w_mu, then w_std, b_l and (sac_wl_in_lds) W_l
    const int tid = threadIdx.x;
    const int e = SINGLE ? tid : (int)fdiv((uint32_t)tid, p.div_A);
    const int a = SINGLE ? 0 : tid - e * A;
    const int lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, half = lane >> 5;
    const int64_t NA = p.N * A;
    const int64_t rstride = 4 * (int64_t)A;
    const int mt0 = NSPLIT == 1 ? wave * MPW : wave % G::MT;  // first gate-row tile of this wavefront
    const int nsub = NSPLIT == 1 ? 0 : wave / G::MT;          // its share of the column tiles

#if FE_LSTM_SAC_HEAD
    {  // the head's weights go to LDS before the recurrent weights fill the registers
        float *s_wstd = s_wout + H, *s_bl = s_wout + 2 * H;
        for (int i = tid; i < H; i += kLstmBlock) {
            s_wout[i] = hd.wmu[i];
            s_wstd[i] = hd.wstd[i];
            s_bl[i] = hd.bl[i];
        }
        if constexpr (sac_wl_in_lds<NT>()) {
            float4 *s_wl = reinterpret_cast<float4 *>(s_wout + 3 * H);
#pragma unroll 1
            for (int i = tid; i < H * H / 4; i += kLstmBlock) s_wl[i] = reinterpret_cast<const float4 *>(hd.wl)[i];
        }
        // the head's scalars and output pointers wait in LDS: as kernel arguments they would occupy SGPRs for the whole
        // launch, and the recurrence has none to spare (its SGPR spills cost VGPRs)
        if (tid == 0) *reinterpret_cast<SacHeadLds *>(s_wout + sac_head_lds_offset(H)) = {hd.stds_out, hd.logp_out, hd.bmu_p ? *hd.bmu_p : hd.bmu, hd.bstd_p ? *hd.bstd_p : hd.bstd};
    }
#endif
    // this wavefront's slice of the weights: A fragments, lane (row = lane & 31, k half = lane >> 5)
    float4 whh[MPW][NG], wx[MPW];
#pragma unroll
    for (int i = 0; i < MPW; ++i) {
        const size_t R = (size_t)32 * (mt0 + i) + col;
        wx[i] = *reinterpret_cast<const float4 *>(r.wx + R * 8 + 4 * half);
#pragma unroll
        for (int g = 0; g < NG; ++g) whh[i][g] = *reinterpret_cast<const float4 *>(r.whh + R * H + 8 * g + 4 * half);
    }
#if !FE_LSTM_SAC_HEAD
    for (int i = tid; i < H; i += kLstmBlock) s_wout[i] = r.wout[i];
#endif

    for (int64_t tile = blockIdx.x; tile < p.num_tiles; tile += gridDim.x) {
        const int64_t n0 = tile * EB;
        const int ebt = (p.N - n0) < (int64_t)EB ? (int)(p.N - n0) : EB;
        const bool active = e < ebt;
        const int64_t n = n0 + e;
        const int64_t sl = n * A + a;
#if FE_LSTM_CRITIC_HEAD
        // (A = 1: pair e is env e) the critic has no accounting: the sleeve field shr holds the pair's action
        if (active) critic_load_pair(cq, n, l.src + e, l.pos + e, l.shr + e);
        (void)sl, (void)l_idx, (void)NA;
#else
        SleeveReg st = rollout_load_state(p, active && !r.forward_only, n, sl);
        if (active) {
            const double pos0 = r.obs_pos[sl];
            l.pos[e * A + a] = pos0;
            if (a == 0) l.src[e] = r.obs_src[n];
            if (r.traj_src) {  // row 0: the state the first policy evaluation sees
                r.traj_pos[sl] = pos0;
                if (a == 0) r.traj_src[n] = r.obs_src[n];
            }
        }
#endif
        __syncthreads();  // also covers the head's weights on the first tile
        const int pairs = ebt * A;
        const int ntiles = (pairs + 31) / 32;
        for (int k = 0; k < r.K; ++k) {
            // ---- policy: W recurrent steps, every wavefront its gate rows for all of its column tiles ----
            const float *xsrc[MAXNT];
            float4 xh[MAXNT], xc[MAXNT];
            float cst[MPW][MAXNT][4];
#pragma unroll
            for (int j = 0; j < MAXNT; ++j) {
                const int q = (nsub + j * NSPLIT) * 32 + col;
                const int qc = q < pairs ? q : pairs - 1;
                const int ee = SINGLE ? qc : (int)fdiv((uint32_t)qc, p.div_A);
                const int aa = SINGLE ? 0 : qc - ee * A;
                xsrc[j] = r.lr32 + l.src[ee] + 4 * aa;
#if FE_LSTM_CRITIC_HEAD
                xh[j] = make_float4((float)l.pos[qc], 1.0f, l.shr[qc], 0.0f);  // slot 6: the action, the same in every row
#else
                xh[j] = make_float4((float)l.pos[qc], 1.0f, 0.0f, 0.0f);
#endif
                xc[j] = half == 0 ? *reinterpret_cast<const float4 *>(xsrc[j]) : xh[j];
#pragma unroll
                for (int i = 0; i < MPW; ++i)
#pragma unroll
                    for (int b = 0; b < 4; ++b) cst[i][j][b] = 0.0f;
            }
            for (int t = 0; t < W; ++t) {
                const float *hprev = s_h + (size_t)((t + 1) & 1) * G::SP * HP;
                float *hnext = s_h + (size_t)(t & 1) * G::SP * HP;
                float4 xn[MAXNT];
                const int tn = t + 1 < W ? t + 1 : t;  // the next step's rows, one step ahead of their use
#pragma unroll
                for (int j = 0; j < MAXNT; ++j)
                    xn[j] = half == 0 ? *reinterpret_cast<const float4 *>(xsrc[j] + (int64_t)tn * rstride) : xh[j];
                // keep the next time step's row loads up here (the scheduler otherwise sinks them towards their use): -6.5 % at
                // H = 128, -1 % at 64, +1.5 % at 32 (tools/fused_bench.py with FUSED_LIB=lstmpin)
                if constexpr (NT >= 2) __builtin_amdgcn_sched_barrier(0);
                // JB column tiles at a time: with MPW row tiles that is MPW * JB >= 2 independent accumulator chains,
                // so a dependent MFMA never waits for its predecessor's 16 passes
#pragma unroll
                for (int j0 = 0; j0 < MAXNT; j0 += JB) {
                    if (nsub + j0 * NSPLIT < ntiles) {  // (a trailing tile of the group past `pairs` computes on clamped rows)
                        f32x16 acc[MPW][JB];
#pragma unroll
                        for (int i = 0; i < MPW; ++i)
#pragma unroll
                            for (int jj = 0; jj < JB; ++jj)
#pragma unroll
                                for (int rr = 0; rr < 16; ++rr) acc[i][jj][rr] = 0.0f;
#pragma unroll
                        for (int m = 0; m < 4; ++m)
#pragma unroll
                            for (int i = 0; i < MPW; ++i)
#pragma unroll
                                for (int jj = 0; jj < JB; ++jj) {
                                    const float4 xv = xc[j0 + jj];
                                    const float xs = m == 0 ? xv.x : (m == 1 ? xv.y : (m == 2 ? xv.z : xv.w));
                                    const float ws = m == 0 ? wx[i].x : (m == 1 ? wx[i].y : (m == 2 ? wx[i].z : wx[i].w));
                                    acc[i][jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(ws, xs, acc[i][jj], 0, 0, 0);
                                }
                        if (t > 0) {
#pragma unroll
                            for (int g = 0; g < NG; ++g) {
                                float4 hb[JB];
#pragma unroll
                                for (int jj = 0; jj < JB; ++jj)
                                    hb[jj] = *reinterpret_cast<const float4 *>(
                                        hprev + (size_t)(32 * (nsub + (j0 + jj) * NSPLIT) + col) * HP + 4 * half + 8 * g);
#pragma unroll
                                for (int m = 0; m < 4; ++m)
#pragma unroll
                                    for (int i = 0; i < MPW; ++i)
#pragma unroll
                                        for (int jj = 0; jj < JB; ++jj) {
                                            const float4 wv = whh[i][g];
                                            const float ws = m == 0 ? wv.x : (m == 1 ? wv.y : (m == 2 ? wv.z : wv.w));
                                            const float hs = m == 0 ? hb[jj].x : (m == 1 ? hb[jj].y : (m == 2 ? hb[jj].z : hb[jj].w));
                                            acc[i][jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(ws, hs, acc[i][jj], 0, 0, 0);
                                        }
                            }
                        }
                        // cell update, in-lane: acc[i][jj][4b + gate] belongs to unit 8 (mt0 + i) + 4 half + b
#pragma unroll
                        for (int i = 0; i < MPW; ++i)
#pragma unroll
                            for (int jj = 0; jj < JB; ++jj) {
                                const int j = j0 + jj;
                                float hv[4], og[4];
#pragma unroll
                                for (int b = 0; b < 4; ++b) {
                                    const v2f sif = lstm_act2<false, false>((v2f){acc[i][jj][4 * b + 0], acc[i][jj][4 * b + 1]});
                                    const v2f tgo = lstm_act2<true, false>((v2f){acc[i][jj][4 * b + 2], acc[i][jj][4 * b + 3]});
                                    const float t1 = sif.y * cst[i][j][b];
                                    const float t2 = sif.x * tgo.x;
                                    cst[i][j][b] = t1 + t2;
                                    og[b] = tgo.y;
                                }
#pragma unroll
                                for (int b = 0; b < 4; b += 2) {
                                    const v2f tc = lstm_act2<true, true>((v2f){cst[i][j][b], cst[i][j][b + 1]});
                                    hv[b] = og[b] * tc.x;
                                    hv[b + 1] = og[b + 1] * tc.y;
                                }
                                *reinterpret_cast<float4 *>(hnext + (size_t)(32 * (nsub + j * NSPLIT) + col) * HP + 8 * (mt0 + i) + 4 * half) =
                                    make_float4(hv[0], hv[1], hv[2], hv[3]);
                            }
                    }
                }
#pragma unroll
                for (int j = 0; j < MAXNT; ++j) xc[j] = xn[j];
                lds_barrier();  // h_t is complete
            }
            float act = 0.0f;
#if FE_LSTM_SAC_HEAD
            {
                // ---- SAC head: z = W_l h_W + b_l on the matrix cores, into the idle h buffer ----
                constexpr int ZT = H / 32;                          // z row tiles
                const float *hW = s_h + (size_t)((W - 1) & 1) * G::SP * HP;
                float *zb = s_h + (size_t)(W & 1) * G::SP * HP;
                // the tiling and addresses below are loop-invariant: hoisted out of the step loop they would hold VGPRs
                // through the whole recurrence (and spill), so they derive from a thread index the compiler cannot see through
                int ztid = tid;
                asm volatile("" : "+v"(ztid));
                const int zl = ztid & 63, zcol = zl & 31, zhalf = zl >> 5;
                const int zt = (ztid >> 6) % ZT, ct = (ztid >> 6) / ZT;  // (wavefront-uniform)
                if (ct < G::SP / 32 && ct < ntiles) {
                    const float4 *wf = (sac_wl_in_lds<NT>() ? reinterpret_cast<const float4 *>(s_wout + 3 * H)
                                                            : reinterpret_cast<const float4 *>(hd.wl)) +
                                       (size_t)zt * NG * 64 + zl;
                    const float *hrow = hW + (size_t)(32 * ct + zcol) * HP + 4 * zhalf;
                    f32x16 acc;
#pragma unroll
                    for (int rr = 0; rr < 16; ++rr) acc[rr] = 0.0f;
#pragma unroll 2
                    for (int g = 0; g < NG; ++g) {
                        const float4 wv = wf[(size_t)g * 64];
                        const float4 hb = *reinterpret_cast<const float4 *>(hrow + 8 * g);
#pragma unroll
                        for (int m = 0; m < 4; ++m) {
                            const float ws = m == 0 ? wv.x : (m == 1 ? wv.y : (m == 2 ? wv.z : wv.w));
                            const float hs = m == 0 ? hb.x : (m == 1 ? hb.y : (m == 2 ? hb.z : hb.w));
                            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ws, hs, acc, 0, 0, 0);
                        }
                    }
                    // acc[4b + c] is unit 32 zt + 8 b + 4 half + c of pair 32 ct + col
                    const float *s_bl = s_wout + 2 * H;
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int u0 = 32 * zt + 8 * b + 4 * zhalf;
                        float zv[4];
#pragma unroll
                        for (int c = 0; c < 4; ++c) zv[c] = acc[4 * b + c] + s_bl[u0 + c];
                        *reinterpret_cast<float4 *>(zb + (size_t)(32 * ct + zcol) * HP + u0) = make_float4(zv[0], zv[1], zv[2], zv[3]);
                    }
                }
                lds_barrier();  // z is complete
                if (active) {
                    const float *zr = zb + (size_t)(e * A + a) * HP;
                    const float *s_wstd = s_wout + H;
                    const SacHeadLds hs = *reinterpret_cast<const SacHeadLds *>(s_wout + sac_head_lds_offset(H));
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
#elif FE_LSTM_CRITIC_HEAD
            // ---- the critic's value, Linear(H, 1) + Identity: the LSTM head's reduction with out_act 2 ----
            if (active) {
                const float *hl = s_h + (size_t)((W - 1) & 1) * G::SP * HP + (size_t)(e * A + a) * HP;
                float o = *cq.net[blockIdx.y].bout;
#pragma unroll 8
                for (int u = 0; u < H; ++u) o = fmaf(s_wout[u], hl[u], o);
                critic_store(cq, n, o);
            }
            (void)act;
#else
            // ---- output layer: the pair's accounting lane reduces its last hidden state ----
            if (active) {
                const float *hl = s_h + (size_t)((W - 1) & 1) * G::SP * HP + (size_t)(e * A + a) * HP;
                float o = r.bout_p ? *r.bout_p : r.bout;
#pragma unroll 8
                for (int u = 0; u < H; ++u) o = fmaf(s_wout[u], hl[u], o);
                act = r.out_act == 0 ? lstm_tanh(o) : (r.out_act == 2 ? o : (o < -1.0f ? -1.0f : (o > 1.0f ? 1.0f : o)));
                if (r.means_out) r.means_out[(int64_t)k * NA + sl] = act;
                if (r.noise && n != p.eval_env) {  // distribution.sample() clamped; the eval env keeps the mean
                    const float dev = r.std * r.noise[(int64_t)k * NA + sl];
                    const float smp = act + dev;
                    act = smp < -1.0f ? -1.0f : (smp > 1.0f ? 1.0f : smp);
                }
                if (r.actions_out) r.actions_out[(int64_t)k * NA + sl] = act;
            }
#endif
#if !FE_LSTM_CRITIC_HEAD
            if (!r.forward_only) {  // (uniform)
                account_keep<SINGLE>(p, l, l_idx, A, e, a, active, n, st, act, r.rew_out + (int64_t)k * p.N,
                                     r.done_out + (int64_t)k * p.N);
                if (active && r.traj_src) {  // row k + 1: the observation this step returns (own LDS entries: no barrier needed)
                    r.traj_pos[(int64_t)(k + 1) * NA + sl] = l.pos[e * A + a];
                    if (a == 0) r.traj_src[(int64_t)(k + 1) * p.N + n] = l.src[e];
                }
            }
#endif
            lds_barrier();  // the new observation's descriptors are complete; everyone is done with h_W (and z)
        }
#if !FE_LSTM_CRITIC_HEAD
        if (!r.forward_only) {
            rollout_store_state(p, active, a, n, sl, st);  // state and descriptors go back to HBM once per launch
            if (active) {
                r.obs_pos[sl] = l.pos[e * A + a];
                if (a == 0) r.obs_src[n] = l.src[e];
            }
        }
#endif
        __syncthreads();
    }
