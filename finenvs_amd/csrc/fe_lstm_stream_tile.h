// fe_lstm_stream_tile.h -- part of fe_env.hip (one translation unit; see the overview there): one row-tile group of one
// time step of the LSTM recurrence at H = 256 / 512 / 1024 with the recurrent weights streamed from L2.  Program TEXT, not
// a header of declarations: it is the body of the loop `for (i0 = 0; i0 < RTW; i0 += kLstmBigRI)` of
// fe_rollout_lstm_big_kernel (fe_lstm_kernel.h) and of the tile loop that fe_lstm_sgrad_forward_kernel and
// fe_critic_sgrad_forward_kernel share (fe_lstm_stream_sgrad_body.h), included there as fe_lstm_rollout_body.h is by the
// register-resident kernels.  The same k order, activations and cell update in all three: the oracle function that
// pins the rollout pins the recomputed forward of the two backward passes bit for bit.
//
// Why text and not __device__ __forceinline__ stages: a callee is optimised before it is inlined, which changes what the
// compiler's alloca-to-vector promotion finds in the kernel.  With a gate-group and a cell function the H = 512 forms of
// all three kernels moved cst / hnew from scratch into indexed VGPRs (scratch 288 -> 32 .. 160 bytes per lane, 11 - 13
// VGPR spills in the two recomputing kernels); with the gate group alone fe_rollout_lstm_big_kernel<false, 4> went from
// 48 to 64 bytes and 4 to 8 spills; with the cell alone the two recomputing kernels moved at H = 512 again (stand-alone
// cross-compiles of the nine + six instantiations, NOTES.md).  Included text compiles to the parent's instructions.
//
// One workgroup (kLstmBlock threads, 8 wavefronts) runs grid-strided 32-pair tiles; wavefront w owns the RTW = H / 64
// gate-row tiles mt0 = w RTW .. mt0 + RTW - 1 and runs them kLstmBigRI at a time, this text once per group:
//   gates   kLstmBigRI accumulators from zero; the input part (K = 8: x_t, four MFMAs per row tile, wx from global
//           memory); for t > 0 the recurrent part, k groups ascending: the A fragments from the fragment-major whh
//           ([row tile][k group][lane][4], one coalesced KiB each) through the queue wq, kLstmBigAhead k groups ahead of
//           their MFMAs, the B fragment h_{t-1} from LDS ([pair][H + 4]), shared by the group's chains.  The queue is
//           primed ONCE per launch and never drains -- so wq and primed belong to the kernel, outside its tile loop;
//   cell    lstm_act2 on the accumulators (acc[i][4b + gate] is unit 8 mt + 4 half + b of pair col), c_t in cst[i0 + i]
//           and the pending h_t in hnew[i0 + i]: indexed by the group loop, i.e. per-lane scratch, touched once per
//           group.  With STASH (the backward's recompute) the activated gates, c_t and h_t also go to the workspace.
// The includer then passes a barrier (every wavefront has read h_{t-1}), copies hnew to LDS and passes another.
// It defines FE_LSTM_STREAM_ARGS, its argument block with .whh (fragment-major) and .wx (packed row order, 8 columns),
// and has in scope: RTW; `constexpr bool STASH` and grow / crow / hout = this lane's (t, pair) row of the gates, of c_t and
// of [h_t | ...] (the h_{t-1} of step t + 1, or h_W), each + 4 * half (null without STASH); i0, t; lane = tid & 63,
// col = lane & 31, half = lane >> 5, mt0 = (tid >> 6) * RTW;
// xc = the lane's B fragment of the input part (half 0: the row's four log-returns; half 1: position, 1, slot 6, 0);
// hrow = s_h + col * (H + 4) + 4 * half; float4 wq[kLstmBigAhead][kLstmBigRI]; bool primed; float cst[RTW][4], hnew[RTW][4].
constexpr int NG = 8 * RTW, RI = kLstmBigRI, AHEAD = kLstmBigAhead;
static_assert(RTW % RI == 0 && NG % AHEAD == 0, "row tiles / k groups must come in whole groups");
f32x16 acc[RI];
#pragma unroll
for (int i = 0; i < RI; ++i)
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) acc[i][rr] = 0.0f;
// input part: four MFMAs per row tile
float4 wxv[RI];
#pragma unroll
for (int i = 0; i < RI; ++i)
    wxv[i] = *reinterpret_cast<const float4 *>(FE_LSTM_STREAM_ARGS.wx + ((size_t)32 * (mt0 + i0 + i) + col) * 8 + 4 * half);
#pragma unroll
for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int i = 0; i < RI; ++i) {
        const float xs = m == 0 ? xc.x : (m == 1 ? xc.y : (m == 2 ? xc.z : xc.w));
        const float ws = m == 0 ? wxv[i].x : (m == 1 ? wxv[i].y : (m == 2 ? wxv[i].z : wxv[i].w));
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(ws, xs, acc[i], 0, 0, 0);
    }
if (t > 0) {
    // fragment-major weights: one coalesced KiB per (row tile, k group), AHEAD groups in flight -- across row-tile
    // groups, time steps, env steps and tiles too: the tail of one k loop already fetches the head of the next (the
    // next group's, or after the last group the first one's again: the matrix never changes)
    const float4 *wbase = reinterpret_cast<const float4 *>(FE_LSTM_STREAM_ARGS.whh) + lane;
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
#pragma unroll 1  // a real loop: unrolled, its hoisted loads spill (NG is up to 128 groups of 4 RI MFMAs)
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
    [[maybe_unused]] const int mt = mt0 + i0 + i;
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
