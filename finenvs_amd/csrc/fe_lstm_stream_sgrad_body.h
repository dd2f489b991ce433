// fe_lstm_stream_sgrad_body.h -- part of fe_env.hip (one translation unit; see the overview there): the whole body of
// fe_lstm_sgrad_forward_kernel<RTW> (FE_LSTM_STREAM_ACTION 0; argument block `g`, a LstmSGradArgs) and of
// fe_critic_sgrad_forward_kernel<RTW, STASH> (FE_LSTM_STREAM_ACTION 1; argument block `a`, a CriticSGradArgs), included by
// both as program text (why text: fe_lstm_stream_tile.h).  The recurrence of fe_rollout_lstm_big_kernel, forward only, one
// asset, over the g.pp / 32 tiles of a chunk; one 32-pair tile per workgroup at a time, c_t and the pending h_t in
// per-lane scratch, as there.
//   STASH    (the head: always) per (t, pair): the activated gates in packed row order, c_t and
//            [h_{t-1} | x_t | 1 | action | 0 ...] into the workspace, h_W beside them; without it nothing is written there
//            and h_W is reduced to q_c as fe_rollout_lstm_big_kernel's accounting lane does (bout from the device);
//   ACTION   the action in input slot 6 (xh.z and column 6 of the stash row), descriptors from given arrays or from the
//            replay ring by logical index, TD3's smoothing applied as the action is loaded, s_act / s_ok in LDS.  The head
//            compiles its own statements, not these with a zero (the lesson of bptt_stash_inputs, fe_bptt_tile.h).
// LDS: src [32] | pos [32] | (ACTION: action [32] | ring index in range [32]) | h [32][H + 4].
constexpr int H = 64 * RTW, HP = H + 4, G4 = 4 * H, VN = H + 32;
extern __shared__ __align__(16) unsigned char smem[];
int64_t *s_src = reinterpret_cast<int64_t *>(smem);      // [32]
float *s_pos = reinterpret_cast<float *>(s_src + 32);    // [32]
#if FE_LSTM_STREAM_ACTION
const LstmSGradArgs &g = a.g;
float *s_act = s_pos + 32;                               // [32]
int *s_ok = reinterpret_cast<int *>(s_act + 32);         // [32] the ring index was in range
float *s_h = s_act + 64;                                 // [32][HP]
#else
constexpr bool STASH = true;
float *s_h = s_pos + 32;                                 // [32][HP]
#endif
const int W = g.W;
const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
const int mt0 = wave * RTW;  // this wavefront's row tiles: mt0 .. mt0 + RTW - 1
const int64_t pp = g.pp, num_tiles = pp / 32;
float4 wq[kLstmBigAhead][kLstmBigRI];  // weight fragments in flight (fe_lstm_stream_tile.h)
bool primed = false;

for (int64_t tile = blockIdx.x; tile < num_tiles; tile += gridDim.x) {
    const int64_t n0 = tile * 32;
    const int pairs = g.cnt - n0 < 32 ? (int)(g.cnt - n0) : 32;
    if (tid < 32) {  // a pair past the batch computes on the last one's descriptor (its upstream gradient is zero)
        const int64_t n = n0 + (tid < pairs ? tid : pairs - 1);
#if FE_LSTM_STREAM_ACTION
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
#else
        s_src[tid] = g.obs_src[n];
        s_pos[tid] = (float)g.obs_pos[n];
#endif
    }
    __syncthreads();
    if constexpr (STASH) {
        for (int i = tid; i < W * 32 * 32; i += kLstmBlock) {  // x_t into the stash
            const int t = i >> 10, p = (i >> 5) & 31, j = i & 31;
#if FE_LSTM_STREAM_ACTION
            const float v = j < 4 ? g.lr32[s_src[p] + 4 * t + j]
                                  : (j == 4 ? s_pos[p] : (j == 5 ? 1.0f : (j == 6 ? s_act[p] : 0.0f)));
#else
            const float v = j < 4 ? g.lr32[s_src[p] + 4 * t + j] : (j == 4 ? s_pos[p] : (j == 5 ? 1.0f : 0.0f));
#endif
            g.vst[((int64_t)t * pp + n0 + p) * VN + H + j] = v;
        }
        for (int i = tid; i < 32 * H; i += kLstmBlock) g.vst[(n0 + i / H) * VN + i % H] = 0.0f;  // h_{-1}
    }

    const float *xsrc = g.lr32 + s_src[col];
#if FE_LSTM_STREAM_ACTION
    const float4 xh = make_float4(s_pos[col], 1.0f, s_act[col], 0.0f);
#else
    const float4 xh = make_float4(s_pos[col], 1.0f, 0.0f, 0.0f);
#endif
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
        // a real loop over the row-tile groups: cst and hnew are indexed dynamically (per-lane scratch, not VGPRs)
#define FE_LSTM_STREAM_ARGS g
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
#if FE_LSTM_STREAM_ACTION
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
#endif
    __syncthreads();  // the descriptors and h are free for the next tile
}
