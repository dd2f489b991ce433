// fe_replay_kernels.h -- part of fe_env.hip (one translation unit; see the overview there): the off-policy replay ring
// of include/finenvs_amd_replay.h.  States are kept as observation descriptors (obs_src, obs_pos) and rendered only
// when a minibatch is sampled.
#pragma once
#include "fe_device_common.h"
#include "fe_step_kernel.h"

namespace {

// Device view of a ring of C transitions (struct fe_replay_ring), SoA
struct ReplayRing {
    int64_t *s_src;   // (C)     state descriptor: window offset into the log-return table
    double *s_pos;    // (C, A)  state descriptor: position feature
    int64_t *n_src;   // (C)     next-state descriptor
    double *n_pos;    // (C, A)
    float *act;       // (C, A)
    float *rew;       // (C)     (float) of the f64 reward: the reference's .float()
    float *done;      // (C)     (float) of the int32 done flag
    int64_t C;
    int32_t A;
};

// The ring's cursor in device memory (struct fe_replay_cursor of include/finenvs_amd_replay_cursor.h) as int64 words.
constexpr int kCursorHead = 0, kCursorSize = 1, kCursorDraws = 2, kCursorTicket = 3;

// Where logical index 0 lives and how many indices there are, by value (cursor == null) or from the cursor: the address is
// the same in every lane, so these are two scalar loads.  A launch that reads the cursor is ordered after the append that
// wrote it by the stream.
__device__ __forceinline__ void ring_window(const int64_t *__restrict__ cursor, int64_t C, int64_t &start, int64_t &size) {
    if (cursor) {
        size = cursor[kCursorSize];
        start = cursor[kCursorHead] - size;
        if (start < 0) start += C;
    }
}

// Append `count` transitions j = first .. first + count - 1 of a step-major source (j = t * N + n, source element
// e = t * ld + n) to ring slots (head + j - first) mod C.  One lane per (transition, asset); f64 actions are cast to f32.
// With a cursor (fe_replay_append_c) one thread then writes the ring's new head and size into it.
template <bool SINGLE, bool ACT_F64>
__global__ __launch_bounds__(kBlock) void fe_replay_append_kernel(const ReplayRing r, int64_t head, int64_t first,
                                                                  int64_t count, int64_t N, int64_t ld,
                                                                  const int64_t *__restrict__ s_src,
                                                                  const double *__restrict__ s_pos,
                                                                  const int64_t *__restrict__ n_src,
                                                                  const double *__restrict__ n_pos,
                                                                  const void *__restrict__ actions,
                                                                  const double *__restrict__ rewards,
                                                                  const int32_t *__restrict__ dones,
                                                                  int64_t *__restrict__ cursor, int64_t new_size) {
    const int A = SINGLE ? 1 : r.A;
    const int64_t total = count * A;
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int64_t k = SINGLE ? i : i / A;  // transition within this append
        const int a = SINGLE ? 0 : (int)(i - k * A);
        const int64_t j = first + k;
        const int64_t t = j / N;
        const int64_t e = t * ld + (j - t * N);  // source element of (step t, env n)
        int64_t slot = head + k;
        if (slot >= r.C) slot -= r.C;  // head < C and count <= C
        const int64_t ea = e * A + a, sa = slot * A + a;
        r.s_pos[sa] = s_pos[ea];
        r.n_pos[sa] = n_pos[ea];
        if constexpr (ACT_F64) r.act[sa] = (float)reinterpret_cast<const double *>(actions)[ea];
        else r.act[sa] = reinterpret_cast<const float *>(actions)[ea];
        if (a == 0) {
            r.s_src[slot] = s_src[e];
            r.n_src[slot] = n_src[e];
            r.rew[slot] = (float)rewards[e];
            r.done[slot] = (float)dones[e];
        }
    }
    if (cursor && blockIdx.x == 0 && threadIdx.x == 0) {  // after this thread's transitions; nobody reads it in this launch
        int64_t h = head + count;
        if (h >= r.C) h -= r.C;
        cursor[kCursorHead] = h;
        cursor[kCursorSize] = new_size;
    }
}

// Bytes of one descriptor tile (src[EB] + pos[EB * A]) in LDS.
__host__ __device__ inline size_t replay_tile_bytes(int EB, int A) {
    return ((size_t)EB * 8 + (size_t)EB * A * 8 + 15) & ~(size_t)15;
}
__host__ __device__ inline size_t replay_lds_bytes(int EB, int A) { return 4 * (size_t)kStageBytes + 2 * replay_tile_bytes(EB, A); }

// Minibatch of p.N logical indices, as f32: states / next_states (B, W, 5A) through stream_tile (the render kernel's
// phase 2), actions (B, A), rewards (B), dones (B).  Logical index i in [0, size) is ring slot (start + i) mod C.  An
// index outside [0, size) reads nothing of the ring: its rows are NaN and it counts into errors[0].  With a cursor
// (fe_replay_sample_c) start and size are the cursor's.
template <int VEC, bool SINGLE>
__global__ __launch_bounds__(kBlock) void fe_replay_sample_kernel(const Params p, const ReplayRing r,
                                                                  const int64_t *__restrict__ indices, int64_t start,
                                                                  int64_t size, float *states, float *next_states,
                                                                  float *actions, float *rewards, float *dones,
                                                                  unsigned long long *errors,
                                                                  const int64_t *__restrict__ cursor) {
    extern __shared__ __align__(16) unsigned char smem[];
    ring_window(cursor, r.C, start, size);
    const int A = SINGLE ? 1 : p.A;
    const int EB = p.EB;
    const TileLds ls = carve_lds(smem + 4 * kStageBytes, EB, EB * A);
    const TileLds ln = carve_lds(smem + 4 * kStageBytes + replay_tile_bytes(EB, A), EB, EB * A);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    float *stage = reinterpret_cast<float *>(smem + wave * kStageBytes);
    const float qnan = __builtin_nanf("");
    const int64_t elems = p.env_elems;
    for (int64_t tile = blockIdx.x; tile < p.num_tiles; tile += gridDim.x) {
        const int64_t b0 = tile * EB;
        const int ebt = (p.N - b0) < (int64_t)EB ? (int)(p.N - b0) : EB;
        // gather through the index map: descriptors into LDS, the scalar fields straight to their outputs
        int bad = 0;
        for (int i = tid; i < ebt; i += kBlock) {
            const int64_t k = indices[b0 + i];
            const bool ok = k >= 0 && k < size;
            int64_t slot = start + (ok ? k : 0);
            if (slot >= r.C) slot -= r.C;
            ls.src[i] = ok ? r.s_src[slot] : 0;  // offset 0: a valid window, overwritten by NaN below
            ln.src[i] = ok ? r.n_src[slot] : 0;
            rewards[b0 + i] = ok ? r.rew[slot] : qnan;
            dones[b0 + i] = ok ? r.done[slot] : qnan;
            if (!ok) {
                atomicAdd(errors, 1ull);
                bad = 1;
            }
        }
        for (int i = tid; i < ebt * A; i += kBlock) {
            const int e = SINGLE ? i : i / A;
            const int64_t k = indices[b0 + e];
            const bool ok = k >= 0 && k < size;
            int64_t slot = start + (ok ? k : 0);
            if (slot >= r.C) slot -= r.C;
            const int64_t sa = slot * A + (i - e * A);
            ls.pos[i] = ok ? r.s_pos[sa] : (double)qnan;
            ln.pos[i] = ok ? r.n_pos[sa] : (double)qnan;
            actions[b0 * A + i] = ok ? r.act[sa] : qnan;
        }
        __syncthreads();
        const int tile_bad = __syncthreads_or(bad);
        stream_tile<float, VEC, SINGLE>(p, ls, stage, A, ebt, states + b0 * elems, lane, wave);
        stream_tile<float, VEC, SINGLE>(p, ln, stage, A, ebt, next_states + b0 * elems, lane, wave);
        if (tile_bad) {  // argument-error path: the tile's observation stores complete before NaN overwrites its bad rows
            __threadfence();
            __syncthreads();
            for (int64_t i = tid; i < (int64_t)ebt * elems; i += kBlock) {
                const int64_t e = i / elems;
                const int64_t k = indices[b0 + e];
                if (k < 0 || k >= size) {
                    states[b0 * elems + i] = qnan;
                    next_states[b0 * elems + i] = qnan;
                }
            }
        }
        __syncthreads();  // the next tile's gather overwrites the descriptors
    }
}

}  // namespace
