// fe_ring_draw_kernels.h -- part of fe_env.hip (one translation unit; see the overview there): a mini-batch drawn and
// gathered from the replay ring's device cursor (include/finenvs_amd_replay_cursor.h), so that a captured update
// iteration follows the ring between its replays.
#pragma once
#include "fe_device_common.h"
#include "fe_replay_kernels.h"

namespace {

struct RingDrawArgs {
    ReplayRing r;
    unsigned long long *errors;  // ring->errors
    int64_t *cursor;             // head, size, draws, ticket (kCursor*)
    uint64_t seed;
    int64_t count;
    int64_t *idx;                // (count) the logical indices drawn
    int64_t *s_src;              // the gathered fields, each null or (count) / (count, A)
    double *s_pos;
    int64_t *n_src;
    double *n_pos;
    float *act, *rew, *done;
};

// Sample b of the launch is logical index (philox_u32(seed, draws + b) * size) >> 32 -- redraw_day's multiply-shift on
// the env's generator -- and lives in slot (head - size + index) mod C.  One lane per (sample, asset), as the append.
//
// head, size and draws come from the cursor.  draws must advance by count once per launch and no workgroup may see the
// advanced value, whenever it starts: thread 0 of every workgroup reads the cursor and publishes it through LDS, and
// after its own elements takes a ticket; the holder of the last ticket -- every workgroup's thread 0 has read by then,
// and nobody else reads -- writes draws + count and resets the ticket (fe_net_update_kernel's pattern for its beta
// powers).  The ticket is the only atomic.  A cursor that describes no sample (size outside [1, C], head outside [0, C))
// reads nothing of the ring: index -1, NaN fields (descriptor offsets 0), and count added to errors[0] by that same
// last thread.
__global__ __launch_bounds__(kBlock) void fe_ring_draw_kernel(const RingDrawArgs d) {
    __shared__ int64_t cur[3];
    if (threadIdx.x == 0) {
        const volatile int64_t *c = d.cursor;
        cur[0] = c[kCursorHead];
        cur[1] = c[kCursorSize];
        cur[2] = c[kCursorDraws];
    }
    __syncthreads();
    const int64_t C = d.r.C, head = cur[0], size = cur[1];
    const uint64_t draws = (uint64_t)cur[2];
    const bool ok = size >= 1 && size <= C && head >= 0 && head < C;
    int64_t start = head - size;
    if (start < 0) start += C;
    const int A = d.r.A;
    const int64_t total = d.count * A;
    const float qnan = __builtin_nanf("");
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int64_t b = A == 1 ? i : i / A;
        const int a = A == 1 ? 0 : (int)(i - b * A);
        int64_t k = -1, slot = 0;
        if (ok) {
            k = (int64_t)(((uint64_t)philox_u32(d.seed, draws + (uint64_t)b) * (uint64_t)size) >> 32);  // < size
            slot = start + k;
            if (slot >= C) slot -= C;
        }
        const int64_t sa = slot * A + a;
        if (d.s_pos) d.s_pos[i] = ok ? d.r.s_pos[sa] : (double)qnan;
        if (d.n_pos) d.n_pos[i] = ok ? d.r.n_pos[sa] : (double)qnan;
        if (d.act) d.act[i] = ok ? d.r.act[sa] : qnan;
        if (a == 0) {
            d.idx[b] = k;
            if (d.s_src) d.s_src[b] = ok ? d.r.s_src[slot] : 0;
            if (d.n_src) d.n_src[b] = ok ? d.r.n_src[slot] : 0;
            if (d.rew) d.rew[b] = ok ? d.r.rew[slot] : qnan;
            if (d.done) d.done[b] = ok ? d.r.done[slot] : qnan;
        }
    }
    if (threadIdx.x == 0) {
        __threadfence();
        unsigned int *ticket = reinterpret_cast<unsigned int *>(d.cursor + kCursorTicket);
        if (atomicAdd(ticket, 1u) == gridDim.x - 1) {
            d.cursor[kCursorDraws] = (int64_t)(draws + (uint64_t)d.count);
            if (!ok) *d.errors += (unsigned long long)d.count;
            *ticket = 0u;
        }
    }
}

}  // namespace
