// fe_ppo_kernels.h -- part of fe_env.hip (one translation unit; see the overview there): the device side of a PPO
// update's mini-batch loop (include/finenvs_amd_ppo.h) -- a mini-batch drawn from a keyed permutation and gathered from
// the trajectory chunk, the epoch counter, and the two losses with their gradients.
#pragma once
#include "fe_device_common.h"

namespace {

constexpr int kPpoCursorEpoch = 0, kPpoCursorErrors = 1;  // FE_PPO_CURSOR_*
constexpr int kPpoMaxColumns = 4;                          // FE_PPO_MAX_COLUMNS
constexpr int kPpoLossMaxGrid = kBlock;                    // workgroups of a loss launch: their partials are one tile of the last one

struct PpoMinibatchArgs {
    const int64_t *obs_src;   // (T + 1, C)
    const double *obs_pos;    // (T + 1, C, A)
    const float *actions;     // (T, C, A)
    const float *col[kPpoMaxColumns];  // (T, N) each, or null
    float *col_out[kPpoMaxColumns];    // (B) each, or null
    int64_t *cursor;          // epoch, errors (kPpoCursor*)
    uint64_t key;             // seed ^ FE_PPO_PERM_SALT
    int64_t epoch_offset;
    int64_t T, N, C;
    int64_t n;                // T * N < 2^32
    int64_t first;            // m * B: the mini-batch's first position
    int64_t B;
    int32_t A;
    int32_t hb;               // half the bits of the Feistel domain
    int64_t *idx;             // (B)
    int64_t *src_out;         // (B) or null
    double *pos_out;          // (B, A) or null
    float *act_out;           // (B, A) or null
};

// One pass of the four-round balanced Feistel network over the 2 * hb bits of x, keyed by (key, epoch).
__device__ __forceinline__ uint32_t ppo_feistel_pass(uint64_t key, uint64_t epoch4, int hb, uint32_t mask, uint32_t x) {
    uint32_t l = x >> hb, r = x & mask;
#pragma unroll
    for (int round = 0; round < 4; ++round) {
        const uint32_t f = philox_u32(key, ((epoch4 + (uint64_t)round) << 16) | (uint64_t)r) & mask;
        const uint32_t t = l ^ f;
        l = r;
        r = t;
    }
    return (l << hb) | r;
}

// pi_epoch(p) by cycle walking, or -1 if the walk did not come back below n within the domain's size (it always
// does: the pass is a bijection of the domain, so p's cycle returns to p < n after at most that many passes).
__device__ __forceinline__ int64_t ppo_permute(uint64_t key, uint64_t epoch, int hb, uint64_t n, uint64_t p) {
    const uint32_t mask = (1u << hb) - 1u;
    const uint64_t domain = (uint64_t)1 << (2 * hb);
    uint32_t x = (uint32_t)p;
    for (uint64_t pass = 0; pass < domain; ++pass) {
        x = ppo_feistel_pass(key, epoch * 4u, hb, mask, x);
        if ((uint64_t)x < n) return (int64_t)x;
    }
    return -1;
}

// One lane per (sample, asset), as the ring draw.  The epoch is read from the cursor by every lane: nothing in this
// launch writes it (fe_ppo_epochs_advance is a launch of its own, after the last gather of a train()).
__global__ __launch_bounds__(kBlock) void fe_ppo_minibatch_kernel(const PpoMinibatchArgs d) {
    const uint64_t epoch = (uint64_t)(d.cursor[kPpoCursorEpoch] + d.epoch_offset);
    const int A = d.A;
    const int64_t total = d.B * A;
    const float qnan = __builtin_nanf("");
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int64_t b = A == 1 ? i : i / A;
        const int a = A == 1 ? 0 : (int)(i - b * A);
        const int64_t s = ppo_permute(d.key, epoch, d.hb, (uint64_t)d.n, (uint64_t)(d.first + b));
        const bool ok = s >= 0;
        const int64_t env = ok ? s / d.T : 0, step = ok ? s % d.T : 0;
        const int64_t row = step * d.C + env;
        if (d.pos_out) d.pos_out[i] = ok ? d.obs_pos[row * A + a] : (double)qnan;
        if (d.act_out) d.act_out[i] = ok ? d.actions[row * A + a] : qnan;
        if (a == 0) {
            d.idx[b] = s;
            if (d.src_out) d.src_out[b] = ok ? d.obs_src[row] : 0;
#pragma unroll
            for (int c = 0; c < kPpoMaxColumns; ++c)
                if (d.col_out[c]) d.col_out[c][b] = ok ? d.col[c][step * d.N + env] : qnan;
            if (!ok) atomicAdd(reinterpret_cast<unsigned long long *>(d.cursor + kPpoCursorErrors), 1ull);
        }
    }
}

__global__ void fe_ppo_epochs_advance_kernel(int64_t *cursor, int64_t count) {
    if (blockIdx.x == 0 && threadIdx.x == 0) cursor[kPpoCursorEpoch] = cursor[kPpoCursorEpoch] + count;
}

// ---- the losses ----
//
// Both launches sum per-sample terms (the loss; the actor's d loss / d log_std) over the batch.  Every thread adds its
// grid-strided samples in index order, the workgroup adds its threads in a binary tree through LDS, thread 0 stores the
// workgroup's partial sums and takes an integer ticket; the workgroup that holds the last ticket adds the partials in
// the same tree and writes the results.  The order of every addition is a function of (count, grid) alone, and no float
// atomic is involved: the same inputs give the same bits.  The ticket is the first 8 bytes of the workspace (zero
// between launches), the partials follow as [workgroup][2].

struct PpoLossArgs {
    const float *x;        // actor: means; value: values
    const float *log_std;  // actor only
    const float *actions;  // actor only
    const float *old_lp;   // actor only
    const float *y;        // actor: advantages; value: returns
    int64_t count;
    double lo, hi;         // 1 -/+ clip_epsilon
    double ent_coef;
    float *loss;
    float *g_x;            // (count)
    float *g_log_std;      // actor only
    double *ws;
};

// Adds v0 / v1 over the workgroup (result valid in thread 0).
__device__ __forceinline__ void ppo_block_sum(double (&s)[2][kBlock], double &v0, double &v1) {
    const int t = threadIdx.x;
    s[0][t] = v0;
    s[1][t] = v1;
    __syncthreads();
#pragma unroll
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if (t < w) {
            s[0][t] += s[0][t + w];
            s[1][t] += s[1][t + w];
        }
        __syncthreads();
    }
    v0 = s[0][0];
    v1 = s[1][0];
    __syncthreads();
}

// The cross-workgroup half of the reduction; true in thread 0 of the one workgroup that ends up holding the totals.
__device__ __forceinline__ bool ppo_grid_sum(double *ws, double (&s)[2][kBlock], double &v0, double &v1) {
    __shared__ bool last;
    unsigned int *ticket = reinterpret_cast<unsigned int *>(ws);
    double *part = ws + 1;
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = v0;
        part[2 * blockIdx.x + 1] = v1;
        // Unlike the tickets of fe_ring_draw_kernel and fe_net_update_kernel, which only order one thread's reads before
        // the last holder's write, this one PUBLISHES data: the last holder reads the other workgroups' partials.  So the
        // stores are released at agent scope and explicitly drained before the ticket is taken (the fence's own wait is
        // not relied on to stay between the stores and the atomic).
        __threadfence();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return false;
    __threadfence();  // the other workgroups' partials, stored before their tickets
    const int t = threadIdx.x;
    const volatile double *p = part;
    v0 = t < (int)gridDim.x ? p[2 * t] : 0.0;  // gridDim.x <= kBlock
    v1 = t < (int)gridDim.x ? p[2 * t + 1] : 0.0;
    ppo_block_sum(s, v0, v1);
    if (t == 0) *ticket = 0u;
    return t == 0;
}

__global__ __launch_bounds__(kBlock) void fe_ppo_actor_loss_kernel(const PpoLossArgs d) {
    __shared__ double s[2][kBlock];
    const double log_std = (double)d.log_std[0];
    const double std = exp(log_std);
    const double var = std * std;
    const double log_scale = log(std);  // Normal.log_prob takes scale.log()
    const double inv_count = 1.0 / (double)d.count;
    constexpr double kHalfLog2Pi = 0.91893853320467274178;  // log(sqrt(2 pi))
    double objective = 0.0, g_ls = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < d.count; i += (int64_t)gridDim.x * kBlock) {
        const double diff = (double)d.actions[i] - (double)d.x[i];
        const double adv = (double)d.y[i];
        const double lp = -(diff * diff) / (2.0 * var) - log_scale - kHalfLog2Pi;
        const double ratio = exp(lp - (double)d.old_lp[i]);
        const double clipped = ratio < d.lo ? d.lo : (ratio > d.hi ? d.hi : ratio);
        const double first = ratio * adv, second = clipped * adv;
        // d min(first, second) / d ratio: torch.minimum gives the gradient to the smaller term and halves it on a tie;
        // clamp passes it on [lo, hi] and nowhere else
        const double through_clamp = (ratio >= d.lo && ratio <= d.hi) ? adv : 0.0;
        double d_ratio;
        if (first < second) d_ratio = adv;
        else if (first > second) d_ratio = through_clamp;
        else if (first == second) d_ratio = 0.5 * adv + 0.5 * through_clamp;
        else d_ratio = first + second;  // a NaN term: NaN, as torch.minimum propagates it
        objective += first < second ? first : (second < first ? second : (first == second ? first : first + second));
        const double d_lp = d_ratio * ratio;  // d exp(lp - old) / d lp = ratio
        d.g_x[i] = (float)(-inv_count * d_lp * (diff / var));
        g_ls += d_lp * (diff * diff / var - 1.0);
    }
    ppo_block_sum(s, objective, g_ls);
    if (ppo_grid_sum(d.ws, s, objective, g_ls)) {
        const double entropy = 0.5 + kHalfLog2Pi + log_scale;
        *d.loss = (float)(-(objective * inv_count + d.ent_coef * entropy));
        *d.g_log_std = (float)(-(g_ls * inv_count + d.ent_coef));  // d entropy / d log_std = 1
    }
}

__global__ __launch_bounds__(kBlock) void fe_ppo_value_loss_kernel(const PpoLossArgs d) {
    __shared__ double s[2][kBlock];
    const double inv_count = 1.0 / (double)d.count;
    double sq = 0.0, unused = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < d.count; i += (int64_t)gridDim.x * kBlock) {
        const double diff = (double)d.y[i] - (double)d.x[i];  // returns - values
        sq += diff * diff;
        d.g_x[i] = (float)(-2.0 * diff * inv_count);
    }
    ppo_block_sum(s, sq, unused);
    if (ppo_grid_sum(d.ws, s, sq, unused)) *d.loss = (float)(sq * inv_count);
}

}  // namespace
