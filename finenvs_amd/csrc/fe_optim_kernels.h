// fe_optim_kernels.h -- included by fe_env.hip: the parameter side of a training step in one launch
// (include/finenvs_amd_optim.h; Python front end finenvs_amd/optim.py).
#pragma once

namespace {

// ---- Adam + soft update + packing over a table of parameter segments ----
// One workgroup owns FE_OPTIM_BLOCK_ELEMS consecutive elements of ONE segment: the segment is found from blockIdx.x alone
// (a binary search over the ascending first_block column), so the lookup is wave-uniform -- scalar loads and scalar
// branches -- and the per-element code has the segment's pointers and kind in SGPRs.  Reads and the in-place writes are
// coalesced (lane = consecutive element); only the packed destinations scatter, within a few KiB.
//
// The two running products b1^t, b2^t live in device memory.  In every workgroup thread 0 alone reads the old products,
// multiplies them and hands the two f32 scalars to the other waves through LDS; the same thread takes an integer ticket
// (st->done) after its elements, and the thread with the last ticket writes the new products back.  The read and the
// ticket are in one thread's program order, so every read of the old products precedes the write: no wave can see a
// product of the step it is computing, and the launch needs nothing step-dependent from the host.
struct OptimArgs {
    const fe_optim_segment *seg;
    fe_optim_state *st;
    int32_t num_segments, mode, soft_update, zero_grad;
    double beta1, beta2, lr;
    float omb1, b2, omb2, eps;
};

struct OptimScalars {
    float omb1, b2, omb2, eps, neg_step_size, bc2s;
};

// torch.optim.Adam's single-tensor step on one element (_single_tensor_adam, amsgrad = False, weight_decay = 0,
// maximize = False), one f32 rounding per torch operation: lerp_, mul_ + addcmul_, sqrt / bias_correction2_sqrt + eps,
// addcdiv_(value = -step_size).  The new parameter.
__device__ __forceinline__ float adam_element(const OptimScalars &k, float p, float g, float *m_io, float *v_io) {
    const float m = __fadd_rn(*m_io, __fmul_rn(k.omb1, __fsub_rn(g, *m_io)));
    const float v = __fadd_rn(__fmul_rn(*v_io, k.b2), __fmul_rn(__fmul_rn(k.omb2, g), g));
    // __builtin_sqrtf is the correctly rounded square root (hipcc's __fsqrt_rn is the approximate native one)
    const float denom = __fadd_rn(__fdiv_rn(__builtin_sqrtf(v), k.bc2s), k.eps);
    *m_io = m;
    *v_io = v;
    return __fadd_rn(p, __fmul_rn(k.neg_step_size, __fdiv_rn(m, denom)));
}

// The reference's soft update (SAC_agent.py:240, TD3_agent.py:263): target * (1 - rho) + p * rho.
__device__ __forceinline__ float soft_element(const fe_optim_segment &s, float t, float p) {
    return __fadd_rn(__fmul_rn(t, s.one_minus_rho), __fmul_rn(p, s.rho));
}

// Packed row of torch row r = gate * H + unit (the inverse of lstm_row_order: R = 32 mt + 8 b + 4 half + gate with
// unit = 8 mt + 4 half + b).
__device__ __forceinline__ int64_t packed_row(int64_t r, int32_t H) {
    const int64_t gate = r / H, u = r % H;
    return 32 * (u / 8) + 8 * (u % 4) + 4 * ((u % 8) / 4) + gate;
}

// [row tile][k group][k half][row & 31][4] of a (rows, cols) matrix: lstm_fragment_major / pack_sac_weights' wl.
__device__ __forceinline__ int64_t fragment_index(int64_t R, int64_t c, int32_t cols) {
    return (((R / 32) * (cols / 8) + c / 8) * 2 + (c % 8) / 4) * 128 + (R % 32) * 4 + c % 4;
}

// Where element e of the segment goes in the packed form (-1: nowhere).  FE_SEG_BIAS_PAIR is handled by its caller.
__device__ __forceinline__ int64_t packed_index(const fe_optim_segment &s, int64_t e) {
    switch (s.kind) {
    case FE_SEG_COPY: return e;
    case FE_SEG_WHH: return packed_row(e / s.H, s.H) * s.H + e % s.H;
    case FE_SEG_WHH_FRAGMENT: return fragment_index(packed_row(e / s.H, s.H), e % s.H, s.H);
    case FE_SEG_WL: return fragment_index(e / s.H, e % s.H, s.H);
    case FE_SEG_WIH: {
        const int64_t c = e % s.cols;
        return packed_row(e / s.cols, s.H) * 8 + (c < 5 ? c : 6);
    }
    default: return -1;
    }
}

// Slots 5..7 of one wx row: the bias sum (one f32 add), the zero of slot 7 and, without an action column, of slot 6.
__device__ __forceinline__ void pack_bias_row(float *wx, const fe_optim_segment &s, int64_t r, float b_ih, float b_hh) {
    float *row = wx + packed_row(r, s.H) * 8;
    row[5] = __fadd_rn(b_ih, b_hh);
    if (s.cols == 5) row[6] = 0.0f;
    row[7] = 0.0f;
}

__global__ __launch_bounds__(kBlock) void fe_net_update_kernel(const OptimArgs a) {
    // the segment of this workgroup: the last one whose first_block <= blockIdx.x
    int lo = 0, hi = a.num_segments - 1;
    const int64_t blk = blockIdx.x;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.seg[mid].first_block <= blk) lo = mid; else hi = mid - 1;
    }
    const fe_optim_segment s = a.seg[lo];
    const int64_t begin = (blk - s.first_block) * FE_OPTIM_BLOCK_ELEMS;
    const int64_t end = begin + FE_OPTIM_BLOCK_ELEMS < s.numel ? begin + FE_OPTIM_BLOCK_ELEMS : s.numel;
    const bool pair = s.kind == FE_SEG_BIAS_PAIR;

    if (a.mode == FE_OPTIM_ZERO_GRAD) {
        for (int64_t e = begin + threadIdx.x; e < end; e += kBlock) {
            if (s.grad) s.grad[e] = 0.0f;  // a parameter that has no gradient yet has nothing to zero
            if (pair && s.grad2) s.grad2[e] = 0.0f;
        }
        return;
    }
    if (a.mode == FE_OPTIM_PACK) {
        for (int64_t e = begin + threadIdx.x; e < end; e += kBlock) {
            if (pair) {
                if (s.packed) pack_bias_row(s.packed, s, e, s.param[e], s.param2[e]);
                if (s.packed_target && s.target) pack_bias_row(s.packed_target, s, e, s.target[e], s.target2[e]);
                continue;
            }
            const int64_t d = packed_index(s, e);
            if (d < 0) continue;
            if (s.packed) s.packed[d] = s.param[e];
            if (s.packed_target && s.target) s.packed_target[d] = s.target[e];
        }
        return;
    }

    // FE_OPTIM_STEP: the products of this step from the ones in memory, then the two f32 scalars.  Only thread 0 reads
    // the products (it is the thread that takes the ticket below); the PACK and ZERO modes returned above, so the
    // barrier is reached by the whole workgroup.
    __shared__ float step_scalars[2];
    double p1 = 0.0, p2 = 0.0;
    if (threadIdx.x == 0) {
        const volatile fe_optim_state *old = a.st;
        p1 = old->beta1_pow * a.beta1;
        p2 = old->beta2_pow * a.beta2;
        step_scalars[0] = -(float)(a.lr / (1.0 - p1));
        step_scalars[1] = (float)__dsqrt_rn(1.0 - p2);
    }
    __syncthreads();
    OptimScalars k;
    k.omb1 = a.omb1; k.b2 = a.b2; k.omb2 = a.omb2; k.eps = a.eps;
    k.neg_step_size = step_scalars[0];
    k.bc2s = step_scalars[1];
    const bool soft = a.soft_update && s.target;

    for (int64_t e = begin + threadIdx.x; e < end; e += kBlock) {
        float m = s.exp_avg[e], v = s.exp_avg_sq[e];
        const float p = adam_element(k, s.param[e], s.grad[e], &m, &v);
        s.exp_avg[e] = m; s.exp_avg_sq[e] = v; s.param[e] = p;
        float t = 0.0f;
        if (soft) {
            t = soft_element(s, s.target[e], p);
            s.target[e] = t;
        }
        if (a.zero_grad) s.grad[e] = 0.0f;
        if (pair) {
            float m2 = s.exp_avg2[e], v2 = s.exp_avg_sq2[e];
            const float q = adam_element(k, s.param2[e], s.grad2[e], &m2, &v2);
            s.exp_avg2[e] = m2; s.exp_avg_sq2[e] = v2; s.param2[e] = q;
            if (s.packed) pack_bias_row(s.packed, s, e, p, q);
            if (soft) {
                const float t2 = soft_element(s, s.target2[e], q);
                s.target2[e] = t2;
                if (s.packed_target) pack_bias_row(s.packed_target, s, e, t, t2);
            }
            if (a.zero_grad) s.grad2[e] = 0.0f;
            continue;
        }
        const int64_t d = packed_index(s, e);
        if (d < 0) continue;
        if (s.packed) s.packed[d] = p;
        if (soft && s.packed_target) s.packed_target[d] = t;
    }

    // the last thread 0 to get here writes the products back: every workgroup's thread 0 has read the old ones by then,
    // and no other thread reads them
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(&a.st->done, 1u) == gridDim.x - 1) {
            a.st->beta1_pow = p1; a.st->beta2_pow = p2; a.st->step += 1;
            a.st->done = 0u;
        }
    }
}

}  // namespace
