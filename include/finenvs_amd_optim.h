/*
 * finenvs_amd_optim.h -- the parameter side of a training step in one launch (same library as finenvs_amd.h).
 *
 * fe_net_update runs torch.optim.Adam's single-tensor step, the reference's soft update of a target network
 * (SAC_agent.py:240, TD3_agent.py:263) and the packing into kernel layout (lstm_pack, pack_critic_weights,
 * pack_sac_weights, lstm_fragment_major of finenvs_amd/) over a device-resident table of parameter segments, one or more
 * networks per table.  Python front end: finenvs_amd/optim.py.  Conventions as in finenvs_amd.h.
 *
 * Per element, every operation one f32 rounding, no FMA contraction:
 *   m += (1 - b1) * (g - m);  v = v * b2 + ((1 - b2) * g) * g;  denom = sqrt(v) / bc2s + eps;  p += (-step_size) * (m / denom)
 * with step_size = lr / (1 - b1^t) and bc2s = sqrt(1 - b2^t) computed in f64 and rounded to f32 once.  b1^t and b2^t are
 * two f64 running products in device memory (fe_optim_state), multiplied once per step by the kernel: no step-dependent
 * value comes from the host.  Then, where the segment lists a target and soft_update is set,
 *   target = target * one_minus_rho + p * rho
 * then the new values go to every packed destination of the online and of the target network, then the gradient is
 * zeroed if zero_grad is set.
 *
 * Errors (FE_ERR_ARG, message naming the function): null desc / segments / state, counts < 1, an unknown mode, a table
 * that is not device memory.  No host synchronisation and no allocation.
 */
#ifndef FINENVS_AMD_OPTIM_H
#define FINENVS_AMD_OPTIM_H

#include "finenvs_amd.h"
#include "finenvs_amd_sac_grad.h"

#ifdef __cplusplus
extern "C" {
#endif

/* How a segment's elements reach the packed form of their network (R = the packed row of torch row r, lstm_row_order). */
enum {
    FE_SEG_PLAIN = 0,       /* no packed form: log_alpha, PPO's log_std */
    FE_SEG_COPY = 1,        /* packed[i] = x[i]: wout, bout, bl, wmu, wstd, bmu, bstd */
    FE_SEG_WHH = 2,         /* (4H, H): packed[R * H + c] */
    FE_SEG_WHH_FRAGMENT = 3,/* (4H, H), H >= 256: lstm_fragment_major of FE_SEG_WHH */
    FE_SEG_WL = 4,          /* (H, H): the SAC actor's last layer, fragment-major without a row permutation */
    FE_SEG_WIH = 5,         /* (4H, cols), cols 5 or 6: packed is wx (4H, 8); column c < 5 -> slot c, column 5 -> slot 6 */
    FE_SEG_BIAS_PAIR = 6    /* b_ih (x) and b_hh (x2), 4H each, owned by one thread: wx slot 5 = b_ih + b_hh, slot 7 = 0 and,
                               with cols == 5 (no action column), slot 6 = 0 */
};

/* One parameter tensor (or the bias pair).  All pointers f32 device memory; target / packed / packed_target may be null. */
typedef struct fe_optim_segment {
    float *param, *grad, *exp_avg, *exp_avg_sq, *target;
    float *param2, *grad2, *exp_avg2, *exp_avg_sq2, *target2; /* FE_SEG_BIAS_PAIR only: b_hh */
    float *packed, *packed_target;                              /* destination bases, by `kind` */
    int64_t numel;
    int64_t first_block;  /* blocks of FE_OPTIM_BLOCK_ELEMS elements before this segment; ascending over the table */
    int32_t kind, H, cols, reserved;
    float one_minus_rho, rho; /* (1 - rho) and rho, each rounded to f32 once */
} fe_optim_segment;

#define FE_OPTIM_BLOCK_ELEMS 1024

/* Device memory, 32 bytes, owned by the caller: {1, 1, 0, 0} before the first step. */
typedef struct fe_optim_state {
    double beta1_pow, beta2_pow; /* b1^t, b2^t: running products */
    int64_t step;                /* t */
    uint32_t done, reserved;     /* workgroups of the running launch that have read the products; 0 between launches */
} fe_optim_state;

enum { FE_OPTIM_STEP = 0, FE_OPTIM_PACK = 1, FE_OPTIM_ZERO_GRAD = 2 };

typedef struct fe_optim_desc {
    const fe_optim_segment *segments; /* device memory */
    fe_optim_state *state;            /* device memory */
    int32_t num_segments;
    int32_t mode;                     /* FE_OPTIM_STEP; FE_OPTIM_PACK: only the packed forms are written, nothing else
                                         changes, the step state included; FE_OPTIM_ZERO_GRAD: only the gradients */
    int64_t num_blocks;               /* sum over segments of ceil(numel / FE_OPTIM_BLOCK_ELEMS) */
    int32_t soft_update, zero_grad;   /* FE_OPTIM_STEP only */
    double beta1, beta2, lr;          /* the f64 the running products and step_size are formed with */
    float one_minus_beta1, beta2_f32, one_minus_beta2, eps; /* each rounded to f32 once */
} fe_optim_desc;

/* One launch over the whole table. */
int fe_net_update(const fe_optim_desc *desc, void *stream);

/*
 * Siblings of the entries that take an output bias by value (finenvs_amd_ext.h, finenvs_amd_sac.h,
 * finenvs_amd_sac_grad.h): the same arguments with each bias (1 f32) read through a device pointer, as
 * fe_critic_weights.bout is, and the same bits for the same bias.  A freshly stepped or soft-updated bias needs no copy
 * to the host.  A null bias pointer is FE_ERR_ARG under the sibling's name; every other error is the by-value entry's,
 * under that entry's name.  fe_sac_backward_p takes bmu for symmetry only: the gradient does not depend on it.
 */
int fe_lstm_forward_p(fe_env *env, const float *logret_f32, const float *whh, const float *wx, const float *wout,
                      const float *bout, int32_t H, int32_t out_activation, const int64_t *obs_src, const double *obs_pos,
                      int64_t count, float *out, void *stream);
int fe_env_rollout_lstm_p(fe_env *env, const float *logret_f32, const float *whh, const float *wx, const float *wout,
                          const float *bout, int32_t H, int32_t out_activation, int32_t K, int64_t *obs_src,
                          double *obs_pos, const float *noise, float noise_std, float *actions_out, float *means_out,
                          double *rewards_out, int32_t *dones_out, int64_t *src_out, double *pos_out, void *stream);
int fe_env_rollout_lstm_split_p(fe_env *env, const float *logret_f32, const float *whh, const float *wx, const float *wout,
                                const float *bout, int32_t H, int32_t out_activation, int32_t K, int64_t *obs_src,
                                double *obs_pos, const float *noise, float noise_std, float *actions_out, float *means_out,
                                double *rewards_out, int32_t *dones_out, int64_t *src_out, double *pos_out,
                                float *workspace, void *stream);
int fe_env_rollout_sac_p(fe_env *env, const float *logret_f32, const float *whh, const float *wx, const float *wl,
                         const float *bl, const float *wmu, const float *bmu, const float *wstd, const float *bstd,
                         int32_t H, int32_t K, int64_t *obs_src, double *obs_pos, const float *noise, float *actions_out,
                         float *means_out, float *stds_out, double *rewards_out, int32_t *dones_out, int64_t *src_out,
                         double *pos_out, void *stream);
int fe_sac_forward_p(fe_env *env, const float *logret_f32, const float *whh, const float *wx, const float *wl,
                     const float *bl, const float *wmu, const float *bmu, const float *wstd, const float *bstd, int32_t H,
                     const int64_t *obs_src, const double *obs_pos, int64_t count, const float *noise, float *actions_out,
                     float *log_probs_out, float *means_out, float *stds_out, void *stream);
int fe_sac_backward_p(fe_env *env, const float *logret_f32, const float *whh, const float *wx, const float *wl,
                      const float *bl, const float *wmu, const float *bmu, const float *wstd, const float *bstd, int32_t H,
                      const int64_t *obs_src, const double *obs_pos, int64_t count, const float *noise,
                      const float *actions, const float *stds, const float *d_actions, const float *d_log_probs,
                      float *workspace, const fe_sac_grads *grads, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FINENVS_AMD_OPTIM_H */
