/*
 * finenvs_amd_replay.h -- the off-policy replay ring of the C ABI (same library as finenvs_amd.h).
 *
 * The reference's TD3 / SAC agents train from one buffer class (finenvs/agents/off_policy_buffer.py, "OPB") that keeps
 * every transition's states and next states as rendered f32 observations and moves O(capacity) bytes per store
 * (torch.cat of the whole container, then index_select).  Here a transition is kept as observation DESCRIPTORS
 * (fe_env_describe / fe_env_step_traj): 2 (8 + 8A) + 4A + 4 + 4 bytes instead of 2 x 20WA, storing is O(1), and the
 * observations are rendered once, when a minibatch is sampled.  Python front end: finenvs_amd/replay.py.  Conventions
 * as in finenvs_amd.h.
 *
 * Ring: C slots, struct-of-arrays, caller-owned device memory.  The caller keeps `head` (the slot the next transition
 * goes to) and `size` (transitions retained, <= C) on the host; logical index i in [0, size) -- the i-th oldest retained
 * transition, OPB's row i -- lives in slot (head - size + i) mod C.
 */
#ifndef FINENVS_AMD_REPLAY_H
#define FINENVS_AMD_REPLAY_H

#include "finenvs_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fe_replay_ring {
    int64_t capacity;      /* C = max_size, >= 1 */
    int32_t num_assets;    /* A */
    int32_t reserved;      /* 0 */
    int64_t *state_src;    /* (C) int64: window offset of the state's observation */
    double *state_pos;     /* (C, A) f64: position feature of the state */
    int64_t *next_src;     /* (C) */
    double *next_pos;      /* (C, A) */
    float *actions;        /* (C, A) f32 */
    float *rewards;        /* (C) f32: (float) of the f64 reward, equal to OPB's .float() bit for bit */
    float *dones;          /* (C) f32: (float) of the int32 done flag */
    uint64_t *errors;      /* (1): fe_replay_sample adds the number of indices outside [0, size) */
} fe_replay_ring;

/*
 * Replaces Buffer.store (OPB:33-47) and Buffer.discard_old_data (OPB:56-66): writes `count` transitions into slots
 * (head + k) mod C, k < count, overwriting the oldest ones once the ring is full -- no copy of the retained data.
 * The source is step-major: transition j = t * num_envs + n (t < steps, n < num_envs) is element e = t * row_stride + n
 * of every source array (state_src (.., row_stride), state_pos (.., row_stride, A), ...), and the call appends
 * transitions j = first .. first + count - 1.  One env step: steps = 1.  A trajectory chunk of descriptors
 * (TrajectoryBuffer(states=True)): steps = T, row_stride = its env capacity, next_src / next_pos = row 1 of its
 * state descriptors.  actions: f32, or f64 when actions_are_f64 (cast to f32); rewards f64; dones int32.
 * No host synchronisation and no allocation (capturable).  Runs on the device of ring->rewards.
 * FE_ERR_ARG: null pointers, count < 1 or > C, head outside [0, C), first + count > steps * num_envs, row_stride < num_envs.
 */
int fe_replay_append(const fe_replay_ring *ring, int64_t head, int64_t steps, int64_t num_envs, int64_t row_stride,
                     int64_t first, int64_t count, const int64_t *state_src, const double *state_pos,
                     const int64_t *next_src, const double *next_pos, const void *actions, int32_t actions_are_f64,
                     const double *rewards, const int32_t *dones, void *stream);

/*
 * Replaces Buffer.get_mini_batch's gather (OPB:68-77) in one launch: for the `count` logical indices (device int64)
 * writes, all f32, states (count, W, 5A) and next_states (count, W, 5A) -- the env's observations of the stored
 * descriptors, equal to .float() of the rendered observation for f64 and f32 envs alike -- actions (count, A),
 * rewards (count) and dones (count).  An index outside [0, size) reads nothing of the ring: its rows are written as NaN
 * and it is counted in ring->errors[0] (the caller reads that counter when it wants to know).  The env supplies the
 * log-return table and W, A; the descriptors must come from an env with the same tables.
 * FE_ERR_ARG: null pointers, count < 0, size outside [1, C], head outside [0, C), an A that is not the env's.
 */
int fe_replay_sample(fe_env *env, const fe_replay_ring *ring, int64_t head, int64_t size, const int64_t *indices,
                     int64_t count, float *states, float *next_states, float *actions, float *rewards, float *dones,
                     void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FINENVS_AMD_REPLAY_H */
