/*
 * finenvs_amd_replay_cursor.h -- the replay ring's cursor in device memory (same library as finenvs_amd.h).
 *
 * fe_replay_append / fe_replay_sample (finenvs_amd_replay.h) and fe_twin_q_target (finenvs_amd_critic.h) take the ring's
 * `head` and `size` by value, from host integers: a hipGraph captured around them samples for ever from the ring as it
 * stood at capture time.  The entries here read `head` and `size` from 32 bytes of caller-owned device memory instead
 * (the CURSOR), which the append writes and the launches after it in stream order see, and fe_ring_draw draws a
 * mini-batch's logical indices on the device from a counter kept in the same cursor.  A captured update iteration then
 * follows the ring while transitions are stored between its replays.  Python front end: finenvs_amd/replay.py
 * (ReplayBuffer(cursor=True), ReplayBuffer.draw) and finenvs_amd/graphed.py.  Conventions as in finenvs_amd.h.
 *
 * The cursor, as four 64-bit words (an int64_t[4] on the device, zero-initialised by the caller):
 *   word FE_CURSOR_HEAD    int64   head: the slot the next transition goes to
 *   word FE_CURSOR_SIZE    int64   size: transitions retained, <= C
 *   word FE_CURSOR_DRAWS   uint64  draws: the Philox counter of the next draw
 *   word FE_CURSOR_TICKET  uint32  ticket of the launch in flight (0 between launches), then 4 bytes of padding
 * The host stays the authority on head and size -- they are pure functions of what was stored, so it needs no
 * synchronisation to know them -- and fe_replay_append_c mirrors them into the cursor.
 */
#ifndef FINENVS_AMD_REPLAY_CURSOR_H
#define FINENVS_AMD_REPLAY_CURSOR_H

#include "finenvs_amd_replay.h"
#include "finenvs_amd_critic.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FE_CURSOR_HEAD 0
#define FE_CURSOR_SIZE 1
#define FE_CURSOR_DRAWS 2
#define FE_CURSOR_TICKET 3
#define FE_CURSOR_WORDS 4

typedef struct fe_replay_cursor {
    int64_t head;
    int64_t size;
    uint64_t draws;
    uint32_t ticket;
    uint32_t reserved;
} fe_replay_cursor;

/*
 * fe_replay_append (finenvs_amd_replay.h) with the cursor: after its transitions, one thread of the same launch writes
 * head = (head + count) mod C and size = new_size into the cursor; `draws` is left alone.  new_size is the ring's size
 * after this append (min(size + first + count, C) in the caller's bookkeeping).
 * FE_ERR_ARG as fe_replay_append, and for a null cursor or new_size outside [count, C].
 */
int fe_replay_append_c(const fe_replay_ring *ring, int64_t head, int64_t steps, int64_t num_envs, int64_t row_stride,
                       int64_t first, int64_t count, const int64_t *state_src, const double *state_pos,
                       const int64_t *next_src, const double *next_pos, const void *actions, int32_t actions_are_f64,
                       const double *rewards, const int32_t *dones, int64_t *cursor, int64_t new_size, void *stream);

/*
 * Draws a mini-batch and gathers its descriptors in one launch.  With head, size and draws read from the cursor:
 *   logical index b:  indices_out[b] = (philox_u32(seed, draws + b) * size) >> 32      (Philox4x32-10, the env's generator)
 *   its slot:         (head - size + indices_out[b]) mod C
 * and that slot's state_src (count) / state_pos (count, A) / next_src / next_pos / actions (count, A) / rewards (count) /
 * dones (count) are copied to the outputs; every output except indices_out may be null and is skipped then.  After the
 * gather `draws` advances by count, exactly once per launch: no workgroup of the launch sees the advanced value.
 * If size in the cursor is 0 the launch writes index -1 and NaN outputs (0 for state_src / next_src) and adds count to
 * ring->errors[0].  No allocation, no host synchronisation (capturable).
 * FE_ERR_ARG: null ring / cursor / indices_out, count < 0, capacity >= 2^32.
 */
int fe_ring_draw(const fe_replay_ring *ring, int64_t *cursor, uint64_t seed, int64_t count, int64_t *indices_out,
                 int64_t *state_src, double *state_pos, int64_t *next_src, double *next_pos, float *actions,
                 float *rewards, float *dones, void *stream);

/*
 * fe_twin_q_target (finenvs_amd_critic.h) with head and size read from the cursor when the launches run.
 * FE_ERR_ARG as fe_twin_q_target (without its head / size checks), and for a null cursor.
 */
int fe_twin_q_target_c(fe_env *env, const float *logret_f32, const fe_critic_weights *c1, const fe_critic_weights *c2,
                       int32_t H, const fe_replay_ring *ring, const int64_t *cursor, const int64_t *indices,
                       int64_t count, const float *next_actions, const float *smooth_noise, float smooth_std,
                       float smooth_clip, const float *log_probs, const float *alpha, float gamma, float reward_scale,
                       float *targets_out, float *q1_out, float *q2_out, void *stream);

/*
 * fe_replay_sample (finenvs_amd_replay.h) with head and size read from the cursor when the launch runs.
 * FE_ERR_ARG as fe_replay_sample (without its head / size checks), and for a null cursor.
 */
int fe_replay_sample_c(fe_env *env, const fe_replay_ring *ring, const int64_t *cursor, const int64_t *indices,
                       int64_t count, float *states, float *next_states, float *actions, float *rewards, float *dones,
                       void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FINENVS_AMD_REPLAY_CURSOR_H */
