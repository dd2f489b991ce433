/*
 * finenvs_amd_ppo.h -- the device side of a PPO update's mini-batch loop (same library as finenvs_amd.h).
 *
 * PPOAgent.train (finenvs/agents/PPO/PPO_agent.py:175-196) shuffles the T * N samples of a trajectory once per epoch
 * (buffer.py:127-146), gathers each mini-batch by fancy indexing and evaluates the clipped-surrogate and the MSE loss
 * with a few dozen element-wise kernels.  The entries here do the same work without a host integer that changes from
 * one update to the next, so that a whole train() can be captured into one hipGraph (finenvs_amd/graphed.py):
 *
 *   fe_ppo_minibatch        the samples of mini-batch m of epoch e drawn from a keyed permutation of [0, T * N) and
 *                           gathered from the trajectory chunk, one launch
 *   fe_ppo_epochs_advance   the epoch counter, kept in device memory, moved on after a train()
 *   fe_ppo_actor_loss       ContinuousActor.compute_actor_loss with its gradients, one launch
 *   fe_ppo_value_loss       Critic.compute_critic_loss with its gradient, one launch
 *
 * Python front end: finenvs_amd/ppo.py (PPOUpdate), finenvs_amd/lstm_head.py (ppo_actor_loss / ppo_critic_loss with
 * fused=True), host mirror of the permutation finenvs_amd/rng.py (ppo_permute).  Conventions as in finenvs_amd.h:
 * every entry returns FE_OK or a negative FE_ERR_*, argument checks come before any GPU call, nothing allocates and
 * nothing waits for the device.
 *
 * The permutation.  For n = T * N samples, 1 <= n < 2^32:
 *   k = max(1, bit_length(n - 1)),  hb = (k + 1) / 2,  mask = 2^hb - 1        (domain 2^(2 hb): >= n and < 4 n)
 *   key = seed ^ FE_PPO_PERM_SALT
 *   one pass over x = (l << hb) | r is four rounds
 *       (l, r) <- (r, l ^ (philox_u32(key, ((epoch * 4 + round) << 16) | r) & mask))          (Philox4x32-10)
 *   pi_epoch(p) = the first x < n among pass(p), pass(pass(p)), ...                            (cycle walking)
 * A balanced Feistel network is a bijection of its domain whatever the round function, and cycle walking restricts a
 * bijection of the domain to one of [0, n).  The walk is bounded by the domain size; a lane that exhausts the bound
 * (impossible for a bijection) writes index -1, NaN fields and adds 1 to the cursor's error word.
 *
 * The cursor: two 64-bit words of caller-owned device memory, zero-initialised by the caller:
 *   word FE_PPO_CURSOR_EPOCH   int64   epochs drawn by the train() calls so far
 *   word FE_PPO_CURSOR_ERRORS  uint64  lanes whose walk did not end (stays 0)
 */
#ifndef FINENVS_AMD_PPO_H
#define FINENVS_AMD_PPO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FE_PPO_PERM_SALT 0x50504F5045524D31ull /* "PPOPERM1": the key's distance from the redraw / ring-draw streams */
#define FE_PPO_CURSOR_EPOCH 0
#define FE_PPO_CURSOR_ERRORS 1
#define FE_PPO_CURSOR_WORDS 2
#define FE_PPO_MAX_COLUMNS 4

/*
 * Mini-batch m of M of epoch e = cursor[FE_PPO_CURSOR_EPOCH] + epoch_offset, B = (T * N) / M samples (the reference
 * drops the remainder, buffer.py:127-146): position p = m * B + b is sample s = pi_e(p), env = s / T, step = s % T
 * (the reference's numbering after reshape, buffer.py:102-109).  Reads of the trajectory chunk
 *   obs_src (T + 1, C) int64, obs_pos (T + 1, C, A) float64, actions (T, C, A) float32      (C >= N: the row stride)
 *   columns[i] (T, N) float32, dense, i < num_columns <= FE_PPO_MAX_COLUMNS                  (old log-probs, advantages, ...)
 * and writes indices_out (B) int64 = s, obs_src_out (B), obs_pos_out (B, A), actions_out (B, A) and columns_out[i] (B).
 * Every output except indices_out may be null (columns_out itself, or any of its entries) and is skipped then.
 * `columns` and `columns_out` are host arrays of device pointers.  epoch_offset and m are by-value: a captured train()
 * has one node per (epoch_offset, m), so they are constants of the graph; only the base epoch is read on the device.
 * FE_ERR_ARG: null obs_src / obs_pos / actions / cursor / indices_out; T < 1, N < 1, C < N, A < 1; T * N >= 2^32;
 * M < 1, M > T * N, m outside [0, M); epoch_offset < 0; num_columns outside [0, 4]; num_columns > 0 with null
 * `columns` or a null entry in it.
 */
int fe_ppo_minibatch(const int64_t *obs_src, const double *obs_pos, const float *actions, int64_t T, int64_t N,
                     int64_t C, int32_t A, const float *const *columns, float *const *columns_out, int32_t num_columns,
                     int64_t *cursor, uint64_t seed, int64_t epoch_offset, int64_t M, int64_t m, int64_t *indices_out,
                     int64_t *obs_src_out, double *obs_pos_out, float *actions_out, void *stream);

/*
 * cursor[FE_PPO_CURSOR_EPOCH] += count, by one thread: once per train(), after its last fe_ppo_minibatch
 * (PPO_agent.py:175, the epochs loop, seen from the next train()).  FE_ERR_ARG: null cursor, count < 0.
 */
int fe_ppo_epochs_advance(int64_t *cursor, int64_t count, void *stream);

/*
 * Doubles of caller-owned device workspace the two loss launches need for `count` samples.  Its first 8 bytes are the
 * launch's ticket: zero before the first launch, and left zero by every launch.  -1 for count < 1.
 */
int64_t fe_ppo_loss_workspace_doubles(int64_t count);

/*
 * ContinuousActor.compute_actor_loss (PPO/continuous_actor.py:59-78) for one action per sample, and its gradients:
 *   new_lp = Normal(means, exp(log_std)).log_prob(actions);  ratio = exp(new_lp - old_log_probs)
 *   loss   = -(mean(min(ratio * adv, clamp(ratio, 1 - clip_epsilon, 1 + clip_epsilon) * adv))
 *              + entropy_coefficient * (0.5 + 0.5 log(2 pi) + log_std))
 *   g_means[b] = d loss / d means[b],  g_log_std = d loss / d log_std
 * with torch's gradient rules: the selected term of `minimum` carries the gradient (a tie splits it in halves), a
 * clamped ratio carries none, and clamp passes gradient on its closed interval.  means, actions, old_log_probs,
 * advantages, g_means: `count` floats; log_std, loss, g_log_std: one float each, all on the device.  The f32 inputs are
 * taken to f64, every sample is evaluated in f64 (exp / log, no fast intrinsics), and each output is rounded to f32
 * once.  The sums are blocked reductions in a fixed order without float atomics: two launches on the same inputs give
 * the same bits.
 * FE_ERR_ARG: a null pointer, count < 1, clip_epsilon < 0.
 */
int fe_ppo_actor_loss(const float *means, const float *log_std, const float *actions, const float *old_log_probs,
                      const float *advantages, int64_t count, double clip_epsilon, double entropy_coefficient,
                      float *loss, float *g_means, float *g_log_std, double *workspace, void *stream);

/*
 * Critic.compute_critic_loss (PPO/critic.py:26-32) and its gradient: loss = mean((returns - values)^2),
 * g_values[b] = 2 (values[b] - returns[b]) / count.  Arithmetic, reduction and workspace as fe_ppo_actor_loss.
 * FE_ERR_ARG: a null pointer, count < 1.
 */
int fe_ppo_value_loss(const float *values, const float *returns, int64_t count, float *loss, float *g_values,
                      double *workspace, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* FINENVS_AMD_PPO_H */
