"""GPU: acting with the SAC LSTM actor at H = 256 / 512 / 1024 (fe_env_rollout_sac_streamed / fe_sac_forward_streamed,
``FusedSACRollout(env, actor, streamed=True)``), after tests/test_sac_rollout_gpu.py and with its helpers.

* env parity: the actions ``run(8, noise, trajectory=)`` recorded, stepped through the oracle's env one step at a time,
  give the same rewards, dones, end state and trajectory descriptors bit for bit; lock-step, the actions are within
  ``2e-5 max|a64| + 4 max|a_torch32 - a64|`` of the f64 torch actor on the oracle's observations (the small kernels' fixed
  1e-5 was set for sums of at most 128 terms);
* bit for bit: the eval env acts on the un-squashed mean; ``forward`` on the trajectory rows equals ``run``'s actions;
  run(8); run(8) equals run(16); the replay ring filled by ``extend`` equals per-step ``store``.
"""
import copy

import numpy as np
import pytest
import torch

from tests.helpers import assert_bits
from tests.test_sac_rollout_gpu import _actor, _make, fe, fo, t2n  # noqa: F401  (fe, fo: fixtures)

pytestmark = pytest.mark.gpu


def _torch_actions(actor, obs, A, eps, eval_on_mean):
    """The torch actor's step actions per pair on a rendered observation (N, W, 5A), in f32 and in f64: (N, A) each."""
    from finenvs_amd.sac import pair_states

    N = obs.shape[0]
    out = []
    for dtype in (torch.float32, torch.float64):
        a = actor if dtype is torch.float32 else copy.deepcopy(actor).double()
        with torch.no_grad():
            dist = a.get_distribution(pair_states(obs.to(dtype), A))
            mu, sd = dist.loc.reshape(N, A), dist.scale.reshape(N, A)
            act = torch.tanh(mu + eps.to(dtype) * sd)
            if eval_on_mean:
                act[-1] = mu[-1]
        out.append(act)
    return out


@pytest.mark.parametrize("N,A,W,H,obs_dtype,evaluate,drop", [
    (300, 1, 4, 256, torch.float64, False, 0.0),
    (40, 3, 16, 256, torch.float32, False, 0.0),
    (77, 3, 4, 512, torch.float64, True, 0.05),     # evaluate mode, several sleeves
    (45, 3, 4, 1024, torch.float64, False, 0.1),
])
def test_run_equals_oracle_env_bit_for_bit(fe, fo, N, A, W, H, obs_dtype, evaluate, drop):  # noqa: F811
    from finenvs_amd.sac import FusedSACRollout
    from finenvs_amd.trajectory import TrajectoryBuffer

    days, bars = 5, 40
    ref, env = _make(fe, fo, N, A, W, days, bars, drop, evaluate, seed=3 * N + W, obs_dtype=obs_dtype)
    actor = _actor(H, W, seed=W + H)
    roll = FusedSACRollout(env, actor, streamed=True)
    obs = ref.reset().copy()
    g = torch.Generator(device="cuda").manual_seed(N)
    K, reps = 8, 2 * (bars + 3) // 8 + 1
    seen, worst = set(), 0.0
    for rep in range(reps):
        noise = torch.randn((K, N, A), generator=g, device="cuda")
        traj = TrajectoryBuffer(K, N, A, states=True)
        acts, rews, dones = roll.run(K, noise=noise, trajectory=traj, record_means=True)
        for k in range(K):
            if obs_dtype == torch.float64:
                assert_bits(t2n(traj.states(env, k)), obs, f"rep {rep} step {k} trajectory state")
            a32, a64 = _torch_actions(actor, torch.from_numpy(obs).cuda(), A, noise[k], not evaluate)
            err = float((acts[k].double() - a64).abs().max())
            tol = 2e-5 * float(a64.abs().max()) + 4 * float((a32.double() - a64).abs().max())
            worst = max(worst, err / tol)
            assert err <= tol, (rep, k, err, tol)
            a_k = t2n(acts[k])
            seen.update(np.unique(np.clip(np.rint(a_k * 5.5), -5, 5)).tolist())
            obs, r_ref, d_ref, _ = ref.step(a_k)
            obs = obs.copy()
            assert_bits(t2n(rews[k]), r_ref, f"rep {rep} step {k} rewards")
            assert_bits(t2n(dones[k]), d_ref, f"rep {rep} step {k} dones")
        if obs_dtype == torch.float64:
            assert_bits(t2n(traj.states(env, K)), obs, f"rep {rep} last trajectory state")
            assert_bits(t2n(roll.observation()), obs, f"rep {rep} observation()")
        assert_bits(t2n(env.cash), ref.cash, f"rep {rep} cash")
        assert_bits(t2n(env.margin), ref.margin, f"rep {rep} margin")
        assert_bits(t2n(env.env_indices), ref.env_idx, f"rep {rep} env_idx")
        if evaluate and int(ref.n_terminated[0]) == N:
            env.reset_evaluation_metrics()
            ref.terminated[:] = 0; ref.episode_returns[:] = 0; ref.n_terminated[0] = 0
    print(f"worst action err / tol {worst:.3f}")
    assert len(seen) >= 4, f"the policy must trade in both directions (share changes seen: {sorted(seen)})"


def _twins(fe, fo, N, A, W, H, evaluate=False, mu_bias=0.0):  # noqa: F811
    from finenvs_amd.sac import FusedSACRollout

    out = []
    for _ in range(2):
        ref, env = _make(fe, fo, N, A, W, 5, 60, 0.05, evaluate, seed=17)
        out.append((env, FusedSACRollout(env, _actor(H, W, seed=5, mu_bias=mu_bias), streamed=True)))
    return out


@pytest.mark.parametrize("H", [256, 1024])
def test_forward_on_trajectory_rows_and_chunking_equal_run_bit_for_bit(fe, fo, H):  # noqa: F811
    from finenvs_amd.trajectory import TrajectoryBuffer

    N, A, W = 75, 3, 4
    (env1, r1), (env2, r2) = _twins(fe, fo, N, A, W, H)
    g = torch.Generator(device="cuda").manual_seed(H)
    noise = torch.randn((16, N, A), generator=g, device="cuda")
    traj = TrajectoryBuffer(16, N, A, states=True)
    acts, rews, dones = r1.run(16, noise=noise, trajectory=traj, record_means=True, record_stds=True)
    a_a, r_a, d_a = r2.run(8, noise=noise[:8].clone())
    a_b, r_b, d_b = r2.run(8, noise=noise[8:].clone())
    assert_bits(t2n(acts), t2n(torch.cat([a_a, a_b])), "run(8); run(8) actions")
    assert_bits(t2n(rews), t2n(torch.cat([r_a, r_b])), "rewards")
    assert_bits(t2n(dones), t2n(torch.cat([d_a, d_b])), "dones")
    assert_bits(t2n(env1.cash), t2n(env2.cash), "cash")
    src, pos = traj.obs_src[:16].reshape(-1), traj.obs_pos[:16].reshape(-1, A)
    f_act, f_lp, f_mu, f_sd = r1.forward(src, pos, noise=noise.reshape(-1, A))
    f_act, f_mu, f_sd = f_act.reshape(16, N, A), f_mu.reshape(16, N, A), f_sd.reshape(16, N, A)
    assert bool(torch.isfinite(f_lp).all()) and float(f_mu.std()) > 0.05
    assert_bits(t2n(f_mu), t2n(r1.means), "forward means == run means")
    assert_bits(t2n(f_sd), t2n(r1.stds), "forward stds == run stds")
    assert_bits(t2n(f_act[:, :-1]), t2n(acts[:, :-1]), "forward actions == run actions")
    assert_bits(t2n(acts[:, -1]), t2n(r1.means[:, -1]), "the eval env acts on the mean")


def test_eval_env_acts_on_the_unsquashed_mean(fe, fo):  # noqa: F811
    N, A, W, H = 150, 1, 4, 256
    (env, roll), _ = _twins(fe, fo, N, A, W, H, mu_bias=1.5)
    noise = torch.randn((8, N, A), device="cuda")
    acts, _, _ = roll.run(8, noise=noise, record_means=True)
    assert_bits(t2n(acts[:, -1]), t2n(roll.means[:, -1]), "eval env")
    assert float(roll.means[:, -1].abs().max()) > 1.0, "the test needs a mean outside [-1, 1] at the eval env"
    assert float(acts[:, :-1].abs().max()) <= 1.0
    # without noise every env acts on the mean
    acts0, _, _ = roll.run(4, record_means=True)
    assert_bits(t2n(acts0), t2n(roll.means), "deterministic form")
    # an evaluate-mode env has no eval env: every env samples
    (ev, rev), _ = _twins(fe, fo, N, A, W, H, evaluate=True, mu_bias=1.5)
    a2, _, _ = rev.run(4, noise=noise[:4].clone())
    assert float(a2.abs().max()) <= 1.0


def test_replay_extend_after_a_fused_chunk_equals_per_step_store(fe, fo):  # noqa: F811
    from finenvs_amd.replay import ReplayBuffer
    from finenvs_amd.trajectory import TrajectoryBuffer

    N, A, W, H, K = 96, 3, 4, 256, 8
    (env, roll), _ = _twins(fe, fo, N, A, W, H)
    rb_x, rb_s = ReplayBuffer(env, max_size=5 * N), ReplayBuffer(env, max_size=5 * N)
    for chunk in range(2):  # the second chunk wraps the ring
        traj = TrajectoryBuffer(K, N, A, states=True)
        roll.run(K, noise=torch.randn((K, N, A), device="cuda"), trajectory=traj)
        rb_x.extend(traj)
        for k in range(K):
            rb_s.store((traj.obs_src[k], traj.obs_pos[k]), traj.actions[k], traj.rewards[k],
                       (traj.obs_src[k + 1], traj.obs_pos[k + 1]), traj.dones[k])
    assert (rb_x.head, rb_x.size()) == (rb_s.head, rb_s.size())
    idx = torch.arange(rb_x.size(), device="cuda")
    bx, bs = rb_x.get_mini_batch(0, indices=idx), rb_s.get_mini_batch(0, indices=idx)
    for key in bx:
        assert_bits(t2n(bx[key]), t2n(bs[key]), key)
