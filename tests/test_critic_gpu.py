"""GPU: the fused twin LSTM critics and their Bellman targets (fe_twin_q_forward / fe_twin_q_target, finenvs_amd/critic.py).

* numerics: ``forward`` on observation descriptors against torch ``CriticLSTM`` in fp32 on the rendered observations
  within 1e-5 absolute (partial tiles, B not a multiple of 32, W = 4 / 16, f32 / f64 envs, ragged days);
* bit for bit: with the action's weight zero a critic equals ``FusedLSTMRollout(output_activation="none").forward``;
  swapping the critics swaps q1 / q2 and keeps the targets; given the kernel's own q1, q2, log_probs and alpha the
  epilogue equals torch's expression;
* ``sac_targets`` / ``td3_targets`` against the torch restatements of both ``compute_targets`` on
  ``get_mini_batch(indices=same)``; ring edge cases (done rows, out-of-range indices); updates seen at once; refusals;
  the SAC example with ``fused_targets=True``.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests.helpers import assert_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMA = 0.99


def t2n(t):
    return t.detach().cpu().numpy()


def _env(N, W, days=12, bars=60, drop=0.0, obs_dtype=torch.float64, A=1, seed=3):
    from finenvs_amd import TimeSeriesEnv
    from finenvs_amd.data import synthetic

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    prices, day_id, _ = synthetic.synthetic_series(days, A, bars, seed, drop)
    return TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=W, num_envs=N, redraw="device", seed=seed,
                         obs_dtype=obs_dtype)


def _critic(H, W, seed):
    """CriticLSTM with the input weights scaled up so that log-returns of ~1e-3 and the action move the gates."""
    from finenvs_amd.critic import CriticLSTM

    torch.manual_seed(seed)
    c = CriticLSTM(H, W)
    with torch.no_grad():
        c.lstm.weight_ih_l0[:, :4].mul_(6.0 * np.sqrt(H))
        c.lstm.weight_ih_l0[:, 5].mul_(3.0)
        c.last_layer[0].weight.mul_(4.0)
    return c.cuda()


def _actor(H, W, seed):
    from finenvs_amd.sac import SACActorLSTM

    torch.manual_seed(seed)
    actor = SACActorLSTM(H=H, W=W, starting_alpha=0.2)
    with torch.no_grad():
        actor.lstm.weight_ih_l0[:, :4].mul_(6.0 * np.sqrt(H))
        actor.mu_layer.weight.mul_(4.0)
    return actor.cuda()


def _filled(env, H, K, seed=1):
    """A SAC rollout of K steps: its trajectory (descriptors of K + 1 rows) and a replay ring holding it."""
    from finenvs_amd.replay import ReplayBuffer
    from finenvs_amd.sac import FusedSACRollout
    from finenvs_amd.trajectory import TrajectoryBuffer

    N = env.num_envs
    roll = FusedSACRollout(env, _actor(H, env.num_intervals, seed))
    traj = TrajectoryBuffer(K, N, 1, device=env._dev, states=True)
    gen = torch.Generator(device=env._dev).manual_seed(seed)
    roll.run(K, noise=torch.randn((K, N, 1), generator=gen, device=env._dev), trajectory=traj)
    buffer = ReplayBuffer(env, max_size=K * N + 7)
    buffer.extend(traj)
    return roll, traj, buffer


def _descriptors(traj):
    return traj.obs_src.reshape(-1).contiguous(), traj.obs_pos.reshape(-1, 1).contiguous()


@pytest.mark.parametrize("N,K,W,H,obs_dtype,drop", [
    (300, 2, 4, 32, torch.float64, 0.0),      # B = 900: partial tiles, not a multiple of 32
    (260, 1, 16, 64, torch.float32, 0.1),     # ragged days
    (77, 2, 4, 128, torch.float64, 0.05),     # B = 231
    (131, 1, 16, 32, torch.float32, 0.0),
    (45, 3, 4, 64, torch.float64, 0.1),
])
def test_forward_against_torch_critics_fp32(N, K, W, H, obs_dtype, drop):
    from finenvs_amd.critic import FusedTwinCritic

    env = _env(N, W, drop=drop, obs_dtype=obs_dtype)
    _, traj, _ = _filled(env, H, K)
    src, pos = _descriptors(traj)
    B = src.numel()
    c1, c2 = _critic(H, W, 10), _critic(H, W, 11)
    actions = torch.rand((B, 1), device="cuda") * 2 - 1
    q1, q2 = FusedTwinCritic(env, c1, c2).forward(src, pos, actions)
    obs = env.render(src, pos).float()
    with torch.no_grad():
        t1, t2 = c1(obs, actions), c2(obs, actions)
    assert q1.shape == (B, 1) and q2.shape == (B, 1)
    np.testing.assert_allclose(t2n(q1), t2n(t1), rtol=0, atol=1e-5)
    np.testing.assert_allclose(t2n(q2), t2n(t2), rtol=0, atol=1e-5)
    assert float(t1.std()) > 1e-2 and float((t1 - t2).abs().max()) > 1e-2  # not degenerate


@pytest.mark.parametrize("H", [32, 64, 128])
def test_zero_action_weight_equals_the_lstm_value_head_bit_for_bit(H):
    from finenvs_amd.critic import FusedTwinCritic
    from finenvs_amd.rollout import FusedLSTMRollout

    env = _env(200, 4)
    _, traj, _ = _filled(env, H, 2)
    src, pos = _descriptors(traj)
    c1, c2 = _critic(H, 4, 20), _critic(H, 4, 21)
    with torch.no_grad():
        c1.lstm.weight_ih_l0[:, 5].zero_()
    q1, _ = FusedTwinCritic(env, c1, c2).forward(src, pos, torch.rand((src.numel(), 1), device="cuda") * 2 - 1)
    lstm = c1.lstm
    head = FusedLSTMRollout(env, lstm.weight_ih_l0[:, :5], lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0,
                            c1.last_layer[0].weight, float(c1.last_layer[0].bias), output_activation="none")
    assert_bits(t2n(q1), t2n(head.forward(src, pos)), "critic with w_ih[:, 5] = 0 == LSTM value head")


def test_swapping_the_critics_swaps_the_values_and_keeps_the_targets_bit_for_bit():
    from finenvs_amd.critic import FusedTwinCritic

    H, W = 64, 4
    env = _env(150, W)
    roll, traj, buffer = _filled(env, H, 3)
    src, pos = _descriptors(traj)
    c1, c2 = _critic(H, W, 30), _critic(H, W, 31)
    a = torch.rand((src.numel(), 1), device="cuda") * 2 - 1
    f12, f21 = FusedTwinCritic(env, c1, c2), FusedTwinCritic(env, c2, c1)
    q1, q2 = f12.forward(src, pos, a)
    p1, p2 = f21.forward(src, pos, a)
    assert_bits(t2n(q1), t2n(p2), "q1 == swapped q2")
    assert_bits(t2n(q2), t2n(p1), "q2 == swapped q1")
    s1, s2 = FusedTwinCritic(env, c1, c1).forward(src, pos, a)
    assert_bits(t2n(s1), t2n(s2), "identical critics")
    idx = torch.randint(0, buffer.size(), (300,), device="cuda")
    eps = torch.randn((300, 1), device="cuda")
    la = roll.actor.log_alpha
    y12 = f12.sac_targets(buffer, idx, roll, eps, GAMMA, la)
    y21 = f21.sac_targets(buffer, idx, roll, eps, GAMMA, la)
    assert_bits(t2n(y12), t2n(y21), "SAC targets under the swap")
    from finenvs_amd.rollout import FusedLSTMRollout

    lstm = nn.LSTM(5, H).cuda()
    lin = nn.Linear(H, 1).cuda()
    target = FusedLSTMRollout.from_modules(env, lstm, lin, output_activation="tanh")
    z12 = f12.td3_targets(buffer, idx, target, eps, GAMMA, 0.2, 0.5)
    z21 = f21.td3_targets(buffer, idx, target, eps, GAMMA, 0.2, 0.5)
    assert_bits(t2n(z12), t2n(z21), "TD3 targets under the swap")


@pytest.mark.parametrize("H,W,obs_dtype", [(32, 4, torch.float64), (128, 16, torch.float32), (64, 4, torch.float32)])
def test_sac_targets_against_torch_and_the_epilogue_bit_for_bit(H, W, obs_dtype):
    from finenvs_amd.critic import FusedTwinCritic, torch_sac_targets

    env = _env(230, W, obs_dtype=obs_dtype, drop=0.05)
    roll, _, buffer = _filled(env, H, 4)
    with torch.no_grad():  # some done rows in the ring
        buffer.dones[::7] = 1.0
    c1, c2 = _critic(H, W, 40), _critic(H, W, 41)
    twin = FusedTwinCritic(env, c1, c2)
    B = 1000
    idx = torch.randint(0, buffer.size(), (B,), device="cuda")
    eps = torch.randn((B, 1), device="cuda")
    y = twin.sac_targets(buffer, idx, roll, eps, GAMMA, roll.actor.log_alpha, reward_scale=0.01)
    b = buffer.get_mini_batch(B, indices=idx)
    want = torch_sac_targets(roll.actor, c1, c2, b["rewards"], b["next_states"], b["dones"], eps, GAMMA, reward_scale=0.01)
    last = twin.last
    with torch.no_grad():
        _, lp_t = roll.actor.get_actions_and_log_probs(b["next_states"], eps)
    dlp = (last["log_probs"] - lp_t).abs()
    assert float(dlp.max()) < 1e-3  # the SAC head's own bound (tests/test_sac_rollout_gpu.py)
    # beyond the critics' 1e-5, a target differs from torch's by gamma * alpha times the log-probability's difference
    bound = 1e-5 + GAMMA * 0.2 * dlp
    assert bool(((y - want).abs() <= bound).all()), float((y - want).abs().max())
    # the epilogue alone, from the kernel's own q1, q2, log_probs and alpha: torch's expression bit for bit
    r, d = b["rewards"] * 0.01, b["dones"]
    expr = r + GAMMA * (1 - d) * (torch.min(last["q1"], last["q2"]) + (-last["alpha"] * last["log_probs"]))
    assert_bits(t2n(y), t2n(expr), "SAC epilogue")
    done = b["dones"][:, 0] == 1
    assert bool(done.any()) and torch.equal(y[done], r[done])  # d = 1: y == r exactly


@pytest.mark.parametrize("H", [32, 128])
def test_td3_targets_against_torch_and_the_epilogue_bit_for_bit(H):
    from finenvs_amd.critic import FusedTwinCritic, torch_td3_targets
    from finenvs_amd.rollout import FusedLSTMRollout

    W = 4
    env = _env(190, W, drop=0.1)
    _, _, buffer = _filled(env, H, 3)
    with torch.no_grad():
        buffer.dones[1::5] = 1.0
    c1, c2 = _critic(H, W, 50), _critic(H, W, 51)
    torch.manual_seed(52)
    lstm, lin = nn.LSTM(5, H, batch_first=True).cuda(), nn.Linear(H, 1).cuda()
    with torch.no_grad():
        lstm.weight_ih_l0[:, :4].mul_(6.0 * np.sqrt(H))
        lin.weight.mul_(6.0)  # actions over the whole range, some beyond the clamp after smoothing
    target = FusedLSTMRollout.from_modules(env, lstm, lin, output_activation="tanh")
    twin = FusedTwinCritic(env, c1, c2)
    B = 777
    idx = torch.randint(0, buffer.size(), (B,), device="cuda")
    eps = torch.randn((B, 1), device="cuda")
    y = twin.td3_targets(buffer, idx, target, eps, GAMMA, 0.2, 0.5)
    b = buffer.get_mini_batch(B, indices=idx)

    def actor(x):
        return torch.tanh(lin(lstm(x)[0][:, -1, :]))

    want = torch_td3_targets(actor, c1, c2, b["rewards"], b["next_states"], b["dones"], eps, GAMMA, 0.2, 0.5)
    np.testing.assert_allclose(t2n(y), t2n(want), rtol=0, atol=1e-5)
    last = twin.last
    expr = b["rewards"] + GAMMA * (1 - b["dones"]) * torch.minimum(last["q1"], last["q2"])
    assert_bits(t2n(y), t2n(expr), "TD3 epilogue")
    # the smoothed action the critics saw: the kernel's q1 equals the forward on the same clamped action
    a = torch.clamp(last["next_actions"] + torch.clamp(eps * 0.2, -0.5, 0.5), -1, 1)
    src, pos = buffer.next_src[buffer.physical(idx)], buffer.next_pos[buffer.physical(idx)]
    q1, _ = twin.forward(src, pos, a)
    assert_bits(t2n(q1), t2n(last["q1"]), "TD3 smoothing in the kernel")


def test_out_of_range_indices_give_nan_rows_and_count():
    from finenvs_amd.critic import FusedTwinCritic

    H, W = 32, 4
    env = _env(64, W)
    roll, _, buffer = _filled(env, H, 2)
    twin = FusedTwinCritic(env, _critic(H, W, 60), _critic(H, W, 61))
    size = buffer.size()
    idx = torch.tensor([0, -1, 5, size, size + 40, size - 1, -1000], device="cuda")
    bad = torch.tensor([False, True, False, True, True, False, True], device="cuda")
    before = int(buffer.errors.item())
    y = twin.sac_targets(buffer, idx, roll, torch.zeros((7, 1), device="cuda"), GAMMA, roll.actor.log_alpha)
    assert int(buffer.errors.item()) - before == 4
    assert bool(torch.isnan(y[bad]).all()) and bool(torch.isfinite(y[~bad]).all())
    assert bool(torch.isnan(twin.last["q1"][bad]).all()) and bool(torch.isnan(twin.last["q2"][bad]).all())
    good = twin.sac_targets(buffer, idx[~bad], roll, torch.zeros((3, 1), device="cuda"), GAMMA, roll.actor.log_alpha)
    assert_bits(t2n(y[~bad]), t2n(good), "valid rows do not depend on the invalid ones")


def test_an_optimizer_step_and_a_soft_update_are_seen_by_the_next_call():
    from finenvs_amd.critic import FusedTwinCritic

    H, W = 64, 4
    env = _env(96, W)
    _, traj, _ = _filled(env, H, 2)
    src, pos = _descriptors(traj)
    c1, c2 = _critic(H, W, 70), _critic(H, W, 71)
    twin = FusedTwinCritic(env, c1, c2)
    a = torch.rand((src.numel(), 1), device="cuda") * 2 - 1
    q1, q2 = twin.forward(src, pos, a)
    obs = env.render(src, pos).float()
    opt = torch.optim.SGD(c1.parameters(), lr=0.5)
    loss = c1(obs, a).square().mean()
    opt.zero_grad()
    loss.backward()
    opt.step()
    src2 = _critic(H, W, 72)
    with torch.no_grad():  # soft update of critic 2 towards another critic
        for t, s in zip(c2.parameters(), src2.parameters()):
            t.mul_(0.5).add_(s, alpha=0.5)
    n1, n2 = twin.forward(src, pos, a)
    with torch.no_grad():
        t1, t2 = c1(obs, a), c2(obs, a)
    assert float((n1 - q1).abs().max()) > 1e-3 and float((n2 - q2).abs().max()) > 1e-3
    np.testing.assert_allclose(t2n(n1), t2n(t1), rtol=0, atol=1e-5)
    np.testing.assert_allclose(t2n(n2), t2n(t2), rtol=0, atol=1e-5)


def test_refusals():
    from finenvs_amd import _lib
    from finenvs_amd.critic import CriticLSTM, FusedTwinCritic

    multi = _env(16, 4, A=2)
    with pytest.raises(ValueError, match="one asset"):
        FusedTwinCritic(multi, _critic(32, 4, 80), _critic(32, 4, 81))
    env = _env(64, 4)
    with pytest.raises(ValueError, match="device"):
        FusedTwinCritic(env, _critic(32, 4, 80), CriticLSTM(32, 4))  # critic 2 on the host
    with pytest.raises(ValueError, match="same hidden size"):
        FusedTwinCritic(env, _critic(32, 4, 80), _critic(64, 4, 81))
    c1 = _critic(32, 4, 80)
    twin = FusedTwinCritic(env, c1, _critic(32, 4, 81))
    _, traj, buffer = _filled(env, 32, 1)
    src, pos = _descriptors(traj)
    B = src.numel()
    with pytest.raises(ValueError, match="actions"):
        twin.forward(src, pos, torch.zeros((B, 1), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="actions"):
        twin.forward(src, pos, torch.zeros((B + 1, 1), device="cuda"))
    with pytest.raises(ValueError, match="obs_pos"):
        twin.forward(src, pos.float(), torch.zeros((B, 1), device="cuda"))
    c1.cpu()
    with pytest.raises(ValueError, match="critic_1"):
        twin.forward(src, pos, torch.zeros((B, 1), device="cuda"))
    c1.cuda()
    with pytest.raises(ValueError, match="FusedLSTMRollout"):
        twin.td3_targets(buffer, None, object(), batch_size=4)
    # the C ABI: an env of two assets (the Python front end refuses it before)
    w = _lib.FeCriticWeights(1, 1, 1, 1)
    lib = env._lib
    rc = lib.fe_twin_q_forward(multi._handle, 1, _ref(w), _ref(w), 32, 1, 1, 1, 4, 1, 1, None)
    assert rc == _lib.FE_ERR_ARG and b"A = 1 only" in lib.fe_last_error()


def _ref(x):
    import ctypes

    return ctypes.byref(x)


def test_example_with_fused_targets_matches_the_unfused_first_update():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import sac_time_series

    kw = dict(num_envs=256, iterations=3, chunk=4, batch=128, hidden=64, quiet=True, seed=5)
    fused = sac_time_series.main(fused_targets=True, **kw)
    plain = sac_time_series.main(fused_targets=False, **kw)
    assert fused and all(np.isfinite([h["critic_loss"], h["actor_loss"], h["alpha_loss"]]).all() for h in fused)
    assert fused[0]["iteration"] == plain[0]["iteration"]
    np.testing.assert_allclose(fused[0]["critic_loss"], plain[0]["critic_loss"], rtol=1e-4, atol=1e-7)
