"""GPU: the SAC LSTM actor's backward pass on descriptors (fe_sac_backward, FusedSACRollout.sample / actor_losses).

* values: ``sample()`` returns ``forward``'s actions / log_probs bit for bit;
* gradients of all ten actor parameters against an f64 torch copy of the modules on the rendered states, within
  ``2e-5 max|g64| + 4 max|g_torch32 - g64|`` (the project's yardstick for the critic gradient), for the full chained
  actor loss through ``FusedTwinCritic.q``, for ``(log_probs * c).sum()`` alone and for ``actions.sum()`` alone
  (H = 32 / 64 / 128, W = 4 / 16, B from 1 to 65 536, f32 / f64 envs); the batch is checked not to be saturated
  (``max|u| < 4``) and no f64 gradient is identically zero;
* the same at the windows and grid-strides the cases above do not reach.  Worst err / tol over kinds and tensors,
  measured on an MI355X: W = 1 (no recurrent step; d w_hh is identically zero there and must come out exactly zero)
  (32, 1, 33) 0.020 and (128, 1, 31) 0.027; one step (64, 2, 33) 0.019; odd W (32, 7, 33) 0.022 and (128, 7, 257) 0.022;
  the reference's default window (32, 390, 33) 0.019 and (128, 390, 33) 0.034; a tile count that is a multiple of no
  workgroup count (32, 4, 16 449) 0.032 and (128, 4, 8 257) 0.043;
* the loss value of ``actor_losses`` against torch, the same form of bound; a wrapped ring;
* two backward calls give the same bits; ``.grad`` accumulates as torch's does; a frozen actor gets nothing and
  launches nothing; either upstream gradient alone works;
* the SAC example with ``fused_actor=True`` trains; refusals.
"""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from tests.helpers import assert_bits as _assert_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("w_ih", "w_hh", "b_ih", "b_hh", "w_l", "b_l", "w_mu", "b_mu", "w_std", "b_std")


def assert_bits(a, b):
    _assert_bits(a.detach().cpu().numpy(), b.detach().cpu().numpy())


def _env(N, W, obs_dtype=torch.float64, A=1, days=12, bars=60, seed=3):
    from finenvs_amd import TimeSeriesEnv
    from finenvs_amd.data import synthetic

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    prices, day_id, _ = synthetic.synthetic_series(days, A, bars, seed, 0.0)
    return TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=W, num_envs=N, redraw="device", seed=seed,
                         obs_dtype=obs_dtype)


def _actor(H, W, seed, A=1):
    """SACActorLSTM with the input weights scaled up so that log-returns of ~1e-3 move the gates, and the std bias
    lowered (the scaling of tools/make_sac_golden.py)."""
    from finenvs_amd.sac import SACActorLSTM

    torch.manual_seed(seed)
    a = SACActorLSTM(H=H, W=W, A=A, starting_alpha=0.7)
    with torch.no_grad():
        a.lstm.weight_ih_l0[:, :4].mul_(6.0 * np.sqrt(H))
        a.std_layer.bias.add_(-0.5)
    return a.cuda()


def _critic(H, W, seed):
    from finenvs_amd.critic import CriticLSTM

    torch.manual_seed(seed)
    c = CriticLSTM(H, W)
    with torch.no_grad():
        c.lstm.weight_ih_l0[:, :4].mul_(6.0 * np.sqrt(H))
        c.lstm.weight_ih_l0[:, 5].mul_(3.0)
        c.last_layer[0].weight.mul_(4.0)
    return c.cuda()


def _descriptors(env, B, seed=1):
    """B observation descriptors of the env's own days: the first B of the (K + 1) N rows a K-step SAC rollout records.
    While ``B <= num_envs`` those are all row 0, the RESET states of a fresh env: ``obs_pos`` is exactly 0.0 and ``obs_src``
    one of the table's day starts (at most one distinct sample per day); stepped rows begin at index ``num_envs``.
    Positions that are not zero and windows all over the table: tests/test_grad_descriptors_gpu.py."""
    from finenvs_amd.sac import FusedSACRollout, SACActorLSTM
    from finenvs_amd.trajectory import TrajectoryBuffer

    N = env.num_envs
    K = max(1, -(-B // N) - 1)
    torch.manual_seed(seed)
    roll = FusedSACRollout(env, SACActorLSTM(H=32, W=env.num_intervals).cuda())
    traj = TrajectoryBuffer(K, N, 1, device=env._dev, states=True)
    gen = torch.Generator(device=env._dev).manual_seed(seed)
    roll.run(K, noise=torch.randn((K, N, 1), generator=gen, device=env._dev), trajectory=traj)
    src, pos = traj.obs_src.reshape(-1)[:B].contiguous(), traj.obs_pos.reshape(-1, 1)[:B].contiguous()
    return src, pos, traj


def _params(actor):
    from finenvs_amd.sac import actor_parameters

    return list(actor_parameters(actor))


def _zero(*modules):
    for m in modules:
        for p in m.parameters():
            p.grad = None


def _loss(kind, actions, log_probs, q_fn, alpha, c):
    """The three scalar functions of (actions, log_probs) every case differentiates."""
    if kind == "chained":  # Actor.compute_losses (SAC/actor.py:63-81)
        mean_lp = log_probs.mean(dim=1, keepdim=True)
        return -(torch.min(*q_fn(actions)) + -alpha * mean_lp).mean()
    if kind == "log_probs":
        return (log_probs * c).sum()
    return actions.sum()


def _torch_grads(kind, actor, c1, c2, states, eps, c, dtype):
    """Loss and the ten actor gradients of copies of the modules in `dtype` on the rendered states; also max|u|."""
    a, d1, d2 = copy.deepcopy(actor).to(dtype), copy.deepcopy(c1).to(dtype), copy.deepcopy(c2).to(dtype)
    _zero(a, d1, d2)
    s = states.to(dtype)
    actions, log_probs = a.get_actions_and_log_probs(s, eps.to(dtype))
    loss = _loss(kind, actions, log_probs, lambda x: (d1(s, x), d2(s, x)), a.log_alpha.detach().exp().to(dtype), c.to(dtype))
    loss.backward()
    with torch.no_grad():
        dist = a.get_distribution(s)
        umax = float((dist.loc + eps.to(dtype) * dist.scale).abs().max())
    return loss.detach(), [p.grad for p in _params(a)], umax


def _fused_grads(kind, roll, twin, src, pos, eps, c):
    _zero(roll.actor, twin.critic_1, twin.critic_2)
    actions, log_probs = roll.sample(src, pos, eps)
    loss = _loss(kind, actions, log_probs, lambda x: twin.q(src, pos, x), roll.actor.log_alpha.detach().exp(), c)
    loss.backward()
    return loss.detach(), [p.grad.clone() for p in _params(roll.actor)], (actions.detach(), log_probs.detach())


def _check_against_f64(kind, roll, twin, env, src, pos, eps, c):
    loss, g, _ = _fused_grads(kind, roll, twin, src, pos, eps, c)
    states = env.render(src, pos)
    l32, g32, _ = _torch_grads(kind, roll.actor, twin.critic_1, twin.critic_2, states.float(), eps, c, torch.float32)
    l64, g64, umax = _torch_grads(kind, roll.actor, twin.critic_1, twin.critic_2, states.double(), eps, c, torch.float64)
    assert umax < 4.0, umax  # not saturated: 1 - tanh(u)^2 stays well above the 1e-7 guard
    for name, gf, gt, gd in zip(NAMES, g, g32, g64):
        assert gf.shape == gd.shape and gf.dtype is torch.float32, name
        # not degenerate; at W = 1 w_hh's only operand is h_0 = 0: its gradient is identically zero, the bound 0
        assert (float(gd.abs().max()) > 0) != (name == "w_hh" and int(env.num_intervals) == 1), (kind, name)
        err = float((gf.double() - gd).abs().max())
        tol = 2e-5 * float(gd.abs().max()) + 4 * float((gt.double() - gd).abs().max())
        print(f"{kind:9s} {name:6s} err {err:.3e} tol {tol:.3e} ratio {err / tol if tol else err:.3f}")
        assert err <= tol, (kind, name, err, tol)
    return loss, l32, l64


CASES = [
    (32, 4, 1, torch.float64),
    (64, 4, 31, torch.float32),
    (128, 4, 256, torch.float64),
    (32, 16, 4097, torch.float32),
    (64, 16, 256, torch.float64),
    (128, 16, 31, torch.float32),
    (32, 4, 65536, torch.float64),
    (64, 4, 65536, torch.float32),
    (128, 4, 65536, torch.float64),
    (32, 1, 33, torch.float64),      # W = 1: no recurrent step at all
    (128, 1, 31, torch.float32),
    (64, 2, 33, torch.float64),      # one recurrent step
    (32, 7, 33, torch.float32),      # odd W
    (128, 7, 257, torch.float64),
    (32, 390, 33, torch.float32),    # the reference's default window
    (128, 390, 33, torch.float64),
    (32, 4, 16449, torch.float32),   # 32 (512 + 1) + 33: 515 tiles, not a multiple of any workgroup count
    (128, 4, 8257, torch.float64),   # 32 (256 + 1) + 33: 259 tiles
]


@pytest.mark.parametrize("H,W,B,obs_dtype", CASES)
def test_gradients_against_f64_torch(H, W, B, obs_dtype):
    from finenvs_amd.critic import FusedTwinCritic
    from finenvs_amd.sac import FusedSACRollout

    env = _env(min(B, 4096), W, obs_dtype=obs_dtype)
    src, pos, _ = _descriptors(env, B)
    assert src.numel() == B
    roll = FusedSACRollout(env, _actor(H, W, 20))
    twin = FusedTwinCritic(env, _critic(H, W, 10), _critic(H, W, 11))
    gen = torch.Generator(device="cuda").manual_seed(5)
    eps = torch.randn((B, 1), generator=gen, device="cuda")
    c = torch.randn((B, 1), generator=gen, device="cuda")
    for kind in ("chained", "log_probs", "actions"):
        _check_against_f64(kind, roll, twin, env, src, pos, eps, c)


def test_sample_values_equal_forward_bit_for_bit_and_backward_is_deterministic():
    from finenvs_amd.critic import FusedTwinCritic
    from finenvs_amd.sac import FusedSACRollout

    for H, W in ((32, 4), (128, 16)):
        env = _env(300, W)
        src, pos, _ = _descriptors(env, 900)
        roll = FusedSACRollout(env, _actor(H, W, 20))
        twin = FusedTwinCritic(env, _critic(H, W, 10), _critic(H, W, 11))
        eps = torch.randn((900, 1), device="cuda")
        c = torch.randn((900, 1), device="cuda")
        fa, fl, fm, fs = roll.forward(src, pos, eps)
        _, g_a, (a, lp) = _fused_grads("chained", roll, twin, src, pos, eps, c)
        assert_bits(a, fa)
        assert_bits(lp, fl)
        assert_bits(roll.last["means"], fm)
        assert_bits(roll.last["stds"], fs)
        _, g_b, _ = _fused_grads("chained", roll, twin, src, pos, eps, c)
        for x, z in zip(g_a, g_b):
            assert_bits(x, z)


def _ring(env, K, max_size):
    from finenvs_amd.replay import ReplayBuffer

    _, _, traj = _descriptors(env, env.num_envs * (K + 1))
    buffer = ReplayBuffer(env, max_size=max_size)
    buffer.extend(traj)
    return buffer


def test_actor_losses_on_a_wrapped_ring_against_f64():
    from finenvs_amd.critic import FusedTwinCritic
    from finenvs_amd.sac import FusedSACRollout

    H, W, N, K, B = 64, 4, 200, 6, 777
    env = _env(N, W)
    buffer = _ring(env, K, N * K // 2 + 37)
    assert buffer.size() == buffer.max_size and buffer.head != 0  # wrapped
    roll = FusedSACRollout(env, _actor(H, W, 20))
    twin = FusedTwinCritic(env, _critic(H, W, 10), _critic(H, W, 11))
    idx = torch.randint(0, buffer.size(), (B,), device="cuda")
    eps = torch.randn((B, 1), device="cuda")
    _zero(roll.actor, twin.critic_1, twin.critic_2)
    roll.actor.log_alpha.grad = None
    loss, alpha_loss = roll.actor_losses(buffer, idx, twin, noise=eps)
    loss.backward()
    g = [p.grad.clone() for p in _params(roll.actor)]
    states = buffer.get_mini_batch(B, indices=idx)["states"]
    c = torch.zeros((B, 1), device="cuda")
    l32, g32, _ = _torch_grads("chained", roll.actor, twin.critic_1, twin.critic_2, states.float(), eps, c, torch.float32)
    l64, g64, _ = _torch_grads("chained", roll.actor, twin.critic_1, twin.critic_2, states.double(), eps, c, torch.float64)
    for name, gf, gt, gd in zip(NAMES, g, g32, g64):
        err = float((gf.double() - gd).abs().max())
        tol = 2e-5 * float(gd.abs().max()) + 4 * float((gt.double() - gd).abs().max())
        assert err <= tol, (name, err, tol)
    # the loss values, the same form of bound
    err, tol = abs(float(loss.detach()) - float(l64)), 2e-5 * abs(float(l64)) + 4 * abs(float(l32) - float(l64))
    print(f"actor loss {float(loss.detach()):.8f} f64 {float(l64):.8f} err {err:.3e} tol {tol:.3e}")
    assert err <= tol, (err, tol)
    # the temperature's loss on the detached log-probabilities (SAC/actor.py:77-80)
    with torch.no_grad():
        a64 = copy.deepcopy(roll.actor).double()
        _, lp64 = a64.get_actions_and_log_probs(states.double(), eps.double())
        ref = float((-a64.log_alpha.exp() * (lp64.mean(dim=1, keepdim=True) + a64.target_entropy)).mean())
    assert abs(float(alpha_loss.detach()) - ref) <= 2e-5 * abs(ref) + 1e-6
    alpha_loss.backward()
    assert roll.actor.log_alpha.grad is not None and torch.isfinite(roll.actor.log_alpha.grad).item()
    bad = idx.clone()
    bad[3] = buffer.size()
    assert torch.isnan(roll.actor_losses(buffer, bad, twin, noise=eps)[0]).item()
    with pytest.raises(ValueError):
        roll.actor_losses(buffer, idx.float(), twin, noise=eps)
    with pytest.raises(ValueError):
        roll.actor_losses(buffer, idx, twin.critic_1, noise=eps)
    other = FusedTwinCritic(_env(8, W), _critic(H, W, 10), _critic(H, W, 11))
    with pytest.raises(ValueError):
        roll.actor_losses(buffer, idx, other, noise=eps)


def test_accumulation_single_outputs_and_a_frozen_actor(monkeypatch):
    from finenvs_amd.critic import FusedTwinCritic
    from finenvs_amd.sac import FusedSACRollout

    H, W, B = 32, 4, 300
    env = _env(B, W)
    src, pos, _ = _descriptors(env, B)
    roll = FusedSACRollout(env, _actor(H, W, 20))
    twin = FusedTwinCritic(env, _critic(H, W, 10), _critic(H, W, 11))
    eps = torch.randn((B, 1), device="cuda")
    c = torch.randn((B, 1), device="cuda")
    _, once, _ = _fused_grads("chained", roll, twin, src, pos, eps, c)
    _zero(roll.actor)
    for _ in range(2):  # no zero_grad in between
        actions, log_probs = roll.sample(src, pos, eps)
        _loss("chained", actions, log_probs, lambda x: twin.q(src, pos, x), roll.actor.log_alpha.detach().exp(), c).backward()
    for p, g in zip(_params(roll.actor), once):
        torch.testing.assert_close(p.grad, 2 * g, rtol=1e-6, atol=0)
    # either upstream gradient alone: the sum of the two is the gradient of the sum (up to f32 rounding)
    _, g_lp, _ = _fused_grads("log_probs", roll, twin, src, pos, eps, c)
    _, g_ac, _ = _fused_grads("actions", roll, twin, src, pos, eps, c)
    _zero(roll.actor)
    actions, log_probs = roll.sample(src, pos, eps)
    ((log_probs * c).sum() + actions.sum()).backward()
    for p, x, z in zip(_params(roll.actor), g_lp, g_ac):
        assert float((x + z).abs().max()) > 0
        torch.testing.assert_close(p.grad, x + z, rtol=1e-4, atol=1e-5 * float((x + z).abs().max()))
    # a frozen actor: no graph, no .grad, no launch of the backward
    calls = []
    real = env._lib.fe_sac_backward
    monkeypatch.setattr(env._lib, "fe_sac_backward", lambda *a: calls.append(1) or real(*a), raising=False)
    roll.actor.requires_grad_(False)
    _zero(roll.actor)
    actions, log_probs = roll.sample(src, pos, eps)
    assert not actions.requires_grad and not log_probs.requires_grad
    q1, q2 = twin.q(src, pos, actions)
    (torch.min(q1, q2).mean() + 0.0 * log_probs.sum()).backward()  # the critics still get their gradients
    assert all(p.grad is None for p in roll.actor.parameters()) and not calls
    roll.actor.requires_grad_(True)
    actions, log_probs = roll.sample(src, pos, eps)
    actions.sum().backward()
    assert calls == [1]
    for p, g in zip(_params(roll.actor), g_ac):
        assert_bits(p.grad, g)


def test_sac_example_with_fused_actor_trains():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import sac_time_series

    hist = sac_time_series.main(num_envs=64, hidden=32, iterations=20, chunk=4, batch=64, days=12, bars=60, quiet=True,
                                fused_targets=True, fused_critics=True, fused_actor=True)
    assert len(hist) == 20
    assert all(np.isfinite(h["critic_loss"]) and np.isfinite(h["actor_loss"]) and np.isfinite(h["alpha_loss"]) for h in hist)
    hist = sac_time_series.main(num_envs=64, hidden=32, iterations=5, chunk=4, batch=64, days=12, bars=60, quiet=True,
                                fused_actor=True)
    assert len(hist) == 5
    assert all(np.isfinite(h["critic_loss"]) and np.isfinite(h["actor_loss"]) for h in hist)


def test_all_three_flags_never_render_a_mini_batch(monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import sac_time_series

    from finenvs_amd.replay import ReplayBuffer

    def refuse(self, *a, **k):
        raise AssertionError("get_mini_batch was called")

    monkeypatch.setattr(ReplayBuffer, "get_mini_batch", refuse)
    hist = sac_time_series.main(num_envs=64, hidden=32, iterations=3, chunk=4, batch=64, days=12, bars=60, quiet=True,
                                fused_targets=True, fused_critics=True, fused_actor=True)
    assert len(hist) == 3


def test_refusals():
    from finenvs_amd.sac import FusedSACRollout, SACActorLSTM

    env2 = _env(8, 4, A=2)
    roll2 = FusedSACRollout(env2, _actor(32, 4, 1))
    src2 = torch.zeros((8,), dtype=torch.int64, device="cuda")
    pos2 = torch.zeros((8, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="one asset"):
        roll2.sample(src2, pos2, torch.zeros((8, 1), device="cuda"))
    # the C ABI refuses the A = 2 env itself, after the null checks and before it touches any other pointer
    from finenvs_amd import _lib

    grads = _lib.FeSacGrads(*([16] * 10))
    rc = env2._lib.fe_sac_backward(env2._handle, 16, 16, 16, 16, 16, 16, 0.0, 16, 0.0, 32, 16, 16, 8, 16, 16, 16, 16, 16,
                                   16, C.byref(grads), None)
    assert rc == _lib.FE_ERR_ARG
    msg = env2._lib.fe_last_error()
    assert b"fe_sac_backward" in msg and b"2 assets" in msg, msg
    env = _env(64, 4)
    with pytest.raises(ValueError):
        FusedSACRollout(env, SACActorLSTM(H=48, W=4).cuda())
    src, pos, _ = _descriptors(env, 64)
    eps = torch.randn((64, 1), device="cuda")
    roll = FusedSACRollout(env, _actor(32, 4, 1))
    for bad in (None, eps.double(), eps.reshape(64), eps[:63], eps.cpu()):
        with pytest.raises(ValueError, match="noise"):
            roll.sample(src, pos, bad)
    roll.actor.double()
    with pytest.raises(ValueError, match="float32"):
        roll.sample(src, pos, eps)
    roll.actor.float().cpu()
    with pytest.raises(ValueError, match="device"):
        roll.sample(src, pos, eps)
