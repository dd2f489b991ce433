"""GPU: the twin LSTM critics' backward pass on descriptors (fe_twin_q_backward, FusedTwinCritic.q / critic_loss).

* values: ``q()`` returns ``forward``'s q1 / q2 bit for bit;
* gradients of every parameter of both critics and of the actions against an f64 torch ``CriticLSTM`` on the rendered
  states, within ``2e-5 max|g64| + 4 max|g_torch32 - g64|`` (H = 32 / 64 / 128, W = 4 / 16, B from 1 to 65 536,
  f32 / f64 envs, a wrapped ring);
* the same at the windows and grid-strides the cases above do not reach.  Worst err / tol over the thirteen tensors,
  measured on an MI355X: W = 1 (no recurrent step; d w_hh is identically zero there and must come out exactly zero)
  (32, 1, 33) 0.028 and (128, 1, 31) 0.021; one step (64, 2, 33) 0.026; odd W (32, 7, 33) 0.032 and (128, 7, 257) 0.023;
  the reference's default window (32, 390, 33) 0.039 and (128, 390, 33) 0.022; a tile count that is a multiple of no
  workgroup count (32, 4, 16 449) 0.031 and (128, 4, 8 257) 0.028;
* two backward calls give the same bits; ``.grad`` accumulates as torch's does; frozen critics and actions without
  ``requires_grad`` get nothing; TD3's actor loss runs critic 1 only;
* one Adam step of ``critic_loss`` matches the torch path; the SAC example with ``fused_critics=True`` trains;
* refusals.
"""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import assert_bits as _assert_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assert_bits(a, b):
    _assert_bits(a.detach().cpu().numpy(), b.detach().cpu().numpy())


def _env(N, W, obs_dtype=torch.float64, A=1, days=12, bars=60, seed=3):
    from finenvs_amd import TimeSeriesEnv
    from finenvs_amd.data import synthetic

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    prices, day_id, _ = synthetic.synthetic_series(days, A, bars, seed, 0.0)
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


def _params(c):
    from finenvs_amd.critic import critic_parameters

    return list(critic_parameters(c))


def _torch_grads(c1, c2, states, actions, y, dtype):
    """Gradients of MSE(q1, y) + MSE(q2, y) of copies of the critics in `dtype`: 12 parameter grads and d actions."""
    d1, d2 = copy.deepcopy(c1).to(dtype), copy.deepcopy(c2).to(dtype)
    for p in d1.parameters():
        p.grad = None
    for p in d2.parameters():
        p.grad = None
    a = actions.detach().to(dtype).clone().requires_grad_()
    s = states.to(dtype)
    loss = F.mse_loss(d1(s, a), y.to(dtype)) + F.mse_loss(d2(s, a), y.to(dtype))
    loss.backward()
    return [p.grad for p in _params(d1) + _params(d2)] + [a.grad]


def _fused_grads(fused, src, pos, actions, y):
    for p in fused.critic_1.parameters():
        p.grad = None
    for p in fused.critic_2.parameters():
        p.grad = None
    a = actions.detach().clone().requires_grad_()
    q1, q2 = fused.q(src, pos, a)
    loss = F.mse_loss(q1, y) + F.mse_loss(q2, y)
    loss.backward()
    return [p.grad.clone() for p in _params(fused.critic_1) + _params(fused.critic_2)] + [a.grad.clone()], (q1, q2)


def _check_against_f64(fused, env, src, pos, actions, y):
    g, _ = _fused_grads(fused, src, pos, actions, y)
    states = env.render(src, pos)
    g32 = _torch_grads(fused.critic_1, fused.critic_2, states.float(), actions, y, torch.float32)
    g64 = _torch_grads(fused.critic_1, fused.critic_2, states.double(), actions, y, torch.float64)
    names = [f"c{c}.{k}" for c in (1, 2) for k in ("w_ih", "w_hh", "b_ih", "b_hh", "w_out", "b_out")] + ["d_actions"]
    for name, gf, gt, gd in zip(names, g, g32, g64):
        assert gf.shape == gd.shape and gf.dtype is torch.float32, name
        err = float((gf.double() - gd).abs().max())
        tol = 2e-5 * float(gd.abs().max()) + 4 * float((gt.double() - gd).abs().max())
        print(f"{name:10s} err {err:.3e} tol {tol:.3e} ratio {err / tol if tol else err:.3f}")
        assert err <= tol, (name, err, tol)
    # not degenerate; at W = 1 w_hh's only operand is h_0 = 0: its gradient is identically zero, the bound above 0
    assert (float(g64[1].abs().max()) > 0) != (int(env.num_intervals) == 1) and float(g64[-1].abs().max()) > 0
    return g


@pytest.mark.parametrize("H,W,B,obs_dtype", [
    (32, 4, 1, torch.float64),
    (64, 4, 31, torch.float32),
    (128, 4, 256, torch.float64),
    (32, 16, 4097, torch.float32),
    (64, 16, 256, torch.float64),
    (128, 16, 31, torch.float32),
    (32, 4, 65536, torch.float64),
    (64, 4, 65536, torch.float32),
    (128, 4, 65536, torch.float64),
    (128, 16, 4097, torch.float64),
    (32, 1, 33, torch.float64),      # W = 1: no recurrent step at all
    (128, 1, 31, torch.float32),
    (64, 2, 33, torch.float64),      # one recurrent step
    (32, 7, 33, torch.float32),      # odd W
    (128, 7, 257, torch.float64),
    (32, 390, 33, torch.float32),    # the reference's default window
    (128, 390, 33, torch.float64),
    (32, 4, 16449, torch.float32),   # 32 (512 + 1) + 33: 515 tiles, not a multiple of any workgroup count
    (128, 4, 8257, torch.float64),   # 32 (256 + 1) + 33: 259 tiles
])
def test_gradients_against_f64_torch(H, W, B, obs_dtype):
    from finenvs_amd.critic import FusedTwinCritic

    env = _env(min(B, 4096), W, obs_dtype=obs_dtype)
    src, pos, _ = _descriptors(env, B)
    assert src.numel() == B
    fused = FusedTwinCritic(env, _critic(H, W, 10), _critic(H, W, 11))
    gen = torch.Generator(device="cuda").manual_seed(5)
    actions = torch.rand((B, 1), generator=gen, device="cuda") * 2 - 1
    y = torch.randn((B, 1), generator=gen, device="cuda")
    _check_against_f64(fused, env, src, pos, actions, y)


def test_q_values_equal_forward_bit_for_bit_and_backward_is_deterministic():
    from finenvs_amd.critic import FusedTwinCritic

    for H, W in ((32, 4), (128, 16)):
        env = _env(300, W)
        src, pos, _ = _descriptors(env, 900)
        fused = FusedTwinCritic(env, _critic(H, W, 10), _critic(H, W, 11))
        actions = torch.rand((900, 1), device="cuda") * 2 - 1
        y = torch.randn((900, 1), device="cuda")
        f1, f2 = fused.forward(src, pos, actions)
        g_a, (q1, q2) = _fused_grads(fused, src, pos, actions, y)
        assert_bits(q1, f1)
        assert_bits(q2, f2)
        g_b, _ = _fused_grads(fused, src, pos, actions, y)
        for x, z in zip(g_a, g_b):
            assert_bits(x, z)


def test_critic_loss_on_a_wrapped_ring_against_f64_and_out_of_range_nan():
    from finenvs_amd.critic import FusedTwinCritic
    from finenvs_amd.replay import ReplayBuffer

    H, W, N, K = 64, 4, 200, 6
    env = _env(N, W)
    _, _, traj = _descriptors(env, N * (K + 1))
    buffer = ReplayBuffer(env, max_size=N * K // 2 + 37)
    buffer.extend(traj)
    assert buffer.size() == buffer.max_size and buffer.head != 0  # wrapped
    fused = FusedTwinCritic(env, _critic(H, W, 10), _critic(H, W, 11))
    idx = torch.randint(0, buffer.size(), (777,), device="cuda")
    y = torch.randn((777, 1), device="cuda")
    for p in fused.critic_1.parameters():
        p.grad = None
    for p in fused.critic_2.parameters():
        p.grad = None
    loss = fused.critic_loss(buffer, idx, y)
    loss.backward()
    g = [p.grad.clone() for p in _params(fused.critic_1) + _params(fused.critic_2)]
    b = buffer.get_mini_batch(777, indices=idx)
    states, actions = b["states"], b["actions"]
    g32 = _torch_grads(fused.critic_1, fused.critic_2, states.float(), actions, y, torch.float32)
    g64 = _torch_grads(fused.critic_1, fused.critic_2, states.double(), actions, y, torch.float64)
    for gf, gt, gd in zip(g, g32, g64):
        err = float((gf.double() - gd).abs().max())
        assert err <= 2e-5 * float(gd.abs().max()) + 4 * float((gt.double() - gd).abs().max()), err
    with torch.no_grad():
        ref = F.mse_loss(fused.critic_1(states, actions), y) + F.mse_loss(fused.critic_2(states, actions), y)
    assert abs(float(loss.detach()) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref)))
    bad = idx.clone()
    bad[3] = buffer.size()
    assert torch.isnan(fused.critic_loss(buffer, bad, y)).item()


def test_accumulation_frozen_critics_and_actions_without_grad():
    from finenvs_amd.critic import FusedTwinCritic

    H, W, B = 32, 4, 300
    env = _env(B, W)
    src, pos, _ = _descriptors(env, B)
    fused = FusedTwinCritic(env, _critic(H, W, 10), _critic(H, W, 11))
    actions = torch.rand((B, 1), device="cuda") * 2 - 1
    y = torch.randn((B, 1), device="cuda")
    once, _ = _fused_grads(fused, src, pos, actions, y)
    for p in fused.critic_1.parameters():
        p.grad = None
    for p in fused.critic_2.parameters():
        p.grad = None
    a = actions.clone().requires_grad_()
    for _ in range(2):  # no zero_grad in between
        q1, q2 = fused.q(src, pos, a)
        (F.mse_loss(q1, y) + F.mse_loss(q2, y)).backward()
    for p, g in zip(_params(fused.critic_1) + _params(fused.critic_2), once[:12]):
        torch.testing.assert_close(p.grad, 2 * g, rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(a.grad, 2 * once[12], rtol=1e-6, atol=1e-7)
    # critic 2 frozen, actions without requires_grad
    for p in fused.critic_1.parameters():
        p.grad = None
    fused.critic_2.requires_grad_(False)
    for p in fused.critic_2.parameters():
        p.grad = None
    a = actions.clone()
    q1, q2 = fused.q(src, pos, a)
    (F.mse_loss(q1, y) + F.mse_loss(q2, y)).backward()
    assert all(p.grad is None for p in fused.critic_2.parameters())
    assert a.grad is None
    for p, g in zip(_params(fused.critic_1), once[:6]):
        assert_bits(p.grad, g)
    # a frozen critic still passes dQ/da on
    fused.critic_1.requires_grad_(False)
    a = actions.clone().requires_grad_()
    q1, q2 = fused.q(src, pos, a)
    (F.mse_loss(q1, y) + F.mse_loss(q2, y)).backward()
    assert_bits(a.grad, once[12])


def test_td3_actor_loss_runs_critic_1_only():
    from finenvs_amd.critic import FusedTwinCritic

    H, W, B = 128, 4, 513
    env = _env(B, W)
    src, pos, _ = _descriptors(env, B)
    fused = FusedTwinCritic(env, _critic(H, W, 10), _critic(H, W, 11))
    a = (torch.rand((B, 1), device="cuda") * 2 - 1).requires_grad_()
    q1, _ = fused.q(src, pos, a)
    (-q1.mean()).backward()  # TD3/actor.py compute_loss
    assert all(p.grad is None for p in fused.critic_2.parameters())
    assert all(p.grad is not None for p in fused.critic_1.parameters())
    states = env.render(src, pos)
    grads = []
    for dtype in (torch.float32, torch.float64):
        c = copy.deepcopy(fused.critic_1).to(dtype)
        at = a.detach().to(dtype).clone().requires_grad_()
        (-c(states.to(dtype), at).mean()).backward()
        grads.append(at.grad)
    err = float((a.grad.double() - grads[1]).abs().max())
    assert err <= 2e-5 * float(grads[1].abs().max()) + 4 * float((grads[0].double() - grads[1]).abs().max()), err


def test_one_adam_step_of_critic_loss_matches_torch():
    from finenvs_amd.critic import FusedTwinCritic
    from finenvs_amd.replay import ReplayBuffer

    H, W, N, K = 128, 4, 256, 4
    env = _env(N, W)
    _, _, traj = _descriptors(env, N * (K + 1))
    buffer = ReplayBuffer(env, max_size=N * K)
    buffer.extend(traj)
    c1, c2 = _critic(H, W, 10), _critic(H, W, 11)
    t1, t2 = copy.deepcopy(c1), copy.deepcopy(c2)
    fused = FusedTwinCritic(env, c1, c2)
    opt = torch.optim.Adam(list(c1.parameters()) + list(c2.parameters()), lr=3e-4)
    topt = torch.optim.Adam(list(t1.parameters()) + list(t2.parameters()), lr=3e-4)
    idx = torch.randint(0, buffer.size(), (256,), device="cuda")
    y = torch.randn((256, 1), device="cuda")
    opt.zero_grad()
    fused.critic_loss(buffer, idx, y).backward()
    opt.step()
    b = buffer.get_mini_batch(256, indices=idx)
    topt.zero_grad()
    (F.mse_loss(t1(b["states"], b["actions"]), y) + F.mse_loss(t2(b["states"], b["actions"]), y)).backward()
    topt.step()
    for p, q in zip(list(c1.parameters()) + list(c2.parameters()), list(t1.parameters()) + list(t2.parameters())):
        assert float((p - q).abs().max()) <= 1e-5


def test_sac_example_with_fused_critics_trains():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import sac_time_series

    hist = sac_time_series.main(num_envs=64, hidden=32, iterations=20, chunk=4, batch=64, days=12, bars=60, quiet=True,
                                fused_targets=True, fused_critics=True)
    assert len(hist) == 20
    assert all(np.isfinite(h["critic_loss"]) and np.isfinite(h["actor_loss"]) for h in hist)
    hist = sac_time_series.main(num_envs=64, hidden=32, iterations=5, chunk=4, batch=64, days=12, bars=60, quiet=True,
                                fused_critics=True)
    assert all(np.isfinite(h["critic_loss"]) for h in hist)


def test_refusals():
    from finenvs_amd.critic import CriticLSTM, FusedTwinCritic

    env2 = _env(8, 4, A=2)
    with pytest.raises(ValueError):
        FusedTwinCritic(env2, _critic(32, 4, 1), _critic(32, 4, 2))
    env = _env(64, 4)
    with pytest.raises(ValueError):
        FusedTwinCritic(env, CriticLSTM(48, 4).cuda(), CriticLSTM(48, 4).cuda())
    fused = FusedTwinCritic(env, _critic(32, 4, 1), _critic(32, 4, 2))
    src, pos, _ = _descriptors(env, 64)
    a = torch.zeros((64, 1), device="cuda", requires_grad=True)
    fused.critic_2.cpu()
    with pytest.raises(ValueError, match="device"):
        fused.q(src, pos, a)
    fused.critic_2.cuda()
    with pytest.raises(ValueError):
        fused.q(src, pos, a.detach().double())
