"""GPU: the one-output LSTM head's backward pass on descriptors (fe_lstm_backward, finenvs_amd/lstm_head.py).

* values: ``head(src, pos)`` returns ``FusedLSTMRollout.from_modules(...).forward(src, pos)`` bit for bit, tanh and none;
* gradients of the six parameters (and of PPO's ``log_std``) against an f64 torch copy of the module on the rendered
  states, within ``2e-5 max|g64| + 4 max|g_torch32 - g64|`` (the project's yardstick for the critic and the SAC actor
  gradients), for the PPO actor loss, the PPO critic loss, the TD3 actor loss chained through ``FusedTwinCritic.q`` and a
  plain ``y.sum()`` (H = 32 / 64 / 128, W = 4 / 16, B in {1, 31, 33, 4 097, 65 536}, f32 / f64 envs); the batch is
  checked not to be saturated (``max|p| < 4``) and no f64 gradient is identically zero;
* the same at the windows and grid-strides the cases above do not reach.  Worst err / tol over kinds and tensors,
  measured on an MI355X: W = 1 (no recurrent step; d w_hh is identically zero there and must come out exactly zero)
  (32, 1, 33) 0.015 and (128, 1, 31) 0.055; one step (64, 2, 33) 0.021; odd W (32, 7, 33) 0.024 and (128, 7, 257) 0.043;
  the reference's default window, one MFMA chain over 32 x 390 columns per weight tile, (32, 390, 33) 0.043 and
  (128, 390, 33) 0.037; a tile count that is a multiple of no workgroup count, so that some workgroups add a second tile
  to their partials and others do not, (32, 4, 16 449) 0.047 and (128, 4, 8 257) 0.069;
* ``td3_actor_loss`` on a wrapped replay ring, the same bound;
* two backward calls give the same bits; ``.grad`` accumulates as torch's does; a frozen head gets nothing and launches
  nothing; B = 0 works;
* the PPO example with ``fused_update=True`` trains without rendering anything, and the kernel acts with the updated
  weights; refusals.
"""
import copy
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests.helpers import assert_bits as _assert_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("w_ih", "w_hh", "b_ih", "b_hh", "w_out", "b_out")
CLIP, ENT = 0.2, 0.01


def assert_bits(a, b):
    _assert_bits(a.detach().cpu().numpy(), b.detach().cpu().numpy())


def _env(N, W, obs_dtype=torch.float64, A=1, days=12, bars=60, seed=3):
    from finenvs_amd import TimeSeriesEnv
    from finenvs_amd.data import synthetic

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    prices, day_id, _ = synthetic.synthetic_series(days, A, bars, seed, 0.0)
    return TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=W, num_envs=N, redraw="device", seed=seed,
                         obs_dtype=obs_dtype)


def _module(H, W, seed, activation="tanh"):
    """LSTMHead with the input weights scaled up so that log-returns of ~1e-3 move the gates (the scaling of
    tests/test_sac_grad_gpu.py::_actor)."""
    from finenvs_amd.lstm_head import LSTMHead

    torch.manual_seed(seed)
    m = LSTMHead(H, W, activation)
    with torch.no_grad():
        m.lstm.weight_ih_l0[:, :4].mul_(6.0 * np.sqrt(H))
    return m.cuda()


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
    """B observation descriptors of the env's own days: the first B of the (K + 1) N rows a K-step rollout records.  While
    ``B <= num_envs`` those are all row 0, the RESET states of a fresh env: ``obs_pos`` is exactly 0.0 and ``obs_src`` one
    of the table's day starts (at most one distinct sample per day); stepped rows begin at index ``num_envs``.  Positions
    that are not zero and windows all over the table: tests/test_grad_descriptors_gpu.py."""
    from finenvs_amd.rollout import FusedLSTMRollout
    from finenvs_amd.trajectory import TrajectoryBuffer

    N = env.num_envs
    K = max(1, -(-B // N) - 1)
    m = _module(32, env.num_intervals, seed)
    roll = FusedLSTMRollout.from_modules(env, m.lstm, m.last_layer[0])
    traj = TrajectoryBuffer(K, N, 1, device=env._dev, states=True)
    gen = torch.Generator(device=env._dev).manual_seed(seed)
    roll.run(K, noise=torch.randn((K, N, 1), generator=gen, device=env._dev), std=0.5, trajectory=traj)
    src, pos = traj.obs_src.reshape(-1)[:B].contiguous(), traj.obs_pos.reshape(-1, 1)[:B].contiguous()
    return src, pos, traj


def _params(module):
    from finenvs_amd.lstm_head import head_parameters

    return list(head_parameters(module))


def _zero(*modules):
    for m in modules:
        for p in m.parameters():
            p.grad = None


def _ppo_inputs(module, states, seed):
    """(log_std, actions, old_log_probs, advantages) of one PPO minibatch: actions drawn from the actor's own policy,
    old log-probs from a perturbed copy of it, standard normal advantages -- zero where the f64 probability ratio lies
    within 1e-4 of 1 +- clip (a branch flip there is a discontinuity of the gradient, not an error)."""
    from torch.distributions import Normal

    B = states.shape[0]
    gen = torch.Generator(device="cuda").manual_seed(seed)
    log_std = torch.full((1, 1), float(np.log(0.5)), device="cuda")
    with torch.no_grad():
        old = copy.deepcopy(module)
        for p in old.parameters():
            p.mul_(1.0 + 0.02 * torch.randn(p.shape, generator=gen, device="cuda"))
        old.last_layer[0].bias.add_(0.15)
        actions = module(states.float()) + log_std.exp() * torch.randn((B, 1), generator=gen, device="cuda")
        old_log_probs = Normal(old(states.float()), log_std.exp()).log_prob(actions)
        advantages = torch.randn((B, 1), generator=gen, device="cuda")
        m64 = copy.deepcopy(module).double()
        new64 = Normal(m64(states.double()), log_std.double().exp()).log_prob(actions.double())
        ratio = (new64 - old_log_probs.double()).exp()
        edge = ((ratio - (1 - CLIP)).abs() < 1e-4) | ((ratio - (1 + CLIP)).abs() < 1e-4)
        advantages = torch.where(edge, torch.zeros_like(advantages), advantages)
        dropped = int(edge.sum())
        assert dropped <= 0.01 * B, (dropped, B)
        clipped = (((ratio < 1 - CLIP) & (advantages < 0)) | ((ratio > 1 + CLIP) & (advantages > 0))) & ~edge
        assert int(clipped.sum()) < 0.5 * (B - dropped), (int(clipped.sum()), B, dropped)
    return log_std, actions, old_log_probs, advantages


def _loss(kind, y, extra, dtype, q_fn=None):
    """The four scalar functions of the head's output every case differentiates."""
    from finenvs_amd.lstm_head import torch_ppo_actor_loss, torch_ppo_critic_loss

    if kind == "ppo_actor":  # PPO/continuous_actor.py:59-78
        log_std, actions, old_log_probs, advantages = extra
        return torch_ppo_actor_loss(y, log_std, actions.to(dtype), old_log_probs.to(dtype), advantages.to(dtype), CLIP, ENT)
    if kind == "ppo_critic":  # PPO/critic.py:26-32
        return torch_ppo_critic_loss(y, extra.to(dtype))
    if kind == "td3":  # TD3/actor.py:50-56
        return -q_fn(y).mean()
    return y.sum()


def _torch_grads(kind, module, critic, states, extra, dtype):
    """Loss and the gradients of a copy of the module in `dtype` on the rendered states; also max|p|."""
    m = copy.deepcopy(module).to(dtype)
    c = copy.deepcopy(critic).to(dtype) if critic is not None else None
    _zero(m)
    s = states.to(dtype)
    if kind == "ppo_actor":
        log_std = extra[0].detach().clone().to(dtype).requires_grad_(True)
        extra = (log_std,) + tuple(extra[1:])
    loss = _loss(kind, m(s), extra, dtype, (lambda a: c(s, a)) if c is not None else None)
    loss.backward()
    with torch.no_grad():
        pmax = float(m.last_layer[0](m.lstm(s)[0][:, -1, :]).abs().max())
    grads = [p.grad for p in _params(m)] + ([log_std.grad] if kind == "ppo_actor" else [])
    return loss.detach(), grads, pmax


def _fused_grads(kind, head, twin, src, pos, extra):
    from finenvs_amd.lstm_head import ppo_actor_loss, ppo_critic_loss

    _zero(head.module)
    if kind == "ppo_actor":  # through the public loss functions, as a learner calls them
        log_std = extra[0].detach().clone().requires_grad_(True)
        loss = ppo_actor_loss(head, log_std, src, pos, extra[1], extra[2], extra[3], CLIP, ENT)
    elif kind == "ppo_critic":
        loss = ppo_critic_loss(head, src, pos, extra)
    else:
        loss = _loss(kind, head(src, pos), extra, torch.float32, (lambda a: twin.q(src, pos, a)[0]) if twin else None)
    loss.backward()
    grads = [p.grad.clone() for p in _params(head.module)] + ([log_std.grad] if kind == "ppo_actor" else [])
    return loss.detach(), grads


def _compare(kind, g, g32, g64, zero=()):
    """`zero`: the tensors whose gradient is identically zero by construction (w_hh at W = 1: h_0 = 0 is its only
    operand); for them the bound is 0, so the fused gradient must be exactly zero too."""
    for name, gf, gt, gd in zip(NAMES + ("log_std",), g, g32, g64):
        assert gf.shape == gd.shape and gf.dtype is torch.float32, (kind, name)
        assert (float(gd.abs().max()) > 0) != (name in zero), (kind, name)  # not degenerate
        err = float((gf.double() - gd).abs().max())
        tol = 2e-5 * float(gd.abs().max()) + 4 * float((gt.double() - gd).abs().max())
        print(f"{kind:10s} {name:7s} err {err:.3e} tol {tol:.3e} ratio {err / tol if tol else err:.3f}")
        assert err <= tol, (kind, name, err, tol)


def _check_against_f64(kind, head, twin, env, src, pos, seed=7):
    states = env.render(src, pos)
    B = int(src.numel())
    if kind == "ppo_actor":
        extra = _ppo_inputs(head.module, states, seed)
    elif kind == "ppo_critic":
        gen = torch.Generator(device="cuda").manual_seed(seed)
        with torch.no_grad():
            extra = head.module(states.float()) + 0.3 * torch.randn((B, 1), generator=gen, device="cuda")  # the returns
    else:
        extra = None
    critic = twin.critic_1 if kind == "td3" else None
    loss, g = _fused_grads(kind, head, twin if kind == "td3" else None, src, pos, extra)
    l32, g32, _ = _torch_grads(kind, head.module, critic, states.float(), extra, torch.float32)
    l64, g64, pmax = _torch_grads(kind, head.module, critic, states.double(), extra, torch.float64)
    assert pmax < 4.0, pmax  # not saturated
    assert len(g) == len(g32) == len(g64) == (7 if kind == "ppo_actor" else 6)
    _compare(kind, g, g32, g64, zero=("w_hh",) if int(env.num_intervals) == 1 else ())
    err, tol = abs(float(loss) - float(l64)), 2e-5 * abs(float(l64)) + 4 * abs(float(l32) - float(l64)) + 1e-7
    assert err <= tol, (kind, "loss", err, tol)


CASES = [
    (32, 4, 1, torch.float64),
    (64, 4, 31, torch.float32),
    (128, 4, 33, torch.float64),
    (32, 16, 4097, torch.float32),
    (64, 16, 33, torch.float64),
    (128, 16, 31, torch.float32),
    (64, 16, 1, torch.float32),
    (128, 16, 4097, torch.float64),
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
    from finenvs_amd.lstm_head import FusedLSTMHead

    env = _env(min(B, 4096), W, obs_dtype=obs_dtype)
    src, pos, _ = _descriptors(env, B)
    assert src.numel() == B
    actor = FusedLSTMHead(env, _module(H, W, 20, "tanh"))
    value = FusedLSTMHead(env, _module(H, W, 21, "none"))
    twin = FusedTwinCritic(env, _critic(H, W, 10), _critic(H, W, 11))
    _check_against_f64("ppo_actor", actor, None, env, src, pos)
    _check_against_f64("ppo_critic", value, None, env, src, pos)
    _check_against_f64("td3", actor, twin, env, src, pos)
    _check_against_f64("sum", actor, None, env, src, pos)
    _check_against_f64("sum", value, None, env, src, pos)


def test_values_equal_forward_bit_for_bit_and_backward_is_deterministic():
    from finenvs_amd.lstm_head import FusedLSTMHead
    from finenvs_amd.rollout import FusedLSTMRollout

    for H, W, activation in ((32, 4, "tanh"), (64, 4, "none"), (128, 16, "tanh"), (128, 16, "none")):
        env = _env(300, W)
        src, pos, _ = _descriptors(env, 900)
        module = _module(H, W, 20, activation)
        head = FusedLSTMHead(env, module)
        ref = FusedLSTMRollout.from_modules(env, module.lstm, module.last_layer[0], output_activation=activation)
        expected = ref.forward(src, pos)
        y = head(src, pos)
        assert tuple(y.shape) == (900, 1) and y.dtype is torch.float32 and y.requires_grad
        assert_bits(y, expected)
        assert_bits(head.rollout.forward(src, pos), expected)
        c = torch.randn((900, 1), device="cuda")
        runs = []
        for _ in range(2):
            _zero(module)
            (head(src, pos) * c).sum().backward()
            runs.append([p.grad.clone() for p in _params(module)])
        for x, z in zip(*runs):
            assert float(x.abs().max()) > 0
            assert_bits(x, z)


def _ring(env, K, max_size):
    from finenvs_amd.replay import ReplayBuffer

    _, _, traj = _descriptors(env, env.num_envs * (K + 1))
    buffer = ReplayBuffer(env, max_size=max_size)
    buffer.extend(traj)
    return buffer


def test_td3_actor_loss_on_a_wrapped_ring_against_f64():
    from finenvs_amd.critic import FusedTwinCritic
    from finenvs_amd.lstm_head import FusedLSTMHead, td3_actor_loss

    H, W, N, K, B = 64, 4, 200, 6, 777
    env = _env(N, W)
    buffer = _ring(env, K, N * K // 2 + 37)
    assert buffer.size() == buffer.max_size and buffer.head != 0  # wrapped
    head = FusedLSTMHead(env, _module(H, W, 20))
    twin = FusedTwinCritic(env, _critic(H, W, 10), _critic(H, W, 11))
    idx = torch.randint(0, buffer.size(), (B,), device="cuda")
    _zero(head.module, twin.critic_1, twin.critic_2)
    loss = td3_actor_loss(head, buffer, idx, twin)
    loss.backward()
    g = [p.grad.clone() for p in _params(head.module)]
    assert all(p.grad is not None for p in twin.critic_1.parameters())  # as in torch: the critic it went through
    assert all(p.grad is None for p in twin.critic_2.parameters())  # the reference passes its first critic only
    states = buffer.get_mini_batch(B, indices=idx)["states"]
    l32, g32, _ = _torch_grads("td3", head.module, twin.critic_1, states.float(), None, torch.float32)
    l64, g64, pmax = _torch_grads("td3", head.module, twin.critic_1, states.double(), None, torch.float64)
    assert pmax < 4.0
    _compare("td3 ring", g, g32, g64)
    err, tol = abs(float(loss.detach()) - float(l64)), 2e-5 * abs(float(l64)) + 4 * abs(float(l32) - float(l64))
    print(f"td3 actor loss {float(loss.detach()):.8f} f64 {float(l64):.8f} err {err:.3e} tol {tol:.3e}")
    assert err <= tol, (err, tol)
    # the head's rollout is the target actor td3_targets takes
    y = twin.td3_targets(buffer, idx, target_actor=head.rollout, noise=torch.randn((B, 1), device="cuda"))
    assert tuple(y.shape) == (B, 1) and bool(torch.isfinite(y).all())
    bad = idx.clone()
    bad[3] = buffer.size()
    assert torch.isnan(td3_actor_loss(head, buffer, bad, twin)).item()
    with pytest.raises(ValueError):
        td3_actor_loss(head, buffer, idx.float(), twin)
    with pytest.raises(ValueError):
        td3_actor_loss(head, buffer, idx, twin.critic_1)
    other = FusedTwinCritic(_env(8, W), _critic(H, W, 10), _critic(H, W, 11))
    with pytest.raises(ValueError):
        td3_actor_loss(head, buffer, idx, other)


def test_accumulation_a_frozen_head_and_an_empty_batch(monkeypatch):
    from finenvs_amd.critic import FusedTwinCritic
    from finenvs_amd.lstm_head import FusedLSTMHead

    H, W, B = 32, 4, 300
    env = _env(B, W)
    src, pos, _ = _descriptors(env, B)
    head = FusedLSTMHead(env, _module(H, W, 20))
    twin = FusedTwinCritic(env, _critic(H, W, 10), _critic(H, W, 11))
    _, once = _fused_grads("td3", head, twin, src, pos, None)
    _zero(head.module)
    for _ in range(2):  # no zero_grad in between
        (-twin.q(src, pos, head(src, pos))[0].mean()).backward()
    for p, g in zip(_params(head.module), once):
        torch.testing.assert_close(p.grad, 2 * g, rtol=1e-6, atol=0)
    # a frozen head: no graph, no .grad, no launch of the backward
    calls = []
    real = env._lib.fe_lstm_backward
    monkeypatch.setattr(env._lib, "fe_lstm_backward", lambda *a: calls.append(1) or real(*a), raising=False)
    head.module.requires_grad_(False)
    _zero(head.module, twin.critic_1)
    y = head(src, pos)
    assert not y.requires_grad
    twin.q(src, pos, y)[0].mean().backward()  # the critic still gets its gradients
    assert all(p.grad is None for p in head.module.parameters()) and not calls
    assert all(p.grad is not None for p in twin.critic_1.parameters())
    # one frozen parameter: the others get theirs, bit for bit what they got before
    head.module.requires_grad_(True)
    head.module.lstm.weight_hh_l0.requires_grad_(False)
    _zero(head.module)
    (-twin.q(src, pos, head(src, pos))[0].mean()).backward()
    assert calls == [1] and head.module.lstm.weight_hh_l0.grad is None
    for k, (p, g) in enumerate(zip(_params(head.module), once)):
        if k != 1:
            assert_bits(p.grad, g)
    head.module.requires_grad_(True)
    # an empty batch: values (0, 1), zero gradients, no launch
    _zero(head.module)
    y = head(src[:0], pos[:0])
    assert tuple(y.shape) == (0, 1)
    y.sum().backward()
    assert calls == [1]
    for p in _params(head.module):
        assert p.grad is not None and float(p.grad.abs().max()) == 0.0


def test_ppo_example_with_fused_update_trains_without_rendering(monkeypatch):
    from finenvs_amd import TimeSeriesEnv, lstm_head
    from finenvs_amd.rollout import FusedLSTMRollout
    from finenvs_amd.trajectory import TrajectoryBuffer

    spec = importlib.util.spec_from_file_location("ppo_lstm_fused", os.path.join(ROOT, "examples", "ppo_lstm_fused.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    heads = []

    class Recording(lstm_head.FusedLSTMHead):
        def __init__(self, env, module):
            super().__init__(env, module)
            heads.append(self)

    def refuse(self, *a, **k):
        raise AssertionError("an observation was rendered")

    monkeypatch.setattr(mod, "FusedLSTMHead", Recording)
    monkeypatch.setattr(TrajectoryBuffer, "minibatch_states", refuse)
    monkeypatch.setattr(TimeSeriesEnv, "render", refuse)
    history = mod.main(envs=512, steps=8, iters=2, hidden=32, window=4, quiet=True, fused_update=True)
    assert len(history) == 2 and len(heads) == 2
    for critic_loss, mean_reward, log in history:
        assert np.isfinite(critic_loss) and np.isfinite(mean_reward)
        assert log["num_training_episodes"] >= 0
    for head, activation in zip(heads, ("tanh", "none")):
        assert head.output_activation == activation
        src, pos = head.rollout.obs_src.clone(), head.rollout.obs_pos.clone()
        acted = head.rollout.forward(src, pos).clone()  # what the kernel runs after the example's last update
        y = head(src, pos)  # re-packs the module's parameters as they stand
        assert_bits(acted, y)
        assert bool(torch.isfinite(y).all())
        # and those are the trained parameters: a rollout object made from the module now gives the same bits
        m = head.module
        fresh = FusedLSTMRollout.from_modules(head.env, m.lstm, m.last_layer[0], output_activation=activation)
        assert_bits(fresh.forward(src, pos), acted)
        untrained = lstm_head.LSTMHead(32, 4, activation)
        assert not torch.equal(m.lstm.weight_hh_l0.cpu(), untrained.lstm.weight_hh_l0)


def test_refusals():
    from finenvs_amd.lstm_head import FusedLSTMHead, LSTMHead

    env2 = _env(8, 4, A=2)
    with pytest.raises(ValueError, match="one asset"):
        FusedLSTMHead(env2, _module(32, 4, 1))
    # the C ABI refuses the A = 2 env itself, after the null checks and before it touches any other pointer
    import ctypes as C

    from finenvs_amd import _lib

    grads = _lib.FeLstmGrads(*([16] * 6))
    rc = env2._lib.fe_lstm_backward(env2._handle, 16, 16, 16, 16, 32, 0, 16, 16, 8, 16, 16, 16, C.byref(grads), None)
    assert rc == _lib.FE_ERR_ARG
    msg = env2._lib.fe_last_error()
    assert b"fe_lstm_backward" in msg and b"2 assets" in msg, msg
    env = _env(64, 4)
    with pytest.raises(ValueError, match="256"):
        FusedLSTMHead(env, LSTMHead(256, 4).cuda())
    with pytest.raises(ValueError):
        FusedLSTMHead(env, LSTMHead(48, 4).cuda())
    with pytest.raises(ValueError, match="clamp"):
        LSTMHead(32, 4, "clamp")
    clamped = _module(32, 4, 1)
    clamped.last_layer[1] = torch.nn.Hardtanh()
    with pytest.raises(ValueError, match="Tanh or Identity"):
        FusedLSTMHead(env, clamped)
    with pytest.raises(ValueError, match="float32"):
        FusedLSTMHead(env, _module(32, 4, 1).double())
    with pytest.raises(ValueError, match="device"):
        FusedLSTMHead(env, _module(32, 4, 1).cpu())
    src, pos, _ = _descriptors(env, 64)
    head = FusedLSTMHead(env, _module(32, 4, 1))
    head.module.double()
    with pytest.raises(ValueError, match="float32"):
        head(src, pos)
    head.module.float().cpu()
    with pytest.raises(ValueError, match="device"):
        head(src, pos)
    head.module.cuda()
    with pytest.raises(ValueError, match="obs_pos"):
        head(src, pos[:63])
