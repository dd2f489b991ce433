"""GPU: the twin MLP critics Q(s, a) on descriptors (include/finenvs_amd_mlp_critic.h, finenvs_amd/mlp_critic.py).

Shapes (H, W, B): (32, 4, 33) a ragged last 32-pair block, (64, 7, 513) a crossed 512-pair split and an odd window,
(128, 40, 33) the largest weight image, (128, 4, 4 097) several splits, (32, 4, 70 001) the grid-stride path.

* anchor: with ``actions = 0``, and with ``wact = 0`` and random actions, q1 and q2 equal ``fe_mlp2_forward`` (output
  none) on the same weights bit for bit; ``q()`` returns ``forward()``'s bits;
* values against an f64 copy of the modules on rendered states within ``2e-5 max|q64| + 4 max|q32_torch - q64|``;
* gradients of all six tensors per critic and ``d_actions`` against the f64 copy within ``2e-5 max|g64| + 4 max|g32_torch -
  g64|`` per tensor, for the critic loss ``MSE(q1, y) + MSE(q2, y)``, ``-q1.mean()`` (critic 2 must not run) and
  ``min(q1, q2).sum()``.  Decided from the f64 copy alone, per batch: no f64 gradient identically zero, the share of
  negative pre-activations of both layers in [0.2, 0.8], samples with any ``|z1|`` or ``|z2| < 1e-5`` (and, for the min
  arm, with ``|q1 - q2| < 1e-4``, where f32 and f64 may pick different critics) get upstream gradient 0 in every arm and
  are at most 2 % of B; a module seed that misses a condition is replaced by the next (``_conditioned``);
* ``td3_actor_loss`` through ``FusedMLP2Head`` + ``FusedTwinMLPCritic``; ``td3_targets`` against ``torch_td3_targets`` on
  rendered next states, an out-of-range index, a ``ReplayDraw``, a ``GraphedUpdate`` replay against an eager twin;
* behaviour (determinism, ``.grad`` accumulation, a frozen critic, B = 0), the memory contract, the window limit, the
  refusals that read the env, and examples/td3_mlp_fused.py.
* banded inputs, an uneven count of 65 569 pairs, every form of the backward and the argument layouts:
  tests/test_mlp_memory_contract_gpu.py; crafted descriptors and the action column alone: tests/test_grad_descriptors_gpu.py.
"""
import copy
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import test_mlp2_head_gpu as t2
from tests import test_mlp_head_gpu as th

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")
F32, F64, I64 = torch.float32, torch.float64, torch.int64
assert_bits, _env, _descriptors, _zero = th.assert_bits, th._env, th._descriptors, th._zero
_window, _bands_intact, SENTINEL = th._window, th._bands_intact, th.SENTINEL
GAMMA = 0.97
SHAPES = [(32, 4, 33, "elu"), (64, 7, 513, "relu"), (128, 40, 33, "tanh"), (128, 4, 4097, "elu"), (32, 4, 70001, "relu")]


def _critic(H, W, seed, activation="elu"):
    """MLPCritic whose observation columns, hidden layer and output layer are those of tests/test_mlp2_head_gpu.py::_module
    (seed), the action column drawn as 0.8 randn(H): the action moves z1 by O(1)."""
    from finenvs_amd.mlp_critic import MLPCritic

    m = t2._module(H, W, seed, activation, "none")
    gen = torch.Generator().manual_seed(5000 + seed)
    c = MLPCritic(H, W, activation)
    with torch.no_grad():
        c.network[0].weight[:, :5 * W].copy_(m.network[0].weight.cpu())
        c.network[0].weight[:, 5 * W].copy_(0.8 * torch.randn((H,), generator=gen))
        for i in (0, 2, 4):
            c.network[i].bias.copy_(m.network[i].bias.cpu())
        c.network[2].weight.copy_(m.network[2].weight.cpu())
        c.network[4].weight.copy_(m.network[4].weight.cpu())
    return c.cuda()


def _head_of(critic, H, W, activation):
    """The MLP2Head (output none) of a critic's observation columns and other layers."""
    from finenvs_amd.mlp2_head import MLP2Head

    m = MLP2Head(H, W, activation, "none").cuda()
    with torch.no_grad():
        m.network[0].weight.copy_(critic.network[0].weight[:, :5 * W])
        for i in (0, 2, 4):
            m.network[i].bias.copy_(critic.network[i].bias)
        m.network[2].weight.copy_(critic.network[2].weight)
        m.network[4].weight.copy_(critic.network[4].weight)
    return m


def _params(critic):
    from finenvs_amd.mlp_critic import mlp_critic_parameters

    return list(mlp_critic_parameters(critic))


def _batch(H, W, B, seed=1):
    env = _env(16 if B < 64 else min(B // 4, 4096), W)
    src, pos, _ = _descriptors(env, B, seed)
    gen = torch.Generator(device="cuda").manual_seed(B + seed)
    actions = torch.rand((B, 1), generator=gen, device="cuda") * 2 - 1
    return env, src, pos.reshape(B), actions


def _pre_activations(critic, states, actions):
    c64 = copy.deepcopy(critic).double()
    with torch.no_grad():
        x = torch.cat([states.double().reshape(states.shape[0], -1), actions.double()], dim=1)
        z1 = c64.network[0](x)
        z2 = c64.network[2](c64.network[1](z1))
    return z1, z2


def _conditions(critic, states, actions):
    """The batch conditions on one critic, from its f64 copy; returns the kink mask (B, 1)."""
    B = states.shape[0]
    z1, z2 = _pre_activations(critic, states, actions)
    for z in (z1, z2):
        neg = float((z < 0).double().mean())
        assert 0.2 <= neg <= 0.8, neg
    kink = (z1.abs() < 1e-5).any(dim=1, keepdim=True) | (z2.abs() < 1e-5).any(dim=1, keepdim=True)
    assert int(kink.sum()) <= 0.02 * B, (int(kink.sum()), B)
    return kink


def _conditioned(states, actions, H, W, seed, activation):
    """The critic of the first seed among ``seed``, ``seed + 1000``, ... whose f64 copy meets ``_conditions``."""
    for s in range(seed, seed + 8000, 1000):
        c = _critic(H, W, s, activation)
        try:
            _conditions(c, states, actions)
        except AssertionError as exc:
            print(f"critic seed {s} misses the batch conditions ({exc}); trying {s + 1000}")
            continue
        return c
    raise AssertionError("no critic seed meets the batch conditions")


# --------------------------------------------------------------------------------------------------------------- anchor
@pytest.mark.parametrize("H,W,B,activation", SHAPES)
def test_zero_action_or_zero_action_weight_equals_the_two_layer_head_bit_for_bit(H, W, B, activation):
    from finenvs_amd.mlp2_head import FusedMLP2Head
    from finenvs_amd.mlp_critic import FusedTwinMLPCritic

    env, src, pos, actions = _batch(H, W, B)
    c1, c2 = _critic(H, W, 3, activation), _critic(H, W, 4, activation)
    twin = FusedTwinMLPCritic(env, c1, c2)
    want = [FusedMLP2Head(env, _head_of(c, H, W, activation)).rollout.forward(src, pos.reshape(B, 1)) for c in (c1, c2)]
    q1, q2 = twin.forward(src, pos, torch.zeros((B, 1), device="cuda"))
    assert q1.shape == (B, 1) and q1.dtype is F32
    assert_bits(q1, want[0], "actions = 0, critic 1")
    assert_bits(q2, want[1], "actions = 0, critic 2")
    r1, r2 = twin.forward(src, pos, actions)
    assert not torch.equal(r1, q1) and not torch.equal(r2, q2)  # the action matters
    d1, d2 = twin.q(src, pos, actions)
    assert_bits(d1, r1, "q() against forward()")
    assert_bits(d2, r2, "q() against forward()")
    with torch.no_grad():
        c1.network[0].weight[:, 5 * W].zero_()
        c2.network[0].weight[:, 5 * W].zero_()
    q1, q2 = twin.forward(src, pos, actions)
    assert_bits(q1, want[0], "wact = 0, critic 1")
    assert_bits(q2, want[1], "wact = 0, critic 2")
    assert float(want[0].std()) > 0.01 and float((want[0] - want[1]).abs().max()) > 0.01


# --------------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("H,W,B,activation", SHAPES)
def test_values_against_the_f64_modules_within_the_yardstick(H, W, B, activation):
    """Measured err / tol on an MI355X: see the docstring of test_gradients_against_f64_torch."""
    from finenvs_amd.mlp_critic import FusedTwinMLPCritic

    env, src, pos, actions = _batch(H, W, B)
    critics = _critic(H, W, 11, activation), _critic(H, W, 12, activation)
    q = FusedTwinMLPCritic(env, *critics).forward(src, pos, actions)
    states = env.render(src, pos.reshape(B, 1))
    for c, qc in zip(critics, q):
        with torch.no_grad():
            q32 = c(states.float(), actions).double()
            q64 = copy.deepcopy(c).double()(states.double(), actions.double())
        err = float((qc.double() - q64).abs().max())
        tol = 2e-5 * float(q64.abs().max()) + 4 * float((q32 - q64).abs().max())
        print(f"values ({H}, {W}, {B}, {activation}): err {err:.3e} tol {tol:.3e} ratio {err / tol:.3f}")
        assert err <= tol, (err, tol)
        assert float(q64.std()) > 0.05


# ------------------------------------------------------------------------------------------------------------ gradients
def _loss(kind, q1, q2, keep, y):
    """Every arm gives the samples outside ``keep`` upstream gradient 0."""
    q1, q2 = torch.where(keep, q1, q1.detach()), torch.where(keep, q2, q2.detach())
    if kind == "critic":
        return F.mse_loss(q1, y.to(q1.dtype)) + F.mse_loss(q2, y.to(q1.dtype))
    if kind == "actor":
        return -q1.mean()
    return torch.minimum(q1, q2).sum()


def _torch_grads(kind, critics, states, actions, keep, y, dtype):
    cs = [copy.deepcopy(c).to(dtype) for c in critics]
    a = actions.detach().to(dtype).requires_grad_(True)
    loss = _loss(kind, cs[0](states.to(dtype), a), cs[1](states.to(dtype), a), keep, y)
    loss.backward()
    return loss.detach(), [p.grad for c in cs for p in _params(c)] + [a.grad]


def _fused_grads(kind, twin, src, pos, actions, keep, y):
    _zero(twin.critic_1, twin.critic_2)
    a = actions.detach().clone().requires_grad_(True)
    loss = _loss(kind, *twin.q(src, pos, a), keep, y)
    loss.backward()
    return loss.detach(), [p.grad for c in (twin.critic_1, twin.critic_2) for p in _params(c)] + [a.grad]


def _compare(kind, g, g32, g64):
    names = [f"c{c}.{n}" for c in (1, 2) for n in NAMES] + ["d_actions"]
    worst = 0.0
    for name, gf, gt, gd in zip(names, g, g32, g64):
        if gd is None:  # the actor arm: critic 2 is not part of the loss
            assert kind == "actor" and name.startswith("c2.") and gf is None and gt is None, (kind, name)
            continue
        assert gf is not None and gf.shape == gd.shape and gf.dtype is F32, (kind, name)
        assert float(gd.abs().max()) > 0, (kind, name)  # no f64 gradient is identically zero
        err = float((gf.double() - gd).abs().max())
        tol = 2e-5 * float(gd.abs().max()) + 4 * float((gt.double() - gd).abs().max())
        print(f"{kind:7s} {name:10s} err {err:.3e} tol {tol:.3e} ratio {err / tol:.3f}")
        worst = max(worst, err / tol)
        assert err <= tol, (kind, name, err, tol)
    return worst


@pytest.mark.parametrize("H,W,B,activation", SHAPES)
def test_gradients_against_f64_torch(H, W, B, activation, monkeypatch):
    """Worst err / tol over the three losses and the thirteen tensors per case, measured on an MI355X:
      (32, 4, 33, elu) 0.014, (64, 7, 513, relu) 0.141, (128, 40, 33, tanh) 0.175, (128, 4, 4 097, elu) 0.174,
      (32, 4, 70 001, relu) 0.272
    and of the values, in the same order: 0.011, 0.018, 0.014, 0.027, 0.018.  No seed was replaced."""
    from finenvs_amd.mlp_critic import FusedTwinMLPCritic

    env, src, pos, actions = _batch(H, W, B)
    states = env.render(src, pos.reshape(B, 1))
    critics = [_conditioned(states, actions, H, W, 20 + H + W + i, activation) for i in (0, 1)]
    kink = _conditions(critics[0], states, actions) | _conditions(critics[1], states, actions)
    assert int(kink.sum()) <= 0.02 * B
    with torch.no_grad():
        q64 = [copy.deepcopy(c).double()(states.double(), actions.double()) for c in critics]
    gen = torch.Generator(device="cuda").manual_seed(H + B)
    y = (0.5 * (q64[0] + q64[1]) + 0.3 * torch.randn((B, 1), generator=gen, device="cuda", dtype=F64)).float()
    twin = FusedTwinMLPCritic(env, *critics)
    seen = []
    real = env._lib.fe_twin_mlpq_backward
    monkeypatch.setattr(env._lib, "fe_twin_mlpq_backward", lambda *a: seen.append(a) or real(*a))
    worst = 0.0
    for kind in ("critic", "actor", "min"):
        keep = ~kink
        if kind == "min":  # f32 and f64 may pick different critics where the two values nearly tie
            tie = (q64[0] - q64[1]).abs() < 1e-4
            assert int((kink | tie).sum()) <= 0.02 * B
            keep = keep & ~tie
        seen.clear()
        loss, g = _fused_grads(kind, twin, src, pos, actions, keep, y)
        l32, g32 = _torch_grads(kind, critics, states, actions, keep, y, F32)
        l64, g64 = _torch_grads(kind, critics, states, actions, keep, y, F64)
        assert len(seen) == 1
        if kind == "actor":  # dq2, grads2: critic 2 does not run
            assert seen[0][11] is None and seen[0][14] is None and seen[0][10] is not None
        worst = max(worst, _compare(kind, g, g32, g64))
        err, tol = abs(float(loss) - float(l64)), 2e-5 * abs(float(l64)) + 4 * abs(float(l32) - float(l64)) + 1e-7
        assert err <= tol, (kind, "loss", err, tol)
    print(f"WORST ({H}, {W}, {B}, {activation}) {worst:.3f}")


# ------------------------------------------------------------------------------------------------------ the replay ring
def _actor(H, W, seed, activation="elu"):
    return t2._module(H, W, seed, activation, "tanh")


def _filled(env, H, K, seed=1, cursor=False, max_size=None):
    """A sampled MLP2 rollout of K steps and a replay ring holding it; the rollout object for more."""
    from finenvs_amd.replay import ReplayBuffer
    from finenvs_amd.trajectory import TrajectoryBuffer

    N = env.num_envs
    roll = t2._rollout(env, _actor(H, env.num_intervals, 900 + seed))
    buffer = ReplayBuffer(env, max_size=max_size or K * N + 7, cursor=cursor, seed=seed)
    gen = torch.Generator(device=env._dev).manual_seed(seed)

    def store(steps=K):
        traj = TrajectoryBuffer(steps, N, 1, device=env._dev, states=True)
        roll.run(steps, noise=torch.randn((steps, N, 1), generator=gen, device=env._dev), std=0.5, trajectory=traj)
        buffer.extend(traj)

    store()
    return buffer, store


def test_td3_actor_loss_through_the_fused_head_and_the_fused_critic():
    """Worst err / tol over the twelve tensors, measured on an MI355X: 0.103 (critic 1's b2); the first seed that meets the
    batch conditions without a kink sample is used."""
    from finenvs_amd.lstm_head import FusedLSTMHead, LSTMHead, td3_actor_loss
    from finenvs_amd.critic import CriticLSTM, FusedTwinCritic
    from finenvs_amd.mlp2_head import FusedMLP2Head, mlp2_head_parameters
    from finenvs_amd.mlp_critic import FusedTwinMLPCritic, torch_td3_actor_loss

    H, W, B = 64, 4, 257
    env = _env(96, W)
    buffer, _ = _filled(env, H, 4)
    idx = torch.randint(0, buffer.size(), (B,), generator=torch.Generator().manual_seed(2)).cuda()
    slots = buffer.physical(idx)
    states = env.render(buffer.state_src[slots], buffer.state_pos[slots])
    for s in range(31, 8031, 1000):  # ELU has no kink; all the same no sample may sit within 1e-5 of one (no mask here)
        actor, c1, c2 = _actor(H, W, s), _critic(H, W, s + 1), _critic(H, W, s + 2)
        with torch.no_grad():
            a64 = copy.deepcopy(actor).double()(states.double())
        try:
            kinks = int(t2._conditions(actor, states).sum()) + int(_conditions(c1, states, a64).sum())
        except AssertionError as exc:
            print(f"seed {s} misses the batch conditions ({exc}); trying {s + 1000}")
            continue
        if kinks == 0:
            break
        print(f"seed {s}: {kinks} samples within 1e-5 of a kink; trying {s + 1000}")
    else:
        raise AssertionError("no seed meets the batch conditions")
    head, twin = FusedMLP2Head(env, actor), FusedTwinMLPCritic(env, c1, c2)
    _zero(actor, c1, c2)
    loss = td3_actor_loss(head, buffer, idx, twin)
    loss.backward()
    got = [p.grad for p in mlp2_head_parameters(actor)] + [p.grad for p in _params(c1)]
    assert all(p.grad is None for p in _params(c2))
    ref = {}
    for dtype in (F32, F64):
        a, c = copy.deepcopy(actor).to(dtype), copy.deepcopy(c1).to(dtype)
        l = torch_td3_actor_loss(a, c, states.to(dtype))
        l.backward()
        ref[dtype] = (l.detach(), [p.grad for p in mlp2_head_parameters(a)] + [p.grad for p in _params(c)])
    names = [f"actor.{n}" for n in NAMES] + [f"c1.{n}" for n in NAMES]
    for name, gf, gt, gd in zip(names, got, ref[F32][1], ref[F64][1]):
        assert float(gd.abs().max()) > 0, name
        err = float((gf.double() - gd).abs().max())
        tol = 2e-5 * float(gd.abs().max()) + 4 * float((gt.double() - gd).abs().max())
        print(f"td3_actor_loss {name:10s} err {err:.3e} tol {tol:.3e} ratio {err / tol:.3f}")
        assert err <= tol, (name, err, tol)
    l32, l64 = float(ref[F32][0]), float(ref[F64][0])
    assert abs(float(loss) - l64) <= 2e-5 * abs(l64) + 4 * abs(l32 - l64) + 1e-7
    # mixed families are refused, either way round; the LSTM family's own message stays
    lstm_head = FusedLSTMHead(env, LSTMHead(32, W, "tanh").cuda())
    lstm_twin = FusedTwinCritic(env, CriticLSTM(32, W).cuda(), CriticLSTM(32, W).cuda())
    with pytest.raises(ValueError, match="do not mix"):
        td3_actor_loss(head, buffer, idx, lstm_twin)
    with pytest.raises(ValueError, match="do not mix"):
        td3_actor_loss(lstm_head, buffer, idx, twin)
    with pytest.raises(ValueError, match="twin must be a FusedTwinCritic of this head's env"):
        td3_actor_loss(lstm_head, buffer, idx, object())


@pytest.mark.parametrize("H,B", [(32, 777), (128, 4097)])
def test_td3_targets_against_torch_on_rendered_next_states(H, B):
    """Measured err / tol on an MI355X: H = 32, B = 777: 0.015; H = 128, B = 4 097: 0.017."""
    from finenvs_amd.critic import torch_td3_targets
    from finenvs_amd.mlp_critic import FusedTwinMLPCritic

    W = 4
    env = _env(190, W)
    buffer, store = _filled(env, H, 2, max_size=3 * 190 - 50)
    store(1)  # wrapped: head != 0
    assert buffer.head != 0 and buffer.size() == buffer.max_size
    with torch.no_grad():
        buffer.dones[1::5] = 1.0
    c1, c2 = _critic(H, W, 50), _critic(H, W, 51)
    actor = _actor(H, W, 52)
    with torch.no_grad():
        actor.network[4].weight.mul_(3.0)  # actions over the whole range, some beyond the clamp after smoothing
    target = t2._rollout(env, actor)
    twin = FusedTwinMLPCritic(env, c1, c2)
    idx = torch.randint(0, buffer.size(), (B,), device="cuda")
    eps = torch.randn((B, 1), device="cuda")
    y = twin.td3_targets(buffer, idx, target, eps, GAMMA, 0.2, 0.5, 0.5)
    b = buffer.get_mini_batch(B, indices=idx)
    ys = []
    for dtype in (F32, F64):
        a, d1, d2 = (copy.deepcopy(m).to(dtype) for m in (actor, c1, c2))
        ys.append(torch_td3_targets(lambda x: a(x.to(dtype)), d1, d2, b["rewards"].to(dtype), b["next_states"].to(dtype),
                                    b["dones"].to(dtype), eps.to(dtype), GAMMA, 0.2, 0.5, 0.5).double())
    err = float((y.double() - ys[1]).abs().max())
    tol = 2e-5 * float(ys[1].abs().max()) + 4 * float((ys[0] - ys[1]).abs().max())
    print(f"td3_targets H = {H}, B = {B}: err {err:.3e} tol {tol:.3e} ratio {err / tol:.3f}")
    assert err <= tol, (err, tol)
    last = twin.last
    expr = b["rewards"] * 0.5 + GAMMA * (1 - b["dones"]) * torch.minimum(last["q1"], last["q2"])
    assert_bits(y, expr, "TD3 epilogue")
    a = torch.clamp(last["next_actions"] + torch.clamp(eps * 0.2, -0.5, 0.5), -1, 1)
    assert bool((a.abs() == 1).any()) and bool((a.abs() < 1).any())
    slots = buffer.physical(idx)
    q1, q2 = twin.forward(buffer.next_src[slots], buffer.next_pos[slots].reshape(B), a)
    assert_bits(q1, last["q1"], "TD3 smoothing in the kernel")
    assert_bits(q2, last["q2"], "TD3 smoothing in the kernel")
    done = b["dones"].reshape(-1) == 1
    assert bool(done.any()) and torch.equal(y[done], (b["rewards"] * 0.5)[done])
    # the entry's SAC form (no smoothing, log-probabilities and alpha): SAC_agent.py:200-227's operations in its order
    logp = torch.randn((B, 1), device="cuda")
    alpha = torch.full((1,), 0.2, device="cuda")
    nxt = last["next_actions"].clone()
    y_sac = twin._targets(buffer, idx, nxt, None, 0.0, 0.0, logp, alpha, GAMMA, 0.5)
    q1, q2 = twin.forward(buffer.next_src[slots], buffer.next_pos[slots].reshape(B), nxt)
    assert_bits(twin.last["q1"], q1, "SAC form: no smoothing")
    expr = b["rewards"] * 0.5 + GAMMA * (1 - b["dones"]) * (torch.minimum(q1, q2) + (-alpha) * logp)
    assert_bits(y_sac, expr, "SAC epilogue")


def test_out_of_range_indices_give_nan_rows_and_count():
    from finenvs_amd.mlp_critic import FusedTwinMLPCritic

    H, W = 32, 4
    env = _env(64, W)
    buffer, _ = _filled(env, H, 2)
    twin = FusedTwinMLPCritic(env, _critic(H, W, 60), _critic(H, W, 61))
    target = t2._rollout(env, _actor(H, W, 62))
    size = buffer.size()
    idx = torch.tensor([0, -1, 5, size, size + 40, size - 1, -1000], device="cuda")
    bad = torch.tensor([False, True, False, True, True, False, True], device="cuda")
    before = int(buffer.errors.item())
    eps = torch.zeros((7, 1), device="cuda")
    y = twin.td3_targets(buffer, idx, target, eps, GAMMA)
    assert int(buffer.errors.item()) - before == 4
    assert bool(torch.isnan(y[bad]).all()) and bool(torch.isfinite(y[~bad]).all())
    assert bool(torch.isnan(twin.last["q1"][bad]).all()) and bool(torch.isnan(twin.last["q2"][bad]).all())
    good = twin.td3_targets(buffer, idx[~bad], target, eps[:3], GAMMA)
    assert_bits(y[~bad], good, "valid rows do not depend on the invalid ones")
    loss = twin.critic_loss(buffer, idx, torch.zeros((7, 1), device="cuda"))
    assert bool(torch.isnan(loss))
    assert bool(torch.isfinite(twin.critic_loss(buffer, idx[~bad], torch.zeros((3, 1), device="cuda"))))


def test_a_replay_draw_gives_the_bits_of_its_indices_as_a_tensor():
    from finenvs_amd.mlp_critic import FusedTwinMLPCritic

    H, W, B = 64, 4, 97
    env = _env(64, W)
    buffer, store = _filled(env, H, 2, cursor=True, max_size=150)
    store(1)  # wrapped
    c1, c2 = _critic(H, W, 70), _critic(H, W, 71)
    twin = FusedTwinMLPCritic(env, c1, c2)
    target = t2._rollout(env, _actor(H, W, 72))
    draw = buffer.draw(B)
    eps = torch.randn((B, 1), device="cuda")
    got = [twin.td3_targets(buffer, draw, target, eps, GAMMA).clone(), twin.last["q1"].clone(), twin.last["q2"].clone()]
    want = [twin.td3_targets(buffer, draw.indices, target, eps, GAMMA), twin.last["q1"], twin.last["q2"]]
    for a, b, name in zip(got, want, ("targets", "q1", "q2")):
        assert bool(torch.isfinite(a).all())
        assert_bits(a, b, name)
    grads = []
    for indices in (draw, draw.indices):
        _zero(c1, c2)
        twin.critic_loss(buffer, indices, got[0]).backward()
        grads.append([p.grad.clone() for c in (c1, c2) for p in _params(c)])
    for a, b in zip(*grads):
        assert_bits(a, b, "critic_loss gradients")


def _graph_arm(graphed):
    """Four critic updates' worth of (draw, targets, loss, backward) at B = 37 with a store between them: eager, or one
    warm-up inside ``GraphedUpdate`` and three replays."""
    from finenvs_amd.graphed import GraphedUpdate
    from finenvs_amd.mlp_critic import FusedTwinMLPCritic

    H, W, B = 32, 4, 37
    env = _env(16, W)
    buffer, store = _filled(env, H, 2, seed=5, cursor=True, max_size=40)
    critics = [_critic(H, W, 80 + i) for i in range(4)]
    twin, twin_t = FusedTwinMLPCritic(env, *critics[:2]), FusedTwinMLPCritic(env, *critics[2:])
    target = t2._rollout(env, _actor(H, W, 84))
    draw = buffer.new_draw(B)
    gen = torch.Generator(device="cuda").manual_seed(6)
    eps = torch.empty((B, 1), device="cuda")

    def fn():
        buffer.draw(B, out=draw)
        y = twin_t.td3_targets(buffer, draw, target, eps, GAMMA, 0.2, 0.5, 0.5)
        loss = twin.critic_loss(buffer, draw, y)
        _zero(*critics[:2])
        loss.backward()
        return [loss.detach(), y] + [p.grad for c in critics[:2] for p in _params(c)]

    def between():
        store(1)
        eps.copy_(torch.randn((B, 1), generator=gen, device="cuda"))

    eps.copy_(torch.randn((B, 1), generator=gen, device="cuda"))
    if graphed:
        g = GraphedUpdate(fn, warmup=1, between=between)
        for _ in range(3):
            out = g.replay()
            between()
    else:
        for _ in range(4):
            out = fn()
            between()
    return [t.clone() for t in out] + [buffer.cursor.clone()]


def test_a_graphed_critic_update_equals_the_eager_one():
    eager, graphed = _graph_arm(False), _graph_arm(True)
    assert len(eager) == len(graphed) == 15
    for k, (a, b) in enumerate(zip(eager, graphed)):
        assert bool(torch.isfinite(a.double()).all()), k
        assert_bits(a, b, f"output {k}")
    assert float(eager[2].abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------ behaviour
def test_backward_is_deterministic_and_grad_accumulates_as_torchs_does():
    from finenvs_amd.mlp_critic import FusedTwinMLPCritic

    for H, W, B, act in ((32, 4, 1057, "elu"), (128, 16, 4097, "relu")):
        env, src, pos, actions = _batch(H, W, B)
        c1, c2 = _critic(H, W, 4, act), _critic(H, W, 5, act)
        twin = FusedTwinMLPCritic(env, c1, c2)
        gen = torch.Generator(device="cuda").manual_seed(H)
        up = torch.randn((2, B, 1), generator=gen, device="cuda")
        a = actions.clone().requires_grad_(True)

        def grads(zero=True):
            if zero:
                _zero(c1, c2)
                a.grad = None
            q1, q2 = twin.q(src, pos, a)
            ((q1 * up[0]).sum() + (q2 * up[1]).sum()).backward()
            return [p.grad.clone() for c in (c1, c2) for p in _params(c)] + [a.grad.clone()]

        g1, g2 = grads(), grads()
        for x, y in zip(g1, g2):
            assert_bits(x, y, "two backward calls")
            assert bool(torch.isfinite(x).all()) and float(x.abs().max()) > 0
        g3 = grads(zero=False)  # .grad accumulates
        for x, y in zip(g3, g1):
            assert_bits(x, y + y, "accumulated")
        # d_actions is critic 1's value plus critic 2's
        parts = []
        for c in range(2):
            a.grad = None
            (twin.q(src, pos, a)[c] * up[c]).sum().backward()
            parts.append(a.grad.clone())
        assert_bits(g1[-1], parts[0] + parts[1], "d_actions = critic 1's + critic 2's")


def test_a_frozen_critic_gets_nothing_and_an_empty_batch_works(monkeypatch):
    from finenvs_amd.mlp_critic import FusedTwinMLPCritic

    H, W, B = 32, 4, 200
    env, src, pos, actions = _batch(H, W, B)
    c1, c2 = _critic(H, W, 9), _critic(H, W, 10)
    twin = FusedTwinMLPCritic(env, c1, c2)
    seen = []
    real = env._lib.fe_twin_mlpq_backward
    monkeypatch.setattr(env._lib, "fe_twin_mlpq_backward", lambda *a: seen.append(a) or real(*a))
    a = actions.clone().requires_grad_(True)
    _zero(c1, c2)
    (twin.q(src, pos, a)[0] + twin.q(src, pos, a)[1]).sum().backward()
    want = a.grad.clone()
    c1.requires_grad_(False)  # frozen: it still passes dQ/da on, and gets nothing
    _zero(c1, c2)
    a.grad = None
    seen.clear()
    q1, q2 = twin.q(src, pos, a)
    (q1 + q2).sum().backward()
    assert len(seen) == 1 and seen[0][10] is not None and seen[0][13] is None and seen[0][14] is not None
    assert all(p.grad is None for p in _params(c1)) and all(p.grad is not None for p in _params(c2))
    assert_bits(a.grad, want, "d_actions with a frozen critic")
    c2.requires_grad_(False)  # both frozen and no action gradient wanted: nothing runs
    seen.clear()
    q1, q2 = twin.q(src, pos, actions)
    assert not q1.requires_grad and seen == []
    c1.requires_grad_(True)
    c2.requires_grad_(True)
    # B = 0
    _zero(c1, c2)
    seen.clear()
    e = torch.zeros((0, 1), device="cuda", requires_grad=True)
    q1, q2 = twin.q(src[:0], pos[:0], e)
    assert q1.shape == (0, 1) and q2.shape == (0, 1)
    (q1.sum() + q2.sum()).backward()
    assert seen == [] and e.grad.shape == (0, 1)
    for p in _params(c1) + _params(c2):
        assert p.grad is not None and float(p.grad.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------ memory contract
@pytest.mark.parametrize("H,W,B", [(32, 4, 1), (64, 7, 33), (128, 16, 1057)])
def test_memory_contract_of_forward_and_backward(H, W, B):
    from finenvs_amd import _lib
    from finenvs_amd.mlp_critic import FusedTwinMLPCritic

    env, src, pos, actions = _batch(H, W, B)
    c1, c2 = _critic(H, W, 13), _critic(H, W, 14)
    twin = FusedTwinMLPCritic(env, c1, c2)
    lib = env._lib
    w = twin._weights()
    packed = twin._packed  # the buffers w points to, kept while the raw calls below use them
    act = actions.reshape(B).contiguous()
    outs = [_window(B, F32, float("nan")) for _ in range(2)]  # exactly B floats each
    _lib.check(lib.fe_twin_mlpq_forward(env._handle, twin._lr32.data_ptr(), C.byref(w[0]), C.byref(w[1]), H, twin.act,
                                        src.data_ptr(), pos.data_ptr(), act.data_ptr(), B, outs[0][1].data_ptr(),
                                        outs[1][1].data_ptr(), env._stream()))
    want = twin.forward(src, pos, actions)
    for (big, win), q in zip(outs, want):
        _bands_intact(big, B, "q")
        assert_bits(win.reshape(B, 1), q)
    # the targets: three outputs of exactly B floats, the ring read by index
    buffer, _ = _filled(env, 32, 1 + B // env.num_envs)
    idx = torch.randint(0, buffer.size(), (B,), device="cuda")
    eps = torch.randn((B,), device="cuda")
    touts = [_window(B, F32, float("nan")) for _ in range(3)]
    _lib.check(lib.fe_twin_mlpq_target(env._handle, twin._lr32.data_ptr(), C.byref(w[0]), C.byref(w[1]), H, twin.act,
                                       C.byref(buffer._desc), buffer.head, buffer.size(), idx.data_ptr(), B, act.data_ptr(),
                                       eps.data_ptr(), 0.2, 0.5, None, None, GAMMA, 1.0, touts[0][1].data_ptr(),
                                       touts[1][1].data_ptr(), touts[2][1].data_ptr(), env._stream()))
    for (big, win), name in zip(touts, ("targets", "q1", "q2")):
        _bands_intact(big, B, name)
        assert bool(torch.isfinite(win).all()), name
    gen = torch.Generator(device="cuda").manual_seed(B)
    up = torch.randn((2, B), generator=gen, device="cuda")
    n_ws = int(lib.fe_twin_mlpq_grad_workspace_floats(H, W, B))
    sizes = {"w1": H * (5 * W + 1), "b1": H, "w2": H * H, "b2": H, "w3": H, "b3": 1}
    results = []
    for poison in (float("nan"), SENTINEL):
        big_ws, ws = _window(n_ws, F32, poison)
        big_da, da = _window(B, F32, poison)
        wins = [{k: _window(n, F32, poison) for k, n in sizes.items()} for _ in range(2)]
        mg = [_lib.FeMlpqGrads(*(x[k][1].data_ptr() for k in NAMES)) for x in wins]
        _lib.check(lib.fe_twin_mlpq_backward(env._handle, twin._lr32.data_ptr(), C.byref(w[0]), C.byref(w[1]), H, twin.act,
                                             src.data_ptr(), pos.data_ptr(), act.data_ptr(), B, up[0].data_ptr(),
                                             up[1].data_ptr(), ws.data_ptr(), C.byref(mg[0]), C.byref(mg[1]), da.data_ptr(),
                                             env._stream()))
        _bands_intact(big_ws, n_ws, "workspace")
        _bands_intact(big_da, B, "d_actions")
        for x in wins:
            for k, n in sizes.items():
                _bands_intact(x[k][0], n, k)
                assert bool(torch.isfinite(x[k][1]).all()), k
        assert bool(torch.isfinite(da).all())
        results.append([x[k][1].clone() for x in wins for k in NAMES] + [da.clone()])
    for a, b in zip(*results):
        assert_bits(a, b, "a NaN-filled workspace against a sentinel-filled one")
    _zero(c1, c2)
    a = actions.clone().requires_grad_(True)
    q1, q2 = twin.q(src, pos, a)
    ((q1.reshape(B) * up[0]).sum() + (q2.reshape(B) * up[1]).sum()).backward()
    front = [p.grad.reshape(-1) for c in (c1, c2) for p in _params(c)] + [a.grad.reshape(-1)]
    for x, y in zip(results[0], front):
        assert_bits(x, y, "against the front end")
    assert len(packed) == 2


# -------------------------------------------------------------------------------------------------- limits and refusals
def test_the_window_limit_at_128_and_the_refusals_that_read_the_env():
    from finenvs_amd import _lib
    from finenvs_amd.mlp_critic import FusedTwinMLPCritic, MLPCritic

    W = _lib.MLP2_MAX_WINDOW[128]
    assert W == 40
    env = _env(8, W + 1)
    with pytest.raises(ValueError, match="does not fit"):
        FusedTwinMLPCritic(env, _critic(128, W + 1, 1), _critic(128, W + 1, 2))
    lib, w, g = env._lib, _lib.FeMlpqWeights(*([16] * 8)), _lib.FeMlpqGrads(*([16] * 6))
    rc = lib.fe_twin_mlpq_forward(env._handle, 16, C.byref(w), C.byref(w), 128, 0, 16, 16, 16, 4, 16, 16, None)
    assert rc == _lib.FE_ERR_ARG
    msg = lib.fe_last_error()
    assert b"fe_twin_mlpq_forward: W1 (128 x 164)" in msg and b"does not fit" in msg, msg
    rc = lib.fe_twin_mlpq_backward(env._handle, 16, C.byref(w), C.byref(w), 128, 0, 16, 16, 16, 4, 16, 16, 16, C.byref(g),
                                   C.byref(g), 16, None)
    assert rc == _lib.FE_ERR_ARG and b"fe_twin_mlpq_backward: W1 (128 x 164)" in lib.fe_last_error()
    twin = FusedTwinMLPCritic(env, _critic(64, W + 1, 1), _critic(64, W + 1, 2))  # H = 64 fits
    roll = t2._rollout(env, _actor(32, W + 1, 3))
    q1, _ = twin.q(roll.obs_src, roll.obs_pos.reshape(-1), torch.zeros((8, 1), device="cuda"))
    q1.sum().backward()
    assert bool(torch.isfinite(q1).all())
    # A != 1
    env2 = _env(8, 4, A=2)
    with pytest.raises(ValueError, match="one asset"):
        FusedTwinMLPCritic(env2, _critic(32, 4, 1), _critic(32, 4, 2))
    rc = lib.fe_twin_mlpq_forward(env2._handle, 16, C.byref(w), C.byref(w), 32, 0, 16, 16, 16, 4, 16, 16, None)
    assert rc == _lib.FE_ERR_ARG and b"fe_twin_mlpq_forward: the env has 2 assets" in lib.fe_last_error()
    rc = lib.fe_twin_mlpq_backward(env2._handle, 16, C.byref(w), C.byref(w), 32, 0, 16, 16, 16, 4, 16, 16, 16, C.byref(g),
                                   C.byref(g), 16, None)
    assert rc == _lib.FE_ERR_ARG and b"fe_twin_mlpq_backward: the env has 2 assets" in lib.fe_last_error()
    # the Python refusals
    env = _env(8, 4)
    with pytest.raises(ValueError, match="same hidden size"):
        FusedTwinMLPCritic(env, _critic(32, 4, 1), _critic(64, 4, 2))
    with pytest.raises(ValueError, match="same activation"):
        FusedTwinMLPCritic(env, _critic(32, 4, 1, "elu"), _critic(32, 4, 2, "relu"))
    with pytest.raises(ValueError, match="in_features must be 21"):
        FusedTwinMLPCritic(env, _critic(32, 4, 1), _critic(32, 7, 2))
    with pytest.raises(ValueError, match="5 W \\+ 1"):
        FusedTwinMLPCritic(env, t2._module(32, 4, 1, "elu", "none"), _critic(32, 4, 2))  # a head: no action input
    with pytest.raises(ValueError, match="critic_2's parameters must live on the env's device"):
        FusedTwinMLPCritic(env, _critic(32, 4, 1), MLPCritic(32, 4))
    twin = FusedTwinMLPCritic(env, _critic(32, 4, 1), _critic(32, 4, 2))
    with pytest.raises(ValueError, match="float32 parameters"):
        FusedTwinMLPCritic(env, _critic(32, 4, 1).double(), _critic(32, 4, 2).double()).q(
            torch.zeros(1, dtype=I64, device="cuda"), torch.zeros(1, dtype=F64, device="cuda"), torch.zeros((1, 1), device="cuda"))
    buffer, _ = _filled(env, 32, 1)
    with pytest.raises(ValueError, match="FusedMLP2Rollout"):
        twin.td3_targets(buffer, None, object(), batch_size=4)
    with pytest.raises(ValueError, match="FusedMLP2Rollout"):  # a critic head is no target actor
        twin.td3_targets(buffer, None, t2._rollout(env, _actor(32, 4, 3), "none"), batch_size=4)


# -------------------------------------------------------------------------------------------------------------- example
def test_td3_example_trains_on_descriptors_only(monkeypatch):
    from finenvs_amd import TimeSeriesEnv
    from finenvs_amd.replay import ReplayBuffer

    spec = importlib.util.spec_from_file_location("td3_mlp_fused", os.path.join(ROOT, "examples", "td3_mlp_fused.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    def refuse(self, *a, **k):
        raise AssertionError("an observation was rendered")

    monkeypatch.setattr(TimeSeriesEnv, "render", refuse)
    monkeypatch.setattr(ReplayBuffer, "get_mini_batch", refuse)
    history, nets = mod.main(num_envs=256, window=4, hidden=32, iterations=6, batch=128, quiet=True)
    assert len(history) == 6 and sum("actor_loss" in e for e in history) == 3
    for e in history:
        assert np.isfinite(e["critic_loss"]) and np.isfinite(e.get("actor_loss", 0.0))
    for name in ("actor", "critic_1", "critic_2", "actor_t", "critic_1t", "critic_2t"):
        for key, p in nets[name].state_dict().items():
            assert bool(torch.isfinite(p).all()), (name, key)
            assert not torch.equal(p, nets["initial"][name][key]), (name, key)  # every tensor moved
