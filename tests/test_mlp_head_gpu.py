"""GPU: the MLP head trained on descriptors (include/finenvs_amd_mlp_head.h, finenvs_amd/mlp_head.py, FusedMLPRollout).

* pack: ``fe_mlp_pack`` equals the oracle's ``mlp_pack`` and ``FusedMLPRollout.set_weights`` bit for bit (W = 1, 7, 64);
* parity: the sampled entry without noise and with the clamp output equals ``FusedMLPRollout.run`` (``fe_env_rollout_mlp``)
  on a twin env bit for bit -- actions, rewards, dones, state -- and ``fe_mlp_forward`` on row k of the recorded state
  descriptors equals ``actions[k]``;
* output activations: ``none`` equals ``clamp`` wherever |p| < 1, ``tanh`` is ``fe_lstm_activations``' tanh of ``none``;
* sampling: ``actions == clamp(means + std * noise, -1, 1)`` in torch f32 bit for bit, the eval env acts on its mean, an
  evaluate-mode env samples everywhere, ``run(3); run(3)`` equals ``run(6)``, the trajectory's fields are the returned views;
* values: ``head(src, pos)`` equals ``rollout.forward(src, pos)`` bit for bit and the f32 torch module within 1e-5;
* gradients of the four parameters (and PPO's ``log_std``) against an f64 torch copy of the module on the rendered states,
  within the project's yardstick ``2e-5 max|g64| + 4 max|g_torch32 - g64|`` per tensor, for ``y.sum()``, the PPO critic
  loss and the PPO actor loss.  On every batch, from the f64 copy: ``max|p| < 4``, no f64 gradient identically zero, the
  share of negative pre-activations in [0.2, 0.8], and the samples with any ``|pre| < 1e-5`` (ReLU's kink: the gradient is
  discontinuous there) get upstream gradient 0 in all three arms and are at most 1 % of B.
  Worst err / tol over kinds and tensors, measured on an MI355X: the docstring of ``test_gradients_against_f64_torch``;
* two backward calls give the same bits; ``.grad`` accumulates as torch's does; a frozen head gets nothing; B = 0 works;
* memory contract: nothing is written outside the workspace, the four gradient buffers, ``out``, ``means_out`` and the
  descriptor rows (sentinel bands on either side, the method of tests/test_memory_contract_gpu.py), and a workspace or
  gradient buffer full of NaN gives the same bits as one full of a finite sentinel;
* examples/ppo_mlp_fused.py with ``fused_update=True`` trains without rendering anything, the kernel acts with the updated
  weights, and one Adam step of a fused head agrees with an eager torch twin on the rendered mini-batch within the
  gradient yardstick propagated through Adam (bound stated at ``_adam_bound``).
* banded inputs, an uneven count of 65 569 pairs and the argument layouts: tests/test_mlp_memory_contract_gpu.py.
"""
import copy
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import test_lstm_grad_gpu as tl
from tests import test_mlp_rollout_gpu as tm
from tests.helpers import assert_bits as _assert_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("w1", "b1", "w2", "b2")
CLIP, ENT = tl.CLIP, tl.ENT
CHUNK = 512  # FE_MLP_GRAD_CHUNK_PAIRS
F32, F64, I64, I32 = torch.float32, torch.float64, torch.int64, torch.int32


def assert_bits(a, b, what=""):
    _assert_bits(a.detach().cpu().numpy(), b.detach().cpu().numpy(), what)


def _env(N, W, obs_dtype=F64, A=1, evaluate=False, seed=3):
    from finenvs_amd import TimeSeriesEnv
    from finenvs_amd.data import synthetic

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    prices, day_id, _ = synthetic.synthetic_series(12, A, max(60, W + 40), 3, 0.0)
    return TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=W, num_envs=N, redraw="device", seed=seed,
                         obs_dtype=obs_dtype, evaluate=evaluate)


def _module(H, W, seed, activation="elu", output="tanh"):
    """MLPHead with the weight scaling of tests/test_mlp_rollout_gpu.py::_weights."""
    from finenvs_amd.mlp_head import MLPHead

    W1, b1, W2, b2 = tm._weights(W, H, seed)
    m = MLPHead(H, W, activation, output)
    with torch.no_grad():
        m.network[0].weight.copy_(torch.from_numpy(W1).t())
        m.network[0].bias.copy_(torch.from_numpy(b1))
        m.network[2].weight.copy_(torch.from_numpy(W2).reshape(1, H))
        m.network[2].bias.fill_(float(b2))
    return m.cuda()


def _rollout(env, module, output="clamp", activation=None):
    """A FusedMLPRollout of the module's parameters through the host packing (set_weights)."""
    from finenvs_amd.mlp_head import mlp_head_parameters
    from finenvs_amd.rollout import FusedMLPRollout

    w1, b1, w2, b2 = mlp_head_parameters(module)
    return FusedMLPRollout(env, w1.detach().t(), b1.detach(), w2.detach(), float(b2.detach()),
                           activation=activation or module.activation, output_activation=output)


def _descriptors(env, B, seed=1):
    """B observation descriptors of the env's own days: the first B of the (K + 1) N rows of a sampled MLP rollout's
    trajectory chunk.  While ``B <= num_envs`` those are all row 0, the RESET states of a fresh env: ``obs_pos`` is exactly
    0.0 and ``obs_src`` one of the table's day starts (at most one distinct sample per day); stepped rows begin at index
    ``num_envs``.  Positions that are not zero and windows all over the table: tests/test_grad_descriptors_gpu.py."""
    from finenvs_amd.trajectory import TrajectoryBuffer

    N = env.num_envs
    K = max(1, -(-B // N) - 1)
    roll = _rollout(env, _module(32, env.num_intervals, seed), "tanh")
    traj = TrajectoryBuffer(K, N, 1, device=env._dev, states=True)
    gen = torch.Generator(device=env._dev).manual_seed(seed)
    roll.run(K, noise=torch.randn((K, N, 1), generator=gen, device=env._dev), std=0.5, trajectory=traj)
    src, pos = traj.obs_src.reshape(-1)[:B].contiguous(), traj.obs_pos.reshape(-1, 1)[:B].contiguous()
    assert src.numel() == B
    return src, pos, traj


def _params(module):
    from finenvs_amd.mlp_head import mlp_head_parameters

    return list(mlp_head_parameters(module))


def _zero(*modules):
    for m in modules:
        for p in m.parameters():
            p.grad = None


# ---------------------------------------------------------------------------------------------------------------- pack
@pytest.mark.parametrize("W,H", [(1, 32), (7, 64), (64, 128)])
def test_pack_equals_the_oracle_and_the_host_packing(W, H):
    from finenvs_amd.mlp_head import FusedMLPHead
    from oracle import fe_oracle as fo

    fo.build()
    env = _env(8, W)
    m = _module(H, W, 5 + W)
    with torch.no_grad():  # a negative zero among the position weights: 0 + (-0) = +0 is part of the contract
        m.network[0].weight.reshape(H, W, 5)[0, :, 4] = -0.0
    head = FusedMLPHead(env, m)
    W1 = m.network[0].weight.detach().t().contiguous().cpu().numpy()
    w1t, wpos = fo.mlp_pack(W1, W)
    _assert_bits(head.rollout.w1t.cpu().numpy(), w1t, "w1t against the oracle")
    _assert_bits(head.rollout.wpos.cpu().numpy(), wpos, "wpos against the oracle")
    host = _rollout(env, m)
    assert_bits(head.rollout.w1t, host.w1t, "w1t against set_weights")
    assert_bits(head.rollout.wpos, host.wpos, "wpos against set_weights")
    assert_bits(head.rollout.b1, host.b1)
    assert_bits(head.rollout.w2, host.w2)
    assert float(head.rollout.b2_dev) == host.b2 and head.rollout.b2 is None


# -------------------------------------------------------------------------------------- parity with the existing kernel
@pytest.mark.parametrize("N,A,W,H", [(300, 1, 8, 32), (77, 3, 7, 64), (131, 5, 4, 32), (200, 1, 16, 128)])
def test_sampled_entry_without_noise_equals_the_plain_rollout_and_forward_equals_its_actions(N, A, W, H):
    from finenvs_amd.trajectory import TrajectoryBuffer

    m = _module(H, W, 3 * N + W, "relu")
    envs = [_env(N, W, A=A), _env(N, W, A=A)]
    plain, sampled = _rollout(envs[0], m), _rollout(envs[1], m)
    K = 5
    for rep in range(3):
        a0, r0, d0 = plain.run(K)
        traj = TrajectoryBuffer(K, N, A, device=envs[1]._dev, states=True)
        a1, r1, d1 = sampled.run(K, trajectory=traj)  # fe_env_rollout_mlp_sampled: no noise, clamp
        what = f"replay {rep}"
        assert_bits(a1, a0, what + " actions")
        assert_bits(r1, r0, what + " rewards")
        assert_bits(d1, d0, what + " dones")
        for name in ("cash", "margin", "long_shares", "short_shares", "env_indices", "env_spots"):
            assert_bits(getattr(envs[1], name), getattr(envs[0], name), f"{what} {name}")
        assert_bits(sampled.obs_src, plain.obs_src, what + " obs_src")
        assert_bits(sampled.obs_pos, plain.obs_pos, what + " obs_pos")
        assert_bits(traj.obs_src[K], sampled.obs_src, what + " last descriptor row")
        assert_bits(traj.obs_pos[K], sampled.obs_pos)
        for k in range(K):  # the head on the recorded state of step k is the action of step k
            assert_bits(sampled.forward(traj.obs_src[k], traj.obs_pos[k]), a0[k], f"{what} forward on row {k}")
    assert float(a0.abs().max()) > 0.3 and float(a0.min()) < 0 < float(a0.max())


@pytest.mark.parametrize("N,A,W,H,activation", [(300, 1, 8, 32, "elu"), (77, 3, 7, 64, "tanh"), (200, 1, 16, 128, "relu")])
def test_output_activations(N, A, W, H, activation):
    m = _module(H, W, N + H, activation)
    env = _env(N, W, A=A)
    heads = {out: _rollout(env, m, out) for out in ("clamp", "none", "tanh")}
    src, pos = heads["clamp"].obs_src, heads["clamp"].obs_pos
    y = {out: h.forward(src, pos) for out, h in heads.items()}
    inside = y["none"].abs() < 1.0
    assert float(inside.float().mean()) >= 0.3
    assert_bits(y["none"][inside], y["clamp"][inside])
    assert bool((y["clamp"][~inside].abs() == 1.0).all())
    p = y["none"].reshape(-1).contiguous()
    sig, tanh = torch.empty_like(p), torch.empty_like(p)
    from finenvs_amd import _lib

    _lib.check(env._lib.fe_lstm_activations(p.data_ptr(), sig.data_ptr(), tanh.data_ptr(), p.numel(), env._stream()))
    assert_bits(y["tanh"].reshape(-1), tanh, "tanh output")


# ------------------------------------------------------------------------------------------------------------ sampling
@pytest.mark.parametrize("N,A,W,H,evaluate", [(300, 1, 8, 32, False), (77, 3, 7, 64, False), (131, 1, 4, 32, True)])
def test_sampling(N, A, W, H, evaluate):
    from finenvs_amd.trajectory import TrajectoryBuffer

    m = _module(H, W, N + 1)
    envs = [_env(N, W, A=A, evaluate=evaluate) for _ in range(2)]
    r6, r33 = _rollout(envs[0], m, "tanh"), _rollout(envs[1], m, "tanh")
    dev = envs[0]._dev
    gen = torch.Generator(device=dev).manual_seed(N)
    noise = torch.randn((6, N, A), generator=gen, device=dev)
    std = 0.7
    traj = TrajectoryBuffer(6, N, A, device=dev, states=True)
    a, r, d = r6.run(6, noise=noise, std=std, record_means=True, trajectory=traj)
    means = r6.means
    assert a.data_ptr() == traj.actions.data_ptr() and r.data_ptr() == traj.rewards.data_ptr()
    assert d.data_ptr() == traj.dones.data_ptr() and len(traj) == 6
    want = (means + torch.tensor(std, dtype=F32, device=dev) * noise).clamp(-1.0, 1.0)
    if not evaluate:
        ev = int(envs[0]._eval_env)  # the evaluation env of a training-mode env: its last
        assert ev == N - 1
        assert_bits(a[:, ev], means[:, ev], "the eval env acts on its mean")
        assert not torch.equal(want[:, ev], means[:, ev])
        want[:, ev] = means[:, ev]
    assert_bits(a, want, "actions = clamp(means + std * noise)")
    assert int((a != means).sum()) > 0.9 * (a.numel() - 6 * A)
    assert bool((a.abs() == 1.0).any()) and bool((means.abs() < 1.0).all())
    # two launches of three steps are one of six
    parts = [r33.run(3, noise=noise[:3].contiguous(), std=std, record_means=True)]
    m0 = r33.means
    parts.append(r33.run(3, noise=noise[3:].contiguous(), std=std, record_means=True))
    assert_bits(torch.cat([m0, r33.means]), means, "means")
    for i, name in enumerate(("actions", "rewards", "dones")):
        assert_bits(torch.cat([parts[0][i], parts[1][i]]), (a, r, d)[i], name)
    assert_bits(r33.obs_src, r6.obs_src)
    assert_bits(r33.obs_pos, r6.obs_pos)
    # the means are the head on the recorded states
    for k in (0, 5):
        assert_bits(r6.forward(traj.obs_src[k], traj.obs_pos[k]), means[k], f"means of step {k}")
    with pytest.raises(ValueError, match="std"):
        r6.run(1, noise=noise[:1].contiguous())
    with pytest.raises(ValueError, match="noise must be"):
        r6.run(2, noise=noise[:1].contiguous(), std=std)
    with pytest.raises(ValueError, match="trajectory must be"):
        r6.run(3, trajectory=TrajectoryBuffer(4, N, A, device=dev, states=True))


# -------------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("H,W,activation,output", [(32, 4, "elu", "tanh"), (64, 7, "relu", "none"), (128, 16, "tanh", "tanh"),
                                                   (128, 64, "elu", "none")])
def test_values_equal_forward_bit_for_bit_and_the_torch_module(H, W, activation, output):
    from finenvs_amd.mlp_head import FusedMLPHead

    env = _env(300, W)
    src, pos, _ = _descriptors(env, 557)
    m = _module(H, W, 11, activation, output)
    head = FusedMLPHead(env, m)
    y = head(src, pos)
    assert y.shape == (557, 1) and y.dtype is F32 and y.requires_grad
    assert_bits(y, head.rollout.forward(src, pos))
    assert_bits(y, _rollout(env, m, output).forward(src, pos), "device packing against host packing")
    with torch.no_grad():
        ref = m(env.render(src, pos).float())
    assert float((y.detach() - ref).abs().max()) <= 1e-5
    assert float(ref.std()) > 0.05


# ----------------------------------------------------------------------------------------------------------- gradients
class _Shaped(nn.Module):
    """An MLPHead under the attribute names tests/test_lstm_grad_gpu.py::_ppo_inputs perturbs (``last_layer[0].bias``)."""

    def __init__(self, m):
        super().__init__()
        self.m = m
        self.last_layer = nn.Sequential(m.network[2], m.network[3])

    def forward(self, states):
        return self.m(states)


def _conditions(module, states):
    """The batch conditions, from the f64 copy; returns the kink mask (B, 1)."""
    B = states.shape[0]
    m64 = copy.deepcopy(module).double()
    with torch.no_grad():
        x = states.double().reshape(B, -1)
        pre = m64.network[0](x)
        p = m64.network[2](m64.network[1](pre))
    assert float(p.abs().max()) < 4.0, float(p.abs().max())  # not saturated
    neg = float((pre < 0).double().mean())
    assert 0.2 <= neg <= 0.8, neg
    kink = (pre.abs() < 1e-5).any(dim=1, keepdim=True)
    assert int(kink.sum()) <= 0.01 * B, (int(kink.sum()), B)
    return kink


def _loss(kind, y, kink, extra, dtype):
    from finenvs_amd.lstm_head import torch_ppo_actor_loss, torch_ppo_critic_loss

    y = torch.where(kink, y.detach(), y)  # upstream gradient 0 at ReLU's kink, in every arm
    if kind == "ppo_actor":
        log_std, actions, old_log_probs, advantages = extra
        return torch_ppo_actor_loss(y, log_std, actions.to(dtype), old_log_probs.to(dtype), advantages.to(dtype), CLIP, ENT)
    if kind == "ppo_critic":
        return torch_ppo_critic_loss(y, extra.to(dtype))
    return y.sum()


def _torch_grads(kind, module, states, kink, extra, dtype):
    m = copy.deepcopy(module).to(dtype)
    _zero(m)
    if kind == "ppo_actor":
        log_std = extra[0].detach().clone().to(dtype).requires_grad_(True)
        extra = (log_std,) + tuple(extra[1:])
    loss = _loss(kind, m(states.to(dtype)), kink, extra, dtype)
    loss.backward()
    return loss.detach(), [p.grad for p in _params(m)] + ([log_std.grad] if kind == "ppo_actor" else [])


def _fused_grads(kind, head, src, pos, kink, extra):
    _zero(head.module)
    if kind == "ppo_actor":
        log_std = extra[0].detach().clone().requires_grad_(True)
        extra = (log_std,) + tuple(extra[1:])
    loss = _loss(kind, head(src, pos), kink, extra, F32)
    loss.backward()
    return loss.detach(), [p.grad.clone() for p in _params(head.module)] + ([log_std.grad] if kind == "ppo_actor" else [])


def _compare(kind, g, g32, g64):
    worst = 0.0
    for name, gf, gt, gd in zip(NAMES + ("log_std",), g, g32, g64):
        assert gf.shape == gd.shape and gf.dtype is F32, (kind, name)
        assert float(gd.abs().max()) > 0, (kind, name)  # not degenerate
        err = float((gf.double() - gd).abs().max())
        tol = 2e-5 * float(gd.abs().max()) + 4 * float((gt.double() - gd).abs().max())
        print(f"{kind:10s} {name:7s} err {err:.3e} tol {tol:.3e} ratio {err / tol:.3f}")
        worst = max(worst, err / tol)
        assert err <= tol, (kind, name, err, tol)
    return worst


def _check_against_f64(kind, head, env, src, pos, seed=7):
    states = env.render(src, pos)
    B = int(src.numel())
    kink = _conditions(head.module, states)
    if kind == "ppo_actor":
        extra = tl._ppo_inputs(_Shaped(head.module), states, seed)
    elif kind == "ppo_critic":
        gen = torch.Generator(device="cuda").manual_seed(seed)
        with torch.no_grad():
            extra = head.module(states.float()) + 0.3 * torch.randn((B, 1), generator=gen, device="cuda")  # the returns
    else:
        extra = None
    loss, g = _fused_grads(kind, head, src, pos, kink, extra)
    l32, g32 = _torch_grads(kind, head.module, states.float(), kink, extra, F32)
    l64, g64 = _torch_grads(kind, head.module, states.double(), kink, extra, F64)
    assert len(g) == len(g32) == len(g64) == (5 if kind == "ppo_actor" else 4)
    worst = _compare(kind, g, g32, g64)
    err, tol = abs(float(loss) - float(l64)), 2e-5 * abs(float(l64)) + 4 * abs(float(l32) - float(l64)) + 1e-7
    assert err <= tol, (kind, "loss", err, tol)
    return worst


def _max_window(H):
    """The largest W whose W1^T fits the LDS next to the rollout's tile of 128 pairs (mlp_lds_bytes of
    finenvs_amd/csrc/fe_rollout_kernels.h at EB = 128, A = 1, against 160 KiB)."""
    def lds(W):
        kp = -(-4 * W // 32) * 32 + 4
        tile = 128 * 8 + 128 * 8 + 128 * 8 + 128 * 4 + 128 * 4 + 128 * 4
        b = ((tile + 7) & ~7) + 128 * 8 + 128 * 4
        b = (b + 15) & ~15
        return (b + H * kp * 4 + 3 * H * 4 + 15) & ~15

    W = 1
    while lds(W + 1) <= 160 * 1024:
        W += 1
    return W


WMAX = _max_window(128)
ACTIVATION_CASES = [(H, 4, 33, act, F64 if (H // 32 + i) % 2 else F32) for H in (32, 64, 128)
                    for i, act in enumerate(("elu", "relu", "tanh"))]
SIZE_CASES = [
    (64, 4, 1, "elu", F64), (32, 4, 31, "elu", F32), (128, 4, 32, "elu", F64), (64, 4, 257, "relu", F32),
    (32, 4, 4097, "elu", F64), (128, 4, 4097, "tanh", F32),
    (64, 4, CHUNK - 1, "elu", F32), (128, 4, CHUNK, "elu", F64), (32, 4, CHUNK + 1, "relu", F64),
    (64, 4, 2 * CHUNK + 33, "tanh", F32),
    (32, 4, 70001, "elu", F64),        # more blocks than the first kernel has wavefronts: its grid-stride
    (32, 1, 33, "elu", F64),           # W = 1: the second lane half reads only zero padding
    (128, 1, 31, "relu", F32),
    (64, 2, 33, "elu", F32),
    (64, 7, 33, "elu", F64),           # odd W: the last row group half empty
    (32, 7, 257, "tanh", F32),
    (128, 64, 257, "elu", F64),        # nine feature tiles
    (128, WMAX, 33, "elu", F32),       # the largest window the LDS admits at H = 128
]


@pytest.mark.parametrize("H,W,B,activation,obs_dtype", ACTIVATION_CASES + SIZE_CASES)
def test_gradients_against_f64_torch(H, W, B, activation, obs_dtype):
    """Worst err / tol over kinds (PPO actor, PPO critic, y.sum() of both heads) and tensors per case (H, W, B, activation),
    measured on an MI355X:
      activations at W = 4, B = 33   H = 32: elu 0.208, relu 0.040, tanh 0.016;  H = 64: 0.119, 0.430, 0.018;
                                     H = 128: 0.063, 0.054, 0.051
      batch sizes at W = 4           (64, 1, elu) 0.028, (32, 31, elu) 0.077, (128, 32, elu) 0.057, (64, 257, relu) 0.111,
                                     (32, 4 097, elu) 0.262, (128, 4 097, tanh) 0.198
      around the split of 512 pairs  (64, 511, elu) 0.308, (128, 512, elu) 0.195, (32, 513, relu) 0.285,
                                     (64, 1 057, tanh) 0.090
      the first kernel's grid-stride (32, 4, 70 001, elu) 0.203
      windows                        W = 1: (32, 33, elu) 0.027, (128, 31, relu) 0.177;  W = 2: (64, 33, elu) 0.114;
                                     W = 7: (64, 33, elu) 0.088, (32, 257, tanh) 0.058;  W = 64: (128, 257, elu) 0.200;
                                     W = 72, the largest at H = 128: (128, 33, elu) 0.059
    No separate ELU bound was needed (v_exp_f32 against libm stays inside the yardstick)."""
    from finenvs_amd.mlp_head import FusedMLPHead

    env = _env(min(B, 4096), W, obs_dtype=obs_dtype)
    src, pos, _ = _descriptors(env, B)
    actor = FusedMLPHead(env, _module(H, W, 20 + H + W, activation, "tanh"))
    value = FusedMLPHead(env, _module(H, W, 21 + H + W, activation, "none"))
    worst = max(_check_against_f64("ppo_actor", actor, env, src, pos),
                _check_against_f64("ppo_critic", value, env, src, pos),
                _check_against_f64("sum", actor, env, src, pos),
                _check_against_f64("sum", value, env, src, pos))
    print(f"WORST ({H}, {W}, {B}, {activation}) {worst:.3f}")


def test_the_largest_window_is_the_largest():
    from finenvs_amd import _lib
    from finenvs_amd.mlp_head import FusedMLPHead

    assert WMAX == 72
    env = _env(8, WMAX + 1)
    m = _module(128, WMAX + 1, 1)
    with pytest.raises(_lib.FinEnvsNativeError, match="does not fit"):
        FusedMLPHead(env, m)(*_descriptors_of(env))
    roll = _rollout(env, m, "tanh")
    with pytest.raises(_lib.FinEnvsNativeError, match="fe_env_rollout_mlp_sampled: W1 .* does not fit"):
        roll.run(1, record_means=True)
    # the C ABI refuses the backward itself too, before it touches a pointer
    lib, w, g = env._lib, _lib.FeMlpWeights(*([16] * 5)), _lib.FeMlpGrads(*([16] * 4))
    rc = lib.fe_mlp_backward(env._handle, 16, C.byref(w), 128, 0, 0, 16, 16, 4, 16, 16, 16, C.byref(g), None)
    assert rc == _lib.FE_ERR_ARG and b"fe_mlp_backward: W1 (128 x 292) does not fit" in lib.fe_last_error()
    FusedMLPHead(env, _module(64, WMAX + 1, 1))(*_descriptors_of(env))  # H = 64 fits


def _descriptors_of(env):
    roll = _rollout(env, _module(32, env.num_intervals, 2))
    return roll.obs_src, roll.obs_pos


# ------------------------------------------------------------------------------- determinism and autograd behaviour
def test_backward_is_deterministic_and_grad_accumulates_as_torchs_does():
    from finenvs_amd.mlp_head import FusedMLPHead

    for H, W, B, act, output in ((32, 4, 1057, "elu", "tanh"), (128, 16, 4097, "relu", "none")):
        env = _env(1024, W)
        src, pos, _ = _descriptors(env, B)
        head = FusedMLPHead(env, _module(H, W, 4, act, output))
        gen = torch.Generator(device="cuda").manual_seed(H)
        up = torch.randn((B, 1), generator=gen, device="cuda")

        def grads(zero=True):
            if zero:
                _zero(head.module)
            (head(src, pos) * up).sum().backward()
            return [p.grad.clone() for p in _params(head.module)]

        g1, g2 = grads(), grads()
        for a, b, name in zip(g1, g2, NAMES):
            assert_bits(a, b, f"two backward calls, {name}")
            assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
        g3 = grads(zero=False)  # .grad accumulates
        for a, b, name in zip(g3, g1, NAMES):
            assert_bits(a, b + b, f"accumulated {name}")
        head.module.zero_grad(set_to_none=False)  # ... into the zeroed buffers, not over them
        g4 = grads(zero=False)
        for a, b in zip(g4, g1):
            assert_bits(a, b)
        # an upstream gradient that arrives expanded, strided or as f64 gives the same bits as its f32 copy
        _zero(head.module)
        (head(src, pos).double() * up.double()).sum().backward()
        for p, b in zip(_params(head.module), g1):
            assert_bits(p.grad, b)


def test_a_frozen_head_launches_nothing_and_an_empty_batch_works(monkeypatch):
    from finenvs_amd.mlp_head import FusedMLPHead

    env = _env(64, 4)
    src, pos, _ = _descriptors(env, 64)
    head = FusedMLPHead(env, _module(32, 4, 9))
    calls = []
    real = env._lib.fe_mlp_backward
    monkeypatch.setattr(env._lib, "fe_mlp_backward", lambda *a: calls.append(1) or real(*a))
    scale = torch.ones((), device="cuda", requires_grad=True)
    head.module.requires_grad_(False)
    y = head(src, pos)
    assert not y.requires_grad
    (y * scale).sum().backward()
    assert calls == [] and all(p.grad is None for p in _params(head.module))
    head.module.requires_grad_(True)
    head.module.network[0].weight.requires_grad_(False)  # partly frozen: one launch, the frozen tensor gets nothing
    head(src, pos).sum().backward()
    assert calls == [1] and head.module.network[0].weight.grad is None
    assert all(p.grad is not None for p in _params(head.module)[1:])
    # B = 0
    head.module.requires_grad_(True)
    _zero(head.module)
    packs = []
    real_pack = env._lib.fe_mlp_pack
    monkeypatch.setattr(env._lib, "fe_mlp_pack", lambda *a: packs.append(1) or real_pack(*a))
    y = head(src[:0], pos[:0])
    assert y.shape == (0, 1)
    y.sum().backward()
    assert calls == [1] and packs == []
    for p in _params(head.module):
        assert p.grad is not None and float(p.grad.abs().max()) == 0.0
    assert head.rollout.forward(src[:0], pos[:0]).shape == (0, 1)


def test_refusals():
    from finenvs_amd import _lib
    from finenvs_amd.mlp_head import FusedMLPHead, MLPHead

    env2 = _env(8, 4, A=2)
    with pytest.raises(ValueError, match="one asset"):
        FusedMLPHead(env2, _module(32, 4, 1))
    lib, w, g = env2._lib, _lib.FeMlpWeights(*([16] * 5)), _lib.FeMlpGrads(*([16] * 4))
    rc = lib.fe_mlp_backward(env2._handle, 16, C.byref(w), 32, 0, 0, 16, 16, 4, 16, 16, 16, C.byref(g), None)
    assert rc == _lib.FE_ERR_ARG and b"fe_mlp_backward: the env has 2 assets" in lib.fe_last_error()
    env = _env(8, 4)
    with pytest.raises(ValueError, match="float32 parameters"):
        FusedMLPHead(env, _module(32, 4, 1).double())
    with pytest.raises(ValueError, match="must live on the env's device"):
        FusedMLPHead(env, MLPHead(32, 4))
    with pytest.raises(ValueError, match="window of 7 rows"):
        FusedMLPHead(env, _module(32, 7, 1))
    head = FusedMLPHead(env, _module(32, 4, 1))
    with pytest.raises(ValueError, match="one position per descriptor"):
        head(head.rollout.obs_src, head.rollout.obs_pos[:3])
    with pytest.raises(ValueError, match="output_activation must be one of"):
        _rollout(env, _module(32, 4, 1), "sigmoid")


# ----------------------------------------------------------------------------------------------------- memory contract
GUARD = 4096
SENTINEL = -12345.5


def _sentinel(dtype):
    return SENTINEL if dtype.is_floating_point else int(SENTINEL)


def _window(n, dtype, fill):
    """A window of n elements inside a larger allocation, GUARD sentinel elements on either side."""
    big = torch.full((n + 2 * GUARD,), _sentinel(dtype), dtype=dtype, device="cuda")
    win = big[GUARD:GUARD + n]
    win.fill_(fill)
    return big, win


def _bands_intact(big, n, what):
    s = _sentinel(big.dtype)
    assert bool((big[:GUARD] == s).all()) and bool((big[GUARD + n:] == s).all()), f"{what}: written outside"


@pytest.mark.parametrize("H,W,B,output", [(32, 4, 1, "tanh"), (64, 7, 33, "none"), (128, 16, 1057, "tanh")])
def test_memory_contract_of_forward_and_backward(H, W, B, output):
    from finenvs_amd import _lib
    from finenvs_amd.mlp_head import FusedMLPHead

    env = _env(min(B, 512), W)
    src, pos, _ = _descriptors(env, B)
    head = FusedMLPHead(env, _module(H, W, 13, "elu", output))
    roll, lib = head.rollout, env._lib
    weights = roll._weights()
    out_act = roll.out_act
    # out: exactly B floats
    big_out, out = _window(B, F32, float("nan"))
    _lib.check(lib.fe_mlp_forward(env._handle, roll._lr32.data_ptr(), C.byref(weights), H, roll.act, out_act, src.data_ptr(),
                                  pos.data_ptr(), B, out.data_ptr(), env._stream()))
    _bands_intact(big_out, B, "out")
    assert_bits(out.reshape(B, 1), roll.forward(src, pos))
    # the backward: workspace of exactly the size the function returns, the four gradient buffers; two poisons
    gen = torch.Generator(device="cuda").manual_seed(B)
    up = torch.randn((B,), generator=gen, device="cuda")
    n_ws = int(lib.fe_mlp_grad_workspace_floats(H, W, B))
    sizes = {"w1": H * 5 * W, "b1": H, "w2": H, "b2": 1}
    results = []
    for poison in (float("nan"), SENTINEL):
        big_ws, ws = _window(n_ws, F32, poison)
        wins = {k: _window(n, F32, poison) for k, n in sizes.items()}
        mg = _lib.FeMlpGrads(*(wins[k][1].data_ptr() for k in NAMES))
        _lib.check(lib.fe_mlp_backward(env._handle, roll._lr32.data_ptr(), C.byref(weights), H, roll.act, out_act,
                                       src.data_ptr(), pos.data_ptr(), B, out.data_ptr(), up.data_ptr(), ws.data_ptr(),
                                       C.byref(mg), env._stream()))
        _bands_intact(big_ws, n_ws, "workspace")
        for k, n in sizes.items():
            _bands_intact(wins[k][0], n, k)
            assert bool(torch.isfinite(wins[k][1]).all()), k
        results.append([wins[k][1].clone() for k in NAMES])
    for a, b, k in zip(results[0], results[1], NAMES):
        assert_bits(a, b, f"{k}: NaN-filled against sentinel-filled buffers")
    _zero(head.module)
    (head(src, pos).reshape(B) * up).sum().backward()
    for a, p, k in zip(results[0], _params(head.module), NAMES):
        assert_bits(a, p.grad.reshape(-1), f"{k} against the front end")


@pytest.mark.parametrize("N,A,W,H", [(131, 1, 4, 32), (77, 3, 7, 64)])
def test_memory_contract_of_the_sampled_rollout(N, A, W, H):
    from finenvs_amd import _lib

    K = 3
    envs = [_env(N, W, A=A), _env(N, W, A=A)]
    m = _module(H, W, 17)
    roll, twin = _rollout(envs[0], m, "tanh"), _rollout(envs[1], m, "tanh")
    dev = envs[0]._dev
    gen = torch.Generator(device=dev).manual_seed(N)
    noise = torch.randn((K, N, A), generator=gen, device=dev)
    a_ref, r_ref, d_ref = twin.run(K, noise=noise, std=0.4, record_means=True)
    nan = float("nan")
    wins = {"actions": _window(K * N * A, F32, nan), "means": _window(K * N * A, F32, nan),
            "rewards": _window(K * N, F64, nan), "dones": _window(K * N, I32, -7),
            "ssrc": _window((K + 1) * N, I64, -7), "spos": _window((K + 1) * N * A, F64, nan)}
    big_noise, nwin = _window(K * N * A, F32, 0.0)
    big_noise.fill_(nan)  # a read past the noise reaches an action
    nwin.copy_(noise.reshape(-1))
    lib, w = envs[0]._lib, roll._weights()
    roll._begin_run()
    _lib.check(lib.fe_env_rollout_mlp_sampled(
        envs[0]._handle, roll._lr32.data_ptr(), C.byref(w), H, roll.act, roll.out_act, K, roll.obs_src.data_ptr(),
        roll.obs_pos.data_ptr(), nwin.data_ptr(), 0.4, wins["actions"][1].data_ptr(), wins["means"][1].data_ptr(),
        wins["rewards"][1].data_ptr(), wins["dones"][1].data_ptr(), wins["ssrc"][1].data_ptr(), wins["spos"][1].data_ptr(),
        envs[0]._stream()))
    roll._end_run()
    for name, (big, win) in wins.items():
        _bands_intact(big, win.numel(), name)
    assert_bits(wins["actions"][1], a_ref.reshape(-1), "actions")
    assert_bits(wins["means"][1], twin.means.reshape(-1), "means")
    assert_bits(wins["rewards"][1], r_ref.reshape(-1), "rewards")
    assert_bits(wins["dones"][1], d_ref.reshape(-1), "dones")
    assert_bits(wins["ssrc"][1][K * N:], twin.obs_src.reshape(-1), "last descriptor row")
    assert_bits(wins["spos"][1][K * N * A:], twin.obs_pos.reshape(-1))
    assert bool((wins["ssrc"][1] >= 0).all()) and bool(torch.isfinite(wins["spos"][1]).all())


# ------------------------------------------------------------------------------------------------------------- example
def _example():
    spec = importlib.util.spec_from_file_location("ppo_mlp_fused", os.path.join(ROOT, "examples", "ppo_mlp_fused.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("fused_optim", [False, True])
def test_ppo_example_with_fused_update_trains_without_rendering(monkeypatch, fused_optim):
    from finenvs_amd import TimeSeriesEnv, mlp_head
    from finenvs_amd.trajectory import TrajectoryBuffer

    mod = _example()
    heads = []

    class Recording(mlp_head.FusedMLPHead):
        def __init__(self, env, module):
            super().__init__(env, module)
            heads.append(self)

    def refuse(self, *a, **k):
        raise AssertionError("an observation was rendered")

    monkeypatch.setattr(mod, "FusedMLPHead", Recording)
    monkeypatch.setattr(TrajectoryBuffer, "minibatch_states", refuse)
    monkeypatch.setattr(TimeSeriesEnv, "render", refuse)
    history = mod.main(envs=256, steps=4, iters=2, hidden=32, window=4, fused_update=True, fused_optim=fused_optim, quiet=True)
    assert len(history) == 2 and len(heads) == 2
    for critic_loss, mean_reward, log in history:
        assert np.isfinite(critic_loss) and np.isfinite(mean_reward)
        assert log["num_training_episodes"] >= 0
    for head, output in zip(heads, ("tanh", "none")):
        assert head.output_activation == output
        src, pos = head.rollout.obs_src.clone(), head.rollout.obs_pos.clone()
        acted = head.rollout.forward(src, pos).clone()  # what the kernel runs after the example's last update
        y = head(src, pos)  # re-packs the module's parameters as they stand
        assert_bits(acted, y)
        assert bool(torch.isfinite(y).all())
        # and those are the trained parameters: a rollout object made from the module now gives the same bits
        assert_bits(_rollout(head.env, head.module, output).forward(src, pos), acted)
        untrained = mlp_head.MLPHead(32, 4, "elu", output)
        with torch.no_grad():
            untrained.network[0].weight.reshape(32, 4, 5)[:, :, :4].mul_(100.0)
        assert not torch.equal(head.module.network[0].weight.cpu(), untrained.network[0].weight)


ADAM_LR, ADAM_EPS = 3e-4, 1e-8


def _adam_bound(theta, g_twin, delta):
    """|theta_fused - theta_twin| after ONE Adam step from equal parameters and zero moments.

    The first step is theta - lr f(g) with f(g) = g / (|g| + eps): the bias corrections cancel the (1 - beta) factors,
    so the step is the gradient's SIGN wherever |g| >> eps, whatever its size -- a bound scaled by lr |g_fused - g_twin|
    would miss that.  (Measured on an MI355X at B = 1 024, H = 32: the parameters of the two arms differ by at most 9.5e-7
    -- one element of the critic's W1 whose gradient lies within delta of zero, bound 6.0e-4 = 2 lr -- and by at most 1e-9
    everywhere else, against bounds of 7e-9 to 5e-6.)  f is increasing, odd and bounded by 1, with f'(g) = eps / (|g| + eps)^2.  If the two gradients
    differ by at most delta (per tensor: the yardstick's tolerance for |g_fused - g64| plus the twin's own
    |g_twin - g64|):
      * an element with |g_twin| <= delta may change sign: |f(g_fused) - f(g_twin)| <= 2;
      * otherwise both lie on one side of zero, at least |g_twin| - delta from it, and the mean value theorem gives
        |f(g_fused) - f(g_twin)| <= delta eps / (|g_twin| - delta + eps)^2.
    On top come the roundings of the update itself: f(g) is a handful of f32 operations (relative error 8 ulp of a
    value <= 1) and the subtraction rounds to theta's grid (1 ulp of theta, each arm)."""
    g = g_twin.abs().double()
    same_side = delta * ADAM_EPS / ((g - delta).clamp_min(0.0) + ADAM_EPS) ** 2
    step = torch.where(g <= delta, torch.full_like(g, 2.0), same_side.clamp_max(2.0))
    ulp = 2.0 ** -23
    return ADAM_LR * (step + 8 * ulp) + 2 * ulp * theta.abs().double()


@pytest.mark.parametrize("kind,output", [("ppo_actor", "tanh"), ("ppo_critic", "none")])
def test_one_adam_step_agrees_with_an_eager_twin_on_the_rendered_minibatch(kind, output):
    """The update of examples/ppo_mlp_fused.py (loss on descriptors, backward, Adam with the example's lr) against an eager
    torch twin doing the same update on the rendered mini-batch: the parameters agree within ``_adam_bound``."""
    from finenvs_amd.lstm_head import ppo_actor_loss, ppo_critic_loss, torch_ppo_actor_loss, torch_ppo_critic_loss
    from finenvs_amd.mlp_head import FusedMLPHead

    H, W, B = 32, 4, 1024
    env = _env(256, W, obs_dtype=F32)
    src, pos, _ = _descriptors(env, B)
    module = _module(H, W, 31, "elu", output)
    twin, m64 = copy.deepcopy(module), copy.deepcopy(module).double()
    head = FusedMLPHead(env, module)
    states = env.render(src, pos)
    kink = _conditions(module, states)
    assert not bool(kink.any())  # (ELU has no kink anyway; the public loss functions take no mask)
    if kind == "ppo_actor":
        log_std, actions, old_logp, adv = tl._ppo_inputs(_Shaped(module), states, 3)
        ls = [log_std.detach().clone().requires_grad_(True) for _ in range(3)]
        fused_loss = ppo_actor_loss(head, ls[0], src, pos, actions, old_logp, adv, CLIP, ENT, fused=True)
        twin_loss = torch_ppo_actor_loss(twin(states.float()), ls[1], actions, old_logp, adv, CLIP, ENT)
        loss64 = torch_ppo_actor_loss(m64(states.double()), ls[2].double(), actions.double(), old_logp.double(), adv.double(),
                                      CLIP, ENT)
    else:
        gen = torch.Generator(device="cuda").manual_seed(3)
        with torch.no_grad():
            returns = module(states.float()) + 0.3 * torch.randn((B, 1), generator=gen, device="cuda")
        fused_loss = ppo_critic_loss(head, src, pos, returns, fused=True)
        twin_loss = torch_ppo_critic_loss(twin(states.float()), returns)
        loss64 = torch_ppo_critic_loss(m64(states.double()), returns.double())
    before = [p.detach().clone() for p in _params(module)]
    opts = [torch.optim.Adam(m.parameters(), ADAM_LR, eps=ADAM_EPS) for m in (module, twin)]
    for loss, opt in zip((fused_loss, twin_loss), opts):
        opt.zero_grad()
        loss.backward()
        opt.step()
    loss64.backward()
    for name, pf, pt, pd, p0 in zip(NAMES, _params(module), _params(twin), _params(m64), before):
        g64 = pd.grad
        tol = 2e-5 * float(g64.abs().max()) + 4 * float((pt.grad.double() - g64).abs().max())
        assert float((pf.grad.double() - g64).abs().max()) <= tol, (kind, name)  # the yardstick itself
        delta = tol + float((pt.grad.double() - g64).abs().max())
        bound = _adam_bound(p0, pt.grad, delta)
        diff = (pf.detach().double() - pt.detach().double()).abs()
        moved = (pt.detach() - p0).abs()
        print(f"{kind} {name}: max diff {float(diff.max()):.3e}, max bound {float(bound.max()):.3e}, "
              f"elements free to flip {int((pt.grad.abs().double() <= delta).sum())} of {pt.numel()}")
        assert bool((diff <= bound).all()), (kind, name, float((diff - bound).max()))
        assert float(moved.max()) > 0.5 * ADAM_LR  # the step happened
        # and the bound bites: most elements are held far tighter than a sign flip's 2 lr
        assert float((bound < 0.01 * ADAM_LR).double().mean()) > 0.5, (kind, name)
    head.refresh()
    assert_bits(head.rollout.forward(src, pos), head(src, pos))
