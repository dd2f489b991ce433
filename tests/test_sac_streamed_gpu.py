"""GPU: the SAC LSTM actor at H = 256 / 512 / 1024 (``FusedSACRollout(env, actor, streamed=True)``, C ABI of
include/finenvs_amd_sac_streamed.h), with the helpers and the yardstick of tests/test_sac_grad_gpu.py and
tests/test_critic_streamed_gpu.py.

* anchors, bit for bit, from an actor with ``last_layer.weight = I`` and ``b_l = 0`` (z = h_W exactly): ``forward()``'s
  means equal ``FusedLSTMRollout.forward(output_activation="none")`` with ``w_out = w_mu``, ``b_out = b_mu``; with
  ``w_std = 0`` and zero noise besides (actions = tanh(mu)) ``fe_sac_backward_streamed`` with ``d_log_probs`` null gives
  ``fe_lstm_backward_streamed``'s (out_activation 0) ``w_ih``, ``w_hh``, ``b_ih``, ``b_hh``, ``w_out`` and ``b_out``;
* values against an f64 ``SACActorLSTM`` on the rendered states within ``2e-5 max|ref64| + 4 max|torch32 - ref64|``
  (log_probs where |u| <= 4, finite everywhere); mu and std do not depend on the noise; ``sample()`` returns
  ``forward()``'s bits;
* the ten gradients against f64 within ``2e-5 max|g64| + 4 max|g_torch32 - g64|`` for the three loss kinds of
  tests/test_sac_grad_gpu.py, the chained one through a ``FusedTwinCritic(streamed=True)``, on f32 and f64 envs.  The
  weights of the ``log_probs`` kind are drawn around 0.5: a zero-mean upstream gradient makes ``d b_mu`` / ``d b_std``
  cancelling sums whose tolerance collapses at thousands of pairs (NOTES.md, 2026-10-17).  (256, 4, chunk + 33) is the
  case that leaves K splits of the last-layer contraction EMPTY: its first chunk has 84 chains of 1024 pairs over 32
  splits of 3 chains each, so splits 28 .. 31 own no chain and must write zeros; (1024, 4, 1100) has two chains (one
  per split) and a partial 32-pair tile.  Worst err / tol over kinds and tensors, measured on an MI355X: MEASURED;
* two backward calls give the same bits; ``.grad`` accumulates; a single used output works; a frozen actor launches
  nothing; B = 0 works; ``actor_losses`` on a wrapped ring and from a ``ReplayDraw``;
* one ``FusedAdam`` step equals ``reference_update`` bit for bit at H = 256, the resident buffers equal
  ``pack_sac_weights``, the version check raises; a captured SAC actor update equals its eager twin;
* ``examples/sac_time_series.py`` at ``hidden=256`` with every ``--fused-*`` flag renders no mini-batch; refusals.
"""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from tests.test_critic_streamed_gpu import _chunk, _scaled
from tests.test_sac_grad_gpu import (NAMES, _actor, _check_against_f64, _descriptors, _env, _fused_grads, _loss, _params,
                                     _torch_grads, _zero, assert_bits)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (H, W, B) -> worst err / tol over the three kinds and the ten tensors, (f64 env, f32 env), measured on an MI355X
MEASURED = {(256, 4, 1): (0.402, 0.407), (256, 4, 33): (0.058, 0.058), (512, 5, 257): (0.048, 0.048),
            (1024, 4, 33): (0.069, 0.069), (256, 1, 33): (0.035, 0.034), (1024, 4, 1100): (0.065, 0.064),
            (256, 4, "chunk + 33"): (0.038, 0.038)}  # (256, 4, 1): d b_mu of the log_probs kind, one pair


def _setup(H, W, B, obs_dtype=torch.float64, twin=True, N=None):
    from finenvs_amd.critic import FusedTwinCritic
    from finenvs_amd.sac import FusedSACRollout

    env = _env(N or min(B, 4096), W, obs_dtype=obs_dtype)
    src, pos, _ = _descriptors(env, B)
    assert src.numel() == B
    roll = FusedSACRollout(env, _actor(H, W, 20), streamed=True)
    assert roll.streamed
    fused = None
    if twin:
        gen = torch.Generator(device="cuda").manual_seed(4)
        n = min(B, 4096)
        actions = torch.rand((n, 1), generator=gen, device="cuda") * 2 - 1
        states = env.render(src[:n], pos[:n])
        fused = FusedTwinCritic(env, _scaled(H, W, 10, states, actions), _scaled(H, W, 11, states, actions), streamed=True)
    return env, roll, fused, src, pos


def _identity_last_layer(actor, zero_std=False):
    with torch.no_grad():
        actor.last_layer[0].weight.copy_(torch.eye(actor.hidden_size, device="cuda"))
        actor.last_layer[0].bias.zero_()
        actor.mu_layer.weight.mul_(4.0)
        if zero_std:
            actor.std_layer.weight.zero_()
    return actor


# ---------------------------------------------------------------- anchors
@pytest.mark.parametrize("H,B", [(256, 33), (1024, 33)])
def test_identity_last_layer_means_equal_the_lstm_head_bit_for_bit(H, B):
    from finenvs_amd.rollout import FusedLSTMRollout
    from finenvs_amd.sac import FusedSACRollout

    W = 4
    env = _env(B, W)
    src, pos, _ = _descriptors(env, B)
    actor = _identity_last_layer(_actor(H, W, 20))
    roll = FusedSACRollout(env, actor, streamed=True)
    _, _, means, stds = roll.forward(src, pos)
    lstm = actor.lstm
    head = FusedLSTMRollout(env, lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0,
                            actor.mu_layer.weight, float(actor.mu_layer.bias.detach()), output_activation="none")
    want = head.forward(src, pos)
    assert float(want.abs().max()) > 0.05 and float(want.std()) > 1e-3 and bool(torch.isfinite(stds).all())
    assert_bits(means.reshape(-1), want.reshape(-1))


@pytest.mark.parametrize("H,W,B", [(256, 4, 33), (512, 5, 257)])
def test_identity_last_layer_backward_equals_the_lstm_heads_bit_for_bit(H, W, B):
    """z = h_W, dz = w_mu dmu and dh_W = I^T dz exactly, so everything the two passes share sees the same bits."""
    from finenvs_amd import _lib
    from finenvs_amd.sac import SAC_GRAD_KEYS, FusedSACRollout

    env = _env(B, W)
    src, pos, _ = _descriptors(env, B)
    actor = _identity_last_layer(_actor(H, W, 20), zero_std=True)
    roll = FusedSACRollout(env, actor, streamed=True)
    noise = torch.zeros((B, 1), device="cuda")
    actions, _, means, stds = roll.forward(src, pos, noise)
    assert float(means.abs().max()) > 0.05 and float(actions.abs().max()) < 1.0
    w, lib = roll._packed, env._lib
    gen = torch.Generator(device="cuda").manual_seed(5)
    d = (torch.randn((B,), generator=gen, device="cuda") - 1.0) / B
    nan = float("nan")  # whatever a kernel leaves unwritten, in a workspace of its own or in an output, stays NaN
    ws_sac = torch.full((int(lib.fe_sac_streamed_grad_workspace_floats(H, W, B)),), nan, device="cuda")
    ws_head = torch.full((int(lib.fe_lstm_streamed_grad_workspace_floats(H, W, B)),), nan, device="cuda")
    shapes = {"w_ih": (4 * H, 5), "w_hh": (4 * H, H), "b_ih": (4 * H,), "b_hh": (4 * H,), "w_l": (H, H), "b_l": (H,),
              "w_mu": (H,), "b_mu": (1,), "w_std": (H,), "b_std": (1,)}
    sac = {k: torch.full(shapes[k], nan, device="cuda") for k in SAC_GRAD_KEYS}
    head = {k: torch.full(shapes[k], nan, device="cuda") for k in ("w_ih", "w_hh", "b_ih", "b_hh", "w_mu", "b_mu")}
    sg = _lib.FeSacGrads(*(sac[k].data_ptr() for k in SAC_GRAD_KEYS))
    lg = _lib.FeLstmGrads(*(head[k].data_ptr() for k in ("w_ih", "w_hh", "b_ih", "b_hh", "w_mu", "b_mu")))
    src, pos = src.reshape(B).contiguous(), pos.reshape(B).contiguous()
    a = actions.reshape(B).contiguous()
    _lib.check(lib.fe_sac_backward_streamed(
        env._handle, roll._lr32.data_ptr(), w["whh"].data_ptr(), w["wx"].data_ptr(), w["wl"].data_ptr(), w["bl"].data_ptr(),
        w["wmu"].data_ptr(), w["bmu"].data_ptr(), w["wstd"].data_ptr(), w["bstd"].data_ptr(), H, src.data_ptr(),
        pos.data_ptr(), B, noise.data_ptr(), a.data_ptr(), stds.data_ptr(), d.data_ptr(), None, ws_sac.data_ptr(),
        C.byref(sg), env._stream()), lib)
    _lib.check(lib.fe_lstm_backward_streamed(
        env._handle, roll._lr32.data_ptr(), w["whh"].data_ptr(), w["wx"].data_ptr(), w["wmu"].data_ptr(), H, 0,
        src.data_ptr(), pos.data_ptr(), B, a.data_ptr(), d.data_ptr(), ws_head.data_ptr(), C.byref(lg), env._stream()), lib)
    for k in sac:  # every element of every output was written by its own call
        assert bool(torch.isfinite(sac[k]).all()), k
    for k in head:
        assert bool(torch.isfinite(head[k]).all()) and float(head[k].abs().max()) > 0, k
        assert_bits(sac[k], head[k])


# ---------------------------------------------------------------- values
def _within(name, got, t32, t64, mask=None):
    if mask is not None:
        got, t32, t64 = got[mask], t32[mask], t64[mask]
    err = float((got.double() - t64).abs().max())
    tol = 2e-5 * float(t64.abs().max()) + 4 * float((t32.double() - t64).abs().max())
    print(f"{name:8s} err {err:.3e} tol {tol:.3e} ratio {err / tol:.3f}")
    assert err <= tol, (name, err, tol)


@pytest.mark.parametrize("H,W,B", [(256, 4, 33), (512, 5, 257), (1024, 4, 1100)])
def test_values_against_f64_and_sample_equals_forward(H, W, B):
    env, roll, _, src, pos = _setup(H, W, B, twin=False)
    eps = torch.randn((B, 1), generator=torch.Generator(device="cuda").manual_seed(3), device="cuda")
    act, lp, mu, sd = roll.forward(src, pos, eps)
    _, _, mu0, sd0 = roll.forward(src, pos)
    assert_bits(mu0, mu)
    assert_bits(sd0, sd)
    states = env.render(src, pos)
    ref = {}
    for dtype in (torch.float32, torch.float64):
        a = copy.deepcopy(roll.actor).to(dtype)
        with torch.no_grad():
            dist = a.get_distribution(states.to(dtype))
            ta, tlp = a.get_actions_and_log_probs(states.to(dtype), eps.to(dtype))
            ref[dtype] = (dist.loc, dist.scale, ta, tlp, dist.loc + eps.to(dtype) * dist.scale)
    r32, r64 = ref[torch.float32], ref[torch.float64]
    for name, got, i in (("mu", mu, 0), ("std", sd, 1), ("tanh(u)", act, 2)):
        assert tuple(got.shape) == (B, 1) and got.dtype is torch.float32
        _within(name, got, r32[i], r64[i])
    assert bool(torch.isfinite(lp).all())
    inner = r64[4].abs() <= 4
    assert bool(inner.any())
    _within("log_prob", lp, r32[3], r64[3], inner)
    assert float(r64[0].std()) > 1e-3 and float(r64[1].std()) > 1e-5, "the head must depend on the observation"
    a2, lp2 = roll.sample(src, pos, eps)
    assert a2.requires_grad and lp2.requires_grad
    assert_bits(a2, act)
    assert_bits(lp2, lp)
    assert_bits(roll.last["means"], mu)
    assert_bits(roll.last["stds"], sd)


# ---------------------------------------------------------------- gradients
GRAD_CASES = [
    (256, 4, 1),
    (256, 4, 33),
    (512, 5, 257),           # crosses a 256-pair head block
    (1024, 4, 33),
    (256, 1, 33),            # W = 1: no recurrent step; d w_hh is identically zero and must come out exactly zero
    (1024, 4, 1100),         # two chains of the last-layer contraction and a partial tile
    (256, 4, "chunk + 33"),  # two passes (the second adds); splits 28 .. 31 of the last-layer contraction own no chain
]


@pytest.mark.parametrize("obs_dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("H,W,B", GRAD_CASES)
def test_gradients_against_f64_torch(H, W, B, obs_dtype):
    if B == "chunk + 33":
        B = _chunk(H, W) + 33
    env, roll, twin, src, pos = _setup(H, W, B, obs_dtype)
    gen = torch.Generator(device="cuda").manual_seed(5)
    eps = torch.randn((B, 1), generator=gen, device="cuda")
    c = 0.5 + 0.25 * torch.randn((B, 1), generator=gen, device="cuda")  # off-centre (see the module's docstring)
    for kind in ("chained", "log_probs", "actions"):
        _check_against_f64(kind, roll, twin, env, src, pos, eps, c)
    g = [p.grad for p in _params(roll.actor)]
    if W == 1:
        assert float(g[1].abs().max()) == 0.0
    assert_bits(g[2], g[3])  # d b_ih = d b_hh


@pytest.mark.parametrize("H,W,B", [(256, 4, "chunk + 33"), (1024, 4, 300)])
def test_backward_is_deterministic(H, W, B):
    if B == "chunk + 33":
        B = _chunk(H, W) + 33
    _, roll, twin, src, pos = _setup(H, W, B)
    eps = torch.randn((B, 1), device="cuda")
    c = 0.5 + 0.25 * torch.randn((B, 1), device="cuda")
    _, a, _ = _fused_grads("chained", roll, twin, src, pos, eps, c)
    _, b, _ = _fused_grads("chained", roll, twin, src, pos, eps, c)
    for x, z in zip(a, b):
        assert float(x.abs().max()) > 0
        assert_bits(x, z)


def test_accumulation_single_outputs_a_frozen_actor_and_an_empty_batch(monkeypatch):
    H, W, B = 256, 4, 300
    env, roll, twin, src, pos = _setup(H, W, B)
    eps = torch.randn((B, 1), device="cuda")
    c = 0.5 + 0.25 * torch.randn((B, 1), device="cuda")
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
    real = env._lib.fe_sac_backward_streamed
    monkeypatch.setattr(env._lib, "fe_sac_backward_streamed", lambda *a: calls.append(1) or real(*a), raising=False)
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
    # an empty batch
    _zero(roll.actor)
    a0, lp0 = roll.sample(src[:0], pos[:0], eps[:0])
    assert tuple(a0.shape) == tuple(lp0.shape) == (0, 1)
    (a0.sum() + lp0.sum()).backward()
    assert calls == [1]
    for p in _params(roll.actor):
        assert p.grad is not None and float(p.grad.abs().max()) == 0.0


# ---------------------------------------------------------------- actor_losses on the ring
def _ring(env, K, max_size, cursor=False, seed=13):
    from finenvs_amd.replay import ReplayBuffer

    _, _, traj = _descriptors(env, env.num_envs * (K + 1))
    buffer = ReplayBuffer(env, max_size=max_size, cursor=cursor, seed=seed)
    buffer.extend(traj)
    assert buffer.size() == buffer.max_size and buffer.head != 0  # wrapped
    return buffer


def _twin_for(env, buffer, idx, H, W):
    from finenvs_amd.critic import FusedTwinCritic

    b = buffer.get_mini_batch(int(idx.numel()), indices=idx)
    return FusedTwinCritic(env, _scaled(H, W, 10, b["states"], b["actions"]), _scaled(H, W, 11, b["states"], b["actions"]),
                           streamed=True), b


def test_actor_losses_on_a_wrapped_ring_against_f64_and_from_a_replay_draw():
    from finenvs_amd.sac import FusedSACRollout

    H, W, N, K, B = 256, 4, 64, 6, 100
    env = _env(N, W)
    buffer = _ring(env, K, N * K // 2 + 37, cursor=True)
    draw = buffer.draw(B)
    idx = draw.indices.clone()
    twin, b = _twin_for(env, buffer, idx, H, W)
    roll = FusedSACRollout(env, _actor(H, W, 20), streamed=True)
    eps = torch.randn((B, 1), device="cuda")

    def losses(indices):
        _zero(roll.actor, twin.critic_1, twin.critic_2)
        roll.actor.log_alpha.grad = None
        loss, alpha_loss = roll.actor_losses(buffer, indices, twin, noise=eps)
        loss.backward()
        return loss.detach().clone(), alpha_loss.detach().clone(), [p.grad.clone() for p in _params(roll.actor)]

    loss, alpha_loss, g = losses(idx)
    states = b["states"]
    c = torch.zeros((B, 1), device="cuda")
    l32, g32, _ = _torch_grads("chained", roll.actor, twin.critic_1, twin.critic_2, states.float(), eps, c, torch.float32)
    l64, g64, _ = _torch_grads("chained", roll.actor, twin.critic_1, twin.critic_2, states.double(), eps, c, torch.float64)
    for name, gf, gt, gd in zip(NAMES, g, g32, g64):
        err = float((gf.double() - gd).abs().max())
        tol = 2e-5 * float(gd.abs().max()) + 4 * float((gt.double() - gd).abs().max())
        assert err <= tol, (name, err, tol)
    err, tol = abs(float(loss) - float(l64)), 2e-5 * abs(float(l64)) + 4 * abs(float(l32) - float(l64))
    print(f"actor loss {float(loss):.8f} f64 {float(l64):.8f} err {err:.3e} tol {tol:.3e}")
    assert err <= tol, (err, tol)
    # from the draw: the bits of its indices
    loss_d, alpha_d, g_d = losses(draw)
    assert_bits(loss_d, loss)
    assert_bits(alpha_d, alpha_loss)
    for x, z in zip(g_d, g):
        assert float(z.abs().max()) > 0
        assert_bits(x, z)
    bad = idx.clone()
    bad[3] = buffer.size()
    assert torch.isnan(roll.actor_losses(buffer, bad, twin, noise=eps)[0]).item()


# ---------------------------------------------------------------- the optimizer and the captured update
def test_one_fused_adam_step_equals_the_reference_update_and_the_packers():
    from finenvs_amd.optim import FusedAdam, initial_state, reference_update
    from finenvs_amd.sac import FusedSACRollout, pack_sac_weights
    from tests.test_optim_gpu import _cpu, _same_bits

    H, W, B = 256, 4, 64
    env = _env(B, W)
    src, pos, _ = _descriptors(env, B)
    actor = _actor(H, W, 20)
    opt = FusedAdam(lr=3e-3)
    opt.add(actor)
    opt.add_tensor(actor.log_alpha)
    roll = FusedSACRollout(env, actor, weights=opt, streamed=True)
    for k, v in pack_sac_weights(actor).items():  # the resident buffers are the packer's before any step
        assert _same_bits(opt.packed(actor)[k], v), k
    eps = torch.randn((B, 1), device="cuda")
    c = 0.5 + 0.25 * torch.randn((B, 1), device="cuda")
    params = opt.parameters()
    ref_p = _cpu(params)
    ref_m, ref_v = [torch.zeros_like(p) for p in ref_p], [torch.zeros_like(p) for p in ref_p]
    opt.zero_grad()
    actions, log_probs = roll.sample(src, pos, eps)
    ((log_probs * c).sum() + actions.sum() + actor.log_alpha.exp()).backward()
    grads = _cpu([p.grad for p in params])
    assert all(float(g.abs().max()) > 0 for g in grads)
    opt.step()
    reference_update(ref_p, grads, ref_m, ref_v, initial_state(), 3e-3)
    for i, p in enumerate(params):
        assert _same_bits(p, ref_p[i]), (i, "param")
    want, got = pack_sac_weights(actor), opt.packed(actor)
    assert set(want) == set(got)
    for k in want:
        assert tuple(got[k].shape) == tuple(want[k].shape) and _same_bits(got[k], want[k]), k
    # the resident front end reads what the step wrote: a fresh one without the optimizer gives the same bits
    fresh = FusedSACRollout(env, actor, streamed=True)
    for x, z in zip(roll.forward(src, pos, eps), fresh.forward(src, pos, eps)):
        assert_bits(x, z)
    # a step between a forward and its backward is an error
    actions, log_probs = roll.sample(src, pos, eps)
    opt.step()  # (the gradients are the zeros the first step left)
    with pytest.raises(RuntimeError):
        actions.sum().backward()


def test_a_captured_sac_update_equals_the_eager_one():
    from finenvs_amd.critic import FusedTwinCritic
    from finenvs_amd.graphed import GraphedUpdate
    from finenvs_amd.optim import FusedAdam
    from finenvs_amd.replay import ReplayBuffer
    from finenvs_amd.sac import FusedSACRollout

    H, W, N, K, B = 256, 4, 64, 4, 64

    def arm(graphed):
        env = _env(N, W)
        _, _, traj = _descriptors(env, N * (K + 1))
        buffer = ReplayBuffer(env, max_size=N * K, cursor=True, seed=19)
        buffer.extend(traj)
        b = buffer.get_mini_batch(B, indices=torch.arange(B, device="cuda"))
        actor = _actor(H, W, 20)
        c1, c2 = _scaled(H, W, 10, b["states"], b["actions"]), _scaled(H, W, 11, b["states"], b["actions"])
        c1.requires_grad_(False)
        c2.requires_grad_(False)
        opt = FusedAdam(lr=3e-3)
        opt.add(actor)
        opt.add_tensor(actor.log_alpha)
        roll = FusedSACRollout(env, actor, weights=opt, streamed=True)
        twin = FusedTwinCritic(env, c1, c2, streamed=True)
        draw = buffer.new_draw(B)
        gen = torch.Generator(device="cuda").manual_seed(6)
        eps = torch.empty((B, 1), device="cuda")

        def refill():
            eps.copy_(torch.randn((B, 1), generator=gen, device="cuda"))

        def fn():
            buffer.draw(B, out=draw)
            actor_loss, alpha_loss = roll.actor_losses(buffer, draw, twin, noise=eps)
            opt.zero_grad()
            actor_loss.backward()
            alpha_loss.backward()
            opt.step()
            return actor_loss.detach()

        refill()
        losses = []
        if graphed:
            g = GraphedUpdate(fn, warmup=1, between=refill)
            for _ in range(3):
                losses.append(g.replay().clone())
                refill()
        else:
            fn()
            refill()
            for _ in range(3):
                losses.append(fn().clone())
                refill()
        state = {n: p.detach().clone() for n, p in actor.named_parameters()}
        state["log_alpha"] = actor.log_alpha.detach().clone()
        for i, x in enumerate(losses):
            state[f"loss{i}"] = x
        state["cursor"] = buffer.cursor.clone()
        return state

    eager, graphed = arm(False), arm(True)
    assert list(eager) == list(graphed)
    for k in eager:
        assert bool(torch.isfinite(eager[k].float()).all()), k
        assert_bits(eager[k], graphed[k])
    assert float((eager["loss0"] - eager["loss2"]).abs()) > 0


# ---------------------------------------------------------------- the example and the refusals
def test_the_sac_example_trains_at_hidden_256_without_rendering_a_mini_batch(monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import sac_time_series

    from finenvs_amd.replay import ReplayBuffer

    def refuse(self, *a, **k):
        raise AssertionError("get_mini_batch was called")

    monkeypatch.setattr(ReplayBuffer, "get_mini_batch", refuse)
    for kw in (dict(), dict(fused_optim=True), dict(graph_update=True)):
        hist = sac_time_series.main(num_envs=64, hidden=256, iterations=3, chunk=4, batch=64, days=12, bars=60, quiet=True,
                                    fused_targets=True, fused_critics=True, fused_actor=True, log_every=1, **kw)
        assert len(hist) == 3, kw
        assert all(np.isfinite([h["critic_loss"], h["actor_loss"], h["alpha_loss"]]).all() for h in hist), (kw, hist)


def test_refusals():
    from finenvs_amd import _lib
    from finenvs_amd.optim import FusedAdam
    from finenvs_amd.sac import FusedSACRollout, SACActorLSTM

    env = _env(64, 4)
    with pytest.raises(ValueError, match="streamed=True"):
        FusedSACRollout(env, SACActorLSTM(H=256, W=4).cuda())
    for H in (2048, 48):
        with pytest.raises(ValueError, match=str(H)):
            FusedSACRollout(env, SACActorLSTM(H=H, W=4).cuda(), streamed=True)
    env2 = _env(8, 4, A=2)
    roll2 = FusedSACRollout(env2, _actor(256, 4, 1), streamed=True)  # acting runs any A the env has
    src2 = torch.zeros((8,), dtype=torch.int64, device="cuda")
    pos2 = torch.zeros((8, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="one asset"):
        roll2.sample(src2, pos2, torch.zeros((8, 1), device="cuda"))
    # the C ABI refuses the A = 2 env itself, after the null checks and H and before it touches any other pointer
    grads = _lib.FeSacGrads(*([16] * 10))
    lib = env2._lib
    rc = lib.fe_sac_backward_streamed(env2._handle, 16, 16, 16, 16, 16, 16, 16, 16, 16, 256, 16, 16, 8, 16, 16, 16, 16, 16,
                                      16, C.byref(grads), None)
    assert rc == _lib.FE_ERR_ARG
    assert lib.fe_last_error().startswith(b"fe_sac_backward_streamed:") and b"2 assets" in lib.fe_last_error()
    rc = lib.fe_sac_backward_streamed(env2._handle, 16, 16, 16, 16, 16, 16, 16, 16, 16, 128, 16, 16, 8, 16, 16, 16, 16, 16,
                                      16, C.byref(grads), None)
    assert rc == _lib.FE_ERR_ARG and b"H must be 256, 512 or 1024" in lib.fe_last_error()  # H comes before A
    # an actor the optimizer does not hold
    opt = FusedAdam(lr=1e-3)
    opt.add(_actor(256, 4, 2))
    with pytest.raises(ValueError):
        FusedSACRollout(env, _actor(256, 4, 3), weights=opt, streamed=True)
    # the small sizes run the register-resident way whether or not streamed is passed
    small = FusedSACRollout(env, _actor(32, 4, 1), streamed=True)
    assert small.H == 32 and not small.streamed
    src, pos, _ = _descriptors(env, 64)
    eps = torch.randn((64, 1), device="cuda")
    roll = FusedSACRollout(env, _actor(256, 4, 1), streamed=True)
    for bad in (None, eps.double(), eps.reshape(64), eps[:63], eps.cpu()):
        with pytest.raises(ValueError, match="noise"):
            roll.sample(src, pos, bad)
