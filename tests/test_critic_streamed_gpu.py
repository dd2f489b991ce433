"""GPU: the twin LSTM critics at H = 256 / 512 / 1024 (``FusedTwinCritic(env, c1, c2, streamed=True)``, C ABI of
include/finenvs_amd_critic_streamed.h), with the helpers and the yardstick of tests/test_critic_grad_gpu.py.

* anchor: with ``w_ih[:, 5] = 0`` a critic's value is ``fe_lstm_forward(out_activation 2)`` on the same weights bit for
  bit;
* the same anchor for the backward: ``fe_twin_q_backward_streamed`` on that critic gives ``fe_lstm_backward_streamed``'s
  ``w_hh``, ``w_ih[:, :5]``, ``b_ih``, ``b_hh``, ``w_out`` and ``b_out`` bit for bit;
* values against an f64 torch ``CriticLSTM`` on the rendered states within ``2e-5 max|q64| + 4 max|q32 - q64|``; ``q()``
  returns ``forward``'s bits;
* the thirteen gradients (twelve parameter tensors and ``d_actions``) against f64 within ``2e-5 max|g64| +
  4 max|g_torch32 - g64|``, on f32 and f64 envs.  The targets are drawn off-centre (``randn - 1``) and the output layers
  scaled so that ``0.5 < max|w_out . h_W| < 4`` on the test's own batch: with a zero-mean upstream gradient ``d b_out``
  is a cancelling sum whose tolerance collapses at thousands of pairs (NOTES.md).  Worst err / tol over the thirteen
  tensors and both env dtypes, measured on an MI355X: MEASURED below;
* two backward calls give the same bits; ``.grad`` accumulates as torch's does; a frozen critic gets nothing and still
  passes ``dQ/da`` on; actions without ``requires_grad`` get nothing; TD3's actor loss runs critic 1 only (critic 2's
  buffers keep a sentinel); B = 0 works;
* ``td3_targets`` / ``sac_targets`` on a wrapped ring against the torch restatements; an out-of-range index; a
  ``ReplayDraw`` gives the bits of its indices;
* ``td3_actor_loss`` with a streamed actor head, ``FusedSACRollout.actor_losses`` through a streamed twin;
* one ``FusedAdam`` step equals ``reference_update`` bit for bit, the resident packed buffers equal
  ``pack_critic_weights``, the version check raises; a captured TD3 critic update equals the eager one;
* ``examples/td3_lstm_fused.py`` trains at ``hidden=256`` without rendering anything; refusals.
"""
import copy
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_critic_grad_gpu import _check_against_f64, _critic, _descriptors, _env, _fused_grads, _params, assert_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMA = 0.97

# (H, W, B) -> worst err / tol over the thirteen tensors, (f64 env, f32 env), measured on an MI355X.  Values (q1, q2):
# (256, 4, 33) 0.030, (512, 5, 257) 0.029, (1024, 4, 1100) 0.070; td3 / sac targets at H = 256: 0.027 / 0.035.
MEASURED = {(256, 4, 1): (0.041, 0.041), (256, 4, 33): (0.049, 0.048), (512, 5, 257): (0.039, 0.037),
            (1024, 4, 33): (0.058, 0.058), (256, 1, 33): (0.061, 0.059), (512, 7, 257): (0.047, 0.047),
            (1024, 4, 1100): (0.031, 0.030), (256, 4, "chunk + 33"): (0.029, 0.029)}


def _chunk(H, W):
    from finenvs_amd import _lib

    return int(_lib.load().fe_lstm_streamed_grad_chunk_pairs(H, W))


def _scaled(H, W, seed, states, actions):
    """``_critic`` of tests/test_critic_grad_gpu.py (input weights scaled so that log-returns and the action move the
    gates), then the output weights scaled so that max|w_out . h_W| (f64, bias excluded) is 1.5 on the test's own
    batch."""
    c = _critic(H, W, seed)
    n = min(int(states.shape[0]), 4096)
    with torch.no_grad():
        c64 = copy.deepcopy(c).double()
        x = torch.cat([states[:n].double(), actions[:n].double().reshape(n, 1, 1).expand(n, W, 1)], dim=2)
        h_w = c64.lstm(x)[0][:, -1, :]
        assert float(h_w.abs().max()) > 0.05, "the gates do not move"
        c.last_layer[0].weight.mul_(1.5 / float((h_w @ c64.last_layer[0].weight.t()).abs().max()))
        pmax = float((h_w @ c.last_layer[0].weight.double().t()).abs().max())
    assert 0.5 < pmax < 4.0, pmax
    return c


def _batch(H, W, B, obs_dtype=torch.float64, seeds=(10, 11)):
    from finenvs_amd.critic import FusedTwinCritic

    env = _env(min(B, 4096), W, obs_dtype=obs_dtype)
    src, pos, _ = _descriptors(env, B)
    assert src.numel() == B
    gen = torch.Generator(device="cuda").manual_seed(5)
    actions = torch.rand((B, 1), generator=gen, device="cuda") * 2 - 1
    y = torch.randn((B, 1), generator=gen, device="cuda") - 1.0  # off-centre: mean(q - y) of the order of its spread
    states = env.render(src[:4096], pos[:4096])
    fused = FusedTwinCritic(env, _scaled(H, W, seeds[0], states, actions), _scaled(H, W, seeds[1], states, actions),
                            streamed=True)
    return env, fused, src, pos, actions, y


def _zero(*modules):
    for m in modules:
        for p in m.parameters():
            p.grad = None


@pytest.mark.parametrize("H,W,B", [(256, 4, 33), (1024, 4, 33)])
def test_zero_action_weight_equals_the_lstm_value_head_bit_for_bit(H, W, B):
    from finenvs_amd.rollout import FusedLSTMRollout

    env, fused, src, pos, actions, _ = _batch(H, W, B)
    c1 = fused.critic_1
    with torch.no_grad():
        c1.lstm.weight_ih_l0[:, 5].zero_()
    q1, q2 = fused.forward(src, pos, actions)
    lstm = c1.lstm
    head = FusedLSTMRollout(env, lstm.weight_ih_l0[:, :5], lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0,
                            c1.last_layer[0].weight, float(c1.last_layer[0].bias.detach()), output_activation="none")
    want = head.forward(src, pos)
    assert float(want.abs().max()) > 0.1 and float((q2 - q1).abs().max()) > 1e-3
    assert_bits(q1, want)


def zero_action_weight_backward(env, src, pos, H, W, B):
    """fe_twin_q_backward_streamed (critic 1 alone, ``w_ih[:, 5] = 0``) and fe_lstm_backward_streamed (no output activation)
    on the same packed weights, descriptors and upstream gradient: ``(critic's six gradient tensors, head's six)``."""
    import ctypes as C

    from finenvs_amd import _lib
    from finenvs_amd.critic import GRAD_KEYS, empty_packed_grads, pack_critic_weights

    lib = env._lib
    c = _critic(H, W, 10)
    with torch.no_grad():
        c.lstm.weight_ih_l0[:, 5].zero_()
    w = pack_critic_weights(c)
    assert float(w["wx"][:, 6].abs().max()) == 0.0
    cw = _lib.FeCriticWeights(*(w[k].data_ptr() for k in ("whh", "wx", "wout", "bout")))
    gen = torch.Generator(device="cuda").manual_seed(5)
    actions = torch.rand((B,), generator=gen, device="cuda") * 2 - 1  # they reach nothing: their weight is zero
    d = (torch.randn((B,), generator=gen, device="cuda") - 1.0) / B
    lr32 = env.log_return_environments.float().contiguous()
    nan = float("nan")  # whatever a kernel leaves unwritten, in a workspace of its own or in an output, stays NaN
    n_ws = int(lib.fe_twin_q_streamed_grad_workspace_floats(H, W, B))
    assert n_ws == int(lib.fe_lstm_streamed_grad_workspace_floats(H, W, B))
    ws_critic, ws_head = (torch.full((n_ws,), nan, device="cuda") for _ in range(2))
    critic = {k: v.fill_(nan) for k, v in empty_packed_grads(H, "cuda").items()}
    head = {k: torch.full((4 * H, 5) if k == "w_ih" else tuple(v.shape), nan, device="cuda") for k, v in critic.items()}
    cg = _lib.FeCriticGrads(*(critic[k].data_ptr() for k in GRAD_KEYS))
    lg = _lib.FeLstmGrads(*(head[k].data_ptr() for k in GRAD_KEYS))
    src, pos = src.reshape(B).contiguous(), pos.reshape(B).contiguous()
    _lib.check(lib.fe_twin_q_backward_streamed(
        env._handle, lr32.data_ptr(), C.byref(cw), C.byref(cw), H, src.data_ptr(), pos.data_ptr(), actions.data_ptr(), B,
        d.data_ptr(), None, ws_critic.data_ptr(), C.byref(cg), None, None, env._stream()), lib)
    _lib.check(lib.fe_lstm_backward_streamed(
        env._handle, lr32.data_ptr(), w["whh"].data_ptr(), w["wx"].data_ptr(), w["wout"].data_ptr(), H, 2, src.data_ptr(),
        pos.data_ptr(), B, None, d.data_ptr(), ws_head.data_ptr(), C.byref(lg), env._stream()), lib)
    return critic, head


# a partial 32-pair tile; a second, partial 256-pair head block
@pytest.mark.parametrize("H,W,B", [(256, 4, 33), (512, 5, 257)])
def test_zero_action_weight_backward_equals_the_lstm_value_heads_bit_for_bit(H, W, B):
    """The backward counterpart of the anchor above: the action's column only adds ``0 x action`` to the forward's chains,
    and the output columns of the weight contraction are independent, so the critic's gradients are the head's."""
    env = _env(min(B, 4096), W)
    src, pos, _ = _descriptors(env, B)
    critic, head = zero_action_weight_backward(env, src, pos, H, W, B)
    for k in critic:  # every element of every output was written by its own call
        assert bool(torch.isfinite(critic[k]).all()) and bool(torch.isfinite(head[k]).all()), k
        assert float(head[k].abs().max()) > 0, k
    for k in ("w_hh", "b_ih", "b_hh", "w_out", "b_out"):
        assert_bits(critic[k], head[k])
    assert_bits(critic["w_ih"][:, :5].contiguous(), head["w_ih"])


@pytest.mark.parametrize("H,W,B", [(256, 4, 33), (512, 5, 257), (1024, 4, 1100)])
def test_values_against_f64_and_q_equals_forward(H, W, B):
    env, fused, src, pos, actions, _ = _batch(H, W, B)
    q = fused.forward(src, pos, actions)
    states = env.render(src, pos)
    for c, got in zip((fused.critic_1, fused.critic_2), q):
        with torch.no_grad():
            q32 = c(states.float(), actions)
            q64 = copy.deepcopy(c).double()(states.double(), actions.double())
        err = float((got.double() - q64).abs().max())
        tol = 2e-5 * float(q64.abs().max()) + 4 * float((q32.double() - q64).abs().max())
        print(f"q ({H}, {W}, {B}) err {err:.3e} tol {tol:.3e} ratio {err / tol:.3f}")
        assert tuple(got.shape) == (B, 1) and got.dtype is torch.float32
        assert err <= tol, (err, tol)
        assert float(q64.std()) > 1e-2
    a = actions.clone().requires_grad_()
    d1, d2 = fused.q(src, pos, a)
    assert d1.requires_grad and d2.requires_grad
    assert_bits(d1, q[0])
    assert_bits(d2, q[1])


GRAD_CASES = [
    (256, 4, 1),
    (256, 4, 33),
    (512, 5, 257),
    (1024, 4, 33),
    (256, 1, 33),            # W = 1: no recurrent step; d w_hh is identically zero and must come out exactly zero
    (512, 7, 257),           # odd W
    (1024, 4, 1100),         # an empty trailing K split: 5 chains over 4 splits
    (256, 4, "chunk + 33"),  # two passes: a full chunk, then a ragged 33-pair tail (later chunks add; d_actions across it)
]


@pytest.mark.parametrize("obs_dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("H,W,B", GRAD_CASES)
def test_gradients_against_f64_torch(H, W, B, obs_dtype):
    if B == "chunk + 33":
        B = _chunk(H, W) + 33
    env, fused, src, pos, actions, y = _batch(H, W, B, obs_dtype)
    g = _check_against_f64(fused, env, src, pos, actions, y)
    for x, p in zip(g[:12], _params(fused.critic_1) + _params(fused.critic_2)):
        assert x.shape == p.shape
    if W == 1:
        assert float(g[1].abs().max()) == 0.0 and float(g[7].abs().max()) == 0.0
    assert_bits(g[2], g[3])  # d b_ih = d b_hh


@pytest.mark.parametrize("H,W,B", [(256, 4, "chunk + 33"), (1024, 4, 300)])
def test_backward_is_deterministic(H, W, B):
    if B == "chunk + 33":
        B = _chunk(H, W) + 33
    _, fused, src, pos, actions, y = _batch(H, W, B)
    a, _ = _fused_grads(fused, src, pos, actions, y)
    b, _ = _fused_grads(fused, src, pos, actions, y)
    for x, z in zip(a, b):
        assert float(x.abs().max()) > 0
        assert_bits(x, z)


def test_accumulation_frozen_critics_actions_without_grad_and_an_empty_batch():
    H, W, B = 256, 4, 300
    _, fused, src, pos, actions, y = _batch(H, W, B)
    once, _ = _fused_grads(fused, src, pos, actions, y)
    _zero(fused.critic_1, fused.critic_2)
    a = actions.clone().requires_grad_()
    for _ in range(2):  # no zero_grad in between
        q1, q2 = fused.q(src, pos, a)
        (F.mse_loss(q1, y) + F.mse_loss(q2, y)).backward()
    for p, g in zip(_params(fused.critic_1) + _params(fused.critic_2), once[:12]):
        torch.testing.assert_close(p.grad, 2 * g, rtol=1e-6, atol=0)
    torch.testing.assert_close(a.grad, 2 * once[12], rtol=1e-6, atol=0)
    # critic 2 frozen, actions without requires_grad
    _zero(fused.critic_1, fused.critic_2)
    fused.critic_2.requires_grad_(False)
    a = actions.clone()
    q1, q2 = fused.q(src, pos, a)
    (F.mse_loss(q1, y) + F.mse_loss(q2, y)).backward()
    assert all(p.grad is None for p in fused.critic_2.parameters()) and a.grad is None
    for p, g in zip(_params(fused.critic_1), once[:6]):
        assert_bits(p.grad, g)
    # a frozen critic still passes dQ/da on, critic 1 first and critic 2 added
    fused.critic_1.requires_grad_(False)
    a = actions.clone().requires_grad_()
    q1, q2 = fused.q(src, pos, a)
    (F.mse_loss(q1, y) + F.mse_loss(q2, y)).backward()
    assert_bits(a.grad, once[12])
    # one critic frozen, the other training: the same d_actions again, and the trained one's gradients
    fused.critic_2.requires_grad_(True)
    _zero(fused.critic_2)
    a = actions.clone().requires_grad_()
    q1, q2 = fused.q(src, pos, a)
    (F.mse_loss(q1, y) + F.mse_loss(q2, y)).backward()
    assert_bits(a.grad, once[12])
    for p, g in zip(_params(fused.critic_2), once[6:12]):
        assert_bits(p.grad, g)
    fused.critic_1.requires_grad_(True)
    # an empty batch
    _zero(fused.critic_1, fused.critic_2)
    a = actions[:0].clone().requires_grad_()
    q1, q2 = fused.q(src[:0], pos[:0], a)
    assert tuple(q1.shape) == tuple(q2.shape) == (0, 1)
    (q1.sum() + q2.sum()).backward()
    assert tuple(a.grad.shape) == (0, 1)
    for p in _params(fused.critic_1) + _params(fused.critic_2):
        assert p.grad is not None and float(p.grad.abs().max()) == 0.0


def test_td3_actor_loss_runs_critic_1_only_and_leaves_critic_2s_buffers_alone():
    import ctypes as C

    from finenvs_amd import _lib
    from finenvs_amd.critic import GRAD_KEYS, empty_packed_grads

    H, W, B = 256, 4, 257
    env, fused, src, pos, actions, _ = _batch(H, W, B)
    _zero(fused.critic_1, fused.critic_2)
    a = actions.clone().requires_grad_()
    q1, _ = fused.q(src, pos, a)
    (-q1.mean()).backward()  # TD3/actor.py compute_loss
    assert all(p.grad is None for p in fused.critic_2.parameters())
    assert all(p.grad is not None for p in fused.critic_1.parameters())
    states = env.render(src, pos)
    grads = []
    for dtype in (torch.float32, torch.float64):
        c = copy.deepcopy(fused.critic_1).to(dtype)
        at = actions.to(dtype).clone().requires_grad_()
        (-c(states.to(dtype), at).mean()).backward()
        grads.append(at.grad)
    err = float((a.grad.double() - grads[1]).abs().max())
    assert err <= 2e-5 * float(grads[1].abs().max()) + 4 * float((grads[0].double() - grads[1]).abs().max()), err
    # through the C entry: dq2 null, critic 2's gradient buffers keep their sentinel
    lib = env._lib
    cw = [_lib.FeCriticWeights(*(x[k].data_ptr() for k in ("whh", "wx", "wout", "bout"))) for x in fused._packed]
    bufs = [empty_packed_grads(H, "cuda") for _ in range(2)]
    for b in bufs:
        for t in b.values():
            t.fill_(-7.5)
    cg = [_lib.FeCriticGrads(*(b[k].data_ptr() for k in GRAD_KEYS)) for b in bufs]
    ws = torch.empty((int(lib.fe_twin_q_streamed_grad_workspace_floats(H, W, B)),), device="cuda")
    dq = torch.full((B,), -1.0 / B, device="cuda")
    da = torch.empty((B,), device="cuda")
    _lib.check(lib.fe_twin_q_backward_streamed(
        env._handle, fused._lr32.data_ptr(), C.byref(cw[0]), C.byref(cw[1]), H, src.data_ptr(), pos.data_ptr(),
        actions.reshape(B).contiguous().data_ptr(), B, dq.data_ptr(), None, ws.data_ptr(), C.byref(cg[0]), C.byref(cg[1]),
        da.data_ptr(), env._stream()), lib)
    assert all(bool((t == -7.5).all()) for t in bufs[1].values())
    assert all(not bool((t == -7.5).any()) for t in bufs[0].values())
    assert_bits(da.reshape(B, 1), a.grad)
    for k, p in zip(GRAD_KEYS, _params(fused.critic_1)):
        assert_bits(bufs[0][k].reshape(p.shape), p.grad)


# ---------------------------------------------------------------- targets from the ring
def _ring(W=4, N=200, K=6):
    from finenvs_amd.replay import ReplayBuffer

    env = _env(N, W)
    _, _, traj = _descriptors(env, N * (K + 1))
    buffer = ReplayBuffer(env, max_size=N * K // 2 + 37)
    buffer.extend(traj)
    assert buffer.size() == buffer.max_size and buffer.head != 0  # wrapped
    with torch.no_grad():
        buffer.dones[::7] = 1.0
    return env, buffer


def _twin_on(env, buffer, idx, H, W, seeds):
    from finenvs_amd.critic import FusedTwinCritic

    b = buffer.get_mini_batch(int(idx.numel()), indices=idx)
    c1, c2 = (_scaled(H, W, s, b["next_states"], b["actions"]) for s in seeds)
    return FusedTwinCritic(env, c1, c2, streamed=True), b


def _within(name, y, y32, y64):
    err = float((y.double() - y64).abs().max())
    tol = 2e-5 * float(y64.abs().max()) + 4 * float((y32.double() - y64).abs().max())
    print(f"{name} err {err:.3e} tol {tol:.3e} ratio {err / tol:.3f}")
    assert err <= tol, (name, err, tol)


def test_td3_targets_on_a_wrapped_ring_against_torch():
    from finenvs_amd.critic import torch_td3_targets
    from finenvs_amd.lstm_head import LSTMHead
    from finenvs_amd.rollout import FusedLSTMRollout

    H, W, B = 256, 4, 333
    env, buffer = _ring(W)
    idx = torch.randint(0, buffer.size(), (B,), device="cuda")
    twin, b = _twin_on(env, buffer, idx, H, W, (50, 51))
    torch.manual_seed(52)
    actor = LSTMHead(32, W, "tanh").cuda()
    with torch.no_grad():
        actor.lstm.weight_ih_l0[:, :4].mul_(6.0 * np.sqrt(32))
        actor.last_layer[0].weight.mul_(6.0)  # actions over the whole range, some beyond the clamp after smoothing
    target = FusedLSTMRollout.from_modules(env, actor.lstm, actor.last_layer[0], output_activation="tanh")
    eps = torch.randn((B, 1), device="cuda")
    y = twin.td3_targets(buffer, idx, target, eps, GAMMA, 0.2, 0.5)
    ys = []
    for dtype in (torch.float32, torch.float64):
        a, c1, c2 = (copy.deepcopy(m).to(dtype) for m in (actor, twin.critic_1, twin.critic_2))
        ys.append(torch_td3_targets(lambda x: a(x.to(dtype)), c1, c2, b["rewards"].to(dtype), b["next_states"].to(dtype),
                                    b["dones"].to(dtype), eps.to(dtype), GAMMA, 0.2, 0.5))
    _within("td3 targets", y, *ys)
    last = twin.last
    expr = b["rewards"] + GAMMA * (1 - b["dones"]) * torch.minimum(last["q1"], last["q2"])
    assert_bits(y, expr)
    done = b["dones"][:, 0] == 1
    assert bool(done.any()) and torch.equal(y[done], b["rewards"][done])
    # the smoothed action the critics saw: the kernel's q1 equals the forward on the same clamped action
    a = torch.clamp(last["next_actions"] + torch.clamp(eps * 0.2, -0.5, 0.5), -1, 1)
    slots = buffer.physical(idx)
    q1, q2 = twin.forward(buffer.next_src[slots], buffer.next_pos[slots], a)
    assert_bits(q1, last["q1"])
    assert_bits(q2, last["q2"])


def test_sac_targets_on_a_wrapped_ring_against_torch():
    from finenvs_amd.critic import torch_sac_targets
    from finenvs_amd.sac import FusedSACRollout
    from tests.test_critic_gpu import _actor

    H, W, B = 256, 4, 333
    env, buffer = _ring(W)
    idx = torch.randint(0, buffer.size(), (B,), device="cuda")
    twin, b = _twin_on(env, buffer, idx, H, W, (40, 41))
    actor = _actor(32, W, 42)
    roll = FusedSACRollout(env, actor)
    eps = torch.randn((B, 1), device="cuda")
    y = twin.sac_targets(buffer, idx, roll, eps, GAMMA, actor.log_alpha, reward_scale=0.01)
    ys = []
    for dtype in (torch.float32, torch.float64):
        a, c1, c2 = (copy.deepcopy(m).to(dtype) for m in (actor, twin.critic_1, twin.critic_2))
        ys.append(torch_sac_targets(a, c1, c2, b["rewards"].to(dtype), b["next_states"].to(dtype), b["dones"].to(dtype),
                                    eps.to(dtype), GAMMA, reward_scale=0.01))
    _within("sac targets", y, *ys)
    last = twin.last
    r, d = b["rewards"] * 0.01, b["dones"]
    expr = r + GAMMA * (1 - d) * (torch.min(last["q1"], last["q2"]) + (-last["alpha"] * last["log_probs"]))
    assert_bits(y, expr)


def test_an_out_of_range_index_gives_nan_and_counts_once():
    from finenvs_amd.lstm_head import LSTMHead
    from finenvs_amd.rollout import FusedLSTMRollout

    H, W, B = 256, 4, 37
    env, buffer = _ring(W)
    idx = torch.randint(0, buffer.size(), (B,), device="cuda")
    twin, _ = _twin_on(env, buffer, idx, H, W, (60, 61))
    torch.manual_seed(62)
    actor = LSTMHead(32, W, "tanh").cuda()
    target = FusedLSTMRollout.from_modules(env, actor.lstm, actor.last_layer[0], output_activation="tanh")
    eps = torch.randn((B, 1), device="cuda")
    good = twin.td3_targets(buffer, idx, target, eps, GAMMA, 0.2, 0.5).clone()
    bad = idx.clone()
    bad[5] = buffer.size()
    before = int(buffer.errors.item())
    y = twin.td3_targets(buffer, bad, target, eps, GAMMA, 0.2, 0.5)
    assert int(buffer.errors.item()) - before == 1
    keep = torch.ones(B, dtype=torch.bool, device="cuda")
    keep[5] = False
    for t in (y, twin.last["q1"], twin.last["q2"]):
        assert bool(torch.isnan(t[5]).all()) and bool(torch.isfinite(t[keep]).all())
    assert_bits(y[keep], good[keep])


def test_a_replay_draw_gives_the_bits_of_its_indices():
    from finenvs_amd.lstm_head import LSTMHead
    from finenvs_amd.replay import ReplayBuffer
    from finenvs_amd.rollout import FusedLSTMRollout

    H, W, N, K, B = 256, 4, 64, 5, 37
    env = _env(N, W)
    _, _, traj = _descriptors(env, N * (K + 1))
    buffer = ReplayBuffer(env, max_size=N * K // 2 + 37, cursor=True, seed=13)
    buffer.extend(traj)
    assert buffer.size() == buffer.max_size and buffer.head != 0
    draw = buffer.draw(B)
    twin, b = _twin_on(env, buffer, draw.indices, H, W, (70, 71))
    torch.manual_seed(72)
    actor = LSTMHead(32, W, "tanh").cuda()
    target = FusedLSTMRollout.from_modules(env, actor.lstm, actor.last_layer[0], output_activation="tanh")
    eps = torch.randn((B, 1), device="cuda")
    got = [twin.td3_targets(buffer, draw, target, eps, GAMMA, 0.2, 0.5).clone(), twin.last["q1"].clone(), twin.last["q2"].clone()]
    want = [twin.td3_targets(buffer, draw.indices, target, eps, GAMMA, 0.2, 0.5), twin.last["q1"], twin.last["q2"]]
    for g, w in zip(got, want):
        assert bool(torch.isfinite(w).all())
        assert_bits(g, w)
    y = got[0]
    _zero(twin.critic_1, twin.critic_2)
    twin.critic_loss(buffer, draw, y).backward()
    by_draw = [p.grad.clone() for p in _params(twin.critic_1) + _params(twin.critic_2)]
    _zero(twin.critic_1, twin.critic_2)
    twin.critic_loss(buffer, draw.indices, y).backward()
    for g, p in zip(by_draw, _params(twin.critic_1) + _params(twin.critic_2)):
        assert float(g.abs().max()) > 0
        assert_bits(g, p.grad)


# ---------------------------------------------------------------- the learners' front ends
def test_td3_actor_loss_with_a_streamed_head_through_a_streamed_twin():
    from finenvs_amd.lstm_head import FusedLSTMHead
    from tests.test_lstm_grad_gpu import _compare
    from tests.test_lstm_grad_gpu import _torch_grads as head_torch_grads
    from tests.test_lstm_grad_streamed_gpu import _module

    H, W, B = 256, 4, 257
    env, buffer = _ring(W)
    idx = torch.randint(0, buffer.size(), (B,), device="cuda")
    from finenvs_amd.lstm_head import td3_actor_loss

    states = buffer.get_mini_batch(B, indices=idx)["states"]
    head = FusedLSTMHead(env, _module(H, W, 20, "tanh", states), streamed=True)
    with torch.no_grad():
        actions = head.module(states.float())
    from finenvs_amd.critic import FusedTwinCritic

    twin = FusedTwinCritic(env, _scaled(H, W, 10, states, actions), _scaled(H, W, 11, states, actions), streamed=True)
    _zero(head.module, twin.critic_1, twin.critic_2)
    loss = td3_actor_loss(head, buffer, idx, twin)
    loss.backward()
    g = [p.grad.clone() for p in head.module.parameters()]
    assert all(p.grad is None for p in twin.critic_2.parameters())
    l32, g32, _ = head_torch_grads("td3", head.module, twin.critic_1, states.float(), None, torch.float32)
    l64, g64, _ = head_torch_grads("td3", head.module, twin.critic_1, states.double(), None, torch.float64)
    err, tol = abs(float(loss.detach()) - float(l64)), 2e-5 * abs(float(l64)) + 4 * abs(float(l32) - float(l64))
    print(f"td3 actor loss {float(loss.detach()):.8f} f64 {float(l64):.8f} err {err:.3e} tol {tol:.3e}")
    assert err <= tol, (err, tol)
    from finenvs_amd.lstm_head import head_parameters

    _compare("td3 streamed twin", [p.grad for p in head_parameters(head.module)], g32, g64)
    assert len(g) == 6


def test_sac_actor_losses_through_a_streamed_twin():
    from finenvs_amd.sac import FusedSACRollout
    from tests.test_critic_gpu import _actor

    H, W, B = 256, 4, 100
    env, buffer = _ring(W)
    idx = torch.randint(0, buffer.size(), (B,), device="cuda")
    twin, b = _twin_on(env, buffer, idx, H, W, (80, 81))
    actor = _actor(32, W, 82)
    roll = FusedSACRollout(env, actor)
    eps = torch.randn((B, 1), device="cuda")
    _zero(actor, twin.critic_1, twin.critic_2)
    actor_loss, alpha_loss = roll.actor_losses(buffer, idx, twin, eps)
    actor_loss.backward()
    alpha_loss.backward()
    # the torch chain on the rendered states (f32): the same loss within the SAC head's own bound on log-probabilities
    states = b["states"].float()
    a, lp = actor.get_actions_and_log_probs(states, eps)
    with torch.no_grad():
        alpha = actor.log_alpha.exp()
    want = (alpha * lp.mean(dim=1, keepdim=True) - torch.min(twin.critic_1(states, a), twin.critic_2(states, a))).mean()
    assert np.isfinite(float(actor_loss)) and abs(float(actor_loss) - float(want)) <= 1e-3 * max(1.0, abs(float(want)))
    grads = [p.grad for n, p in actor.named_parameters() if n != "log_alpha"]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads) and any(float(g.abs().max()) > 0 for g in grads)


# ---------------------------------------------------------------- the optimizer and the captured update
def _optim_setup(env, H, W, states, actions, lr=3e-3, rho=0.05):
    from finenvs_amd.critic import FusedTwinCritic
    from finenvs_amd.optim import FusedAdam

    c1, c2 = _scaled(H, W, 10, states, actions), _scaled(H, W, 11, states, actions)
    t1, t2 = copy.deepcopy(c1), copy.deepcopy(c2)
    with torch.no_grad():
        for t in (t1, t2):
            for p in t.parameters():
                p.mul_(0.9)
    opt = FusedAdam(lr=lr)
    opt.add(c1, target=t1, rho=rho)
    opt.add(c2, target=t2, rho=rho)
    return opt, (c1, c2, t1, t2), FusedTwinCritic(env, c1, c2, weights=opt, streamed=True), \
        FusedTwinCritic(env, t1, t2, weights=opt, streamed=True)


def test_one_fused_adam_step_equals_the_reference_update_and_the_packers():
    from finenvs_amd.critic import pack_critic_weights
    from finenvs_amd.optim import initial_state, reference_update
    from tests.test_optim_gpu import _cpu, _same_bits

    H, W, B = 256, 4, 64
    env, buffer = _ring(W, N=64, K=5)
    idx = torch.randint(0, buffer.size(), (B,), device="cuda")
    b = buffer.get_mini_batch(B, indices=idx)
    opt, nets, twin, twin_t = _optim_setup(env, H, W, b["states"], b["actions"])
    for module in nets:  # the resident buffers are the packers' before any step
        for k, v in pack_critic_weights(module).items():
            assert _same_bits(opt.packed(module)[k], v), k
    y = torch.randn((B, 1), device="cuda") - 1.0
    params, targets = opt.parameters(), opt.targets()
    ref_p, ref_t = _cpu(params), _cpu(targets)
    ref_m, ref_v = [torch.zeros_like(p) for p in ref_p], [torch.zeros_like(p) for p in ref_p]
    opt.zero_grad()
    twin.critic_loss(buffer, idx, y).backward()
    grads = _cpu([p.grad for p in params])
    assert all(float(g.abs().max()) > 0 for g in grads)
    opt.step()
    reference_update(ref_p, grads, ref_m, ref_v, initial_state(), 3e-3, targets=ref_t, rho=opt.rhos())
    for i, p in enumerate(params):
        assert _same_bits(p, ref_p[i]), (i, "param")
        assert _same_bits(targets[i], ref_t[i]), (i, "target")
    for module in nets:
        want, got = pack_critic_weights(module), opt.packed(module)
        assert set(want) == set(got)
        for k in want:
            assert tuple(got[k].shape) == tuple(want[k].shape) and _same_bits(got[k], want[k]), k
    # the resident front ends read what the step wrote: a fresh front end without the optimizer gives the same bits
    from finenvs_amd.critic import FusedTwinCritic

    slots = buffer.physical(idx)
    src, pos, act = buffer.state_src[slots], buffer.state_pos[slots].reshape(B), buffer.actions[slots].reshape(B, 1)
    for resident, (m1, m2) in ((twin, nets[:2]), (twin_t, nets[2:])):
        fresh = FusedTwinCritic(env, m1, m2, streamed=True)
        for got, want in zip(resident.forward(src, pos, act), fresh.forward(src, pos, act)):
            assert_bits(got, want)
    # a step between a forward and its backward is an error
    loss = twin.critic_loss(buffer, idx, y)
    opt.step()  # (the gradients are the zeros the first step left)
    with pytest.raises(RuntimeError):
        loss.backward()


def test_a_captured_td3_critic_update_equals_the_eager_one():
    from finenvs_amd.graphed import GraphedUpdate
    from finenvs_amd.lstm_head import LSTMHead
    from finenvs_amd.replay import ReplayBuffer
    from finenvs_amd.rollout import FusedLSTMRollout

    H, W, N, K, B = 256, 4, 64, 4, 64

    def arm(graphed):
        env = _env(N, W)
        _, _, traj = _descriptors(env, N * (K + 1))
        buffer = ReplayBuffer(env, max_size=N * K, cursor=True, seed=19)
        buffer.extend(traj)
        b = buffer.get_mini_batch(B, indices=torch.arange(B, device="cuda"))
        opt, nets, twin, twin_t = _optim_setup(env, H, W, b["states"], b["actions"])
        torch.manual_seed(90)
        actor = LSTMHead(32, W, "tanh").cuda()
        target = FusedLSTMRollout.from_modules(env, actor.lstm, actor.last_layer[0], output_activation="tanh")
        draw = buffer.new_draw(B)
        gen = torch.Generator(device="cuda").manual_seed(6)
        eps = torch.empty((B, 1), device="cuda")

        def refill():
            eps.copy_(torch.randn((B, 1), generator=gen, device="cuda"))

        def fn():
            buffer.draw(B, out=draw)
            y = twin_t.td3_targets(buffer, draw, target, eps, GAMMA, 0.2, 0.5, 0.5)
            loss = twin.critic_loss(buffer, draw, y)
            opt.zero_grad()
            loss.backward()
            opt.step()
            return loss.detach()

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
        state = {f"{i}.{n}": p.detach().clone() for i, m in enumerate(nets) for n, p in m.named_parameters()}
        for i, x in enumerate(losses):
            state[f"loss{i}"] = x
        state["cursor"] = buffer.cursor.clone()
        return state

    eager, graphed = arm(False), arm(True)
    assert list(eager) == list(graphed)
    assert [int(x) for x in eager["cursor"].cpu()][2] == 4 * B
    for k in eager:
        assert bool(torch.isfinite(eager[k].float()).all()), k
        assert_bits(eager[k], graphed[k])
    assert float((eager["loss0"] - eager["loss2"]).abs()) > 0


def test_the_td3_lstm_example_trains_at_hidden_256_without_rendering(monkeypatch):
    from finenvs_amd import TimeSeriesEnv
    from finenvs_amd.critic import CriticLSTM
    from finenvs_amd.replay import ReplayBuffer

    spec = importlib.util.spec_from_file_location("td3_lstm_fused", os.path.join(ROOT, "examples", "td3_lstm_fused.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    def refuse(self, *a, **k):
        raise AssertionError("an observation was rendered")

    monkeypatch.setattr(TimeSeriesEnv, "render", refuse)
    monkeypatch.setattr(ReplayBuffer, "get_mini_batch", refuse)
    for kw in (dict(), dict(fused_optim=True), dict(graph_update=True)):
        history, nets = mod.main(num_envs=64, hidden=256, window=4, iterations=3, batch=64, quiet=True, log_every=1, seed=7, **kw)
        assert [e["iteration"] for e in history] == [0, 1, 2], kw
        for e in history:
            assert np.isfinite(e["critic_loss"]), (kw, e)
            assert ("actor_loss" in e) == (e["iteration"] % 2 == 0) and np.isfinite(e.get("actor_loss", 0.0)), (kw, e)
        assert nets["critic_1"].lstm.hidden_size == 256 and nets["actor"].lstm.hidden_size == 256
        torch.manual_seed(7)
        for name in ("actor", "critic_1", "critic_2"):  # the parameters moved
            m = nets[name]
            assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
            assert not torch.equal(m.lstm.weight_hh_l0.detach().cpu(), nets["initial"][name]["lstm.weight_hh_l0"].cpu()), name
    assert isinstance(nets["critic_1"], CriticLSTM)


def test_refusals():
    import ctypes as C

    from finenvs_amd import _lib
    from finenvs_amd.critic import CriticLSTM, FusedTwinCritic
    from finenvs_amd.optim import FusedAdam

    env = _env(64, 4)
    with pytest.raises(ValueError, match="streamed=True"):
        FusedTwinCritic(env, CriticLSTM(256, 4).cuda(), CriticLSTM(256, 4).cuda())
    with pytest.raises(ValueError, match="same hidden size"):
        FusedTwinCritic(env, CriticLSTM(256, 4).cuda(), CriticLSTM(512, 4).cuda(), streamed=True)
    with pytest.raises(ValueError, match="2048"):
        FusedTwinCritic(env, CriticLSTM(2048, 4).cuda(), CriticLSTM(2048, 4).cuda(), streamed=True)
    env2 = _env(8, 4, A=2)
    with pytest.raises(ValueError, match="one asset"):
        FusedTwinCritic(env2, CriticLSTM(256, 4).cuda(), CriticLSTM(256, 4).cuda(), streamed=True)
    # the C ABI refuses the A = 2 env itself, after the null checks and before it touches any other pointer
    w, g = _lib.FeCriticWeights(16, 16, 16, 16), _lib.FeCriticGrads(*([16] * 6))
    lib = env2._lib
    assert lib.fe_twin_q_forward_streamed(env2._handle, 16, C.byref(w), C.byref(w), 256, 16, 16, 16, 4, 16, 16,
                                          None) == _lib.FE_ERR_ARG
    assert lib.fe_last_error().startswith(b"fe_twin_q_forward_streamed:") and b"2 assets" in lib.fe_last_error()
    assert lib.fe_twin_q_backward_streamed(env2._handle, 16, C.byref(w), C.byref(w), 256, 16, 16, 16, 4, 16, 16, 16,
                                           C.byref(g), C.byref(g), 16, None) == _lib.FE_ERR_ARG
    assert lib.fe_last_error().startswith(b"fe_twin_q_backward_streamed:") and b"2 assets" in lib.fe_last_error()
    # a critic the optimizer does not hold
    c1, c2 = CriticLSTM(256, 4).cuda(), CriticLSTM(256, 4).cuda()
    opt = FusedAdam(lr=1e-3)
    opt.add(c1)
    with pytest.raises(ValueError):
        FusedTwinCritic(env, c1, c2, weights=opt, streamed=True)
    # the small sizes run the register-resident way whether or not streamed is passed
    small = FusedTwinCritic(env, _critic(32, 4, 1), _critic(32, 4, 2), streamed=True)
    assert small.H == 32 and not small.streamed
