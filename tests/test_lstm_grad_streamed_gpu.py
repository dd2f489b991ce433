"""GPU: the one-output LSTM head's backward pass at H = 256 / 512 / 1024 (fe_lstm_backward_streamed,
``FusedLSTMHead(env, module, streamed=True)``), with the helpers and the yardstick of tests/test_lstm_grad_gpu.py.

* gradients of the six parameters (and of PPO's ``log_std``) against an f64 torch copy of the module on the rendered
  states, within ``2e-5 max|g64| + 4 max|g_torch32 - g64|``: a plain ``y.sum()`` on a tanh and on a none head and the
  PPO critic loss in every case, the PPO actor loss and the TD3 actor loss chained through ``FusedTwinCritic.q`` at
  B >= 257 (``_ppo_inputs`` caps the clipped share below 50 %: at B = 31 13 of 31 samples were clipped, at B = 257
  8 - 27 %).  The output layer is scaled so that ``0.5 < max|p| < 4``: unscaled, max|p| is 0.006 - 0.03 at these sizes
  and the tanh head's ``1 - y^2`` factor would never be exercised.  The last case crosses a chunk boundary with a
  ragged tail;
* the same at the windows and K splits those cases do not reach.  Worst err / tol over kinds and tensors, measured on an
  MI355X: W = 1 (256, 1, 33) 0.046 (d w_hh identically and exactly zero); odd W (512, 7, 257) 0.192; the reference's
  default window (256, 390, 33) 0.178 and (1024, 390, 33) 0.082, the latter with the 256-pair minimum chunk; empty
  trailing K splits (1024, 4, 1100) 0.829 (``ppo_critic`` b_out, a cancelling sum of the upstream gradient; every other
  kind below 0.12) and (512, 4, 4200) 0.230;
* values: after an in-place perturbation of all six parameters ``head(src, pos)`` is a fresh
  ``FusedLSTMRollout.from_modules(...).forward(src, pos)`` bit for bit (``refresh()`` packs fragment-major);
* two backward calls give the same bits; ``.grad`` accumulates as torch's does; a frozen head gets nothing and launches
  nothing; B = 0 works; ``td3_actor_loss`` on a wrapped replay ring; the PPO example at ``hidden=256`` with
  ``fused_update=True`` trains without rendering anything; refusals.
"""
import copy
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests.test_lstm_grad_gpu import (_check_against_f64, _compare, _critic, _descriptors, _env, _fused_grads, _params,
                                      _torch_grads, _zero, assert_bits)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _chunk(H, W):
    from finenvs_amd import _lib

    return int(_lib.load().fe_lstm_streamed_grad_chunk_pairs(H, W))


def _module(H, W, seed, activation, states):
    """LSTMHead with the input weights scaled up so that log-returns of ~1e-3 move the gates (as
    tests/test_lstm_grad_gpu.py::_module), then the output weights scaled so that max|w_out . h_W| (f64, bias excluded)
    is 1.5 on the test's own rendered batch ``states``."""
    from finenvs_amd.lstm_head import LSTMHead

    torch.manual_seed(seed)
    m = LSTMHead(H, W, activation)
    with torch.no_grad():
        m.lstm.weight_ih_l0[:, :4].mul_(6.0 * np.sqrt(H))
    m = m.cuda()
    with torch.no_grad():
        m64 = copy.deepcopy(m).double()
        h_w = m64.lstm(states.double())[0][:, -1, :]
        m.last_layer[0].weight.mul_(1.5 / float((h_w @ m64.last_layer[0].weight.t()).abs().max()))
        pmax = float(copy.deepcopy(m).double().last_layer[0](h_w).abs().max())
    assert 0.5 < pmax < 4.0, pmax
    return m


# The last two cases leave trailing K splits of the weight contraction without a chain; they must write zeros for the
# final kernel to add.  From the rule of include/finenvs_amd_lstm_grad_streamed.h and the kernel's constants: the pass
# holds B rounded up to 32 pairs, one MFMA chain covers 1024 (step, pair) columns, there are at most 4 / 16 / 32 splits at
# H = 1024 / 512 / 256, and every split takes ceil(chains / splits) consecutive chains.
#   (1024, 4, 1100): 1120 pairs x 4 steps = 4480 columns = 5 chains, 4 splits of 2: chains 0-1, 2-3, 4, none;
#   (512, 4, 4200): 4224 x 4 = 16 896 columns = 17 chains, 16 splits of 2: nine splits hold chains, seven hold none.
CASES = [
    (256, 4, 1, torch.float64),
    (256, 4, 31, torch.float32),
    (512, 4, 33, torch.float64),
    (1024, 16, 33, torch.float32),
    (256, 5, 257, torch.float64),
    (512, 16, 257, torch.float32),
    (1024, 5, 257, torch.float64),
    (1024, 4, 4097, torch.float64),
    (256, 4, "chunk + 33", torch.float32),
    (256, 1, 33, torch.float64),     # W = 1: no recurrent step at all
    (512, 7, 257, torch.float32),    # odd W
    (256, 390, 33, torch.float64),   # the reference's default window
    (1024, 390, 33, torch.float32),  # the chunk is the 256-pair minimum (a full one's stash, 2.5 GB, exceeds 2 GiB)
    (1024, 4, 1100, torch.float64),  # an empty trailing K split, see above
    (512, 4, 4200, torch.float32),   # seven empty trailing K splits
]


@pytest.mark.parametrize("H,W,B,obs_dtype", CASES)
def test_gradients_against_f64_torch(H, W, B, obs_dtype):
    from finenvs_amd.critic import FusedTwinCritic
    from finenvs_amd.lstm_head import FusedLSTMHead

    if B == "chunk + 33":  # two passes: a full chunk, then a ragged 33-pair tail
        B = _chunk(H, W) + 33
    env = _env(min(B, 4096), W, obs_dtype=obs_dtype)
    src, pos, _ = _descriptors(env, B)
    assert src.numel() == B
    states = env.render(src, pos)
    actor = FusedLSTMHead(env, _module(H, W, 20, "tanh", states), streamed=True)
    value = FusedLSTMHead(env, _module(H, W, 21, "none", states), streamed=True)
    _check_against_f64("sum", actor, None, env, src, pos)
    _check_against_f64("sum", value, None, env, src, pos)
    _check_against_f64("ppo_critic", value, None, env, src, pos)
    if B >= 257:
        twin = FusedTwinCritic(env, _critic(32, W, 10), _critic(32, W, 11))
        _check_against_f64("ppo_actor", actor, None, env, src, pos)
        _check_against_f64("td3", actor, twin, env, src, pos)


@pytest.mark.parametrize("H,W,activation", [(256, 4, "tanh"), (512, 5, "none"), (1024, 4, "tanh"), (1024, 16, "none")])
def test_values_equal_a_fresh_rollout_bit_for_bit_after_an_update(H, W, activation):
    from finenvs_amd.lstm_head import FusedLSTMHead
    from finenvs_amd.rollout import FusedLSTMRollout

    env = _env(300, W)
    src, pos, _ = _descriptors(env, 333)
    module = _module(H, W, 20, activation, env.render(src, pos))
    head = FusedLSTMHead(env, module, streamed=True)
    gen = torch.Generator(device="cuda").manual_seed(5)
    with torch.no_grad():  # what an optimizer step does: every parameter moves in place
        for p in _params(module):
            p.mul_(1.0 + 0.05 * torch.randn(p.shape, generator=gen, device="cuda"))
    y = head(src, pos)
    assert tuple(y.shape) == (333, 1) and y.dtype is torch.float32 and y.requires_grad
    fresh = FusedLSTMRollout.from_modules(env, module.lstm, module.last_layer[0], output_activation=activation)
    expected = fresh.forward(src, pos)
    assert float(expected.abs().max()) > 0
    assert_bits(y, expected)
    assert_bits(head.rollout.forward(src, pos), expected)
    assert_bits(head.rollout.whh, fresh.whh)  # fragment-major on both sides


@pytest.mark.parametrize("H,W,B", [(256, 4, "chunk + 33"), (1024, 4, 300)])
def test_backward_is_deterministic(H, W, B):
    from finenvs_amd.lstm_head import FusedLSTMHead

    if B == "chunk + 33":
        B = _chunk(H, W) + 33
    env = _env(min(B, 4096), W)
    src, pos, _ = _descriptors(env, B)
    module = _module(H, W, 20, "tanh", env.render(src[:4096], pos[:4096]))
    head = FusedLSTMHead(env, module, streamed=True)
    c = torch.randn((B, 1), device="cuda")
    runs = []
    for _ in range(2):
        _zero(module)
        (head(src, pos) * c).sum().backward()
        runs.append([p.grad.clone() for p in _params(module)])
    for x, z in zip(*runs):
        assert float(x.abs().max()) > 0
        assert_bits(x, z)


def test_accumulation_a_frozen_head_and_an_empty_batch(monkeypatch):
    from finenvs_amd.lstm_head import FusedLSTMHead

    H, W, B = 256, 4, 300
    env = _env(B, W)
    src, pos, _ = _descriptors(env, B)
    head = FusedLSTMHead(env, _module(H, W, 20, "tanh", env.render(src, pos)), streamed=True)
    c = torch.randn((B, 1), device="cuda")
    _, once = _fused_grads("sum", head, None, src, pos, None)
    assert all(float(g.abs().max()) > 0 for g in once)
    _zero(head.module)
    for _ in range(2):  # no zero_grad in between
        head(src, pos).sum().backward()
    for p, g in zip(_params(head.module), once):
        torch.testing.assert_close(p.grad, 2 * g, rtol=1e-6, atol=0)
    # a frozen head: no graph, no .grad, no launch of the backward
    calls = []
    real = env._lib.fe_lstm_backward_streamed
    monkeypatch.setattr(env._lib, "fe_lstm_backward_streamed", lambda *a: calls.append(1) or real(*a), raising=False)
    head.module.requires_grad_(False)
    _zero(head.module)
    y = head(src, pos)
    assert not y.requires_grad
    probe = c.clone().requires_grad_(True)
    (y * probe).sum().backward()
    assert all(p.grad is None for p in head.module.parameters()) and not calls and probe.grad is not None
    # one frozen parameter: the others get theirs, bit for bit what they got before
    head.module.requires_grad_(True)
    head.module.lstm.weight_hh_l0.requires_grad_(False)
    _zero(head.module)
    head(src, pos).sum().backward()
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


def test_td3_actor_loss_on_a_wrapped_ring_against_f64():
    from finenvs_amd.critic import FusedTwinCritic
    from finenvs_amd.lstm_head import FusedLSTMHead, td3_actor_loss
    from finenvs_amd.replay import ReplayBuffer

    H, W, N, K, B = 256, 4, 200, 6, 777
    env = _env(N, W)
    _, _, traj = _descriptors(env, N * (K + 1))
    buffer = ReplayBuffer(env, max_size=N * K // 2 + 37)
    buffer.extend(traj)
    assert buffer.size() == buffer.max_size and buffer.head != 0  # wrapped
    idx = torch.randint(0, buffer.size(), (B,), device="cuda")
    states = buffer.get_mini_batch(B, indices=idx)["states"]
    head = FusedLSTMHead(env, _module(H, W, 20, "tanh", states), streamed=True)
    twin = FusedTwinCritic(env, _critic(32, W, 10), _critic(32, W, 11))
    _zero(head.module, twin.critic_1, twin.critic_2)
    loss = td3_actor_loss(head, buffer, idx, twin)
    loss.backward()
    g = [p.grad.clone() for p in _params(head.module)]
    l32, g32, _ = _torch_grads("td3", head.module, twin.critic_1, states.float(), None, torch.float32)
    l64, g64, pmax = _torch_grads("td3", head.module, twin.critic_1, states.double(), None, torch.float64)
    assert 0.5 < pmax < 4.0
    _compare("td3 ring", g, g32, g64)
    err, tol = abs(float(loss.detach()) - float(l64)), 2e-5 * abs(float(l64)) + 4 * abs(float(l32) - float(l64))
    print(f"td3 actor loss {float(loss.detach()):.8f} f64 {float(l64):.8f} err {err:.3e} tol {tol:.3e}")
    assert err <= tol, (err, tol)


def test_ppo_example_at_hidden_256_with_fused_update_trains_without_rendering(monkeypatch):
    from finenvs_amd import TimeSeriesEnv, lstm_head
    from finenvs_amd.rollout import FusedLSTMRollout
    from finenvs_amd.trajectory import TrajectoryBuffer

    spec = importlib.util.spec_from_file_location("ppo_lstm_fused", os.path.join(ROOT, "examples", "ppo_lstm_fused.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    heads = []

    class Recording(lstm_head.FusedLSTMHead):
        def __init__(self, env, module, **kwargs):
            assert kwargs == {"streamed": True}
            super().__init__(env, module, **kwargs)
            heads.append(self)

    def refuse(self, *a, **k):
        raise AssertionError("an observation was rendered")

    monkeypatch.setattr(mod, "FusedLSTMHead", Recording)
    monkeypatch.setattr(TrajectoryBuffer, "minibatch_states", refuse)
    monkeypatch.setattr(TimeSeriesEnv, "render", refuse)
    history = mod.main(envs=256, steps=4, iters=1, hidden=256, window=4, quiet=True, fused_update=True)
    assert len(history) == 1 and len(heads) == 2
    for critic_loss, mean_reward, log in history:
        assert np.isfinite(critic_loss) and np.isfinite(mean_reward)
    for head, activation in zip(heads, ("tanh", "none")):
        assert head.H == 256 and head.output_activation == activation
        src, pos = head.rollout.obs_src.clone(), head.rollout.obs_pos.clone()
        acted = head.rollout.forward(src, pos).clone()  # what the kernel runs after the example's last update
        assert bool(torch.isfinite(acted).all())
        m = head.module
        fresh = FusedLSTMRollout.from_modules(head.env, m.lstm, m.last_layer[0], output_activation=activation)
        assert_bits(fresh.forward(src, pos), acted)
        untrained = lstm_head.LSTMHead(256, 4, activation)
        assert not torch.equal(m.lstm.weight_hh_l0.cpu(), untrained.lstm.weight_hh_l0)


def test_refusals():
    import ctypes as C

    from finenvs_amd import _lib
    from finenvs_amd.lstm_head import FusedLSTMHead, LSTMHead

    env2 = _env(8, 4, A=2)
    with pytest.raises(ValueError, match="one asset"):
        FusedLSTMHead(env2, LSTMHead(256, 4).cuda(), streamed=True)
    # the C ABI refuses the A = 2 env itself, after the null checks and before it touches any other pointer
    grads = _lib.FeLstmGrads(*([16] * 6))
    rc = env2._lib.fe_lstm_backward_streamed(env2._handle, 16, 16, 16, 16, 256, 0, 16, 16, 8, 16, 16, 16, C.byref(grads),
                                             None)
    assert rc == _lib.FE_ERR_ARG
    msg = env2._lib.fe_last_error()
    assert msg.startswith(b"fe_lstm_backward_streamed:") and b"2 assets" in msg, msg
    env = _env(64, 4)
    with pytest.raises(ValueError, match="2048"):
        FusedLSTMHead(env, LSTMHead(2048, 4).cuda(), streamed=True)
    with pytest.raises(ValueError, match="streamed=True"):  # the refusal of the default path says how to opt in
        FusedLSTMHead(env, LSTMHead(256, 4).cuda())
    with pytest.raises(ValueError, match="float32"):
        FusedLSTMHead(env, LSTMHead(256, 4).cuda().double(), streamed=True)
    with pytest.raises(ValueError, match="device"):
        FusedLSTMHead(env, LSTMHead(256, 4), streamed=True)
