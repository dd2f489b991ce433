"""GPU: the SAC MLP actor with the folded head (include/finenvs_amd_mlp_sac.h, finenvs_amd/mlp_sac.py).

Shapes (H, W, B): (32, 4, 33) a ragged last 32-pair block; (64, 7, 513) an odd window and a crossed 512-pair split;
(128, 72, 33) the largest image; (128, 4, 4 097) several splits; (32, 4, 70 001) the grid-stride path.

* anchor, bit for bit: ``means`` equals ``fe_mlp_forward`` (output none) on ``(W1, b1, v_mu, c_mu)`` from ``.folded()``,
  the pre-softplus std row likewise on ``(v_s, c_s)``; ``sample()`` returns ``forward()``'s bits; ``forward`` on a
  trajectory's rows equals what ``run`` recorded; ``run(16)`` equals two ``run(8)``; two backward calls give the same bits;
* values: mu, std and tanh(u) against the f64 copy on rendered states within ``2e-5 max|x64| + 4 max|x32_torch - x64|``,
  log_probs within the same bound where ``|u| <= 4`` and finite everywhere;
* gradients: all eight tensors against the f64 copy within ``2e-5 max|g64| + 4 max|g32_torch - g64|`` per tensor, for the
  chained actor loss through ``FusedTwinMLPCritic.q``, ``(log_probs * c).sum()`` alone and ``actions.sum()`` alone (the
  batches and their conditions: tests/mlp_sac_cases.py, checked on the CPU by tests/test_mlp_sac_host.py);
* env parity with the oracle env, ``sac_targets`` against torch, behaviour (``.grad`` accumulates, a frozen actor launches
  nothing, B = 0, the window limit, the refusals that read the env, the example), and the memory contract.

Worst err / tol per case, as measured on an MI355X:
gradients, over the eight tensors (chained | log_probs | actions):
  (32, 4, 33) relu      0.031 | 0.011 | 0.036        (64, 7, 513) tanh     0.032 | 0.029 | 0.029
  (128, 72, 33) elu     0.035 | 0.017 | 0.026        (128, 4, 4 097) elu   0.014 | 0.012 | 0.132
  (32, 4, 70 001) relu  0.003 | 0.015 | 0.041
values, over mu, std, tanh(u) and log_probs (|u| <= 4): 0.006, 0.012, 0.010, 0.019, 0.015 in that order of shapes;
sac_targets at H = 64, B = 777: 0.014.

The entries have no output for the pre-softplus std.  Its anchor is bit for bit all the same: with ``std_layer.bias``
raised by 40 every q exceeds softplus's threshold of 20, where the kernels return q itself, so ``stds`` must equal
``fe_mlp_forward`` on ``(v_s, c_s)``, in the forward and in the rollout.  At the cases' own biases the row is also
compared with ``stds`` through torch's softplus, within 4e-7 of the largest value.
"""
import copy
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import mlp_sac_cases as cases
from tests import test_mlp_critic_gpu as tq
from tests import test_mlp_head_gpu as th
from tests.helpers import assert_bits as np_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64, I64 = torch.float32, torch.float64, torch.int64
assert_bits, _env, _zero = th.assert_bits, th._env, th._zero
_window, _bands_intact, SENTINEL = th._window, th._bands_intact, th.SENTINEL
NAMES, KINDS, SHAPES = cases.NAMES, cases.KINDS, cases.SHAPES
GAMMA = 0.97


def t2n(t):
    return t.detach().cpu().numpy()


def _params(actor):
    from finenvs_amd.mlp_sac import mlp_sac_parameters

    return list(mlp_sac_parameters(actor))


@pytest.fixture(scope="module")
def gpu_case():
    """The CPU case of a shape on the device, made once per shape: the env, the modules' copies, the descriptors, the
    rendered states and the fused objects."""
    made = {}

    def make(H, W, B, activation):
        from finenvs_amd.mlp_critic import FusedTwinMLPCritic
        from finenvs_amd.mlp_sac import FusedMLPSACRollout

        key = (H, W, B, activation)
        if key not in made:
            case = cases.conditioned(H, W, B, activation)
            env = _env(16, W)
            src, pos = case["src"].cuda(), case["pos"].cuda()
            env.check_descriptors(src)
            states = env.render(src, pos)
            assert float((states.cpu().double() - case["states"]).abs().max()) <= 1e-12  # the batch the CPU conditions saw
            actor = copy.deepcopy(case["actor"]).cuda()
            c1, c2 = (copy.deepcopy(c).cuda() for c in case["critics"])
            made[key] = dict(case=case, env=env, src=src, pos=pos.reshape(B), states=states, actor=actor, c1=c1, c2=c2,
                             eps=case["eps"].cuda(), c=case["c"].cuda(), roll=FusedMLPSACRollout(env, actor),
                             twin=FusedTwinMLPCritic(env, c1, c2))
        return made[key]

    return make


# --------------------------------------------------------------------------------------------------------------- anchor
def _head_row(env, roll, f, v, c, src, pos):
    """``fe_mlp_forward`` (output none) of the one-layer head ``(w1t, wpos, b1, v, c)`` on the descriptors: (B, 1)."""
    from finenvs_amd import _lib

    B = int(src.numel())
    w = _lib.FeMlpWeights(f["w1t"].data_ptr(), f["wpos"].data_ptr(), f["b1"].data_ptr(), v.data_ptr(), c.data_ptr())
    out = torch.empty((B, 1), dtype=F32, device="cuda")
    _lib.check(env._lib.fe_mlp_forward(env._handle, roll._lr32.data_ptr(), C.byref(w), roll.H, roll.act, 2, src.data_ptr(),
                                       pos.data_ptr(), B, out.data_ptr(), env._stream()), env._lib)
    return out


@pytest.mark.parametrize("H,W,B,activation", SHAPES)
def test_means_and_pre_softplus_stds_are_the_one_layer_heads_bits(gpu_case, H, W, B, activation):
    from finenvs_amd.mlp_sac import FusedMLPSACRollout, fold_head
    from finenvs_amd.trajectory import TrajectoryBuffer

    g = gpu_case(H, W, B, activation)
    env, roll, src, pos, eps = g["env"], g["roll"], g["src"], g["pos"], g["eps"]
    actions, log_probs, means, stds = roll.forward(src, pos, eps)
    f = roll.folded()
    assert_bits(means, _head_row(env, roll, f, f["v_mu"], f["c_mu"], src, pos), "means == fe_mlp_forward on (W1, b1, v_mu, c_mu)")
    q = _head_row(env, roll, f, f["v_s"], f["c_s"], src, pos)  # the pre-softplus std row
    dev_sp = torch.where(q > 20, q, torch.log1p(torch.exp(q)))
    assert float((stds - dev_sp).abs().max()) <= 4e-7 * float(dev_sp.abs().max())  # log1pf / expf against torch's
    # The pre-softplus std row, bit for bit: with std_layer.bias raised by 40 every q exceeds softplus's threshold of 20,
    # where the kernels return q itself -- so stds IS the (v_s, c_s) row, in the forward and in the rollout.
    hot = copy.deepcopy(g["actor"])
    with torch.no_grad():
        hot.std_layer.bias.add_(40.0)
    hot_roll = FusedMLPSACRollout(env, hot)
    _, _, hot_means, hot_stds = hot_roll.forward(src, pos, eps)
    hf = hot_roll.folded()
    hot_q = _head_row(env, hot_roll, hf, hf["v_s"], hf["c_s"], src, pos)
    assert float(hot_q.min()) > 20.0 and float(q.max()) < 20.0, (float(hot_q.min()), float(q.max()))
    assert_bits(hot_stds, hot_q, "forward: stds == fe_mlp_forward on (W1, b1, v_s, c_s) above the softplus threshold")
    assert_bits(hot_means, means, "the std bias does not reach the means")
    K, N = 3, env.num_envs
    traj = TrajectoryBuffer(K, N, 1, device=env._dev, states=True)
    gen = torch.Generator(device="cuda").manual_seed(B)
    hot_roll.run(K, noise=0.01 * torch.randn((K, N, 1), generator=gen, device="cuda"), record_means=True, record_stds=True,
                 trajectory=traj)
    hf = hot_roll.folded()
    for k in range(K):
        ksrc, kpos = traj.obs_src[k].contiguous(), traj.obs_pos[k].reshape(N).contiguous()
        row = _head_row(env, hot_roll, hf, hf["v_s"], hf["c_s"], ksrc, kpos)
        assert float(row.min()) > 20.0
        assert_bits(hot_roll.stds[k], row, f"rollout step {k}: stds == the (v_s, c_s) row")
        assert_bits(hot_roll.means[k], _head_row(env, hot_roll, hf, hf["v_mu"], hf["c_mu"], ksrc, kpos), f"rollout step {k}: means")
    # the pack kernel's fold against its host mirror: both sum in f64 and round once (the orders differ: <= 1 ulp)
    host = fold_head(g["actor"])
    for k in ("v_mu", "v_s", "c_mu", "c_s"):
        a, b = f[k].reshape(-1), host[k].reshape(-1)
        assert float((a - b).abs().max()) <= 1.2e-7 * float(b.abs().max()), k
    # without noise: the same means and stds, no actions
    a0, l0, m0, s0 = roll.forward(src, pos)
    assert a0 is None and l0 is None
    assert_bits(m0, means, "means without noise")
    assert_bits(s0, stds, "stds without noise")
    # sample() returns forward()'s bits
    sa, sl = roll.sample(src, pos, eps)
    assert_bits(sa, actions, "sample actions")
    assert_bits(sl, log_probs, "sample log_probs")
    assert_bits(roll.last["means"], means, "sample means")
    assert_bits(roll.last["stds"], stds, "sample stds")


def _twins(N, A, W, H, activation="elu", evaluate=False):
    from finenvs_amd.mlp_sac import FusedMLPSACRollout

    out = []
    for _ in range(2):
        env = _env(N, W, A=A, evaluate=evaluate)
        out.append((env, FusedMLPSACRollout(env, _rollout_actor(H, W, 5, activation))))
    return out


def _rollout_actor(H, W, seed, activation="elu"):
    """An actor whose means and stds spread over a trading range (tests/test_sac_rollout_gpu.py::_actor)."""
    a = cases.actor(H, W, seed, activation)
    with torch.no_grad():
        a.mu_layer.weight.mul_(8.0)
        a.std_layer.weight.mul_(4.0)
    return a


@pytest.mark.parametrize("H,A,activation", [(32, 3, "relu"), (64, 1, "tanh"), (128, 3, "elu")])
def test_forward_on_trajectory_rows_and_chunking_equal_run_bit_for_bit(H, A, activation):
    from finenvs_amd.trajectory import TrajectoryBuffer

    N, W = 203, 4
    (env1, r1), (env2, r2) = _twins(N, A, W, H, activation)
    g = torch.Generator(device="cuda").manual_seed(H)
    noise = torch.randn((16, N, A), generator=g, device="cuda")
    traj = TrajectoryBuffer(16, N, A, states=True)
    acts, rews, dones = r1.run(16, noise=noise, trajectory=traj, record_means=True, record_stds=True)
    a_a, r_a, d_a = r2.run(8, noise=noise[:8].clone())
    a_b, r_b, d_b = r2.run(8, noise=noise[8:].clone())
    assert_bits(acts, torch.cat([a_a, a_b]), "run(8); run(8) actions")
    assert_bits(rews, torch.cat([r_a, r_b]), "rewards")
    assert_bits(dones, torch.cat([d_a, d_b]), "dones")
    assert_bits(env1.cash, env2.cash, "cash")
    src, pos = traj.obs_src[:16].reshape(-1), traj.obs_pos[:16].reshape(-1, A)
    f_act, f_lp, f_mu, f_sd = r1.forward(src, pos, noise=noise.reshape(-1, A))
    f_act, f_mu, f_sd = f_act.reshape(16, N, A), f_mu.reshape(16, N, A), f_sd.reshape(16, N, A)
    assert_bits(f_mu, r1.means, "forward means == run means")
    assert_bits(f_sd, r1.stds, "forward stds == run stds")
    assert_bits(f_act[:, :-1], acts[:, :-1], "forward actions == run actions")
    assert_bits(acts[:, -1], r1.means[:, -1], "the eval env acts on the mean")
    assert bool(torch.isfinite(f_lp).all()) and float(f_sd.min()) > 0
    # without noise every env acts on the mean
    acts0, _, _ = r1.run(4, record_means=True)
    assert_bits(acts0, r1.means, "deterministic form")


# --------------------------------------------------------------------------------------------------------------- values
def _bound(got, x32, x64, what, keep=None):
    if keep is not None:
        got, x32, x64 = got[keep], x32[keep], x64[keep]
    err = float((got.double() - x64).abs().max())
    tol = 2e-5 * float(x64.abs().max()) + 4 * float((x32.double() - x64).abs().max())
    print(f"{what}: err {err:.3e} tol {tol:.3e} ratio {err / tol:.3f}")
    assert err <= tol, (what, err, tol)


@pytest.mark.parametrize("H,W,B,activation", SHAPES)
def test_values_against_the_f64_copy_within_the_yardstick(gpu_case, H, W, B, activation):
    g = gpu_case(H, W, B, activation)
    actions, log_probs, means, stds = g["roll"].forward(g["src"], g["pos"], g["eps"])
    ref = {}
    for dtype in (F32, F64):
        a = copy.deepcopy(g["actor"]).to(dtype)
        with torch.no_grad():
            s, e = g["states"].to(dtype), g["eps"].to(dtype)
            dist = a.get_distribution(s)
            act, lp = a.get_actions_and_log_probs(s, e)
            ref[dtype] = (dist.loc, dist.scale, act, lp, dist.loc + e * dist.scale)
    tag = f"values ({H}, {W}, {B})"
    _bound(means, ref[F32][0], ref[F64][0], f"{tag} mu")
    _bound(stds, ref[F32][1], ref[F64][1], f"{tag} std")
    _bound(actions, ref[F32][2], ref[F64][2], f"{tag} tanh(u)")
    inner = ref[F64][4].abs() <= 4
    assert bool(inner.any())
    _bound(log_probs, ref[F32][3], ref[F64][3], f"{tag} log_probs", inner)
    assert bool(torch.isfinite(log_probs).all())
    assert float(ref[F64][0].std()) > 1e-3 and float(ref[F64][1].std()) > 1e-4, "the head must depend on the observation"


# ------------------------------------------------------------------------------------------------------------ gradients
def _fused_grads(kind, g, keep):
    roll, twin, src, pos = g["roll"], g["twin"], g["src"], g["pos"]
    _zero(g["actor"], g["c1"], g["c2"])
    actions, log_probs = roll.sample(src, pos, g["eps"])
    value = cases.loss(kind, actions, log_probs, lambda x: twin.q(src, pos, x), g["actor"].log_alpha.detach().exp(), g["c"], keep)
    value.backward()
    return value.detach(), [p.grad.clone() for p in _params(g["actor"])]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,W,B,activation", SHAPES)
def test_gradients_against_f64_torch(gpu_case, H, W, B, activation, kind, monkeypatch):
    g = gpu_case(H, W, B, activation)
    env, case = g["env"], g["case"]
    keep = case["keep"][kind].cuda()
    seen = []
    real = env._lib.fe_mlp_sac_backward
    monkeypatch.setattr(env._lib, "fe_mlp_sac_backward", lambda *a: seen.append(a) or real(*a))
    value, got = _fused_grads(kind, g, keep)
    assert len(seen) == 1  # it launched, with the upstream gradients this loss has (arguments 11 and 12)
    assert (seen[0][11] is not None) == (kind != "log_probs") and (seen[0][12] is not None) == (kind != "actions")
    v32, g32 = cases.torch_grads(kind, g["actor"], g["c1"], g["c2"], g["states"].float(), g["eps"], g["c"], keep, F32)
    v64, g64 = case["g64"][kind]
    worst = 0.0
    for name, gf, gt, gd in zip(NAMES, got, g32, g64):
        gd = gd.cuda()
        assert gf.shape == gd.shape and gf.dtype is F32, name
        err = float((gf.double() - gd).abs().max())
        tol = 2e-5 * float(gd.abs().max()) + 4 * float((gt.double() - gd).abs().max())
        worst = max(worst, err / tol)
        print(f"({H}, {W}, {B}) {kind:9s} {name:6s} err {err:.3e} tol {tol:.3e} ratio {err / tol:.3f}")
        assert err <= tol, (kind, name, err, tol)
    print(f"({H}, {W}, {B}) {kind:9s} worst err / tol {worst:.3f}")
    assert abs(float(value) - float(v64)) <= 2e-5 * abs(float(v64)) + 4 * abs(float(v32) - float(v64)) + 1e-7


def test_backward_is_deterministic_grad_accumulates_and_reference_backward_agrees(gpu_case):
    from finenvs_amd.mlp_sac import reference_backward

    for shape in (SHAPES[1], SHAPES[3]):
        g = gpu_case(*shape)
        B = shape[2]
        roll, src, pos, eps, actor = g["roll"], g["src"], g["pos"], g["eps"], g["actor"]
        gen = torch.Generator(device="cuda").manual_seed(B)
        up = torch.randn((2, B, 1), generator=gen, device="cuda")

        def grads(zero=True):
            if zero:
                _zero(actor)
            a, lp = roll.sample(src, pos, eps)
            ((a * up[0]).sum() + (lp * up[1]).sum()).backward()
            return [p.grad.clone() for p in _params(actor)]

        g1, g2 = grads(), grads()
        for x, y in zip(g1, g2):
            assert_bits(x, y, "two backward calls")
            assert bool(torch.isfinite(x).all()) and float(x.abs().max()) > 0
        g3 = grads(zero=False)  # .grad accumulates
        for x, y in zip(g3, g1):
            assert_bits(x, y + y, "accumulated")
        # the host mirror of the rank-two algebra on the rendered states, in f32 and f64: the yardstick again
        r32 = reference_backward(actor, g["states"].float(), eps, up[0], up[1])
        r64 = reference_backward(copy.deepcopy(actor).double(), g["states"].double(), eps.double(), up[0].double(), up[1].double())
        for name, x, y32, y64 in zip(NAMES, g1, r32, r64):
            err = float((x.double() - y64).abs().max())
            assert err <= 2e-5 * float(y64.abs().max()) + 4 * float((y32.double() - y64).abs().max()), name


def test_a_frozen_actor_launches_nothing_and_an_empty_batch_works(gpu_case, monkeypatch):
    g = gpu_case(*SHAPES[0])
    env, roll, src, pos, eps, actor = g["env"], g["roll"], g["src"], g["pos"], g["eps"], g["actor"]
    seen = []
    real_b, real_f = env._lib.fe_mlp_sac_backward, env._lib.fe_mlp_sac_forward
    monkeypatch.setattr(env._lib, "fe_mlp_sac_backward", lambda *a: seen.append("backward") or real_b(*a))
    monkeypatch.setattr(env._lib, "fe_mlp_sac_forward", lambda *a: seen.append("forward") or real_f(*a))
    actor.requires_grad_(False)
    try:
        a, lp = roll.sample(src, pos, eps)
        assert not a.requires_grad and not lp.requires_grad and seen == ["forward"]
    finally:
        actor.requires_grad_(True)
    # one frozen tensor gets nothing, the others their gradients
    _zero(actor)
    actor.network[2].weight.requires_grad_(False)
    try:
        a, lp = roll.sample(src, pos, eps)
        (a.sum() + lp.sum()).backward()
        assert actor.network[2].weight.grad is None and all(p.grad is not None for p in _params(actor) if p.requires_grad)
    finally:
        actor.network[2].weight.requires_grad_(True)
    # B = 0
    _zero(actor)
    seen.clear()
    a, lp = roll.sample(src[:0], pos[:0], eps[:0])
    assert a.shape == (0, 1) and lp.shape == (0, 1)
    (a.sum() + lp.sum()).backward()
    assert seen == []
    for p in _params(actor):
        assert p.grad is not None and float(p.grad.abs().max()) == 0.0
    assert env._lib.fe_mlp_sac_forward(env._handle, roll._lr32.data_ptr(), C.byref(roll._weights()), 32, roll.act, 16, 16, 0,
                                       None, None, None, 16, 16, None) == 0  # count = 0 does nothing


# ----------------------------------------------------------------------------------------------------------- env parity
@pytest.mark.parametrize("N,A,H,activation,evaluate", [(33, 1, 32, "elu", False), (200, 3, 64, "relu", False),
                                                       (200, 1, 128, "tanh", True), (33, 3, 32, "elu", True)])
def test_run_equals_the_oracle_env_bit_for_bit(N, A, H, activation, evaluate):
    import finenvs_amd as fe
    from finenvs_amd.mlp_sac import FusedMLPSACRollout
    from finenvs_amd.trajectory import TrajectoryBuffer
    from oracle import fe_oracle as fo
    from tests import test_sac_rollout_gpu as tsr

    fo.build()
    W, K = 4, 8
    ref, env = tsr._make(fe, fo, N, A, W, 5, 40, 0.05, evaluate, seed=3 * N + H)
    roll = FusedMLPSACRollout(env, _rollout_actor(H, W, H + A, activation))
    obs = ref.reset().copy()
    gen = torch.Generator(device="cuda").manual_seed(N)
    noise = torch.randn((K, N, A), generator=gen, device="cuda")
    traj = TrajectoryBuffer(K, N, A, states=True)
    acts, rews, dones = roll.run(K, noise=noise, trajectory=traj, record_means=True)
    seen = set()
    for k in range(K):
        np_bits(t2n(traj.states(env, k)), obs, f"step {k} trajectory state")
        if not evaluate:
            assert_bits(acts[k, -1], roll.means[k, -1], "the evaluation env acts on mu")
        assert float(acts[k, :-1].abs().max()) <= 1.0
        a_k = t2n(acts[k])
        seen.update(np.unique(np.clip(np.rint(a_k * 5.5), -5, 5)).tolist())
        obs, r_ref, d_ref, _ = ref.step(a_k)
        obs = obs.copy()
        np_bits(t2n(rews[k]), r_ref, f"step {k} rewards")
        np_bits(t2n(dones[k]), d_ref, f"step {k} dones")
    np_bits(t2n(traj.states(env, K)), obs, "last trajectory state")
    np_bits(t2n(roll.observation()), obs, "observation()")
    np_bits(t2n(env.cash), ref.cash, "cash")
    np_bits(t2n(env.margin), ref.margin, "margin")
    np_bits(t2n(env.env_indices), ref.env_idx, "env_idx")
    assert len(seen) >= 4, f"the policy must trade in both directions (share changes seen: {sorted(seen)})"


# -------------------------------------------------------------------------------------------------------------- targets
def _filled(env, roll, K, seed=1, cursor=False, max_size=None):
    from finenvs_amd.replay import ReplayBuffer
    from finenvs_amd.trajectory import TrajectoryBuffer

    N = env.num_envs
    buffer = ReplayBuffer(env, max_size=max_size or K * N + 7, cursor=cursor, seed=seed)
    gen = torch.Generator(device=env._dev).manual_seed(seed)

    def store(steps=K):
        traj = TrajectoryBuffer(steps, N, 1, device=env._dev, states=True)
        roll.run(steps, noise=torch.randn((steps, N, 1), generator=gen, device=env._dev), trajectory=traj)
        buffer.extend(traj)

    store()
    return buffer, store


def test_sac_targets_against_torch_on_rendered_next_states():
    from finenvs_amd.critic import FusedTwinCritic, CriticLSTM, torch_sac_targets
    from finenvs_amd.mlp_critic import FusedTwinMLPCritic
    from finenvs_amd.mlp_sac import FusedMLPSACRollout
    from finenvs_amd.sac import FusedSACRollout, SACActorLSTM

    H, W, B = 64, 4, 777
    env = _env(190, W)
    actor = cases.actor(H, W, 52)
    roll = FusedMLPSACRollout(env, actor)
    buffer, store = _filled(env, roll, 2, max_size=3 * 190 - 50)
    store(1)  # wrapped: head != 0
    assert buffer.head != 0 and buffer.size() == buffer.max_size
    with torch.no_grad():
        buffer.dones[1::5] = 1.0
    c1, c2 = tq._critic(H, W, 50), tq._critic(H, W, 51)
    twin = FusedTwinMLPCritic(env, c1, c2)
    idx = torch.randint(0, buffer.size(), (B,), device="cuda")
    eps = torch.randn((B, 1), device="cuda")
    y = twin.sac_targets(buffer, idx, roll, eps, GAMMA, actor.log_alpha, 0.5)
    b = buffer.get_mini_batch(B, indices=idx)
    ys = []
    for dtype in (F32, F64):
        a, d1, d2 = (copy.deepcopy(m).to(dtype) for m in (actor, c1, c2))
        ys.append(torch_sac_targets(a, d1, d2, b["rewards"].to(dtype), b["next_states"].to(dtype), b["dones"].to(dtype),
                                    eps.to(dtype), GAMMA, 0.5).double())
    err = float((y.double() - ys[1]).abs().max())
    tol = 2e-5 * float(ys[1].abs().max()) + 4 * float((ys[0] - ys[1]).abs().max())
    print(f"sac_targets H = {H}, B = {B}: err {err:.3e} tol {tol:.3e} ratio {err / tol:.3f}")
    assert err <= tol, (err, tol)
    last = twin.last
    alpha = actor.log_alpha.detach().exp().float().reshape(1)
    expr = b["rewards"] * 0.5 + GAMMA * (1 - b["dones"]) * (torch.minimum(last["q1"], last["q2"]) + (-alpha) * last["log_probs"])
    assert_bits(y, expr, "SAC epilogue")
    done = b["dones"].reshape(-1) == 1
    assert bool(done.any()) and torch.equal(y[done], (b["rewards"] * 0.5)[done])
    # an out-of-range index: NaN, counted
    size = buffer.size()
    bad_idx = torch.tensor([0, -1, 5, size, size + 40, size - 1, -1000], device="cuda")
    bad = torch.tensor([False, True, False, True, True, False, True], device="cuda")
    before = int(buffer.errors.item())
    yb = twin.sac_targets(buffer, bad_idx, roll, eps[:7], GAMMA, actor.log_alpha)
    assert int(buffer.errors.item()) - before == 4
    assert bool(torch.isnan(yb[bad]).all()) and bool(torch.isfinite(yb[~bad]).all())
    good = twin.sac_targets(buffer, bad_idx[~bad], roll, eps[:7][~bad], GAMMA, actor.log_alpha)
    assert_bits(yb[~bad], good, "valid rows do not depend on the invalid ones")
    # the families do not mix; the LSTM family's own message stays
    lstm_roll = FusedSACRollout(env, SACActorLSTM(32, W).cuda())
    lstm_twin = FusedTwinCritic(env, CriticLSTM(32, W).cuda(), CriticLSTM(32, W).cuda())
    with pytest.raises(ValueError, match="FusedMLPSACRollout of this env"):
        twin.sac_targets(buffer, idx, lstm_roll, eps, GAMMA, actor.log_alpha)
    with pytest.raises(ValueError, match="actor_roll must be a FusedSACRollout \\(the SAC actor's head\\)"):
        lstm_twin.sac_targets(buffer, idx, roll, eps, GAMMA, actor.log_alpha)
    with pytest.raises(ValueError, match="FusedMLPSACRollout of this env"):
        twin.sac_targets(buffer, idx, FusedMLPSACRollout(_env(8, W), actor), eps, GAMMA, actor.log_alpha)
    with pytest.raises(ValueError, match="twin must be a FusedTwinMLPCritic"):
        roll.actor_losses(buffer, idx, lstm_twin, eps)


def test_a_replay_draw_gives_the_bits_of_its_indices_as_a_tensor():
    from finenvs_amd.mlp_critic import FusedTwinMLPCritic
    from finenvs_amd.mlp_sac import FusedMLPSACRollout, torch_sac_mlp_actor_losses

    H, W, B = 32, 4, 97
    env = _env(64, W)
    actor = cases.actor(H, W, 72)
    roll = FusedMLPSACRollout(env, actor)
    buffer, store = _filled(env, roll, 2, cursor=True, max_size=150)
    store(1)  # wrapped
    c1, c2 = tq._critic(H, W, 70), tq._critic(H, W, 71)
    twin = FusedTwinMLPCritic(env, c1, c2)
    draw = buffer.draw(B)
    eps = torch.randn((B, 1), device="cuda")
    got = [twin.sac_targets(buffer, draw, roll, eps, GAMMA, actor.log_alpha).clone(), twin.last["q1"].clone(),
           twin.last["log_probs"].clone()]
    want = [twin.sac_targets(buffer, draw.indices, roll, eps, GAMMA, actor.log_alpha), twin.last["q1"], twin.last["log_probs"]]
    for a, b, name in zip(got, want, ("targets", "q1", "log_probs")):
        assert bool(torch.isfinite(a).all())
        assert_bits(a, b, name)
    results = []
    for indices in (draw, draw.indices):
        _zero(actor, c1, c2)
        actor.log_alpha.grad = None
        actor_loss, alpha_loss = roll.actor_losses(buffer, indices, twin, eps)
        actor_loss.backward()
        results.append([actor_loss.detach().clone(), alpha_loss.detach().clone()] + [p.grad.clone() for p in _params(actor)])
    for a, b in zip(*results):
        assert_bits(a, b, "actor_losses")
    # the losses' values against torch on the rendered mini-batch
    slots = buffer.physical(draw.indices)
    states = env.render(buffer.state_src[slots], buffer.state_pos[slots])
    ref = {}
    for dtype in (F32, F64):
        a, d1, d2 = (copy.deepcopy(m).to(dtype) for m in (actor, c1, c2))
        ref[dtype] = [float(x.detach()) for x in torch_sac_mlp_actor_losses(a, d1, d2, states.to(dtype), eps.to(dtype))]
    for k in range(2):
        assert abs(float(results[0][k]) - ref[F64][k]) <= 2e-5 * abs(ref[F64][k]) + 4 * abs(ref[F32][k] - ref[F64][k]) + 1e-7


# ------------------------------------------------------------------------------------------------------ memory contract
@pytest.mark.parametrize("H,W,B", [(32, 4, 1), (64, 7, 33), (128, 16, 1057)])
def test_memory_contract_of_forward_rollout_and_backward(H, W, B):
    from finenvs_amd import _lib
    from finenvs_amd.mlp_sac import FusedMLPSACRollout, mlp_sac_grad_shapes

    env = _env(16 if B < 64 else 264, W)
    src, pos, _ = th._descriptors(env, B)
    pos = pos.reshape(B).contiguous()
    roll = FusedMLPSACRollout(env, cases.actor(H, W, 13, "relu"))
    lib = env._lib
    w = roll._weights()
    packed = roll._packed  # the buffers w points to, kept while the raw calls below use them
    # the pack: five outputs of exactly H * 4W, H, H, H and 2 floats, equal to what the front end packed
    x = packed
    pouts = {k: _window(n, F32, float("nan")) for k, n in (("w1t", H * 4 * W), ("wpos", H), ("vmu", H), ("vstd", H), ("cfold", 2))}
    _lib.check(lib.fe_mlp_sac_pack(x["_w1"].data_ptr(), x["w2"].data_ptr(), x["b2"].data_ptr(), x["wmu"].data_ptr(),
                                   x["bmu"].data_ptr(), x["wstd"].data_ptr(), x["bstd"].data_ptr(), H, W,
                                   *(pouts[k][1].data_ptr() for k in ("w1t", "wpos", "vmu", "vstd", "cfold")), env._stream()), lib)
    for k, (big, win) in pouts.items():
        _bands_intact(big, win.numel(), f"pack {k}")
        assert_bits(win, x[k].reshape(-1), f"pack {k}")
    gen = torch.Generator(device="cuda").manual_seed(B)
    eps = torch.randn((B,), generator=gen, device="cuda")
    outs = {k: _window(B, F32, float("nan")) for k in ("actions", "log_probs", "means", "stds")}  # exactly B floats each
    _lib.check(lib.fe_mlp_sac_forward(env._handle, roll._lr32.data_ptr(), C.byref(w), H, roll.act, src.data_ptr(),
                                      pos.data_ptr(), B, eps.data_ptr(), outs["actions"][1].data_ptr(),
                                      outs["log_probs"][1].data_ptr(), outs["means"][1].data_ptr(), outs["stds"][1].data_ptr(),
                                      env._stream()), lib)
    want = dict(zip(("actions", "log_probs", "means", "stds"), roll.forward(src, pos, eps.reshape(B, 1))))
    for k, (big, win) in outs.items():
        _bands_intact(big, B, k)
        assert_bits(win.reshape(B, 1), want[k], k)
    # the rollout: every output of exactly its documented size
    N, K = env.num_envs, 3
    routs = {k: _window(K * N, F32, float("nan")) for k in ("actions", "means", "stds")}
    rew, done = _window(K * N, F64, float("nan")), _window(K * N, torch.int32, -7)
    tsrc, tpos = _window((K + 1) * N, I64, -7), _window((K + 1) * N, F64, float("nan"))
    noise = torch.randn((K, N, 1), generator=gen, device="cuda")
    roll._begin_run()
    _lib.check(lib.fe_env_rollout_mlp_sac(env._handle, roll._lr32.data_ptr(), C.byref(w), H, roll.act, K, roll.obs_src.data_ptr(),
                                          roll.obs_pos.data_ptr(), noise.data_ptr(), routs["actions"][1].data_ptr(),
                                          routs["means"][1].data_ptr(), routs["stds"][1].data_ptr(), rew[1].data_ptr(),
                                          done[1].data_ptr(), tsrc[1].data_ptr(), tpos[1].data_ptr(), env._stream()), lib)
    roll._end_run()
    for k, (big, win) in routs.items():
        _bands_intact(big, K * N, k)
        assert bool(torch.isfinite(win).all()), k
    for big, n, name in ((rew[0], K * N, "rewards"), (done[0], K * N, "dones"), (tsrc[0], (K + 1) * N, "states_src"),
                         (tpos[0], (K + 1) * N, "states_pos")):
        _bands_intact(big, n, name)
    assert bool(torch.isfinite(rew[1]).all()) and bool((done[1] >= 0).all()) and bool((tsrc[1] >= 0).all())
    # the backward: the workspace of exactly the exported size, eight gradients of exactly torch's sizes
    a, s = want["actions"].reshape(B).contiguous(), want["stds"].reshape(B).contiguous()
    up = torch.randn((2, B), generator=gen, device="cuda")
    n_ws = int(lib.fe_mlp_sac_grad_workspace_floats(H, W, B))
    sizes = {k: int(np.prod(shape)) for k, shape in zip(NAMES, mlp_sac_grad_shapes(H, W))}
    results = []
    for poison in (float("nan"), SENTINEL):
        big_ws, ws = _window(n_ws, F32, poison)
        wins = {k: _window(n, F32, poison) for k, n in sizes.items()}
        sg = _lib.FeMlpSacGrads(*(wins[k][1].data_ptr() for k in NAMES))
        _lib.check(lib.fe_mlp_sac_backward(env._handle, roll._lr32.data_ptr(), C.byref(w), H, roll.act, src.data_ptr(),
                                           pos.data_ptr(), B, eps.data_ptr(), a.data_ptr(), s.data_ptr(), up[0].data_ptr(),
                                           up[1].data_ptr(), ws.data_ptr(), C.byref(sg), env._stream()), lib)
        _bands_intact(big_ws, n_ws, "workspace")
        for k, n in sizes.items():
            _bands_intact(wins[k][0], n, k)
            assert bool(torch.isfinite(wins[k][1]).all()), k
        results.append([wins[k][1].clone() for k in NAMES])
    for x, y in zip(*results):
        assert_bits(x, y, "a NaN-filled workspace against a sentinel-filled one")
    _zero(roll.actor)
    sa, sl = roll.sample(src, pos, eps.reshape(B, 1))
    ((sa.reshape(B) * up[0]).sum() + (sl.reshape(B) * up[1]).sum()).backward()
    for x, p in zip(results[0], _params(roll.actor)):
        assert_bits(x, p.grad.reshape(-1), "against the front end")
    del packed  # (kept until here: w points into its buffers)


# -------------------------------------------------------------------------------------------------- limits and refusals
def test_the_window_limit_and_the_refusals_that_read_the_env():
    from finenvs_amd import _lib
    from finenvs_amd.mlp_sac import FusedMLPSACRollout, SACActorMLP

    W = _lib.MLP_SAC_MAX_WINDOW[128]
    assert W == cases.WMAX == 72
    env = _env(8, W + 1)
    with pytest.raises(ValueError, match="does not fit"):
        FusedMLPSACRollout(env, cases.actor(128, W + 1, 1))
    lib, w, g = env._lib, _lib.FeMlpSacWeights(*([16] * 12)), _lib.FeMlpSacGrads(*([16] * 8))
    rc = lib.fe_mlp_sac_forward(env._handle, 16, C.byref(w), 128, 0, 16, 16, 4, None, None, None, 16, 16, None)
    assert rc == _lib.FE_ERR_ARG
    msg = lib.fe_last_error()
    assert b"fe_mlp_sac_forward: W1 (128 x 292)" in msg and b"does not fit" in msg, msg
    rc = lib.fe_mlp_sac_backward(env._handle, 16, C.byref(w), 128, 0, 16, 16, 4, 16, 16, 16, 16, 16, 16, C.byref(g), None)
    assert rc == _lib.FE_ERR_ARG and b"fe_mlp_sac_backward: W1 (128 x 292)" in lib.fe_last_error()
    rc = lib.fe_env_rollout_mlp_sac(env._handle, 16, C.byref(w), 128, 0, 2, 16, 16, None, None, None, None, 16, 16, None, None, None)
    assert rc == _lib.FE_ERR_ARG and b"fe_env_rollout_mlp_sac: W1 (128 x 292)" in lib.fe_last_error()
    roll = FusedMLPSACRollout(env, cases.actor(64, W + 1, 1))  # H = 64 fits
    a, lp = roll.sample(roll.obs_src, roll.obs_pos, torch.randn((8, 1), device="cuda"))
    (a.sum() + lp.sum()).backward()
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(roll.actor.network[0].weight.grad).all())
    # A != 1: the rollout and the forward run, the gradient is refused
    env2 = _env(8, 4, A=2)
    roll2 = FusedMLPSACRollout(env2, cases.actor(32, 4, 1))
    acts, _, _ = roll2.run(2, noise=torch.randn((2, 8, 2), device="cuda"))
    assert bool(torch.isfinite(acts).all())
    with pytest.raises(ValueError, match="one asset"):
        roll2.sample(roll2.obs_src, roll2.obs_pos, torch.randn((8, 1), device="cuda"))
    rc = lib.fe_mlp_sac_backward(env2._handle, 16, C.byref(w), 32, 0, 16, 16, 4, 16, 16, 16, 16, 16, 16, C.byref(g), None)
    assert rc == _lib.FE_ERR_ARG and b"fe_mlp_sac_backward: the env has 2 assets" in lib.fe_last_error()
    # the Python refusals
    env = _env(8, 4)
    with pytest.raises(ValueError, match="in_features must be 20"):
        FusedMLPSACRollout(env, cases.actor(32, 7, 2))
    with pytest.raises(ValueError, match="must live on the env's device"):
        FusedMLPSACRollout(env, SACActorMLP(32, 4))
    with pytest.raises(ValueError, match="float32 parameters"):
        FusedMLPSACRollout(env, cases.actor(32, 4, 1).double())
    roll = FusedMLPSACRollout(env, cases.actor(32, 4, 1))
    with pytest.raises(ValueError, match="noise must be a"):
        roll.run(2, noise=torch.randn((2, 8), device="cuda"))
    with pytest.raises(ValueError, match="sample needs noise"):
        roll.sample(roll.obs_src, roll.obs_pos, None)
    # an optimizer step is seen by the next call: the parameters are re-packed per call
    _, _, m0, _ = roll.forward(roll.obs_src, roll.obs_pos)
    with torch.no_grad():
        roll.actor.mu_layer.bias.add_(0.25)
    _, _, m1, _ = roll.forward(roll.obs_src, roll.obs_pos)
    assert float((m1 - m0 - 0.25).abs().max()) < 1e-6


# -------------------------------------------------------------------------------------------------------------- example
def test_sac_mlp_example_trains_on_descriptors_only(monkeypatch):
    from finenvs_amd import TimeSeriesEnv
    from finenvs_amd.replay import ReplayBuffer

    spec = importlib.util.spec_from_file_location("sac_mlp_fused", os.path.join(ROOT, "examples", "sac_mlp_fused.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    def refuse(self, *a, **k):
        raise AssertionError("an observation was rendered")

    monkeypatch.setattr(TimeSeriesEnv, "render", refuse)
    monkeypatch.setattr(ReplayBuffer, "get_mini_batch", refuse)
    history, nets = mod.main(num_envs=256, window=4, hidden=32, iterations=6, batch=128, quiet=True)
    assert len(history) == 6
    for e in history:
        assert all(np.isfinite(e[k]) for k in ("critic_loss", "actor_loss", "alpha_loss", "alpha"))
    for name in ("actor", "critic_1", "critic_2", "critic_1t", "critic_2t"):
        for key, p in nets[name].state_dict().items():
            assert bool(torch.isfinite(p).all()), (name, key)
            assert not torch.equal(p, nets["initial"][name][key]), (name, key)  # every tensor moved
