"""GPU: the ES population with two hidden layers (csrc/fe_evo_kernels.h, ``fe_evo2_rollout``,
``finenvs_amd.evo.FusedPopulationMLP2Rollout``).

* lock-step parity with the oracle env (no action noise): member weights rebuilt from ``pop.noise``; the device's actions
  within ``ACTION_TOL`` of an f64 forward of the same f32 member weights (``_forward2`` of tests/test_evo2_host.py, the
  function pinned against the reference's ParallelMLP there); fed to ``OracleEnv`` they give the device's rewards, dones,
  cash, margin, env indices, spots, running returns, step counters and episode slots bit for bit.  Shapes: 100 pairs with a
  ragged last tile; three assets (the exchange buffer reused per asset); H = 128 (theta above 64 KiB at W = 8); W = 1 and 3 at
  every H (5W rows fewer than, or not dividing among, the row groups); A = 17 and 100 (PB = 7 and 1: the waves of a tile
  run different numbers of units); per H the largest window ``fe_evo2_lds_bytes`` admits, and the one above it refused;
* eval members equal the unperturbed forward, swapping the signs or dropping the perturbation changes the actions;
* ``run(32); run(32)`` equals ``run(64)`` bit for bit with action noise on; ``record=False`` equals ``record=True``;
* the action noise against the host mirror of the stream; generation 1; the memory contract of ``fe_evo2_rollout`` through
  the C ABI; the gradient at the new P, one ``train()``, the example; the refusals.

``ACTION_TOL``.  The reference value is the f64 forward; two summation orders of up to 640 + 128 f32 terms legitimately
differ by a few ulps per layer.  Measured on an MI355X over every lock-step case below (worst |action - y64| of the kernel,
and of the plain f32 torch forward, per H):
    H = 32:  device 5.08e-06, torch f32 4.97e-06  (both at the largest window, W = 246)    -> 4 x 5.08e-06 -> 3e-5
    H = 64:  device 2.89e-06, torch f32 3.51e-06  (both at the largest window, W = 112)    -> 4 x 3.51e-06 -> 2e-5
    H = 128: device 5.22e-06 (W = 8, 85 steps), torch f32 5.24e-06 (W = 1)                 -> 4 x 5.24e-06 -> 3e-5
Per H the bound is 4 times the larger of the two, rounded up to one digit; it stays below 1e-4, where it would no longer
separate a wrong element (sigma = 0.5 moves an action by more than 1e-2) from rounding.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from tests.helpers import assert_bits, evo_action_noise_reference
from tests.test_evo2_host import _forward2
from tests.test_evo_rollout_gpu import _make, _member_weights, t2n
from tests.test_memory_contract_gpu import (F32, F64, I32, I64, NAN, SENTINEL, _floats, _index, _same_bits, _two_poisons,
                                             _Window, _written)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTION_TOL = {32: 3e-5, 64: 2e-5, 128: 3e-5}  # per H: see the module docstring
Z_BOUND = 1e-4  # tests/test_evo_shapes_gpu.py: the host mirror's bound on one normal
MAX_LDS = 160 * 1024
SEED = 0x9E3779B97F4A7C15
CHUNKS = (1, 5, 7, 32, 40)
_worst = {}  # H -> [device, torch f32]: printed by every lock-step case


@pytest.fixture(scope="module")
def fe():
    import finenvs_amd

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return finenvs_amd


@pytest.fixture(scope="module")
def fo():
    from oracle import fe_oracle

    fe_oracle.build()
    return fe_oracle


def _population(*args, **kwargs):
    from finenvs_amd.evo import FusedPopulationMLP2Rollout

    return FusedPopulationMLP2Rollout(*args, **kwargs)


def _layers2(W, H, seed):
    """ParallelMLP-shaped layers (three weights, three biases) scaled so that the hidden units and the actions spread over
    (-1, 1) on these observations."""
    g = torch.Generator().manual_seed(seed)
    W1 = torch.randn((5 * W, H), generator=g) * (12.0 / W ** 0.5)
    W1[4::5, :] = torch.randn((W, H), generator=g) * (3.0 / W)
    b1 = torch.randn((1, H), generator=g) * 0.3
    W2 = torch.randn((H, H), generator=g) * (1.5 / H ** 0.5)
    b2 = torch.randn((1, H), generator=g) * 0.3
    W3 = torch.randn((H, 1), generator=g) * (2.0 / H ** 0.5)
    b3 = torch.full((1, 1), 0.03)
    return [W1, W2, W3], [b1, b2, b3]


def _fwd(pop, w, obs):
    return _forward2(w, torch.as_tensor(obs, device=w.device), pop.env.num_intervals, pop.H)


def _stagger(env, ref, bars):
    """Env n starts at the row of its day from which 1 + 7 n mod min(bars, 12) steps are left, on the device env and on the
    oracle alike, so that short runs finish episodes at different steps in different envs."""
    N, W = env.num_envs, env.num_intervals
    left = 1 + (7 * np.arange(N)) % min(bars, 12)
    first = bars - left
    env.env_spots = torch.as_tensor(first).unsqueeze(1) + torch.arange(W)
    if ref is not None:
        ref.spot0[:] = first
    return left


class _Lockstep:
    """The device population and the oracle env side by side, chunk by chunk, with the host's own bookkeeping."""

    def __init__(self, pop, ref, env):
        self.pop, self.ref, self.env = pop, ref, env
        N = env.num_envs
        self.obs = ref.reset().copy()
        assert_bits(t2n(pop.observation()), self.obs, "initial obs")
        self.ret = np.zeros(N, dtype=np.float32)
        self.ts = np.zeros(N, dtype=np.float32)
        self.slots = [[] for _ in range(N)]
        self.total = 0
        self.err_dev = self.err_t32 = self.spread = 0.0
        self.first_bad = None

    def clear(self):
        self.ret[:] = 0
        self.ts[:] = 0
        self.slots = [[] for _ in self.slots]
        self.total = 0

    def run(self, K, w, what):
        pop, ref, env, h = self.pop, self.ref, self.env, self.pop.num_pairs
        w64 = w.double()
        acts, rews, dones = pop.run(K, record=True)
        assert_bits(t2n(pop.means), t2n(acts), "means == actions without action noise")
        for k in range(K):
            a_dev = t2n(acts[k])
            x32 = torch.as_tensor(self.obs, device=w.device).float()  # the policy's input is the f32 observation
            y64 = t2n(_fwd(pop, w64, x32))
            self.err_t32 = max(self.err_t32, float(np.abs(t2n(_fwd(pop, w, x32)).astype(np.float64) - y64).max()))
            err = float(np.abs(a_dev.astype(np.float64) - y64).max())
            self.err_dev = max(self.err_dev, err)
            self.spread = max(self.spread, float(np.abs(a_dev[:h] - a_dev[h:2 * h]).max()))
            if err > ACTION_TOL[pop.H] and self.first_bad is None:
                self.first_bad = f"{what} step {k}: |action - y64| = {err:.3g}"
            obs, r_ref, d_ref, _ = ref.step(a_dev)
            self.obs = obs.copy()
            assert_bits(t2n(rews[k]), r_ref, f"{what} step {k} rewards")
            assert_bits(t2n(dones[k]), d_ref, f"{what} step {k} dones")
            self.ret = (self.ret.astype(np.float64) + r_ref).astype(np.float32)
            self.ts += 1
            for n in np.nonzero(d_ref)[0]:
                self.slots[n].append(self.ret[n])
                self.total += int(self.ts[n])
                self.ret[n] = 0.0
                self.ts[n] = 0.0
        assert_bits(t2n(env.cash), ref.cash, what + " cash")
        assert_bits(t2n(env.margin), ref.margin, what + " margin")
        assert_bits(t2n(env.env_indices), ref.env_idx, what + " env_idx")
        assert_bits(t2n(env.env_spots[:, 0]), ref.spot0, what + " spot0")
        assert_bits(t2n(pop.observation()), self.obs, what + " observation()")
        assert_bits(t2n(pop.returns), self.ret, what + " running returns")
        assert_bits(t2n(pop.timesteps), self.ts, what + " steps since the last done")
        assert pop.total_timesteps() == self.total, what + " steps of the finished episodes"
        ep, cnt = pop.episodes()
        assert t2n(cnt).tolist() == [len(s) for s in self.slots], what + " episode counts"
        table = np.zeros((len(self.slots), pop.max_episodes), dtype=np.float32)
        for n, s in enumerate(self.slots):
            table[n, :len(s)] = s
        assert_bits(t2n(ep), table, what + " episode slots")
        assert pop.num_finished() == sum(len(s) for s in self.slots) and not pop.overflowed()

    def report(self, label):
        """Print the figures, then hold the actions to the bound (the bit-exact checks above have passed)."""
        H = self.pop.H
        rec = _worst.setdefault(H, [0.0, 0.0])
        rec[0], rec[1] = max(rec[0], self.err_dev), max(rec[1], self.err_t32)
        print(f"{label}: worst |action - y64|: device {self.err_dev:.3g}, torch f32 {self.err_t32:.3g}; "
              f"so far at H = {H}: device {rec[0]:.3g}, torch f32 {rec[1]:.3g}")
        assert self.err_dev <= ACTION_TOL[H], self.first_bad
        assert self.spread > 1e-2, "the perturbation must spread each pair's actions"


def _case(fe, fo, N, A, W, H, num_eval, days, bars, stagger):
    ref, env = _make(fe, fo, N, A, W, days, bars, seed=N + A)
    left = _stagger(env, ref, bars) if stagger else None
    pop = _population(env, num_eval, H, 0.5, seed=4, action_noise_std=0.0, max_episodes=16)
    pop.set_parameters(*_layers2(W, H, seed=H + A))
    return _Lockstep(pop, ref, env), left


def _members(run, w):
    """Eval members act with theta itself; swapping the signs of the mirrored members changes the actions."""
    pop = run.pop
    N, h, n_train = pop.env.num_envs, pop.num_pairs, pop.num_training_envs
    obs_now = pop.observation()
    theta_only = _fwd(pop, pop.theta.unsqueeze(0).repeat(N, 1), obs_now)
    member = _fwd(pop, w, obs_now)
    assert torch.equal(member[n_train:], theta_only[n_train:])
    swapped = w.clone()
    swapped[:h], swapped[h:2 * h] = w[h:2 * h], w[:h]
    assert float((_fwd(pop, swapped, obs_now)[:n_train] - member[:n_train]).abs().max()) > 1e-2


# ---------------------------------------------------------------- lock-step parity
@pytest.mark.parametrize("N,A,H,num_eval", [
    (203, 1, 64, 3),    # 100 pairs: a ragged last pair tile
    (77, 3, 32, 5),     # three assets: the exchange buffer is reused per asset
    (131, 1, 128, 1),   # theta above 64 KiB at W = 8: the big-LDS launch
])
def test_lockstep_parity_with_the_oracle(fe, fo, N, A, H, num_eval):
    from finenvs_amd import _lib

    W = 8
    run, _ = _case(fe, fo, N, A, W, H, num_eval, 5, 40, stagger=False)
    pop = run.pop
    assert pop.num_params == 5 * W * H + H * H + 3 * H + 1
    if H == 128:
        assert _lib.load().fe_evo2_lds_bytes(W, A, H) > 64 * 1024
    w = _member_weights(pop)
    n_train = pop.num_training_envs
    assert torch.equal(w[n_train:], pop.theta.unsqueeze(0).repeat(num_eval, 1))
    for rep, K in enumerate(CHUNKS):
        run.run(K, w, f"chunk {rep}")
    assert pop.num_finished() > N
    _members(run, w)
    run.report(f"(N, A, W, H) = ({N}, {A}, {W}, {H})")


GEOMETRIES = [  # N, A, W, H, num_eval, days, bars
    (35, 1, 1, 32, 3, 4, 8),      # 5 rows for 8 row groups: three idle in the first layer
    (35, 1, 3, 32, 1, 4, 10),     # 15 rows for 8 row groups
    (35, 1, 1, 64, 3, 4, 8),      # 5 rows for 4 row groups: 5 % 4 = 1
    (35, 1, 3, 64, 1, 4, 10),     # 15 % 4 = 3
    (35, 1, 1, 128, 3, 4, 8),     # 5 rows for 2 row groups
    (35, 1, 3, 128, 1, 4, 10),    # 15 % 2 = 1
    (41, 17, 4, 64, 3, 4, 11),    # PB = 7: waves take 2, 2, 2, 1 units; the last pair tile holds 5 pairs
    (7, 100, 2, 128, 1, 4, 9),    # PB = 1: three wavefronts idle through the unit loop
]


@pytest.mark.parametrize("N,A,W,H,num_eval,days,bars", GEOMETRIES)
def test_lockstep_parity_at_ragged_rows_and_uneven_unit_counts(fe, fo, N, A, W, H, num_eval, days, bars):
    run, left = _case(fe, fo, N, A, W, H, num_eval, days, bars, stagger=True)
    w = _member_weights(run.pop)
    for rep, K in enumerate((1, 5, 7)):
        run.run(K, w, f"chunk {rep}")
    assert min(len(s) for s in run.slots) >= 1 and left.min() == 1 and run.total > N
    _members(run, w)
    run.report(f"(N, A, W, H) = ({N}, {A}, {W}, {H})")


@pytest.mark.parametrize("H", [32, 64, 128])
def test_the_largest_window_runs_and_the_next_is_refused(fe, fo, H):
    """The largest window at one asset, found from ``fe_evo2_lds_bytes`` (the rule, not a literal)."""
    from finenvs_amd import _lib
    from finenvs_amd.evo import FusedPopulationMLPRollout

    lib = _lib.load()
    W = 1
    while lib.fe_evo2_lds_bytes(W + 1, 1, H) <= MAX_LDS:
        W += 1
    assert 8 < W < 400 and lib.fe_evo2_lds_bytes(W, 1, H) <= MAX_LDS < lib.fe_evo2_lds_bytes(W + 1, 1, H)
    N, num_eval, days, bars = 23, 3, 3, W + 9
    run, left = _case(fe, fo, N, 1, W, H, num_eval, days, bars, stagger=True)
    w = _member_weights(run.pop)
    for rep, K in enumerate((1, 5, 7)):
        run.run(K, w, f"chunk {rep}")
    assert min(len(s) for s in run.slots) >= 1
    run.report(f"largest window at H = {H}: W = {W}, {lib.fe_evo2_lds_bytes(W, 1, H)} bytes of LDS")
    _, big = _make(fe, fo, N, 1, W + 1, days, bars, seed=N + 1, oracle=False)
    with pytest.raises(ValueError, match="does not fit the 160 KiB LDS"):
        _population(big, num_eval, H, 0.5, seed=4)
    # the C ABI's own refusal, with a one-layer population's struct at this width (no pointer is read before the refusal)
    one = FusedPopulationMLPRollout(big, num_eval, 32, 0.5, seed=4)
    one.run(1)
    one._pop.hidden = H
    rc = big._lib.fe_evo2_rollout(big._handle, C.byref(one._pop), 1, None, None, None, None, big._stream())
    assert rc == _lib.FE_ERR_ARG and b"fe_evo2_rollout: theta" in big._lib.fe_last_error()
    assert b"does not fit the 160 KiB LDS" in big._lib.fe_last_error()


# ---------------------------------------------------------------- bit exactness
@pytest.mark.parametrize("N,A,H,num_eval", [(131, 1, 128, 1), (77, 3, 32, 5), (203, 1, 64, 3)])
def test_chunking_is_bit_exact_with_action_noise(fe, fo, N, A, H, num_eval):
    W, nu = 8, 0.01
    runs = []
    for split in ((32, 32), (64,)):
        _, env = _make(fe, fo, N, A, W, 5, 40, seed=21, oracle=False)
        pop = _population(env, num_eval, H, 0.3, seed=8, action_noise_std=nu, max_episodes=8)
        pop.set_parameters(*_layers2(W, H, seed=1))
        outs = [pop.run(K, record=True) + (pop.means,) for K in split]
        acts, rews, dones, means = (torch.cat([o[i] for o in outs]) for i in range(4))
        runs.append((acts, rews, dones, means, pop, env))
    (a1, r1, d1, m1, p1, e1), (a2, r2, d2, m2, p2, e2) = runs
    for x, y, what in ((a1, a2, "actions"), (r1, r2, "rewards"), (d1, d2, "dones"), (m1, m2, "means"),
                       (p1.returns, p2.returns, "running returns"), (p1.timesteps, p2.timesteps, "timesteps"),
                       (p1.episode_returns, p2.episode_returns, "slots"), (p1.episode_counts, p2.episode_counts, "counts"),
                       (e1.cash, e2.cash, "cash"), (e1.margin, e2.margin, "margin"), (p1.counters, p2.counters, "counters"),
                       (p1.obs_src, p2.obs_src, "obs_src"), (p1.obs_pos, p2.obs_pos, "obs_pos")):
        assert_bits(t2n(x), t2n(y), what)
    n_train = p1.num_training_envs
    assert p1.num_finished() > 0 and p1.step == 64
    assert torch.equal(a1[:, n_train:], m1[:, n_train:]), "eval envs take no action noise"
    assert not torch.equal(a1[:, :n_train], m1[:, :n_train])


def test_run_without_record_equals_run_with_record(fe, fo):
    N, A, W, H, num_eval, nu, bars = 77, 3, 8, 32, 5, 0.01, 12
    sides = []
    for record in (True, False):
        _, env = _make(fe, fo, N, A, W, 4, bars, seed=40, oracle=False)
        _stagger(env, None, bars)
        pop = _population(env, num_eval, H, 0.3, seed=SEED, action_noise_std=nu, max_episodes=8)
        pop.set_parameters(*_layers2(W, H, seed=6))
        for K in (5, 9):
            out = pop.run(K, record=record)
            assert (out is not None) == record and (pop.means is not None) == record
        sides.append((env, pop))
    (e1, p1), (e2, p2) = sides
    assert p1.num_finished() > N and p1.total_timesteps() > 0 and float(p1.timesteps.max()) > 0
    for name in ("cash", "margin", "long_shares", "short_shares", "env_indices", "env_spots"):
        assert_bits(t2n(getattr(e1, name)), t2n(getattr(e2, name)), "env." + name)
    for name in ("returns", "timesteps", "episode_returns", "episode_counts", "counters", "obs_src", "obs_pos"):
        assert_bits(t2n(getattr(p1, name)), t2n(getattr(p2, name)), name)
    assert_bits(t2n(p1.observation()), t2n(p2.observation()), "observation()")


# ---------------------------------------------------------------- action noise
def test_action_noise_equals_the_host_mirror(fe, fo):
    """``actions - means`` of the training envs is ``nu xi(n, step, a)`` of the unchanged stream (five assets: all four words
    and the next counter domain); zero on the eval envs; the step counts across launches."""
    N, A, W, H, num_eval, nu = 41, 5, 4, 64, 3, 0.25
    _, env = _make(fe, fo, N, A, W, 4, 11, seed=35, oracle=False)
    pop = _population(env, num_eval, H, 0.3, seed=SEED, action_noise_std=nu, max_episodes=8)
    pop.set_parameters(*_layers2(W, H, seed=A))
    n_train = pop.num_training_envs
    chunks = (3, 4)
    outs = [(pop.run(K, record=True)[0], pop.means) for K in chunks]
    acts, means = (torch.cat([o[i] for o in outs]) for i in range(2))
    steps = sum(chunks)
    assert tuple(acts.shape) == (steps, N, A) and pop.step == steps
    assert_bits(t2n(acts[:, n_train:]), t2n(means[:, n_train:]), "eval envs take no action noise")
    a64, m64 = t2n(acts[:, :n_train]).astype(np.float64), t2n(means[:, :n_train]).astype(np.float64)
    noise = a64 - m64
    xi = evo_action_noise_reference(SEED, 0, np.arange(steps)[:, None, None], np.arange(n_train)[None, :, None],
                                    np.arange(A)[None, None, :])
    # the mirror's bound on xi, and the f32 rounding of means + nu xi (nu = 2^-2: the product is exact)
    tol = nu * Z_BOUND + 2.0 ** -22 * np.maximum(1.0, np.abs(a64))
    err = np.abs(noise - nu * xi)
    bad = np.argwhere(err > tol)
    assert bad.size == 0, f"{bad.shape[0]} of {err.size} elements off, first (step, env, asset) = {tuple(bad[0])}"
    assert float(np.abs(noise).max()) > nu


# ---------------------------------------------------------------- generation 1
def test_generation_1_runs_on_its_own_noise(fe, fo):
    run, _ = _case(fe, fo, 51, 1, 7, 64, 3, 4, 14, stagger=True)
    pop = run.pop
    w0 = _member_weights(pop)
    for rep, K in enumerate((5, 7)):
        run.run(K, w0, f"generation 0 chunk {rep}")
    assert pop.num_finished() > 0 and pop.total_timesteps() > 0 and float(pop.timesteps.max()) > 0
    pop.next_generation()
    assert pop.generation == 1 and pop.step == 0
    for name in ("returns", "timesteps", "episode_returns", "episode_counts", "counters"):
        assert not bool(getattr(pop, name).any()), f"{name} is not cleared"
    run.clear()
    w1 = _member_weights(pop)
    h = pop.num_pairs
    assert_bits(t2n(pop.noise(torch.arange(h), generation=1)), t2n(pop.noise(torch.arange(h))), "noise() renders generation 1")
    assert float((w1[:h] - w0[:h]).abs().max()) > 0.5  # sigma = 0.5: other draws, not a rounding difference
    assert torch.equal(w1[2 * h:], w0[2 * h:])
    run.run(7, w1, "generation 1")  # the oracle carries on
    assert pop.num_finished() > 0
    run.report("generation 1")


# ---------------------------------------------------------------- the memory contract of fe_evo2_rollout
STATE = ("obs_src", "obs_pos", "returns", "timesteps", "episode_returns", "episode_counts", "counters", "scratch_rewards",
         "scratch_dones")
OUTPUTS = ("actions", "means", "rewards", "dones")


def _contract_population(fe, fo):
    N, A, W, H, bars = 41, 3, 7, 64, 4
    _, env = _make(fe, fo, N, A, W, 4, bars, seed=50, oracle=False)
    _stagger(env, None, bars)
    pop = _population(env, 3, H, 0.3, seed=SEED, action_noise_std=0.01, max_episodes=4)
    pop.set_parameters(*_layers2(W, H, seed=9))
    return env, pop


def _banded(data):
    flat = data.detach().reshape(-1)
    return _Window(flat.numel(), flat.dtype, SENTINEL if flat.is_floating_point() else -9, flat)


def _state_windows(pop):
    N = pop.env.num_envs
    return {
        "obs_src": _index(pop.obs_src), "obs_pos": _banded(pop.obs_pos), "returns": _banded(pop.returns),
        "timesteps": _banded(pop.timesteps),
        "episode_returns": _banded(torch.full_like(pop.episode_returns, SENTINEL)),
        "episode_counts": _banded(pop.episode_counts), "counters": _banded(pop.counters),
        "scratch_rewards": _banded(torch.zeros((N,), dtype=F64, device="cuda")),
        "scratch_dones": _banded(torch.zeros((N,), dtype=I32, device="cuda")),
    }


def _abi_rollout(env, pop, K, state, ins, outs):
    """``fe_evo2_rollout`` with the struct ``run`` builds, its pointers replaced by the windows; an output missing from
    ``outs`` is passed as null."""
    from finenvs_amd import _lib

    s = _lib.FeEvoPopulation()
    s.num_train, s.hidden, s.max_episodes = pop.num_training_envs, pop.H, pop.max_episodes
    s.noise_std, s.action_noise_std, s.seed = pop.noise_std_dev, pop.action_noise_std, pop.seed & (2 ** 64 - 1)
    s.generation, s.step = pop.generation, pop.step
    s.logret_f32, s.theta = ins["logret_f32"].ptr, ins["theta"].ptr
    for name in STATE:
        setattr(s, name, state[name].ptr)
    ptr = lambda k: outs[k].ptr if k in outs else None  # noqa: E731
    pop._begin_run()
    _lib.check(env._lib.fe_evo2_rollout(env._handle, C.byref(s), K, ptr("actions"), ptr("means"), ptr("rewards"),
                                        ptr("dones"), env._stream()))
    pop._end_run()
    torch.cuda.synchronize()


def test_evo2_rollout_memory_contract(fe, fo):
    """Every pointer of ``fe_evo2_rollout`` is a window inside a larger allocation the test owns: NaN bands round the two
    inputs (theta's window is exactly P floats), sentinel bands round the four outputs and the nine state arrays."""
    K = 6
    env0, pop0 = _contract_population(fe, fo)
    N, A, M = env0.num_envs, env0.num_assets, pop0.max_episodes
    acts, rews, dones = pop0.run(K, record=True)
    want = {"actions": acts, "means": pop0.means, "rewards": rews, "dones": dones}
    counts = pop0.episode_counts.tolist()
    assert max(counts) == 2 and min(counts) == 1 and not pop0.overflowed()  # slots are filled to different depths
    assert not torch.equal(acts[:, :pop0.num_training_envs], pop0.means[:, :pop0.num_training_envs])
    ins = {"theta": _floats(pop0.theta), "logret_f32": _floats(pop0._lr32.reshape(-1))}
    assert ins["theta"].n == pop0.num_params
    sizes = {"actions": (K * N * A, F32), "means": (K * N * A, F32), "rewards": (K * N, F64), "dones": (K * N, I32)}
    kept = []  # the envs behind the launches stay alive until the checks are done

    def check_state(state, what):
        for name, win in state.items():
            assert win.bands_intact(), f"{what}: {name}: store outside [0, N)"
        for name in ("obs_src", "obs_pos", "returns", "timesteps", "episode_counts", "counters"):
            assert _same_bits(state[name].win, getattr(pop0, name).reshape(-1)), f"{what}: {name} differs from run()"
        slots = state["episode_returns"].win.view(N, M)
        filled = torch.arange(M, device="cuda").unsqueeze(0) < pop0.episode_counts.to(I64).unsqueeze(1)
        assert _same_bits(slots[filled], pop0.episode_returns[filled]), f"{what}: finished episodes differ from run()"
        assert bool((slots[~filled] == SENTINEL).all()), f"{what}: a slot at or above episode_counts was written"

    def launcher(names):
        outs = {k: _written(*sizes[k]) for k in names}
        states = []

        def launch():
            env, pop = _contract_population(fe, fo)
            kept.append((env, pop))
            assert _same_bits(pop.theta, pop0.theta) and _same_bits(pop._lr32.reshape(-1), ins["logret_f32"].win)
            states.append(_state_windows(pop))
            _abi_rollout(env, pop, K, states[-1], ins, outs)
        return outs, states, launch

    outs, states, launch = launcher(OUTPUTS)
    got = _two_poisons(launch, outs, None, ins)
    for k in OUTPUTS:
        assert _same_bits(got[k], want[k].reshape(-1)), f"{k}: differs from FusedPopulationMLP2Rollout.run"
    for i, state in enumerate(states):
        check_state(state, f"poison {i}")
    # no output at all, then each output missing on its own: what remains keeps its bits
    for missing in (OUTPUTS,) + tuple((k,) for k in OUTPUTS):
        names = tuple(k for k in OUTPUTS if k not in missing)
        outs, states, launch = launcher(names)
        for w in outs.values():
            w.poison(NAN)
        launch()
        what = "without " + ", ".join(missing)
        for k in names:
            assert outs[k].bands_intact(), f"{what}: {k}: store outside the buffer"
            assert _same_bits(outs[k].win, want[k].reshape(-1)), f"{what}: {k} differs from run()"
        check_state(states[0], what)
        env, pop = kept[-1]
        for name in ("cash", "margin", "env_indices", "env_spots"):
            assert_bits(t2n(getattr(env, name)), t2n(getattr(env0, name)), f"{what}: env.{name}")
    for k, w in ins.items():
        assert w.unchanged(), f"{k}: an input was written"


# ---------------------------------------------------------------- the update
def test_gradient_at_the_new_parameter_count(fe, fo):
    from finenvs_amd import evo

    _, env = _make(fe, fo, 333, 1, 8, 4, 40, seed=5, oracle=False)
    pop = _population(env, 3, 32, 0.02, seed=99)
    pop.set_parameters(*_layers2(8, 32, seed=2))
    assert pop.num_params == 40 * 32 + 32 * 32 + 96 + 1
    g = torch.Generator().manual_seed(3)
    diffed = (torch.rand((pop.num_pairs,), generator=g) - 0.5).to(env._dev)
    s1, s2 = pop.gradient(diffed), pop.gradient(diffed)
    assert tuple(s1.shape) == (pop.num_params,) and s1.dtype == torch.float64
    assert_bits(t2n(s1), t2n(s2), "two gradient calls")
    z = pop.noise(torch.arange(pop.num_pairs)).double()
    want = (diffed.double().unsqueeze(1) * z).mean(dim=0) - 0.005 * pop.theta.double()
    got = evo.es_gradient(s1, pop.num_pairs, pop.theta, 0.005).double()
    np.testing.assert_allclose(t2n(got), t2n(want), rtol=1e-5, atol=1e-6 * float(want.abs().max()))


def test_one_train_step_matches_the_torch_restatement(fe, fo):
    from finenvs_amd import evo

    _, env = _make(fe, fo, 258, 1, 8, 5, 40, seed=12, oracle=False)
    agent = evo.FusedEvoAgent(env, hidden_dim=32, hidden_layers=2, num_eval_envs=2, seed=3, max_episodes=8)
    pop = agent.population
    assert isinstance(pop, evo.FusedPopulationMLP2Rollout) and agent.hidden_layers == 2
    w, b = evo.init_parameters(40, 32, torch.Generator().manual_seed(3), hidden_layers=2)
    for got, want in zip(sum(pop.parameters(), []), w + b):
        assert torch.equal(got.cpu(), want)
    done = agent.collect(300, chunk=16)
    assert done >= 300 and pop.generation == 0
    theta0 = pop.theta.clone()
    ep, cnt = (t.clone() for t in pop.episodes())
    z = pop.noise(torch.arange(pop.num_pairs)).double()
    eval_mean = agent.train()
    ranks = evo.final_ranks(ep, cnt)
    diffed = evo.fitness(ranks, pop.num_training_envs)
    grad = ((diffed.double().unsqueeze(1) * z).mean(dim=0)).float() - 0.005 * theta0
    zero = torch.zeros_like(theta0)
    theta1, _, _ = evo.adam_step(theta0, grad, zero, zero.clone(), 1, 0.01)
    np.testing.assert_allclose(t2n(pop.theta), t2n(theta1), rtol=1e-5, atol=1e-7)
    assert not torch.equal(pop.theta, theta0)
    assert pop.generation == 1 and pop.step == 0 and pop.num_finished() == 0
    log = agent.log_progress()
    assert log["num_episodes"] == done and log["timesteps"] > 0 and log["mean_eval_return"] == eval_mean
    pop.run(4)  # the next generation runs on the new theta
    assert pop.step == 4
    # the default agent is the one-layer population it was
    _, env1 = _make(fe, fo, 20, 1, 8, 5, 40, seed=12, oracle=False)
    one = evo.FusedEvoAgent(env1, hidden_dim=32)
    assert type(one.population) is evo.FusedPopulationMLPRollout and one.population.num_params == 40 * 32 + 65


def test_example_runs_two_generations_with_two_hidden_layers(fe):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import es_time_series
    finally:
        sys.path.pop(0)
    hist = es_time_series.main(num_envs=258, num_eval_envs=2, window=8, hidden=32, hidden_layers=2, generations=2, days=6,
                               bars=40, quiet=True)
    assert len(hist) == 2
    assert all(h["num_episodes"] >= 2 * 258 for h in hist)
    assert hist[0]["L2_norm"] != hist[1]["L2_norm"]


# ---------------------------------------------------------------- refusals
def test_refusals(fe, fo):
    from finenvs_amd import _lib
    from finenvs_amd.data import synthetic

    prices, day_id, _ = synthetic.synthetic_series(4, 1, 40, 1)
    ev = fe.TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=8, num_envs=20, evaluate=True)
    with pytest.raises(ValueError, match="training-mode"):
        _population(ev, 2, 32, 0.02, 0)
    host = fe.TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=8, num_envs=20, redraw="torch")
    with pytest.raises(ValueError, match="redraw"):
        _population(host, 2, 32, 0.02, 0)
    env = fe.TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=8, num_envs=20, redraw="device")
    with pytest.raises(ValueError, match="even"):
        _population(env, 3, 32, 0.02, 0)
    with pytest.raises(ValueError, match="hidden_dim"):
        _population(env, 2, 256, 0.02, 0)
    with pytest.raises(ValueError, match="hidden_dim"):
        _population(env, 2, 48, 0.02, 0)
    pop = _population(env, 2, 32, 0.02, 0)
    good_w, good_b = _layers2(8, 32, seed=0)
    one_w, one_b = [good_w[0], good_w[2]], [good_b[0], good_b[2]]
    with pytest.raises(ValueError, match="three weight"):
        pop.set_parameters(one_w, one_b)  # the one-layer lists
    with pytest.raises(ValueError, match="expected"):
        pop.set_parameters([good_w[0], torch.zeros(32, 1), good_w[2]], good_b)
    with pytest.raises(ValueError, match="expected"):
        pop.set_parameters([good_w[0], good_w[1], torch.zeros(32, 2)], good_b)
    bad = [t.clone() for t in good_w]
    bad[1][31, 31] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        pop.set_parameters(bad, good_b)
    assert not bool(pop.theta.any())  # a refused set_parameters leaves theta as it was
    pop.set_parameters(good_w, good_b)
    for got, want in zip(sum(pop.parameters(), []), good_w + good_b):
        assert torch.equal(got.cpu(), want) and got.data_ptr() >= pop.theta.data_ptr()
    env.step(torch.zeros((20, 1), device=env._dev))
    with pytest.raises(RuntimeError, match="stale"):
        pop.run(2)
    pop.sync_from_env()
    pop.run(2)
    # the C ABI's own checks: H, an odd training population
    pop._pop.hidden = 256
    rc = env._lib.fe_evo2_rollout(env._handle, C.byref(pop._pop), 1, None, None, None, None, env._stream())
    assert rc == _lib.FE_ERR_ARG and b"H must be 32, 64 or 128" in env._lib.fe_last_error()
    pop._pop.hidden = 32
    pop._pop.num_train = 17
    rc = env._lib.fe_evo2_rollout(env._handle, C.byref(pop._pop), 1, None, None, None, None, env._stream())
    assert rc == _lib.FE_ERR_ARG and b"even" in env._lib.fe_last_error()
    _, wide = _make(fe, fo, 4, 129, 2, 3, 6, seed=1, oracle=False)
    with pytest.raises(ValueError, match="at most 128 assets"):
        _population(wide, 2, 32, 0.02, seed=0)
