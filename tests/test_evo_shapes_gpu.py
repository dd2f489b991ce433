"""GPU: the ES population (csrc/fe_evo_kernels.h, finenvs_amd/evo.py) away from the shapes tests/test_evo_rollout_gpu.py runs.

* the two noise streams, element by element, against the host mirror of include/finenvs_amd_evo.h (tests/helpers.py,
  pinned by tests/test_evo_streams_host.py): the rendered ``z`` at three (H, W), two generations and two seeds, and the
  action noise ``actions - means`` at A in {1, 3, 5, 17}, across two launches and into generation 1;
* lock-step parity with the oracle at windows whose 5W rows do not divide among the row groups of ``evo_policy_unit``
  (W = 1, 3, 7), at the largest windows the LDS admits (W = 126 at H = 64, W = 254 at H = 32: the launch above 64 KiB), and
  at pair tiles of 7, 4 and 1 pairs (A = 17, 30, 100); the per-env and the global step counters against a host count;
  the window above the largest and A = 129 refused;
* generation 1: cleared episode state, weights rebuilt from ``noise(generation=1)``, the oracle carrying on;
* ``run(K, record=False)`` equals ``run(K, record=True)`` in every array the launch leaves behind;
* the memory contract of ``fe_evo_rollout`` through the C ABI: four optional outputs, two inputs and nine state arrays
  between guard bands;
* ``fe_evo_gradient`` at 1, 64, 65 and 4 097 pairs against the exact f64 sum.

The envs of the lock-step cases start at staggered rows of their days (``_stagger``), so that episodes of 1 to 12 steps
finish at different steps in different envs and every env finishes at least one within the 13 steps a case runs.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.helpers import assert_bits, evo_action_noise_reference, evo_z_reference
from tests.test_evo_rollout_gpu import _forward, _layers, _make, _member_weights, t2n
from tests.test_memory_contract_gpu import (F32, F64, I32, I64, NAN, SENTINEL, _floats, _index, _same_bits, _two_poisons,
                                             _Window, _written)

pytestmark = pytest.mark.gpu

# |z - z64| on every element: about a hundred f32 ulps of the largest radius, sqrt(48 ln 2) = 5.77.  An identity check of
# the stream (a wrong word, counter slot or key is off by order 1), not an accuracy claim.
Z_BOUND = 1e-4
MAX_LDS = 160 * 1024
SEEDS = (0x0123456789ABCDEF, 0x9E3779B97F4A7C15)  # both halves non-zero; the second is above 2^63


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
    from finenvs_amd.evo import FusedPopulationMLPRollout

    return FusedPopulationMLPRollout(*args, **kwargs)


def _stagger(env, ref, bars):
    """Move env n to the row of its day from which 1 + 7 n mod min(bars, 12) steps are left (a day of ``bars`` bars ends an
    episode after ``bars`` steps from row 0), on the device env and on the oracle alike.  Returns the episode lengths."""
    N, W = env.num_envs, env.num_intervals
    m = min(bars, 12)
    left = 1 + (7 * np.arange(N)) % m
    first = bars - left
    env.env_spots = torch.as_tensor(first).unsqueeze(1) + torch.arange(W)
    if ref is not None:
        ref.spot0[:] = first
    return left


# ---------------------------------------------------------------- a. the rendered noise against the mirror
@pytest.mark.parametrize("H,W,bars", [(32, 1, 8), (64, 8, 14), (64, 126, 160)])
def test_noise_equals_the_host_mirror(fe, fo, H, W, bars):
    """``fe_evo_noise`` against ``evo_z_reference`` (f64, written from the header): every element within 1e-4.
    Measured on an MI355X: max |z - z64| = 4.5e-7, 5.1e-7 and 7.9e-7 at the three shapes (the hardware log2 / sin / cos and
    f32 rounding at a radius of up to 5.77): below 2.5e-5, so the bound stands as set."""
    _, env = _make(fe, fo, 23, 1, W, 3, bars, seed=3, oracle=False)
    worst = 0.0
    for seed in SEEDS:
        pop = _population(env, 3, H, 0.02, seed=seed)
        last = pop.num_pairs - 1
        assert last == 9
        for pairs in ([0, last], [7, 0, last, 3, 3, 1]):  # the first, the last, unsorted and repeated
            for g in (0, 3):
                z = t2n(pop.noise(pairs, generation=g))
                z64 = evo_z_reference(seed, g, pairs, pop.num_params)
                assert z.shape == z64.shape == (len(pairs), 5 * W * H + 2 * H + 1) and bool(np.isfinite(z).all())
                diff = float(np.abs(z.astype(np.float64) - z64).max())
                worst = max(worst, diff)
                assert diff <= Z_BOUND, f"seed {seed:#x} generation {g} pairs {pairs}: max |z - z64| = {diff:.3g}"
    print(f"H = {H}, W = {W}: max |z - z64| = {worst:.3g}")


# ---------------------------------------------------------------- b. the action noise against the mirror
@pytest.mark.parametrize("A", [1, 3, 5, 17])
def test_action_noise_equals_the_host_mirror(fe, fo, A):
    """``actions - means`` of the training envs is ``nu xi(n, step, a)`` of the mirror; the step counts from the generation's
    start across launches; eval envs take none; members of one pair, neighbouring assets, assets four apart (the same
    word of the next counter domain) and consecutive steps draw different noise."""
    N, W, H, num_eval, nu, seed = 41, 4, 32, 3, 0.25, SEEDS[1]
    _, env = _make(fe, fo, N, A, W, 4, 11, seed=30 + A, oracle=False)
    pop = _population(env, num_eval, H, 0.3, seed=seed, action_noise_std=nu, max_episodes=8)
    pop.set_parameters(*_layers(W, H, seed=A))
    n_train, half = pop.num_training_envs, pop.num_pairs
    worst = 0.0
    for g, chunks in ((0, (3, 4)), (1, (2,))):
        if g:
            pop.next_generation()
        assert pop.generation == g and pop.step == 0
        outs = [(pop.run(K, record=True)[0], pop.means) for K in chunks]
        acts, means = (torch.cat([o[i] for o in outs]) for i in range(2))
        steps = sum(chunks)
        assert tuple(acts.shape) == (steps, N, A) and pop.step == steps
        assert_bits(t2n(acts[:, n_train:]), t2n(means[:, n_train:]), "eval envs take no action noise")
        a64, m64 = t2n(acts[:, :n_train]).astype(np.float64), t2n(means[:, :n_train]).astype(np.float64)
        noise = a64 - m64
        xi = evo_action_noise_reference(seed, g, np.arange(steps)[:, None, None], np.arange(n_train)[None, :, None],
                                        np.arange(A)[None, None, :])
        # the mirror's bound on xi, and the f32 rounding of means + nu xi (nu = 2^-2: the product is exact)
        tol = nu * Z_BOUND + 2.0 ** -22 * np.maximum(1.0, np.abs(a64))
        err = np.abs(noise - nu * xi)
        worst = max(worst, float((err / tol).max()))
        bad = np.argwhere(err > tol)
        assert bad.size == 0, (f"generation {g}: {bad.shape[0]} of {err.size} elements off, first (step, env, asset) = "
                               f"{tuple(bad[0])}: {noise[tuple(bad[0])]!r} against {nu * xi[tuple(bad[0])]!r}")
        assert float(np.abs(noise).max()) > nu  # the noise is there
        # columns that must differ: 1e-3 is 4e-3 standard deviations of nu xi, rounding is below 3e-7
        assert bool((np.abs(noise[:, :half] - noise[:, half:]).max(axis=(0, 2)) > 1e-3).all()), "members p and half + p"
        for d in (1, 4):
            if A > d:
                assert bool((np.abs(noise[:, :, :-d] - noise[:, :, d:]).max(axis=(0, 1)) > 1e-3).all()), f"assets a, a + {d}"
        assert bool((np.abs(noise[:-1] - noise[1:]).max(axis=(1, 2)) > 1e-3).all()), "steps k and k + 1"
    print(f"A = {A}: worst err / tol of actions - means against nu xi64: {worst:.3g}")


# ---------------------------------------------------------------- c, d. lock-step parity
def _forward64(pop, w, obs):
    """``_forward`` in f64 on the same f32 weights and the same f32 inputs: (N, A)."""
    N, W, H, A = pop.env.num_envs, pop.env.num_intervals, pop.H, pop.env.num_assets
    O = 5 * W
    w = w.double()
    W1, b1 = w[:, :O * H].reshape(N, O, H), w[:, O * H:O * H + H].reshape(N, 1, H)
    W2, b2 = w[:, O * H + H:O * H + 2 * H].reshape(N, H, 1), w[:, O * H + 2 * H:].reshape(N, 1, 1)
    x = torch.as_tensor(obs, device=w.device).float().double()
    out = []
    for a in range(A):
        xa = x[:, :, 5 * a:5 * a + 5].reshape(N, 1, O)
        out.append(torch.tanh(torch.bmm(torch.tanh(torch.bmm(xa, W1) + b1), W2) + b2).reshape(N))
    return torch.stack(out, 1)


class _Lockstep:
    """The procedure of test_evo_rollout_gpu.py::test_lockstep_parity_with_the_oracle, chunk by chunk, with the host's own
    count of steps: per env since its last done, and summed over the finished episodes."""

    def __init__(self, pop, ref, env):
        self.pop, self.ref, self.env = pop, ref, env
        N = env.num_envs
        self.obs = ref.reset().copy()
        assert_bits(t2n(pop.observation()), self.obs, "initial obs")
        self.ret = np.zeros(N, dtype=np.float32)
        self.ts = np.zeros(N, dtype=np.float32)
        self.slots = [[] for _ in range(N)]
        self.total = 0
        self.ratio = 0.0
        self.spread = 0.0

    def clear(self):
        self.ret[:] = 0
        self.ts[:] = 0
        self.slots = [[] for _ in self.slots]
        self.total = 0

    def run(self, K, w, what):
        pop, ref, env, h = self.pop, self.ref, self.env, self.pop.num_pairs
        acts, rews, dones = pop.run(K, record=True)
        assert_bits(t2n(pop.means), t2n(acts), "means == actions without action noise")
        for k in range(K):
            a_dev = t2n(acts[k])
            y32, y64 = t2n(_forward(pop, w, self.obs)).astype(np.float64), t2n(_forward64(pop, w, self.obs))
            # the project's evo action tolerance plus f32 torch's own error at this shape
            tol = 1e-5 + 4 * float(np.abs(y32 - y64).max())
            err = float(np.abs(a_dev.astype(np.float64) - y64).max())
            self.ratio = max(self.ratio, err / tol)
            assert err <= tol, f"{what} step {k} actions: err {err:.3g} > tol {tol:.3g}"
            self.spread = max(self.spread, float(np.abs(a_dev[:h] - a_dev[h:2 * h]).max()))
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
        self.check_slots(what)

    def check_slots(self, what):
        pop = self.pop
        ep, cnt = pop.episodes()
        assert t2n(cnt).tolist() == [len(s) for s in self.slots], what + " episode counts"
        table = np.zeros((len(self.slots), pop.max_episodes), dtype=np.float32)
        for n, s in enumerate(self.slots):
            table[n, :len(s)] = s
        assert_bits(t2n(ep), table, what + " episode slots")
        assert pop.num_finished() == sum(len(s) for s in self.slots) and not pop.overflowed()


def _lockstep_case(fe, fo, N, A, W, H, num_eval, days, bars):
    ref, env = _make(fe, fo, N, A, W, days, bars, seed=N + A)
    left = _stagger(env, ref, bars)
    pop = _population(env, num_eval, H, 0.5, seed=4, action_noise_std=0.0, max_episodes=16)
    pop.set_parameters(*_layers(W, H, seed=H + A))
    return _Lockstep(pop, ref, env), left


def _evo_lds_bytes(EB, A, P):
    """``evo_lds`` of csrc/fe_evo_kernels.h restated: the tile's account state, the redrawn days, the actions, theta."""
    S = EB * A
    b = EB * 8 + S * 8 + S * 8 + S * 4 + S * 4 + EB * 4
    b = (b + 7) & ~7
    b += EB * 8
    b += S * 4
    b = (b + 15) & ~15
    b += P * 4
    return (b + 15) & ~15


LOCKSTEP_CASES = [  # N, A, W, H, num_eval, days, bars
    (35, 1, 1, 32, 3, 4, 8),        # 5 rows for R = 8 row groups: three of them idle
    (35, 1, 3, 64, 1, 4, 10),       # 15 rows for R = 4: 15 % 4 = 3
    (51, 1, 7, 32, 3, 4, 14),       # 35 rows for R = 8: 35 % 8 = 3
    (23, 1, 126, 64, 3, 3, 160),    # the largest window at H = 64: 162 576 bytes of LDS
    (23, 1, 254, 32, 1, 3, 262),    # the largest window at H = 32: 163 600 bytes
    (41, 17, 4, 32, 3, 4, 11),      # PB = 7: waves take 2, 2, 2, 1 units; the last pair tile holds 5 pairs
    (21, 30, 4, 64, 3, 4, 11),      # PB = 4: the last pair tile holds 1 pair
    (7, 100, 2, 32, 1, 4, 9),       # PB = 1: three pair tiles of one pair, three wavefronts idle through the unit loop
]


@pytest.mark.parametrize("N,A,W,H,num_eval,days,bars", LOCKSTEP_CASES)
def test_lockstep_parity_at_untested_geometries(fe, fo, N, A, W, H, num_eval, days, bars):
    """State, rewards, dones, running returns, episode slots and both step counters bit for bit against the oracle; actions
    within ``1e-5 + 4 max|y32 - y64|`` of an f64 forward of the same f32 member weights.  Worst err / tol measured on an
    MI355X, in the order of LOCKSTEP_CASES: 0.054, 0.061, 0.062, 0.170, 0.129, 0.069, 0.062, 0.053."""
    from finenvs_amd import _lib

    run, left = _lockstep_case(fe, fo, N, A, W, H, num_eval, days, bars)
    pop = run.pop
    PB = max(1, min(8, 128 // A))
    lds = _evo_lds_bytes(2 * PB, A, pop.num_params)
    assert lds <= MAX_LDS
    w = _member_weights(pop)
    for rep, K in enumerate((1, 5, 7)):
        run.run(K, w, f"chunk {rep}")
    assert min(len(s) for s in run.slots) >= 1 and left.min() == 1 and run.total > N
    assert len({len(s) for s in run.slots}) > 1 or bars > 12, "some envs finish twice"
    assert run.spread > 1e-2, "the perturbation must change the actions"
    print(f"(N, A, W, H) = ({N}, {A}, {W}, {H}): LDS {lds} bytes, worst action err / tol {run.ratio:.3g}")
    if lds > 64 * 1024:  # the largest window: the next one is refused, and the restated formula agrees with both outcomes
        assert _evo_lds_bytes(2 * PB, A, 5 * (W + 1) * H + 2 * H + 1) > MAX_LDS
        _, big = _make(fe, fo, N, A, W + 1, days, bars, seed=N + A, oracle=False)
        bp = _population(big, num_eval, H, 0.5, seed=4)
        with pytest.raises(_lib.FinEnvsNativeError, match="LDS"):
            bp.run(1)


def test_more_than_128_assets_are_refused(fe, fo):
    from finenvs_amd import _lib

    _, env = _make(fe, fo, 4, 129, 2, 3, 6, seed=1, oracle=False)
    pop = _population(env, 2, 32, 0.02, seed=0)
    with pytest.raises(_lib.FinEnvsNativeError, match="at most 128 assets"):
        pop.run(1)


def test_generation_1_runs_on_its_own_noise(fe, fo):
    """After ``next_generation()`` the episode state is cleared, the rollout perturbs with ``noise(generation=1)`` and the
    envs (and the oracle) carry on where generation 0 left them."""
    N, A, W, H, num_eval, days, bars = LOCKSTEP_CASES[2]
    run, _ = _lockstep_case(fe, fo, N, A, W, H, num_eval, days, bars)
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
    assert_bits(t2n(pop.noise(torch.arange(pop.num_pairs), generation=1)), t2n(pop.noise(torch.arange(pop.num_pairs))),
                "noise() renders the current generation")
    h = pop.num_pairs
    assert float((w1[:2 * h] - w0[:2 * h]).abs().min(dim=1).values.max()) > 0 and not torch.equal(w1[:2 * h], w0[:2 * h])
    assert float((w1[:h] - w0[:h]).abs().max()) > 0.5  # sigma = 0.5: other draws, not a rounding difference
    assert torch.equal(w1[2 * h:], w0[2 * h:])
    run.run(7, w1, "generation 1")
    assert pop.num_finished() > 0
    print(f"generation 1: worst action err / tol {run.ratio:.3g}")


# ---------------------------------------------------------------- e. the scratch reward and done buffers
def test_run_without_record_equals_run_with_record(fe, fo):
    N, A, W, H, num_eval, nu, bars = 77, 3, 8, 32, 5, 0.01, 12
    sides = []
    for record in (True, False):
        _, env = _make(fe, fo, N, A, W, 4, bars, seed=40, oracle=False)
        _stagger(env, None, bars)
        pop = _population(env, num_eval, H, 0.3, seed=SEEDS[0], action_noise_std=nu, max_episodes=8)
        pop.set_parameters(*_layers(W, H, seed=6))
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


# ---------------------------------------------------------------- f. the memory contract of fe_evo_rollout
STATE = ("obs_src", "obs_pos", "returns", "timesteps", "episode_returns", "episode_counts", "counters", "scratch_rewards",
         "scratch_dones")
OUTPUTS = ("actions", "means", "rewards", "dones")


def _contract_population(fe, fo):
    N, A, W, H, bars = 41, 3, 7, 64, 4
    _, env = _make(fe, fo, N, A, W, 4, bars, seed=50, oracle=False)
    _stagger(env, None, bars)
    pop = _population(env, 3, H, 0.3, seed=SEEDS[1], action_noise_std=0.01, max_episodes=4)
    pop.set_parameters(*_layers(W, H, seed=9))
    return env, pop


def _banded(data):
    """A state array the launch reads and writes: its data between sentinel bands."""
    flat = data.detach().reshape(-1)
    return _Window(flat.numel(), flat.dtype, SENTINEL if flat.is_floating_point() else -9, flat)


def _state_windows(pop):
    """The nine state arrays of ``fe_evo_population`` as windows holding what a fresh population holds; every slot of
    ``episode_returns`` pre-filled with the sentinel.  The bands of ``obs_src`` repeat a valid descriptor."""
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
    """``fe_evo_rollout`` with the struct ``FusedPopulationMLPRollout.run`` builds, its pointers replaced by the windows;
    an output missing from ``outs`` is passed as null."""
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
    _lib.check(env._lib.fe_evo_rollout(env._handle, C.byref(s), K, ptr("actions"), ptr("means"), ptr("rewards"),
                                       ptr("dones"), env._stream()))
    pop._end_run()
    torch.cuda.synchronize()


def test_evo_rollout_memory_contract(fe, fo):
    """Every pointer of ``fe_evo_rollout`` is a window inside a larger allocation the test owns: NaN bands round the two
    inputs, sentinel bands round the four outputs and the nine state arrays."""
    K = 6
    env0, pop0 = _contract_population(fe, fo)
    N, A, M = env0.num_envs, env0.num_assets, pop0.max_episodes
    acts, rews, dones = pop0.run(K, record=True)
    want = {"actions": acts, "means": pop0.means, "rewards": rews, "dones": dones}
    counts = pop0.episode_counts.tolist()
    assert max(counts) == 2 and min(counts) == 1 and not pop0.overflowed()  # slots are filled to different depths
    assert not torch.equal(acts[:, :pop0.num_training_envs], pop0.means[:, :pop0.num_training_envs])
    ins = {"theta": _floats(pop0.theta), "logret_f32": _floats(pop0._lr32.reshape(-1))}
    sizes = {"actions": (K * N * A, F32), "means": (K * N * A, F32), "rewards": (K * N, F64), "dones": (K * N, I32)}
    kept = []  # the envs behind the launches stay alive until the checks are done

    def check_state(state, what):
        for name, win in state.items():
            assert win.bands_intact(), f"{what}: {name}: store outside the buffer"
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

    # all four outputs, from NaN-filled and from sentinel-filled windows, on two fresh twins of env0
    outs, states, launch = launcher(OUTPUTS)
    got = _two_poisons(launch, outs, None, ins)
    for k in OUTPUTS:
        assert _same_bits(got[k], want[k].reshape(-1)), f"{k}: differs from FusedPopulationMLPRollout.run"
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


# ---------------------------------------------------------------- g. the gradient's block and parameter edges
@pytest.mark.parametrize("H,W,pairs", [(H, W, p) for H, W in ((64, 8), (32, 1)) for p in (1, 64, 65, 4097)] + [(64, 126, 65)])
def test_gradient_block_edges(H, W, pairs):
    """``fe_evo_gradient`` at one pair, one full 64-pair block, one pair more, and 65 blocks of which the last holds one
    pair; P = 5WH + 2H + 1 is never a multiple of the four parameters a thread renders.  Against the exact f64 sum of
    ``diffed[p] z`` with the bound tests/test_memory_contract_gpu.py derives."""
    from finenvs_amd import _lib

    lib = _lib.load()
    params, seed, generation = 5 * W * H + 2 * H + 1, SEEDS[1], 2
    assert params % 4 == 1
    st = torch.cuda.current_stream().cuda_stream
    diffed = torch.rand((pairs,), generator=torch.Generator(device="cuda").manual_seed(pairs + H), device="cuda") - 0.5
    index = torch.arange(pairs, device="cuda")
    z = torch.empty((pairs, params), dtype=F32, device="cuda")
    _lib.check(lib.fe_evo_noise(seed, generation, index.data_ptr(), pairs, params, z.data_ptr(), st), lib)
    blocks = (pairs + 63) // 64
    assert int(lib.fe_evo_gradient_workspace_doubles(pairs, params)) == blocks * params
    ws = _written(blocks * params, F64)
    ins = {"diffed": _floats(diffed)}
    outs = {"out": _written(params, F64)}
    got = _two_poisons(lambda: _lib.check(lib.fe_evo_gradient(seed, generation, pairs, params, ins["diffed"].ptr, ws.ptr,
                                                              outs["out"].ptr, st), lib), outs, ws, ins)["out"]
    terms = diffed.double().unsqueeze(1) * z.double()  # exact: f32 x f32 in f64
    want = terms.sum(dim=0)
    bound = 2 * pairs * 2.0 ** -53 * terms.abs().sum(dim=0)
    assert float(want.abs().max()) > 0 and bool(((got - want).abs() <= bound).all())
