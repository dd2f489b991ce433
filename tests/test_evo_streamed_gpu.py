"""GPU: the streamed two-hidden-layer ES population (csrc/fe_evo_streamed.hip, ``fe_evo2_rollout_streamed``,
``FusedPopulationMLP2Rollout(..., streamed=True)``): theta read through L2 instead of an LDS copy, H up to the reference's 256.

* bit for bit against the resident kernel (``fe_evo2_rollout``) wherever both take the shape: twin envs, action noise on,
  staggered starts, two generations, every output, every state array of the population and of the env; row counts that do
  not divide among the row groups, PB = 7 and 1, three assets, and a grid above the cap (2 501 tiles for 2 048 workgroups);
* lock-step with the oracle env at H = 256 (one row group of 64 lanes, no butterfly) and at a window the resident kernel
  refuses at H = 128, with tests/test_evo2_rollout_gpu.py's ``_Lockstep``: state, rewards, dones, returns, counters and
  episode slots bit for bit, actions within ``ACTION_TOL_256`` of the f64 forward of the same f32 member weights;
* ``run(16); run(16)`` equals ``run(32)``; ``record=False`` equals ``record=True``; the memory contract of the C entry
  (the sibling's two-poison protocol, theta in a window of exactly P floats between NaN bands); the gradient at the new P,
  one ``train()`` of ``FusedEvoAgent`` at the reference's default shape, the example; the refusals.

``ACTION_TOL_256``.  As in the sibling file the reference value is the f64 forward, and the bound is 4 times the worst
|y32 - y64| of the plain f32 torch forward (``_forward2``) over the H = 256 lock-step cases below, rounded up to one digit:
two legitimate f32 summation orders of up to 320 + 256 terms.  Measured on an MI355X over those cases:
    H = 256: device 1.36e-05, torch f32 1.13e-05  (both at 17 assets, W = 4)    -> 4 x 1.13e-05 -> 5e-5
(per case, device / torch f32: W = 1 4.54e-06 / 5.85e-06; W = 3 6.66e-06 / 5.72e-06; A = 100 7.26e-06 / 9.96e-06; 100 pairs,
85 steps 1.15e-05 / 9.45e-06; W = 64 6.78e-06 / 6.75e-06).  The bound stays below 1e-4, where it would no longer separate
a wrong element from rounding.  The H = 128 case at W = 36 gave 3.95e-06 / 3.53e-06 and is held to the sibling's
``ACTION_TOL[128]``.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import tests.test_evo2_rollout_gpu as resident
from tests.helpers import assert_bits
from tests.test_evo2_rollout_gpu import SEED, _layers2, _Lockstep, _members, _stagger
from tests.test_evo_rollout_gpu import _make, _member_weights, t2n

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTION_TOL_256 = 5e-5  # see the module docstring
POP_STATE = ("returns", "timesteps", "episode_returns", "episode_counts", "counters", "obs_src", "obs_pos")
ENV_STATE = ("cash", "margin", "long_shares", "short_shares", "env_indices", "env_spots")


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


@pytest.fixture
def tol256(monkeypatch):
    """``_Lockstep`` reads the sibling's ``ACTION_TOL[pop.H]``: the H = 256 bound of this file, for the length of a test."""
    assert 256 not in resident.ACTION_TOL and ACTION_TOL_256 < 1e-4
    monkeypatch.setitem(resident.ACTION_TOL, 256, ACTION_TOL_256)


def _population(*args, streamed=True, **kwargs):
    from finenvs_amd.evo import FusedPopulationMLP2Rollout

    return FusedPopulationMLP2Rollout(*args, streamed=streamed, **kwargs)


def _same(p1, p2, e1, e2, what):
    for name in POP_STATE:
        assert_bits(t2n(getattr(p1, name)), t2n(getattr(p2, name)), f"{what}: {name}")
    assert_bits(t2n(p1.observation()), t2n(p2.observation()), f"{what}: observation()")
    for name in ENV_STATE:
        assert_bits(t2n(getattr(e1, name)), t2n(getattr(e2, name)), f"{what}: env.{name}")


# ---------------------------------------------------------------- bit for bit against the resident kernel
def _twins(fe, fo, N, A, W, H, num_eval, days, bars, max_episodes):
    sides = []
    for streamed in (False, True):
        _, env = _make(fe, fo, N, A, W, days, bars, seed=N + A, oracle=False)
        _stagger(env, None, bars)
        pop = _population(env, num_eval, H, 0.3, seed=SEED, action_noise_std=0.01, max_episodes=max_episodes, streamed=streamed)
        pop.set_parameters(*_layers2(W, H, seed=H + A))
        sides.append((env, pop))
    (e1, p1), (e2, p2) = sides
    assert p1._ENTRY == "fe_evo2_rollout" and p2._ENTRY == "fe_evo2_rollout_streamed" and p2.streamed and not p1.streamed
    return e1, p1, e2, p2


def _chunk_equal(p1, p2, e1, e2, K, what):
    outs = []
    for pop in (p1, p2):
        acts, rews, dones = pop.run(K, record=True)
        outs.append((acts, pop.means, rews, dones))
    for x, y, name in zip(outs[0], outs[1], ("actions", "means", "rewards", "dones")):
        assert_bits(t2n(x), t2n(y), f"{what}: {name}")
    _same(p1, p2, e1, e2, what)
    return outs[0]


@pytest.mark.parametrize("N,A,W,H,num_eval,days,bars", [
    (35, 1, 3, 128, 1, 4, 10),    # 15 rows for 2 row groups: 15 % 2 = 1
    (41, 17, 4, 64, 3, 4, 11),    # PB = 7: waves take 2, 2, 2, 1 units
    (7, 100, 2, 128, 1, 4, 9),    # PB = 1: three wavefronts idle through the unit loop
    (77, 3, 8, 32, 5, 4, 12),     # three assets; 8 row groups
])
def test_streamed_equals_the_resident_kernel_bit_for_bit(fe, fo, N, A, W, H, num_eval, days, bars):
    e1, p1, e2, p2 = _twins(fe, fo, N, A, W, H, num_eval, days, bars, max_episodes=16)
    n_train = p1.num_training_envs
    noisy = False
    for rep, K in enumerate((1, 5, 7)):
        acts, means, _, dones = _chunk_equal(p1, p2, e1, e2, K, f"generation 0 chunk {rep}")
        noisy = noisy or not torch.equal(acts[:, :n_train], means[:, :n_train])
    assert noisy and p1.num_finished() >= N and not p1.overflowed()  # action noise is on; episodes ended
    for pop in (p1, p2):
        pop.next_generation()
    assert p2.generation == 1 and p2.step == 0
    _chunk_equal(p1, p2, e1, e2, 5, "generation 1")
    assert p2.num_finished() > 0 and p2.total_timesteps() > 0


def test_streamed_equals_the_resident_kernel_in_the_tile_loop(fe, fo):
    """2 500 pair tiles and one eval tile for a grid of at most 2 048 workgroups: 453 workgroups take a second tile."""
    N, A, W, H, num_eval, bars = 40_000, 1, 3, 64, 2, 10
    e1, p1, e2, p2 = _twins(fe, fo, N, A, W, H, num_eval, 4, bars, max_episodes=8)
    assert (p1.num_pairs + 7) // 8 + 1 == 2501
    for rep, K in enumerate((3, 4)):
        _chunk_equal(p1, p2, e1, e2, K, f"chunk {rep}")
    assert p2.num_finished() > N // 2 and not p2.overflowed()


# ---------------------------------------------------------------- lock-step with the oracle
def _case(fe, fo, N, A, W, H, num_eval, days, bars, stagger):
    ref, env = _make(fe, fo, N, A, W, days, bars, seed=N + A)
    left = _stagger(env, ref, bars) if stagger else None
    pop = _population(env, num_eval, H, 0.5, seed=4, action_noise_std=0.0, max_episodes=16)
    pop.set_parameters(*_layers2(W, H, seed=H + A))
    return _Lockstep(pop, ref, env), left


LOCKSTEP = [  # N, A, W, H, num_eval, days, bars, chunks, check the members
    (35, 1, 1, 256, 3, 4, 8, (1, 5, 7), False),      # 5 rows
    (35, 1, 3, 256, 1, 4, 10, (1, 5, 7), True),      # 15 rows
    (41, 17, 4, 256, 3, 4, 11, (1, 5, 7), False),    # PB = 7
    (7, 100, 2, 256, 1, 4, 9, (1, 5, 7), False),     # PB = 1
    (203, 1, 8, 256, 3, 5, 40, (1, 5, 7, 32, 40), True),  # 100 pairs: a ragged last pair tile
    (23, 1, 64, 256, 3, 3, 73, (1, 5, 7), False),    # a window no resident width of that size could hold
    (23, 1, 36, 128, 3, 3, 45, (1, 5, 7), False),    # the first window the resident kernel refuses at H = 128
]


@pytest.mark.parametrize("N,A,W,H,num_eval,days,bars,chunks,members", LOCKSTEP)
def test_lockstep_parity_with_the_oracle(fe, fo, tol256, N, A, W, H, num_eval, days, bars, chunks, members):
    from finenvs_amd import _lib

    stagger = len(chunks) == 3
    run, left = _case(fe, fo, N, A, W, H, num_eval, days, bars, stagger)
    pop = run.pop
    assert pop.streamed and pop.num_params == 5 * W * H + H * H + 3 * H + 1
    lib = _lib.load()
    if H == 128:
        assert lib.fe_evo2_lds_bytes(W - 1, A, H) <= 160 * 1024 < lib.fe_evo2_lds_bytes(W, A, H)
    if W == 64:
        assert 4 * pop.num_params > 3 * 160 * 1024  # theta alone is several LDS
    w = _member_weights(pop)
    for rep, K in enumerate(chunks):
        run.run(K, w, f"chunk {rep}")
    if stagger:
        assert min(len(s) for s in run.slots) >= 1 and left.min() == 1 and run.total > N
    else:
        assert pop.num_finished() > N
    if members:
        _members(run, w)
    run.report(f"streamed (N, A, W, H) = ({N}, {A}, {W}, {H})")


# ---------------------------------------------------------------- chunking and recording at H = 256
def test_chunking_is_bit_exact_with_action_noise_at_256(fe, fo):
    N, A, W, H, num_eval, nu = 131, 1, 8, 256, 1, 0.01
    runs = []
    for split in ((16, 16), (32,)):
        _, env = _make(fe, fo, N, A, W, 5, 40, seed=21, oracle=False)
        _stagger(env, None, 40)
        pop = _population(env, num_eval, H, 0.3, seed=8, action_noise_std=nu, max_episodes=8)
        pop.set_parameters(*_layers2(W, H, seed=1))
        outs = [pop.run(K, record=True) + (pop.means,) for K in split]
        runs.append(tuple(torch.cat([o[i] for o in outs]) for i in range(4)) + (pop, env))
    (a1, r1, d1, m1, p1, e1), (a2, r2, d2, m2, p2, e2) = runs
    for x, y, what in ((a1, a2, "actions"), (r1, r2, "rewards"), (d1, d2, "dones"), (m1, m2, "means")):
        assert_bits(t2n(x), t2n(y), what)
    _same(p1, p2, e1, e2, "run(16); run(16) against run(32)")
    n_train = p1.num_training_envs
    assert p1.num_finished() > 0 and p1.step == 32 == p2.step
    assert torch.equal(a1[:, n_train:], m1[:, n_train:]), "eval envs take no action noise"
    assert not torch.equal(a1[:, :n_train], m1[:, :n_train])


def test_run_without_record_equals_run_with_record_at_256(fe, fo):
    N, A, W, H, num_eval, nu, bars = 77, 3, 8, 256, 5, 0.01, 12
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
    _same(p1, p2, e1, e2, "record=False against record=True")


# ---------------------------------------------------------------- the memory contract of fe_evo2_rollout_streamed
def test_evo2_rollout_streamed_memory_contract(fe, fo, monkeypatch):
    """tests/test_evo2_rollout_gpu.py's two-poison protocol (theta in a window of exactly P floats between NaN bands, the
    four outputs and nine state arrays between sentinel bands, all outputs null, then each on its own, inputs unchanged)
    with the population and the entry replaced: N = 41, A = 3, W = 7, H = 256, K = 6, four slots."""
    from finenvs_amd import _lib

    calls = []

    def contract_population(fe, fo):
        N, A, W, H, bars = 41, 3, 7, 256, 4
        _, env = _make(fe, fo, N, A, W, 4, bars, seed=50, oracle=False)
        _stagger(env, None, bars)
        pop = _population(env, 3, H, 0.3, seed=SEED, action_noise_std=0.01, max_episodes=4)
        pop.set_parameters(*_layers2(W, H, seed=9))
        assert pop.num_params == 35 * 256 + 256 * 256 + 769
        return env, pop

    def abi_rollout(env, pop, K, state, ins, outs):
        s = _lib.FeEvoPopulation()
        s.num_train, s.hidden, s.max_episodes = pop.num_training_envs, pop.H, pop.max_episodes
        s.noise_std, s.action_noise_std, s.seed = pop.noise_std_dev, pop.action_noise_std, pop.seed & (2 ** 64 - 1)
        s.generation, s.step = pop.generation, pop.step
        s.logret_f32, s.theta = ins["logret_f32"].ptr, ins["theta"].ptr
        for name in resident.STATE:
            setattr(s, name, state[name].ptr)
        ptr = lambda k: outs[k].ptr if k in outs else None  # noqa: E731
        pop._begin_run()
        _lib.check(env._lib.fe_evo2_rollout_streamed(env._handle, C.byref(s), K, ptr("actions"), ptr("means"), ptr("rewards"),
                                                     ptr("dones"), env._stream()))
        pop._end_run()
        torch.cuda.synchronize()
        calls.append(tuple(sorted(outs)))

    monkeypatch.setattr(resident, "_contract_population", contract_population)
    monkeypatch.setattr(resident, "_abi_rollout", abi_rollout)
    resident.test_evo2_rollout_memory_contract(fe, fo)
    # two poisons with every output, none, then each of the four missing on its own: all through the streamed entry
    assert len(calls) == 7 and calls[0] == calls[1] == tuple(sorted(resident.OUTPUTS)) and calls[2] == ()
    assert sorted(len(c) for c in calls[3:]) == [3, 3, 3, 3]


# ---------------------------------------------------------------- the update and the agent
def test_gradient_at_the_reference_parameter_count(fe, fo):
    from finenvs_amd import evo

    _, env = _make(fe, fo, 333, 1, 8, 4, 40, seed=5, oracle=False)
    pop = _population(env, 3, 256, 0.02, seed=99)
    pop.set_parameters(*_layers2(8, 256, seed=2))
    assert pop.num_params == 40 * 256 + 256 * 256 + 769
    g = torch.Generator().manual_seed(3)
    diffed = (torch.rand((pop.num_pairs,), generator=g) - 0.5).to(env._dev)
    s1, s2 = pop.gradient(diffed), pop.gradient(diffed)
    assert tuple(s1.shape) == (pop.num_params,) and s1.dtype == torch.float64
    assert_bits(t2n(s1), t2n(s2), "two gradient calls")
    z = pop.noise(torch.arange(pop.num_pairs)).double()
    want = (diffed.double().unsqueeze(1) * z).mean(dim=0) - 0.005 * pop.theta.double()
    got = evo.es_gradient(s1, pop.num_pairs, pop.theta, 0.005).double()
    np.testing.assert_allclose(t2n(got), t2n(want), rtol=1e-5, atol=1e-6 * float(want.abs().max()))


def test_one_train_step_at_the_reference_default_shape(fe, fo):
    from finenvs_amd import evo

    _, env = _make(fe, fo, 258, 1, 8, 5, 40, seed=12, oracle=False)
    agent = evo.FusedEvoAgent(env, hidden_dim=256, hidden_layers=2, num_eval_envs=2, seed=3, max_episodes=8)
    pop = agent.population
    assert isinstance(pop, evo.FusedPopulationMLP2Rollout) and pop.streamed and pop.H == 256 and agent.hidden_layers == 2
    assert pop._ENTRY == "fe_evo2_rollout_streamed"
    w, b = evo.init_parameters(40, 256, torch.Generator().manual_seed(3), hidden_layers=2)
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
    # the choice: resident where the shape fits, streamed where it does not or where it is asked for
    for hidden, window, streamed, want in ((128, 8, None, False), (128, 8, True, True), (128, 36, None, True), (32, 8, None, False)):
        _, e = _make(fe, fo, 20, 1, window, 3, window + 9, seed=12, oracle=False)
        a = evo.FusedEvoAgent(e, hidden_dim=hidden, hidden_layers=2, streamed=streamed)
        assert a.population.streamed is want, (hidden, window, streamed)
    _, env1 = _make(fe, fo, 20, 1, 8, 5, 40, seed=12, oracle=False)
    one = evo.FusedEvoAgent(env1, hidden_dim=32)
    assert type(one.population) is evo.FusedPopulationMLPRollout and one.population.num_params == 40 * 32 + 65


def test_example_runs_two_generations_at_the_reference_default_shape(fe):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import es_time_series
    finally:
        sys.path.pop(0)
    hist = es_time_series.main(num_envs=258, num_eval_envs=2, window=8, hidden=256, hidden_layers=2, generations=2, days=6,
                               bars=40, quiet=True)
    assert len(hist) == 2
    assert all(h["num_episodes"] >= 2 * 258 for h in hist)
    assert hist[0]["L2_norm"] != hist[1]["L2_norm"]


# ---------------------------------------------------------------- refusals
def test_refusals(fe, fo):
    from finenvs_amd import _lib, evo
    from finenvs_amd.data import synthetic

    prices, day_id, _ = synthetic.synthetic_series(4, 1, 40, 1)
    ev = fe.TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=8, num_envs=20, evaluate=True)
    with pytest.raises(ValueError, match="training-mode"):
        _population(ev, 2, 256, 0.02, 0)
    host = fe.TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=8, num_envs=20, redraw="torch")
    with pytest.raises(ValueError, match="redraw"):
        _population(host, 2, 256, 0.02, 0)
    env = fe.TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=8, num_envs=20, redraw="device")
    with pytest.raises(ValueError, match="even"):
        _population(env, 3, 256, 0.02, 0)
    for hidden in (512, 48):
        with pytest.raises(ValueError, match="hidden_dim"):
            _population(env, 2, hidden, 0.02, 0)
    with pytest.raises(ValueError, match="theta lives in the 160 KiB LDS"):  # the resident class's message
        evo.FusedEvoAgent(env, hidden_dim=256, hidden_layers=2, streamed=False)
    with pytest.raises(ValueError, match="theta lives in the 160 KiB LDS"):
        _population(env, 2, 256, 0.02, 0, streamed=False)
    pop = _population(env, 2, 256, 0.02, 0)
    pop.set_parameters(*_layers2(8, 256, seed=0))
    pop.run(2)
    # the C ABI's own checks: H, an odd training population
    pop._pop.hidden = 512
    rc = env._lib.fe_evo2_rollout_streamed(env._handle, C.byref(pop._pop), 1, None, None, None, None, env._stream())
    assert rc == _lib.FE_ERR_ARG and b"fe_evo2_rollout_streamed: H must be 32, 64, 128 or 256" in env._lib.fe_last_error()
    pop._pop.hidden = 256
    pop._pop.num_train = 17
    rc = env._lib.fe_evo2_rollout_streamed(env._handle, C.byref(pop._pop), 1, None, None, None, None, env._stream())
    assert rc == _lib.FE_ERR_ARG and b"even" in env._lib.fe_last_error()
    # the resident entry still stops at 128
    pop._pop.num_train = 18
    rc = env._lib.fe_evo2_rollout(env._handle, C.byref(pop._pop), 1, None, None, None, None, env._stream())
    assert rc == _lib.FE_ERR_ARG and b"H must be 32, 64 or 128" in env._lib.fe_last_error()
    _, wide = _make(fe, fo, 4, 129, 2, 3, 6, seed=1, oracle=False)
    with pytest.raises(ValueError, match="at most 128 assets"):
        _population(wide, 2, 256, 0.02, seed=0)
