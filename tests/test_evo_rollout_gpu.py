"""GPU: the fused ES population (finenvs_amd/evo.py, fe_evo_rollout / fe_evo_gradient / fe_evo_noise).

* noise: the rendered z is standard normal, differs across pairs and generations, and renders the same twice;
* lock-step parity (no action noise): per-env weights rebuilt from the rendered noise and a plain f32 torch forward on the
  rendered observation give the device's actions within 1e-5; fed to the oracle env those actions give the device's
  rewards, dones, state, running returns and episode slots bit for bit;
* chunking: run(32); run(32) equals run(64) bit for bit with action noise on;
* gradient: f64 torch restatement on the rendered noise, bit-identical repeats, one full train();
* the example at small size, the slot-overflow refusal and the argument refusals.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from tests.helpers import assert_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def t2n(t):
    return t.detach().cpu().numpy()


def _make(fe, fo, N, A, W, days, bars, seed, oracle=True):
    from finenvs_amd.data import synthetic

    prices, day_id, _ = synthetic.synthetic_series(days, A, bars, seed, 0.0)
    P, LR, *_ = fo.tables_from_series(prices, day_id, W)
    D = P.shape[0]
    idx = (np.arange(N) * 5 + 1) % D
    kw = dict(num_intervals=W, evaluate=False, starting_balance=2000)
    ref = None
    if oracle:
        ref = fo.OracleEnv(P, LR, env_indices=idx, redraw_mode=1, seed=9, auto_emit=False, **kw)
        ref.redraw_counter[0] = 1
    env = fe.TimeSeriesEnv(tables=(P, LR), env_indices=idx, redraw="device", seed=9, **kw)
    return ref, env


def _layers(W, H, seed):
    """ParallelMLP-shaped layers scaled so that the actions spread over (-1, 1) on these observations."""
    g = torch.Generator().manual_seed(seed)
    W1 = torch.randn((5 * W, H), generator=g) * (12.0 / W ** 0.5)
    W1[4::5, :] = torch.randn((W, H), generator=g) * (3.0 / W)
    b1 = torch.randn((1, H), generator=g) * 0.3
    W2 = torch.randn((H, 1), generator=g) * (2.0 / H ** 0.5)
    b2 = torch.full((1, 1), 0.03)
    return [W1, W2], [b1, b2]


def _member_weights(pop):
    """(N, P) f32: theta + s_i * fl(sigma * z_p) per env, from the rendered noise."""
    N, h = pop.env.num_envs, pop.num_pairs
    z = pop.noise(torch.arange(h))
    e = z * torch.tensor(pop.noise_std_dev, dtype=torch.float32, device=z.device)
    w = pop.theta.unsqueeze(0).repeat(N, 1)
    w[:h] = w[:h] + e
    w[h:2 * h] = w[h:2 * h] - e
    return w


def _forward(pop, w, obs):
    """Plain f32 torch forward of every env's network on every asset of obs (N, W, 5A) f64: (N, A)."""
    N, W, H, A = pop.env.num_envs, pop.env.num_intervals, pop.H, pop.env.num_assets
    O = 5 * W
    W1, b1 = w[:, :O * H].reshape(N, O, H), w[:, O * H:O * H + H].reshape(N, 1, H)
    W2, b2 = w[:, O * H + H:O * H + 2 * H].reshape(N, H, 1), w[:, O * H + 2 * H:].reshape(N, 1, 1)
    x = torch.as_tensor(obs, device=w.device).float()
    out = []
    for a in range(A):
        xa = x[:, :, 5 * a:5 * a + 5].reshape(N, 1, O)
        out.append(torch.tanh(torch.bmm(torch.tanh(torch.bmm(xa, W1) + b1), W2) + b2).reshape(N))
    return torch.stack(out, 1)


def test_noise_is_standard_normal_and_reproducible(fe, fo):
    from finenvs_amd.evo import FusedPopulationMLPRollout

    _, env = _make(fe, fo, 802, 1, 8, 4, 40, seed=3, oracle=False)
    pop = FusedPopulationMLPRollout(env, 2, 64, 0.02, seed=17)
    z = pop.noise(torch.arange(pop.num_pairs))
    assert z.numel() >= 10 ** 6
    zd = z.double()
    assert abs(float(zd.mean())) < 5e-3
    assert abs(float(zd.var()) - 1.0) < 1e-2
    assert abs(float((zd ** 4).mean()) - 3.0) < 0.05  # normal tails, not a uniform
    assert bool(torch.isfinite(z).all())
    assert_bits(t2n(pop.noise(torch.arange(pop.num_pairs))), t2n(z), "rendered twice")
    assert not torch.equal(z[0], z[1])
    assert not torch.equal(pop.noise([0], generation=1)[0], z[0])
    assert_bits(t2n(pop.noise([5, 0])), t2n(z[[5, 0]]), "pair list order")


@pytest.mark.parametrize("N,A,H,num_eval", [
    (203, 1, 64, 3),   # 100 pairs: not a multiple of the 8-pair tile
    (77, 3, 32, 5),    # three assets
    (151, 3, 64, 1),
    (130, 1, 32, 2),
])
def test_lockstep_parity_with_the_oracle(fe, fo, N, A, H, num_eval):
    from finenvs_amd.evo import FusedPopulationMLPRollout

    W = 8
    ref, env = _make(fe, fo, N, A, W, 5, 40, seed=N + A)
    pop = FusedPopulationMLPRollout(env, num_eval, H, 0.5, seed=4, action_noise_std=0.0, max_episodes=16)
    pop.set_parameters(*_layers(W, H, seed=H + A))
    w = _member_weights(pop)
    h, n_train = pop.num_pairs, pop.num_training_envs
    obs = ref.reset().copy()
    assert_bits(t2n(pop.observation()), obs, "initial obs")
    ret = np.zeros(N, dtype=np.float32)
    slots = [[] for _ in range(N)]
    worst, spread = 0.0, []
    for rep, K in enumerate((1, 5, 7, 32, 40)):
        acts, rews, dones = pop.run(K, record=True)
        assert_bits(t2n(pop.means), t2n(acts), "means == actions without action noise")
        for k in range(K):
            a_dev = t2n(acts[k])
            a_ref = t2n(_forward(pop, w, obs))
            worst = max(worst, float(np.abs(a_dev.astype(np.float64) - a_ref).max()))
            np.testing.assert_allclose(a_dev, a_ref, rtol=0, atol=1e-5, err_msg=f"chunk {rep} step {k} actions")
            spread.append(np.abs(a_dev[:h] - a_dev[h:2 * h]).max())
            obs, r_ref, d_ref, _ = ref.step(a_dev)
            obs = obs.copy()
            what = f"chunk {rep} step {k}"
            assert_bits(t2n(rews[k]), r_ref, what + " rewards")
            assert_bits(t2n(dones[k]), d_ref, what + " dones")
            ret = (ret.astype(np.float64) + r_ref).astype(np.float32)
            for n in np.nonzero(d_ref)[0]:
                slots[n].append(ret[n])
                ret[n] = 0.0
        assert_bits(t2n(env.cash), ref.cash, f"chunk {rep} cash")
        assert_bits(t2n(env.margin), ref.margin, f"chunk {rep} margin")
        assert_bits(t2n(env.env_indices), ref.env_idx, f"chunk {rep} env_idx")
        assert_bits(t2n(env.env_spots[:, 0]), ref.spot0, f"chunk {rep} spot0")
        assert_bits(t2n(pop.observation()), obs, f"chunk {rep} observation()")
        assert_bits(t2n(pop.returns), ret, f"chunk {rep} running returns")
    ep, cnt = pop.episodes()
    assert t2n(cnt).tolist() == [len(s) for s in slots]
    table = np.zeros((N, pop.max_episodes), dtype=np.float32)
    for n, s in enumerate(slots):
        table[n, :len(s)] = s
    assert_bits(t2n(ep), table, "episode slots")
    assert pop.num_finished() == sum(len(s) for s in slots) > N
    assert not pop.overflowed()
    # eval members act with theta itself, mirrored members with theta +- the same sigma z
    obs_now = pop.observation()
    theta_only = _forward(pop, pop.theta.unsqueeze(0).repeat(N, 1), obs_now)
    member = _forward(pop, w, obs_now)
    assert torch.equal(member[n_train:], theta_only[n_train:])
    swapped = w.clone()
    swapped[:h], swapped[h:2 * h] = w[h:2 * h], w[:h]
    assert float((_forward(pop, swapped, obs_now)[:n_train] - member[:n_train]).abs().max()) > 1e-2
    assert max(spread) > 1e-2, "the perturbation must change the actions"
    print(f"worst |device - torch| action difference {worst:.3g}")


def test_chunking_is_bit_exact_and_action_noise_has_the_stated_std(fe, fo):
    from finenvs_amd.evo import FusedPopulationMLPRollout

    N, A, W, H, num_eval, nu = 419, 1, 8, 64, 3, 0.01
    runs = []
    for split in ((32, 32), (64,)):
        _, env = _make(fe, fo, N, A, W, 5, 40, seed=21, oracle=False)
        pop = FusedPopulationMLPRollout(env, num_eval, H, 0.3, seed=8, action_noise_std=nu, max_episodes=8)
        pop.set_parameters(*_layers(W, H, seed=1))
        outs = [pop.run(K, record=True) + (pop.means,) for K in split]
        acts, rews, dones, means = (torch.cat([o[i] for o in outs]) for i in range(4))
        runs.append((acts, rews, dones, means, pop, env))
    (a1, r1, d1, m1, p1, e1), (a2, r2, d2, m2, p2, e2) = runs
    for x, y, what in ((a1, a2, "actions"), (r1, r2, "rewards"), (d1, d2, "dones"), (m1, m2, "means"),
                       (p1.returns, p2.returns, "running returns"), (p1.episode_returns, p2.episode_returns, "slots"),
                       (p1.episode_counts, p2.episode_counts, "counts"), (e1.cash, e2.cash, "cash"),
                       (p1.counters, p2.counters, "counters")):
        assert_bits(t2n(x), t2n(y), what)
    n_train = p1.num_training_envs
    assert torch.equal(a1[:, n_train:], m1[:, n_train:]), "eval envs take no action noise"
    noise = (a1[:, :n_train] - m1[:, :n_train]).double()
    assert abs(float(noise.std()) / nu - 1.0) < 0.05
    assert abs(float(noise.mean())) < 3e-4
    # different steps and envs draw different noise
    assert not torch.equal(noise[0], noise[1])


def test_gradient_matches_f64_torch_and_repeats_bit_for_bit(fe, fo):
    from finenvs_amd import evo

    _, env = _make(fe, fo, 333, 1, 8, 4, 40, seed=5, oracle=False)
    pop = evo.FusedPopulationMLPRollout(env, 3, 32, 0.02, seed=99)
    pop.set_parameters(*_layers(8, 32, seed=2))
    g = torch.Generator().manual_seed(3)
    diffed = (torch.rand((pop.num_pairs,), generator=g) - 0.5).to(env._dev)
    s1, s2 = pop.gradient(diffed), pop.gradient(diffed)
    assert_bits(t2n(s1), t2n(s2), "two gradient calls")
    z = pop.noise(torch.arange(pop.num_pairs)).double()
    want = (diffed.double().unsqueeze(1) * z).mean(dim=0) - 0.005 * pop.theta.double()
    got = evo.es_gradient(s1, pop.num_pairs, pop.theta, 0.005).double()
    np.testing.assert_allclose(t2n(got), t2n(want), rtol=1e-5, atol=1e-6 * float(want.abs().max()))


def test_one_train_step_matches_the_torch_restatement(fe, fo):
    from finenvs_amd import evo

    _, env = _make(fe, fo, 258, 1, 8, 5, 40, seed=12, oracle=False)
    agent = evo.FusedEvoAgent(env, hidden_dim=32, num_eval_envs=2, seed=3, max_episodes=8)
    pop = agent.population
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
    assert pop.generation == 1 and pop.step == 0 and pop.num_finished() == 0
    log = agent.log_progress()
    assert log["num_episodes"] == done and log["timesteps"] > 0
    assert log["mean_eval_return"] == eval_mean
    assert abs(log["L2_norm"] - float(theta1.double().norm())) < 1e-4 * log["L2_norm"]
    for key in ("std_dev_eval_return", "mean_training_return", "std_dev_training_return"):
        assert key in log
    pop.run(4)  # the next generation runs on the new theta
    assert pop.step == 4


def test_example_runs_two_generations(fe):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import es_time_series
    finally:
        sys.path.pop(0)
    hist = es_time_series.main(num_envs=258, num_eval_envs=2, window=8, hidden=32, generations=2, days=6, bars=40,
                               quiet=True)
    assert len(hist) == 2
    assert all(h["num_episodes"] >= 2 * 258 for h in hist)
    assert hist[0]["L2_norm"] != hist[1]["L2_norm"]


def test_slot_overflow_makes_train_refuse(fe, fo):
    from finenvs_amd import evo

    _, env = _make(fe, fo, 66, 1, 8, 4, 30, seed=2, oracle=False)
    agent = evo.FusedEvoAgent(env, hidden_dim=32, num_eval_envs=2, max_episodes=1)
    agent.population.run(80)  # episodes of at most 23 steps: every env finishes more than one
    assert agent.population.overflowed()
    with pytest.raises(RuntimeError, match="max_episodes"):
        agent.train()


def test_refusals(fe, fo):
    from finenvs_amd import _lib
    from finenvs_amd.evo import FusedPopulationMLPRollout
    from finenvs_amd.data import synthetic

    prices, day_id, _ = synthetic.synthetic_series(4, 1, 40, 1)
    ev = fe.TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=8, num_envs=20, evaluate=True)
    with pytest.raises(ValueError, match="training-mode"):
        FusedPopulationMLPRollout(ev, 2, 32, 0.02, 0)
    host = fe.TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=8, num_envs=20, redraw="torch")
    with pytest.raises(ValueError, match="redraw"):
        FusedPopulationMLPRollout(host, 2, 32, 0.02, 0)
    env = fe.TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=8, num_envs=20, redraw="device")
    with pytest.raises(ValueError, match="even"):
        FusedPopulationMLPRollout(env, 3, 32, 0.02, 0)
    with pytest.raises(ValueError, match="hidden_dim"):
        FusedPopulationMLPRollout(env, 2, 128, 0.02, 0)
    pop = FusedPopulationMLPRollout(env, 2, 32, 0.02, 0)
    with pytest.raises(ValueError):
        pop.set_parameters([torch.zeros(40, 32), torch.zeros(32, 2)], [torch.zeros(1, 32), torch.zeros(1, 1)])
    env.step(torch.zeros((20, 1), device=env._dev))
    with pytest.raises(RuntimeError, match="stale"):
        pop.run(2)
    pop.sync_from_env()
    pop.run(2)
    # the C ABI's own checks: an odd training population and a theta larger than the LDS
    pop._pop.num_train = 17
    rc = env._lib.fe_evo_rollout(env._handle, C.byref(pop._pop), 1, None, None, None, None, env._stream())
    assert rc == _lib.FE_ERR_ARG and b"even" in env._lib.fe_last_error()
    # W = 130, H = 64: theta is 41 729 floats, 163 KiB
    prices, day_id, _ = synthetic.synthetic_series(3, 1, 160, 1)
    big = fe.TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=130, num_envs=20, redraw="device")
    bp = FusedPopulationMLPRollout(big, 2, 64, 0.02, 0)
    with pytest.raises(_lib.FinEnvsNativeError, match="LDS"):
        bp.run(1)
