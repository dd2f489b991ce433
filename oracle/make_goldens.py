#!/usr/bin/env python3
"""Generate tests/golden/*.npz by RUNNING THE REFERENCE in the build container.

TEST INFRASTRUCTURE ONLY -- runs where /root/reference exists (never on the
GPU box, never from the product).  The reference's Python is imported from a
scratch copy under /tmp (it writes a bounds-cache JSON next to its CSVs,
TSE:122-124, and __pycache__), with a six-line stand-in for the one class of
the absent ``gym`` package it touches (``spaces.Box``, TSE:224-234).  Nothing
of the reference is written into this repository: only arrays (inputs we
generated ourselves + the outputs the reference computed from them).

    python oracle/make_goldens.py            # rewrites tests/golden/*.npz
    python oracle/make_goldens.py tables_ibm.npz rollout_spy_w4.npz   # only the named fixtures

Inputs are the build's own seeded synthetic CSVs (finenvs_amd.data.synthetic),
plus one real-data case: the reference's smallest test fixture
(finenvs/data/OIH/dummy.csv, 1050 rows), whose market-hours rows are stored in
the fixture as a plain (T, 4) array.
"""
from __future__ import annotations

import glob
import json
import os
import shutil
import sys
import types

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from finenvs_amd.data import synthetic  # noqa: E402

REF = "/root/reference"
WORK = "/tmp/fe_oracle_work"
GOLD = os.path.join(REPO, "tests", "golden")
ONLY = set(a for a in sys.argv[1:] if a.endswith(".npz"))  # empty = write everything


def wanted(fname: str) -> bool:
    return not ONLY or os.path.basename(fname) in ONLY


def save_npz(path: str, **arrays) -> None:
    """np.savez_compressed unless the fixture was filtered out on the command line (existing files stay
    byte-identical when only new fixtures are added)."""
    if wanted(path):
        np.savez_compressed(path, **arrays)
    else:
        print("   (kept)", os.path.basename(path))



def setup_reference():
    if os.path.isdir(WORK):
        shutil.rmtree(WORK)
    os.makedirs(WORK)
    shutil.copytree(
        os.path.join(REF, "finenvs"),
        os.path.join(WORK, "refcopy", "finenvs"),
        ignore=shutil.ignore_patterns("isaac_gym_envs", "__pycache__", "data"),
    )
    os.makedirs(os.path.join(WORK, "data"))
    # stand-in for gym.spaces.Box: the env only stores these objects
    gym = types.ModuleType("gym")
    spaces = types.ModuleType("gym.spaces")

    class Box:  # noqa: D401
        def __init__(self, low, high, dtype=None):
            self.low, self.high, self.dtype, self.shape = low, high, dtype, np.shape(low)

    spaces.Box = Box
    gym.spaces = spaces
    sys.modules["gym"] = gym
    sys.modules["gym.spaces"] = spaces
    sys.path.insert(0, os.path.join(WORK, "refcopy"))


def data_dir(name: str) -> str:
    # the path must contain the substring "data" to be taken verbatim (TSE:47-51)
    return os.path.join(WORK, "data", name)


def make_env(name: str, W: int, **kw):
    from finenvs.environments.time_series_env import TimeSeriesEnv

    d = data_dir(name)
    for f in glob.glob(os.path.join(d, "*_bounds_cache.json")):
        os.remove(f)  # the cache ignores num_intervals (TSE:104-106)
    env = TimeSeriesEnv(d, "dummy", num_intervals=W, device_id=-1, **kw)
    with open(os.path.join(d, "dummy_bounds_cache.json")) as f:
        cache = json.load(f)
    return env, cache


def scale_env(env, N: int):
    """Appendix B of SURVEY.md: replicate to N envs, env n -> day n mod D."""
    D = env.price_environments.shape[0]
    W = env.num_intervals
    S = env.starting_balance
    env.env_indices = torch.arange(N) % D
    env.num_envs = N
    env.env_pointers = torch.zeros((N,), dtype=torch.int64)
    env.env_spots = torch.arange(0, W).repeat(N, 1)
    env.cash = S * torch.ones((N, 1))
    env.long_shares = torch.zeros((N, 1))
    env.short_shares = torch.zeros((N, 1))
    env.margin = torch.zeros((N, 1))
    if env.evaluate:
        env.reset_evaluation_metrics()


def write_case_csv(name, num_days, bars, seed=1234, drop=0.0, premarket=2, asset=0, num_assets=1,
                   spikes=None):
    prices, day_id, minute = synthetic.synthetic_series(num_days, num_assets, bars, seed, drop)
    if spikes:
        rng = np.random.default_rng(seed + 99)
        rows = rng.choice(prices.shape[0], size=spikes, replace=False)
        for r in rows:
            f = rng.uniform(1.3, 2.5)
            for a in range(num_assets):
                prices[r, 4 * a + 1] = np.round(prices[r, 4 * a + 1] * f, 4)  # High
                if rng.random() < 0.5:
                    prices[r, 4 * a + 3] = np.round(prices[r, 4 * a + 3] * f, 4)  # Close
    for a in range(num_assets):
        nm = name if num_assets == 1 else f"{name}_a{a}"
        synthetic.write_csv(os.path.join(data_dir(nm), "dummy.csv"), prices, day_id, minute, a, premarket)
    return prices, day_id, minute


def tables_case(fname, name, W, prices, day_id, minute):
    env, cache = make_env(name, W, evaluate=True)
    save_npz(
        os.path.join(GOLD, fname),
        W=np.int64(W),
        series_prices=prices,
        series_day_id=day_id,
        series_minute=minute,
        ref_dataset=env.dataset.numpy(),
        ref_log_return_dataset=env.log_return_dataset.numpy(),
        ref_start_indices=np.asarray(cache["start_indices"], dtype=np.int64),
        ref_stop_indices=np.asarray(cache["stop_indices"], dtype=np.int64),
        ref_max_length=np.int64(cache["max_length"]),
        ref_price_environments=env.price_environments.numpy(),
        ref_log_return_environments=env.log_return_environments.numpy(),
    )
    print(fname, tuple(env.price_environments.shape))
    return env


def real_series_of(env):
    """(day_id, minute, second) per market-hours row, from the reference's own filtered dataframe."""
    df = env.dataframe
    dates = df["Date"].values
    uniq = {s_: i for i, s_ in enumerate(dict.fromkeys(dates))}
    day_id = np.asarray([uniq[s_] for s_ in dates], dtype=np.int64)
    hms = [[int(x) for x in str(t).strip().split(":")] + [0] for t in df["Time"].values]
    second = np.asarray([h[0] * 3600 + h[1] * 60 + h[2] for h in hms], dtype=np.int64)
    return day_id, second // 60, second


def real_tables_case(inst, W, fname):
    if not os.path.isdir(data_dir(inst)):
        os.makedirs(data_dir(inst))
        shutil.copy(os.path.join(REF, "finenvs", "data", inst, "dummy.csv"), os.path.join(data_dir(inst), "dummy.csv"))
    env, cache = make_env(inst, W, evaluate=True)
    day_id, minute, second = real_series_of(env)
    save_npz(
        os.path.join(GOLD, fname),
        W=np.int64(W),
        series_prices=env.dataset.numpy(),
        series_day_id=day_id,
        series_minute=minute,
        series_second=second,
        ref_dataset=env.dataset.numpy(),
        ref_log_return_dataset=env.log_return_dataset.numpy(),
        ref_start_indices=np.asarray(cache["start_indices"], dtype=np.int64),
        ref_stop_indices=np.asarray(cache["stop_indices"], dtype=np.int64),
        ref_max_length=np.int64(cache["max_length"]),
        ref_price_environments=env.price_environments.numpy(),
        ref_log_return_environments=env.log_return_environments.numpy(),
    )
    print(fname, tuple(env.price_environments.shape))


def state_of(env):
    return dict(
        cash=env.cash.squeeze(1).numpy().copy(),
        margin=env.margin.squeeze(1).double().numpy().copy(),
        long=env.long_shares.squeeze(1).numpy().copy(),
        short=env.short_shares.squeeze(1).numpy().copy(),
        spot0=env.env_spots[:, 0].numpy().copy(),
        env_idx=env.env_indices.numpy().copy(),
    )


def rollout(env, T, action_seed=7, action_kind="uniform", stop_on_returns=False, full_obs=True):
    N = env.num_envs
    g = torch.Generator().manual_seed(action_seed)
    rec = {k: [] for k in ("actions", "rewards", "dones", "cash", "margin", "long", "short", "spot0",
                           "env_idx", "obs")}
    obs0 = env.reset()
    init = state_of(env)
    returns = None
    for t in range(T):
        if action_kind == "uniform":
            a = torch.rand((N, 1), generator=g) * 2 - 1
        elif action_kind == "bangbang":
            a = torch.where(torch.rand((N, 1), generator=g) < 0.5, -1.0, 1.0) * torch.ones((N, 1))
            hold = torch.rand((N, 1), generator=g) < 0.6
            a = torch.where(hold, torch.zeros_like(a), a)
        elif action_kind == "edge":
            a = torch.rand((N, 1), generator=g) * 2 - 1
            specials = [float("nan"), float("inf"), float("-inf"), 7.5, -123.0, -0.0, 1e-30, 0.0909090909]
            if t % 9 == 4:
                for k, sp in enumerate(specials):
                    a[(t + 3 * k) % N, 0] = sp
        else:
            raise ValueError(action_kind)
        a = a.float()
        obs, rew, done, info = env.step(a)
        st = state_of(env)
        rec["actions"].append(a.squeeze(1).numpy().copy())
        rec["rewards"].append(rew.numpy().copy())
        rec["dones"].append(done.numpy().copy())
        for k in ("cash", "margin", "long", "short", "spot0", "env_idx"):
            rec[k].append(st[k])
        rec["obs"].append(obs.numpy().copy() if full_obs else obs[:, -1, :].numpy().copy())
        if "returns" in info:
            returns = info["returns"].numpy().copy()
            if stop_on_returns:
                break
    out = {k: np.stack(v) for k, v in rec.items()}
    out["obs_reset"] = obs0.numpy().copy()
    for k, v in init.items():
        out["init_" + k] = v
    if returns is not None:
        out["returns"] = returns
    return out


def save_rollout(fname, env, roll, extra=None):
    meta = dict(
        W=np.int64(env.num_intervals),
        N=np.int64(env.num_envs),
        evaluate=np.int64(bool(env.evaluate)),
        max_shares=np.int64(env.max_shares),
        starting_balance=np.float64(env.starting_balance),
        commission=np.float64(env.per_share_commission),
        imr=np.float64(env.initial_margin_requirement),
        mmr=np.float64(env.maintenance_margin_requirement),
        prices=env.price_environments.numpy(),
        logret=env.log_return_environments.numpy(),
    )
    meta.update(roll)
    if extra:
        meta.update(extra)
    save_npz(os.path.join(GOLD, fname), **meta)
    nd = int(roll["dones"].sum())
    print(f"{fname}: steps={roll['dones'].shape[0]} N={env.num_envs} dones={nd}")


def f64_actions_case(fname="rollout_f64_actions.npz", action_seed=64, **econ):
    """step() with float64 actions: the reference computes its share changes in f64 (TSE:298-302) and REBINDS long_shares /
    short_shares to f64 tensors (TSE:353-361, 367-374) -- from then on, also under later f32 actions, the commission
    products and the liquidation fee are f64 products (TSE:363-365, 288-289).  Steps 0-59 f64 actions, 60-99 f32 actions (on
    the promoted env), 100-129 f64 again; small balance + price spikes so that every trade leg, illegal trades, margin calls
    and bankruptcies occur; a few non-finite / out-of-range actions.  `econ`: non-default economics -- with an
    initial_margin_requirement that is not exact in f32 (1.4) the promoted `imr * short_shares` product (TSE:376-379, f64 once
    short_shares is f64) differs from the f32 one."""
    if not wanted(fname):
        print("   (kept)", fname)
        return
    write_case_csv("SYN_stress64", 7, 40, seed=19, spikes=40)
    env, _ = make_env("SYN_stress64", 8, evaluate=True, **{"starting_balance": 400, **econ})
    scale_env(env, 48)
    N = env.num_envs
    g = torch.Generator().manual_seed(action_seed)
    rec = {k: [] for k in ("actions", "act_f64", "rewards", "dones", "cash", "margin", "long", "short", "spot0", "env_idx", "obs_last_row")}
    obs0 = env.reset()
    assert env.long_shares.dtype == torch.float32
    specials = [float("nan"), float("inf"), float("-inf"), 7.5, -123.0, -0.0, 1e-30, 0.0909090909, 0.09090909090909091, 0.4545454545454545]
    for t in range(130):
        f64 = t < 60 or t >= 100
        a = torch.rand((N, 1), generator=g, dtype=torch.float64) * 2 - 1
        if t % 9 == 4:
            for k, sp in enumerate(specials):
                a[(t + 3 * k) % N, 0] = sp
        a = a if f64 else a.float()
        obs, rew, done, info = env.step(a)
        if t == 0:
            assert env.long_shares.dtype == torch.float64 and env.short_shares.dtype == torch.float64  # the promotion
            assert env.cash.dtype == torch.float32 and env.commissions.dtype == torch.float32
        st = state_of(env)
        rec["actions"].append(a.double().squeeze(1).numpy().copy())  # (an f32 action is exact as an f64)
        rec["act_f64"].append(np.int64(f64))
        rec["rewards"].append(rew.numpy().copy())
        rec["dones"].append(done.numpy().copy())
        for k in ("cash", "margin", "long", "short", "spot0", "env_idx"):
            rec[k].append(np.asarray(st[k], dtype=np.float64) if k in ("long", "short") else st[k])
        rec["obs_last_row"].append(obs[:, -1, :].numpy().copy())
    roll = {k: np.stack(v) for k, v in rec.items()}
    roll["obs_reset"] = obs0.numpy().copy()
    save_rollout(fname, env, roll)


class RngLog:
    """Logs every torch.rand / torch.randint call made while active (name code, shape, low, high): the draws the reference
    takes from torch's GLOBAL generator -- which a caller seeding that generator shares with its own sampling."""

    def __enter__(self):
        self.calls = []
        self._rand, self._randint = torch.rand, torch.randint

        def rand(*size, **kw):
            shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)
            if kw.get("generator") is None:
                self.calls.append((0, shape[0], shape[1] if len(shape) > 1 else -1, 0, 0))
            return self._rand(*size, **kw)

        def randint(*args, **kw):
            low, high, shape = (0, args[0], args[1]) if len(args) == 2 else args[:3]
            if kw.get("generator") is None:
                self.calls.append((1, tuple(shape)[0], -1, int(low), int(high)))
            return self._randint(*args, **kw)

        torch.rand, torch.randint = rand, randint
        return self

    def __exit__(self, *exc):
        torch.rand, torch.randint = self._rand, self._randint


def rng_calls_case():
    """Which draws the reference takes from torch's global generator, and when: at construction one torch.rand per day
    that needs NaN padding (TSE:207-210) and one torch.randint for the evaluation env's first day (TSE:253-255); per
    step one torch.randint exactly when the evaluation env finished (TSE:510-513).  Ragged days (bars dropped), native
    training mode (N = D + 1).  The build's redraw="torch" mode must make the same calls in the same order -- a caller who
    seeds the global generator then sees the same stream position after any number of steps."""
    fname = "rng_calls.npz"
    if not wanted(fname):
        print("   (kept)", fname)
        return
    prices, day_id, minute = write_case_csv("SYN_rng", 9, 40, seed=77, drop=0.15)
    torch.manual_seed(4242)
    with RngLog() as log:
        env, _ = make_env("SYN_rng", 8)
    construct = np.asarray(log.calls, dtype=np.int64).reshape(-1, 5)
    N = env.num_envs
    g = torch.Generator().manual_seed(3)
    acts, step_calls, eval_done, env_idx, rewards, dones = [], [], [], [], [], []
    init_env_idx = env.env_indices.numpy().copy()
    for t in range(260):
        a = (torch.rand((N, 1), generator=g) * 2 - 1).float()
        with RngLog() as log:
            _, rew, done, _ = env.step(a)
        acts.append(a.squeeze(1).numpy().copy())
        step_calls.append(np.asarray(log.calls, dtype=np.int64).reshape(-1, 5))
        eval_done.append(int(done[-1]))
        env_idx.append(env.env_indices.numpy().copy())
        rewards.append(rew.numpy().copy()); dones.append(done.numpy().copy())
    n_calls = np.asarray([c.shape[0] for c in step_calls], dtype=np.int64)
    assert (n_calls == np.asarray(eval_done)).all() and n_calls.sum() >= 5
    save_npz(os.path.join(GOLD, fname), W=np.int64(8), N=np.int64(N), series_prices=prices, series_day_id=day_id,
             construct_calls=construct, step_call_counts=n_calls,
             step_calls=np.concatenate([c for c in step_calls if c.shape[0]], axis=0),
             actions=np.stack(acts), eval_done=np.asarray(eval_done, dtype=np.int64), init_env_idx=init_env_idx,
             env_idx=np.stack(env_idx), rewards=np.stack(rewards), dones=np.stack(dones),
             call_columns=np.asarray([0, 1, 2, 3, 4], dtype=np.int64))  # (kind 0 rand / 1 randint, shape[0], shape[1] or -1, low, high)
    print(fname, "construction calls", construct.tolist(), "step redraws", int(n_calls.sum()))


def agent_stats_case():
    """Runs the reference's own PPOAgent.store / log_progress (PPO_agent.py:110-168) -- without its networks --
    on a reference training rollout and records what they compute: the running return per env after every
    step, and at every log point the evaluation return, the number of finished training episodes and their
    mean / std."""
    import finenvs.agents.PPO.PPO_agent as agmod

    class _NoBuffer:  # the trajectory half of store() is not what is pinned here
        def __init__(self):
            self.n = 0

        def store(self, *a):
            self.n += 1

        def size(self):
            return self.n

    agent = object.__new__(agmod.PPOAgentMLP)
    torch.manual_seed(99)
    env, _ = make_env("SYN_stress", 8, starting_balance=800)
    scale_env(env, 40)
    N = env.num_envs
    agent.num_envs = N
    agent.device = "cpu"
    agent.buffer = _NoBuffer()
    agent.current_returns = torch.zeros((N,))
    agent.training_returns = torch.zeros((0, 1))
    agent.evaluation_return = None
    agent.num_samples = 0
    agent.num_steps = 0
    agent.save_interval = 0
    agent.write_to_csv = False
    g = torch.Generator().manual_seed(17)
    T, LOG_EVERY = 160, 20
    rec = {k: [] for k in ("actions", "rewards", "dones", "env_idx", "running")}
    logs = []
    init = state_of(env)
    env.reset()
    for t in range(T):
        a = (torch.rand((N, 1), generator=g) * 2 - 1).float()
        obs, rew, done, _ = env.step(a)
        agent.store(obs, a, rew, done, torch.zeros((N, 1)), torch.zeros((N, 1)))
        rec["actions"].append(a.squeeze(1).numpy().copy())
        rec["rewards"].append(rew.numpy().copy())
        rec["dones"].append(done.numpy().copy())
        rec["env_idx"].append(env.env_indices.numpy().copy())
        rec["running"].append(agent.current_returns.numpy().copy())
        if (t + 1) % LOG_EVERY == 0:
            tr = agent.training_returns.clone()
            ev = agent.evaluation_return
            logged = agent.log_progress()
            logs.append((t, -1.0 if ev is None else float(ev), float(ev is not None), float(tr.shape[0]),
                         float(tr.mean().item()) if tr.numel() else float("nan"),
                         float(tr.std().item()) if tr.numel() > 1 else float("nan"), float(bool(logged))))
    save_npz(
        os.path.join(GOLD, "agent_stats.npz"),
        W=np.int64(8), N=np.int64(N), starting_balance=np.float64(800), torch_seed=np.int64(99),
        prices=env.price_environments.numpy(), logret=env.log_return_environments.numpy(),
        init_env_idx=init["env_idx"],
        log_every=np.int64(LOG_EVERY),
        # columns: step, evaluation_return, has_evaluation_return, num_training_episodes, mean, std, logged
        logs=np.asarray(logs, dtype=np.float64),
        **{k: np.stack(v) for k, v in rec.items()},
    )
    print("agent_stats.npz logs:", [(int(l[0]), int(l[3])) for l in logs])


def lstm_actor_case():
    """Runs the reference's own actor network of the time-series scripts -- ContinuousActorLSTM(shape=(5, H, 1),
    sequence_length=W) (finenvs/agents/PPO/continuous_actor.py:104-126 over finenvs/agents/networks/lstm.py:7-57) --
    on observations the reference env produced, exactly as examples/time_series/PPO_LSTM_testing_SPY.py:46 calls it
    (``test_actor.forward(states.float())``), and records inputs, parameters and the actions it returned.  Pins the
    LSTM head of the fused rollout (fo_policy_lstm / fe_env_rollout_lstm) at the tolerance stated in the tests."""
    from finenvs.agents.PPO.continuous_actor import ContinuousActorLSTM

    out = {}
    for tag, H, W, steps in (("h128_w4", 128, 4, 12), ("h32_w8", 32, 8, 6)):
        torch.manual_seed(4242 + H)
        actor = ContinuousActorLSTM(shape=(5, H, 1), sequence_length=W)
        with torch.no_grad():  # default init is tiny against log-returns of 1e-3: scale so that the gates move
            actor.lstm.weight_ih_l0[:, :4].mul_(60.0 * np.sqrt(H))
            actor.lstm.weight_ih_l0[:, 4].mul_(4.0)
            actor.last_layer[0].weight.mul_(6.0)
        env, _ = make_env("SYN_stress", W, starting_balance=800, evaluate=True)
        states = env.reset()
        obs, acts = [], []
        for _ in range(steps):
            actions = actor.forward(states.float()).detach()
            obs.append(states.numpy().copy())
            acts.append(actions.numpy().copy())
            states, _, _, _ = env.step(actions)
        sd = {k: v.detach().numpy().copy() for k, v in actor.state_dict().items()}
        out.update({f"{tag}_obs": np.stack(obs), f"{tag}_actions": np.stack(acts), f"{tag}_H": np.int64(H),
                    f"{tag}_W": np.int64(W), f"{tag}_weight_ih": sd["lstm.weight_ih_l0"],
                    f"{tag}_weight_hh": sd["lstm.weight_hh_l0"], f"{tag}_bias_ih": sd["lstm.bias_ih_l0"],
                    f"{tag}_bias_hh": sd["lstm.bias_hh_l0"], f"{tag}_weight_out": sd["last_layer.0.weight"],
                    f"{tag}_bias_out": sd["last_layer.0.bias"]})
        a = np.stack(acts)
        print(f"lstm_actor {tag}: obs {np.stack(obs).shape} actions std {a.std():.3f} range [{a.min():.3f}, {a.max():.3f}]")
    save_npz(os.path.join(GOLD, "lstm_actor.npz"), **out)


def sleeves_case(fname, name, A, N, W, T, days, bars, csv_seed, action_seed, full_obs, f64_from=None, starting_balance=10000):
    """The multi-asset "sleeve" contract pinned to the reference: A reference
    envs (one per asset, same calendar) stepped side by side on column a of one (N, A) action tensor.  Observation =
    their observations concatenated along the feature axis (asset a in columns 5a..5a+4, TSE:423-445), reward = their
    rewards added in asset order (f64), done = their common done flag."""
    if not wanted(fname):
        print("   (kept)", fname)
        return
    write_case_csv(name, days, bars, seed=csv_seed, num_assets=A)
    envs = []
    for a in range(A):
        e, _ = make_env(f"{name}_a{a}", W, evaluate=True, starting_balance=starting_balance)
        scale_env(e, N)
        envs.append(e)
    g = torch.Generator().manual_seed(action_seed)
    act_f64 = []
    acts, rews, dones, obss, last_rows, full_steps = [], [], [], [], [], []
    st = {k: [] for k in ("cash", "margin", "long", "short", "spot0")}
    obs0 = torch.cat([e.reset() for e in envs], dim=2)
    for t in range(T):
        if f64_from is not None and t >= f64_from and (t - f64_from) % 9 < 5:
            # float64 actions: every side-by-side reference promotes its share tensors (TSE:353-374); f32 steps in between
            a = torch.rand((N, A), generator=g, dtype=torch.float64) * 2 - 1
        else:
            a = (torch.rand((N, A), generator=g) * 2 - 1).float()
        act_f64.append(np.int64(a.dtype == torch.float64))
        o_l, r_l, d_l = [], [], []
        for k, e in enumerate(envs):
            # evaluate mode keeps the RNG redraw out of it; clearing the metrics before each
            # step keeps TSE:526-528 from zeroing rewards of already-terminated envs
            e.reset_evaluation_metrics()
            o, r, dn, _ = e.step(a[:, k : k + 1].contiguous())
            o_l.append(o); r_l.append(r); d_l.append(dn)
        assert all(torch.equal(d_l[0], x) for x in d_l), "sleeves must finish together in this fixture"
        r = r_l[0]
        for x in r_l[1:]:
            r = r + x  # sequential sum in asset order, f64
        acts.append(a.double().numpy().copy() if f64_from is not None else a.numpy().copy())
        rews.append(r.numpy().copy()); dones.append(d_l[0].numpy().copy())
        obs = torch.cat(o_l, dim=2).numpy().copy()
        if full_obs or t < 3 or bool(d_l[0].any()) or t == T - 1:
            full_steps.append(t)
            obss.append(obs)
        last_rows.append(obs[:, -1, :].copy())
        for k2 in st:
            col = np.stack([state_of(e)[k2] for e in envs], axis=1)
            st[k2].append(col.astype(np.float64) if (f64_from is not None and k2 in ("long", "short")) else col)
    extra = {} if full_obs else {"obs_steps": np.asarray(full_steps, dtype=np.int64), "obs_last_row": np.stack(last_rows)}
    if f64_from is not None:
        extra["act_f64"] = np.asarray(act_f64)
    save_npz(
        os.path.join(GOLD, fname),
        W=np.int64(W), N=np.int64(N), A=np.int64(A), evaluate=np.int64(1),
        max_shares=np.int64(5), starting_balance=np.float64(starting_balance), commission=np.float64(0.01),
        imr=np.float64(1.5), mmr=np.float64(0.25),
        prices=np.concatenate([e.price_environments.numpy() for e in envs], axis=2),
        logret=np.concatenate([e.log_return_environments.numpy() for e in envs], axis=2),
        actions=np.stack(acts), rewards=np.stack(rews), dones=np.stack(dones), obs=np.stack(obss),
        obs_reset=obs0.numpy(), init_env_idx=(np.arange(N) % envs[0].price_environments.shape[0]),
        **{k2: np.stack(v) for k2, v in st.items()}, **extra,
    )
    print(fname, "dones=", int(np.stack(dones).sum()), "full observations at", len(full_steps), "steps")


def main():
    os.makedirs(GOLD, exist_ok=True)
    setup_reference()

    # ---------------- tables (a18-a20) ----------------
    p, d, m = write_case_csv("SYN_full", 5, 40)
    tables_case("tables_full.npz", "SYN_full", 8, p, d, m)
    p, d, m = write_case_csv("SYN_ragged", 7, 40, seed=77, drop=0.10)
    tables_case("tables_ragged.npz", "SYN_ragged", 8, p, d, m)
    p, d, m = write_case_csv("SYN_skip2", 6, 40, seed=5)
    tables_case("tables_skip2.npz", "SYN_skip2", 50, p, d, m)
    # real data: the reference's own three fixtures (tests/unit/test_time_series_env.py:10-14); the
    # market-hours rows the reference's pandas parse kept are stored as plain arrays
    for inst, W, fname in (("OIH", 32, "tables_oih.npz"), ("IBM", 390, "tables_ibm.npz"), ("SPY", 390, "tables_spy.npz"),
                           ("IBM", 4, "tables_ibm_w4.npz"), ("SPY", 4, "tables_spy_w4.npz")):
        real_tables_case(inst, W, fname)
    # the three data files themselves, byte for byte: the native reader's input in tests/test_csv_native.py
    save_npz(os.path.join(GOLD, "csv_reference_files.npz"),
             **{inst: np.frombuffer(open(os.path.join(REF, "finenvs", "data", inst, "dummy.csv"), "rb").read(), dtype=np.uint8)
                for inst in ("OIH", "IBM", "SPY")})

    # ---------------- rollouts (a2-a17) ----------------
    write_case_csv("SYN_roll", 7, 40, seed=1234)
    # native training mode: N = D + 1, eval env redraws from torch's global generator
    torch.manual_seed(123)
    env, _ = make_env("SYN_roll", 8)
    roll = rollout(env, 150)
    save_rollout("rollout_train_native.npz", env, roll, {"torch_seed": np.int64(123)})

    # replicated to N = 64 (training mode; last env redraws)
    torch.manual_seed(321)
    env, _ = make_env("SYN_roll", 8)
    scale_env(env, 64)
    roll = rollout(env, 150)
    save_rollout("rollout_train_n64.npz", env, roll, {"torch_seed": np.int64(321)})

    # evaluate mode, native N = D, until info["returns"] appears
    env, _ = make_env("SYN_roll", 8, evaluate=True)
    roll = rollout(env, 400, stop_on_returns=True)
    assert "returns" in roll
    save_rollout("rollout_eval.npz", env, roll)

    # evaluate mode on ragged days: envs terminate at different steps, so rewards of
    # terminated envs get zeroed while others still run (TSE:526-528)
    write_case_csv("SYN_rag_roll", 8, 40, seed=42, drop=0.15)
    env, _ = make_env("SYN_rag_roll", 8, evaluate=True)
    roll = rollout(env, 400, stop_on_returns=True)
    assert "returns" in roll
    save_rollout("rollout_eval_ragged.npz", env, roll)

    # stress: small balances + price spikes -> illegal long/short, margin call, bankruptcy
    write_case_csv("SYN_stress", 7, 40, seed=9, spikes=40)
    for bal in (60, 150, 400, 1500):
        env, _ = make_env("SYN_stress", 8, starting_balance=bal, evaluate=True)
        scale_env(env, 48)
        roll = rollout(env, 120, action_seed=1000 + bal, action_kind="bangbang" if bal in (60, 1500) else "uniform")
        save_rollout(f"rollout_stress_{bal}.npz", env, roll)
    # non-default economics
    env, _ = make_env("SYN_stress", 8, starting_balance=2500.0, max_shares=9, per_share_commission=0.035,
                      initial_margin_requirement=1.4, maintenance_margin_requirement=0.3, evaluate=True)
    scale_env(env, 48)
    roll = rollout(env, 120, action_seed=5)
    save_rollout("rollout_econ.npz", env, roll)

    # real data: OIH, ragged NaN-padded days
    torch.manual_seed(2024)
    env, _ = make_env("OIH", 32)
    roll = rollout(env, 700, full_obs=False)
    save_rollout("rollout_oih.npz", env, roll, {"torch_seed": np.int64(2024)})

    # the reference's other two fixtures, at the default window (TSE:19) and at the example's
    # (examples/time_series/PPO_LSTM_training_SPY.py:8); native training mode (N = D + 1, eval env redraws)
    for inst, W, T, seed in (("IBM", 390, 900, 11), ("SPY", 390, 900, 12), ("IBM", 4, 900, 13), ("SPY", 4, 900, 14)):
        fname = f"rollout_{inst.lower()}_w{W}.npz"
        if not wanted(fname):
            print("   (kept)", fname)
            continue
        torch.manual_seed(seed)
        env, _ = make_env(inst, W)
        roll = rollout(env, T, action_seed=100 + seed, full_obs=False)
        roll["obs_reset"] = roll["obs_reset"][:, -1, :]  # last row only (W=390 windows are large)
        save_rollout(fname, env, roll, {"torch_seed": np.int64(seed), "obs_reset_last_row_only": np.int64(1)})

    # edge-case actions: NaN, +-inf, out-of-range, -0.0 (a diverged policy must not crash or desync parity)
    env, _ = make_env("SYN_roll", 8, evaluate=True, starting_balance=3000)
    scale_env(env, 24)
    roll = rollout(env, 90, action_seed=77, action_kind="edge")
    save_rollout("rollout_edge_actions.npz", env, roll)

    # float64 actions: the reference's dtype promotion of its share tensors (missing #3 of VERDICT round 3)
    f64_actions_case()
    # ... with economics whose imr / commission are not exact in f32 (advisor finding of round 4: imr * short_shares is an f64
    # product on the promoted env)
    f64_actions_case("rollout_f64_actions_econ.npz", action_seed=65, starting_balance=700.0, max_shares=9, per_share_commission=0.035,
                     initial_margin_requirement=1.4, maintenance_margin_requirement=0.3)
    # the global-generator draws of the training mode, as a call log (weak #1 (ii) of VERDICT round 3)
    rng_calls_case()

    # ---------------- multi-asset sleeve contract: A reference envs side by side ----------------
    sleeves_case("rollout_sleeves3.npz", "SYN_multi", A=3, N=20, W=8, T=70, days=6, bars=40, csv_seed=31, action_seed=11, full_obs=True)
    # BASELINE configs 3-5 are 30-asset portfolios: the (N, W, 150) observation layout, reward = sum in asset order and the
    # shared done flag of that shape against 30 reference envs on one calendar (crosses a day end; no bankruptcies, so the
    # side-by-side references stay in step).  Full observations at a few steps, the newest window row at every step.
    sleeves_case("rollout_sleeves30.npz", "SYN_multi30", A=30, N=9, W=8, T=64, days=5, bars=40, csv_seed=47, action_seed=29, full_obs=False)
    # the sleeve contract under the reference's f64 promotion: three reference envs side by side, float64 actions from step 3 on
    # in runs of five with float32 steps between them (actions stored as f64 + the per-step dtype flag)
    sleeves_case("rollout_sleeves3_f64.npz", "SYN_multi", A=3, N=20, W=8, T=70, days=6, bars=40, csv_seed=31, action_seed=12, full_obs=False,
                 f64_from=3, starting_balance=3000)

    # ---------------- rounding probes (a3) ----------------
    env, _ = make_env("SYN_roll", 8, evaluate=True)
    probes = np.asarray(
        [0.5 / 5.5, -0.5 / 5.5, 1.5 / 5.5, 2.5 / 5.5, -2.5 / 5.5, 3.5 / 5.5, 4.5 / 5.5, 5.4999 / 5.5,
         1.0, -1.0, 0.99999994, -0.2, 0.0, -0.0, 0.09090909, 0.0909091, 0.27272728, 0.45454547,
         0.6363636, 0.8181818, 1e-9, -1e-9, 0.9090909, 0.90909094, 1.5, -3.0],
        dtype=np.float32,
    )
    sc = env.get_share_changes_from_actions(torch.from_numpy(probes).unsqueeze(1)).squeeze(1).numpy()
    env9, _ = make_env("SYN_roll", 8, evaluate=True, max_shares=9)
    sc9 = env9.get_share_changes_from_actions(torch.from_numpy(probes).unsqueeze(1)).squeeze(1).numpy()
    # f32 (op)= f64 in place: computed in f64, rounded ONCE on store (the dtype rule every cash update of
    # TSE:353-475 relies on), e.g. 1f += 2^-24 + 2^-50 -> 1.00000012 (ties would give 1.0)
    rng = np.random.default_rng(5)
    base = np.concatenate([np.asarray([1.0, 1.0, 1.0, 10000.0, 9999.9990234375, 16777216.0, -0.0, 1e-38], dtype=np.float32),
                           rng.uniform(-2e4, 2e4, 56).astype(np.float32)])
    delta = np.concatenate([np.asarray([2.0 ** -24 + 2.0 ** -50, 2.0 ** -24, 2.0 ** -24 - 2.0 ** -60, 0.00048828125 + 1e-13,
                                        0.0009765625 / 2, 1.0 + 2.0 ** -30, 0.0, 1e-46], dtype=np.float64),
                            rng.uniform(-700, 700, 56) * (1 + rng.uniform(-1e-9, 1e-9, 56))])
    x = torch.from_numpy(base.copy())
    x += torch.from_numpy(delta)  # f32 += f64
    y = torch.from_numpy(base.copy())
    y -= torch.from_numpy(delta)  # f32 -= f64
    assert x.dtype == torch.float32 and float(x[0]) == float(np.float32(1.00000012))
    save_npz(os.path.join(GOLD, "rounding.npz"), actions=probes, share_changes_ms5=sc, share_changes_ms9=sc9,
             f32_base=base, f64_delta=delta, f32_iadd_f64=x.numpy(), f32_isub_f64=y.numpy())
    print("rounding.npz", sc.tolist())

    # ---------------- f1: PPO buffer discounted returns (buffer.py:80-100) ----------------
    from finenvs.agents.PPO.buffer import Buffer

    import finenvs.agents.PPO.buffer as bufmod
    bufmod.set_device = lambda device_id: "cpu"
    T, N = 24, 10
    g = torch.Generator().manual_seed(3)
    buf = Buffer(gamma=0.99, device_id=-1)
    rew = torch.randn((T, N), generator=g, dtype=torch.float64)
    done = (torch.rand((T, N), generator=g) < 0.15).int()
    val = torch.randn((T, N, 1), generator=g)
    last = torch.randn((N, 1), generator=g)
    for t in range(T):
        buf.store(torch.zeros((N, 2, 5), dtype=torch.float64), torch.zeros((N, 1)), rew[t], done[t],
                  torch.zeros((N, 1)), val[t])
    buf.compute_returns_and_advantages(last)
    save_npz(
        os.path.join(GOLD, "ppo_returns.npz"),
        gamma=np.float64(0.99), rewards=rew.numpy(), dones=done.numpy(), values=val.squeeze(-1).numpy(),
        last_values=last.squeeze(-1).numpy(),
        returns=buf.container["returns"].squeeze(-1).numpy().T.copy(),       # (T, N)
        advantages=buf.container["advantages"].squeeze(-1).numpy().T.copy(),  # (T, N)
    )
    print("ppo_returns.npz", buf.container["returns"].dtype, buf.container["advantages"].dtype)

    # ---------------- f4: the agents' return bookkeeping (PPO_agent.py:110-168) ----------------
    if wanted("agent_stats.npz"):
        agent_stats_case()

    # ---------------- f2: the LSTM actor of the time-series scripts (lstm.py, continuous_actor.py) ----------------
    if wanted("lstm_actor.npz"):
        lstm_actor_case()

    # the reference tree must be untouched
    dirty = [p for p in glob.glob(os.path.join(REF, "finenvs", "data", "*", "*.json"))]
    assert not dirty, dirty
    tot = sum(os.path.getsize(f) for f in glob.glob(os.path.join(GOLD, "*.npz")))
    print(f"golden fixtures: {tot/1e6:.2f} MB")


if __name__ == "__main__":
    main()
