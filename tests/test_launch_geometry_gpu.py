"""GPU: kernel results do not depend on the launch geometry.  Every test pushes small, oracle-sized problems into the
regimes that the automatic geometry reaches only at full size -- several tiles per workgroup, grid-strided tile loops,
ragged and single-env tiles, grids that are not multiples of 8 or exceed the tile count, the U = 1 returns scan -- and
compares bit for bit with the C oracle (oracle/fe_oracle.c), as the rest of the suite does at the automatic geometry.
The override runs must also equal the automatic run exactly.  Tolerances are those of the existing tests of the same
kernel: MLP ELU actions 2e-6, evo actions 1e-5, evo2 actions ``ACTION_TOL`` of tests/test_evo2_rollout_gpu.py.

The rollouts that SAMPLE (section 2b: fe_rollout_mlp_sampled_kernel, fe_rollout_mlp2_sampled_kernel,
fe_rollout_mlp_sac_kernel, fe_rollout_sac_kernel, fe_rollout_sac_big_kernel) take a (K, N, A) noise tensor indexed by
``(k, n0 + ee, aa)`` and compare ``n0 + ee`` with the evaluation env: their override runs equal the automatic run and the
oracle env bit for bit, ``forward`` on the trajectory's rows returns what ``run`` recorded, only the evaluation env acts on
its mean, and the recorded means meet the f64 torch forward within ``2e-5 max|x64| + 4 max|x32_torch - x64|``
(tests/test_mlp_sac_gpu.py::_bound).  fe_evo2_rollout_kernel walks a second tile at N = 40 000 and, with A = 17, at 28 663.
"""
import copy
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from tests.helpers import assert_bits

pytestmark = pytest.mark.gpu


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


def _tables(fo, num_days, A, bars, W, seed=1234, drop=0.0):
    from finenvs_amd.data import synthetic

    prices, day_id, _ = synthetic.synthetic_series(num_days, A, bars, seed, drop)
    P, LR, *_ = fo.tables_from_series(prices, day_id, W)
    return P, LR


def _cdiv(a, b):
    return (a + b - 1) // b


def _num_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _chunked(policy, obs, *args, **kw):
    """An oracle policy on env chunks in parallel threads: each env's action depends on its own observation only, so the
    result is the single call's, bit for bit (the ctypes call releases the GIL)."""
    parts = np.array_split(np.arange(obs.shape[0]), 8)
    with ThreadPoolExecutor(8) as ex:
        outs = list(ex.map(lambda ix: policy(obs[ix[0]:ix[-1] + 1], *args, **kw), [p for p in parts if p.size]))
    return np.concatenate(outs)


# ----------------------------------------------------------------------------- 1. step kernel geometry matrix
# form: lean = fe_env_step (redraw="device", no outputs); full = fe_env_step_traj (descriptors_out, actions_out);
# notify = fe_env_step_notify (redraw="torch": reverse tile walk); fullnotify = evaluate mode (host flag, evaluate
# bookkeeping, reverse walk); promo / promo_notify = fe_env_step_promoted with f64 actions (training / evaluate mode).
STEP_CASES = [
    # id, N, A, W, f32, form, tile_envs, grid -- vec width in the id
    ("f64x2-lean-38tiles-grid8", 301, 1, 8, False, "lean", 8, 8),         # 4-5 tiles per workgroup, ragged last (5 envs)
    ("f64x1-notify-tile7-grid3", 301, 1, 5, False, "notify", 7, 3),       # 14-15 tiles per workgroup, reverse walk, ragged first
    ("f32x4-full-tile1-grid13", 257, 1, 8, True, "full", 1, 13),          # single-env tiles, grid not a multiple of 8
    ("f32x2-fullnotify-tile3-grid16", 150, 1, 6, True, "fullnotify", 3, 16),
    ("f32x1-lean-grid>tiles", 100, 1, 5, True, "lean", 64, 16),            # 2 tiles, 14 idle workgroups
    ("f64x1-A3-notify-tile7-grid5", 200, 3, 7, False, "notify", 7, 5),   # multi-asset tile loop, reverse walk
    ("f32x4-A3-full-tile1-grid13", 123, 3, 4, True, "full", 1, 13),
    ("f64x2-A30-fullnotify-tile3-grid8", 97, 30, 4, False, "fullnotify", 3, 8),
    ("f32x2-A2-lean-grid>tiles", 700, 2, 3, True, "lean", 13, 64),
    ("f64x2-promo-pipeline-tile7-grid3", 301, 1, 8, False, "promo", 7, 3),
    ("f64x1-promo-pipeline-notify-tile8-grid5", 150, 1, 5, False, "promo_notify", 8, 5),
    ("f32x4-promo-tileloop-tile3-grid13", 200, 1, 8, True, "promo", 3, 13),
    ("f64x2-A3-promo-tileloop-notify-tile1-grid8", 120, 3, 4, False, "promo_notify", 1, 8),
]


@pytest.mark.parametrize("cid,N,A,W,f32,form,tile,grid", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_step_kernel_results_do_not_depend_on_tile_or_grid(fe, fo, cid, N, A, W, f32, form, tile, grid):
    """fe_env_kernel / fe_env_promoted_kernel under set_launch(tile_envs=, grid=): the single-asset software pipeline
    across 3+ tiles per workgroup (prefetch of the next tile's state and the action two tiles ahead), the notify forms'
    reverse walk with the ragged last tile first, the multi-asset tile loop, single-env tiles, tiles that are not a whole
    phase-2 iteration, grids that are not multiples of 8 or exceed the tile count; reset() (RESET_ONLY) and render()
    after the override.  obs, rewards, dones, account state, spot and day equal the oracle's at every step, across
    episode ends, and the automatic-geometry env's exactly."""
    evaluate = form in ("fullnotify", "promo_notify")
    redraw = "torch" if form == "notify" else "device"
    promoted = form.startswith("promo")
    P, LR = _tables(fo, 5, A, 24, W, seed=N + 7 * A + W, drop=0.05)
    D = P.shape[0]
    idx = (np.arange(N) * 7 + 3) % D
    kw = dict(num_intervals=W, evaluate=evaluate, starting_balance=900)
    ref = fo.OracleEnv(P, LR, env_indices=idx, obs_f32=f32, redraw_mode=1 if redraw == "device" else 0, seed=99, **kw)
    ref.redraw_counter[0] = 1  # the envs used draw 0 for the eval env's first day
    mk = lambda: fe.TimeSeriesEnv(tables=(P, LR), env_indices=idx, redraw=redraw, seed=99,  # noqa: E731
                                  obs_dtype=torch.float32 if f32 else torch.float64, obs_buffers=0, **kw)
    auto, env = mk(), mk()
    if redraw == "torch":  # each construction drew the eval env's first day from torch's generator: use auto's
        from finenvs_amd import _lib

        _lib.check(env._lib.fe_env_set_day(env._handle, N - 1, int(auto.env_indices[-1]), env._stream()))
        ref.set_day(N - 1, int(auto.env_indices[-1]))
    assert (env._flag is not None) == (form in ("notify", "fullnotify", "promo_notify"))
    before = env.launch_info()
    info = env.set_launch(tile_envs=tile, grid=grid)
    assert info["tile_envs"] == tile and info["grid"] == grid, info  # the override is in effect
    assert (before["tile_envs"], before["grid"]) != (tile, grid)
    num_tiles = _cdiv(N, tile)
    assert num_tiles >= 3 * grid or grid > num_tiles, "3+ tiles per workgroup, or idle workgroups"

    def check_reset(what):
        want = ref.reset().copy()
        assert_bits(t2n(env.reset()), want, what + " reset() obs")
        assert_bits(t2n(auto.reset()), want, what + " reset() obs, automatic geometry")
        src, pos = env.describe()
        assert_bits(t2n(env.render(src, pos)), want, what + " render(describe())")

    check_reset("initial")
    g = torch.Generator().manual_seed(N * 31 + W)
    outs = lambda e: (torch.empty((N,), dtype=torch.int64, device=e.device),  # noqa: E731
                      torch.empty((N, A), dtype=torch.float64, device=e.device))
    ndone = nret = 0
    for t in range(60):  # 24-bar days: every env crosses two or more episode ends
        if promoted:
            a = torch.rand((N, A), generator=g, dtype=torch.float64) * 2.4 - 1.2
        else:
            a = (torch.rand((N, A), generator=g) * 2.4 - 1.2).float()
        if t % 7 == 3:
            a = torch.sign(a)  # max-size trades
        o_r, r_r, d_r, i_r = ref.step(a.numpy())
        res = []
        for e in (env, auto):
            step_kw = {}
            if form == "full" or (form in ("fullnotify", "promo", "promo_notify") and t % 3 == 1):
                step_kw["descriptors_out"] = outs(e)
            if form == "full":
                step_kw["actions_out"] = torch.empty((N, A), dtype=torch.float32, device=e.device)
            rng = torch.cuda.get_rng_state(e.device)
            o, r, d, i = e.step(a.to(e.device), **step_kw)
            if e is env:
                torch.cuda.set_rng_state(rng, e.device)  # the torch-redraw envs draw the same eval-env day
            res.append((o, r, d, i, step_kw))
        if redraw == "torch":
            ref.set_day(N - 1, int(env.env_indices[-1]))
        what = f"{cid} step {t}"
        (o, r, d, i, step_kw), (o2, r2, d2, i2, _) = res
        assert_bits(t2n(o), o_r, what + " obs")
        assert_bits(t2n(r), r_r, what + " rewards")
        assert_bits(t2n(d), d_r, what + " dones")
        assert_bits(t2n(env.cash), ref.cash, what + " cash")
        assert_bits(t2n(env.margin), ref.margin, what + " margin")
        assert_bits(t2n(env.long_shares).astype(ref.long.dtype), ref.long, what + " long")
        assert_bits(t2n(env.short_shares).astype(ref.short.dtype), ref.short, what + " short")
        assert_bits(t2n(env.env_spots[:, 0]), ref.spot0, what + " spot0")
        assert_bits(t2n(env.env_indices), ref.env_idx, what + " env_idx")
        assert ("returns" in i) == ("returns" in i_r)
        if "returns" in i:
            assert_bits(t2n(i["returns"]), i_r["returns"], what + " returns")
            assert_bits(t2n(i2["returns"]), i_r["returns"], what + " returns, automatic geometry")
            nret += 1
        for x, y, name in ((o, o2, "obs"), (r, r2, "rewards"), (d, d2, "dones"), (env.cash, auto.cash, "cash"),
                           (env.margin, auto.margin, "margin"), (env.long_shares, auto.long_shares, "long"),
                           (env.env_spots[:, 0], auto.env_spots[:, 0], "spot0"), (env.env_indices, auto.env_indices, "env_idx")):
            assert_bits(t2n(x), t2n(y), f"{what} {name}: override vs automatic geometry")
        if "descriptors_out" in step_kw:
            assert_bits(t2n(env.render(*step_kw["descriptors_out"])), t2n(o), what + " render(descriptors_out)")
        if "actions_out" in step_kw:
            assert torch.equal(step_kw["actions_out"], a.to(env.device)), what + " actions_out"
        ndone += int(d_r.sum())
        if t in (17, 41):
            check_reset(what)
    assert ndone > N, "the run must cross episode ends"
    assert not evaluate or nret >= 1
    assert env.shares_promoted == promoted
    assert env.launch_info()["grid"] == grid and env.launch_info()["tile_envs"] == tile


# ----------------------------------------------------------------------------- 2. fused rollouts in the tile loop
def _rollout_envs(fe, fo, N, A, W, tiles, seed, days=6, bars=14, evaluate=False, stagger=False):
    """Oracle, automatic-geometry env and one env per rollout_tile_envs override, all on the same tables and days.
    ``stagger`` (full days, no dropped bars): env n starts at the row of its day from which 1 + 7 n mod 12 steps are left
    (tests/test_evo2_rollout_gpu.py::_stagger), so that a run of a few steps crosses episode ends in most envs."""
    P, LR = _tables(fo, days, A, bars, W, seed=seed, drop=0.0 if stagger else 0.05)
    D = P.shape[0]
    idx = (np.arange(N) * 7 + 1) % D
    kw = dict(num_intervals=W, evaluate=evaluate, starting_balance=2000)
    ref = fo.OracleEnv(P, LR, env_indices=idx, redraw_mode=1, seed=9, auto_emit=False, nthreads=8, **kw)
    ref.redraw_counter[0] = 1
    first = bars - (1 + (7 * np.arange(N)) % min(bars, 12))
    if stagger:
        ref.spot0[:] = first
    envs = []
    for tile in (0,) + tuple(tiles):
        env = fe.TimeSeriesEnv(tables=(P, LR), env_indices=idx, redraw="device", seed=9, obs_buffers=0, **kw)
        if stagger:
            env.env_spots = torch.as_tensor(first).unsqueeze(1) + torch.arange(W)
        if tile:
            step_geometry = env.launch_info()
            assert env.set_launch(rollout_tile_envs=tile) == step_geometry, "the step kernel's geometry stays automatic"
        envs.append(env)
    return P, LR, ref, envs


def _lockstep(ref, envs, rolls, policy, K, reps, what, atol=0.0, before_step=None, after_step=None):
    """The pattern of test_mlp_rollout_relu_equals_oracle_loop_bit_for_bit: every roll runs K steps per launch, the oracle
    steps with policy(obs).  atol > 0: the device's actions are within atol of the oracle's and the oracle steps with
    the automatic run's actions (lock-step); everything else is bit for bit.  Every run equals the automatic one
    (rolls[0]) exactly.  before_step(ref) / after_step(obs) track what a policy needs besides the observation."""
    obs = ref.reset().copy()
    for roll in rolls:
        assert_bits(t2n(roll.observation()), obs, what + " initial obs")
    ndone = 0
    for rep in range(reps):
        res = [roll.run(K) for roll in rolls]
        for k in range(K):
            a_ref = policy(obs)
            if atol > 0:
                a_dev = t2n(res[0][0][k])
                np.testing.assert_allclose(a_dev, a_ref, rtol=0, atol=atol, err_msg=f"{what} launch {rep} step {k} actions")
                a_ref = a_dev
            if before_step is not None:
                before_step(ref)
            obs, r_ref, d_ref, _ = ref.step(a_ref)
            obs = obs.copy()
            if after_step is not None:
                after_step(obs)
            ndone += int(d_ref.sum())
            for j, (acts, rews, dones) in enumerate(res):
                w = f"{what} run {j} launch {rep} step {k}"
                assert_bits(t2n(acts[k]), a_ref, w + " actions")
                assert_bits(t2n(rews[k]), r_ref, w + " rewards")
                assert_bits(t2n(dones[k]), d_ref, w + " dones")
        for j, (env, roll) in enumerate(zip(envs, rolls)):
            w = f"{what} run {j} after launch {rep}"
            assert_bits(t2n(env.cash), ref.cash, w + " cash")
            assert_bits(t2n(env.margin), ref.margin, w + " margin")
            assert_bits(t2n(env.long_shares), ref.long, w + " long")
            assert_bits(t2n(env.env_indices), ref.env_idx, w + " env_idx")
            assert_bits(t2n(env.env_spots[:, 0]), ref.spot0, w + " spot0")
            assert_bits(t2n(roll.observation()), obs, w + " observation()")
    return ndone


@pytest.mark.parametrize("form,N,A,W,tiles", [
    ("window", 3000, 1, 8, (1, 7, 200)),    # 3000 single-env tiles > kMaxGrid; 200 > the default 64 (replace)
    ("window", 2100, 3, 5, (1, 33, 85)),    # 85 = kBlock / A, above the default 21
    ("table", 3000, 1, 8, (1, 3)),          # shrink-only override
    ("table", 2100, 3, 5, (1, 7)),
])
def test_linear_rollout_tile_loop_equals_oracle(fe, fo, form, N, A, W, tiles):
    """fe_rollout_linear_kernel / fe_rollout_table_kernel under set_launch(rollout_tile_envs=): at tile 1 there are more
    tiles than kMaxGrid workgroups, so workgroups revisit tiles -- state reload, descriptor write-back and LDS reuse
    between tiles -- over two launches and episode ends; odd tiles and, for the window form, one above the default."""
    from finenvs_amd.rollout import FusedLinearRollout

    P, LR, ref, envs = _rollout_envs(fe, fo, N, A, W, tiles, seed=5 * N + W + A)
    assert N > 2048  # tiles at rollout_tile_envs=1 > kMaxGrid
    rng = np.random.default_rng(W + A)
    weights = rng.normal(0, 3.0, (W, 5))
    weights[:, 4] *= 40.0
    bias = 0.05
    rolls = [FusedLinearRollout(e, torch.from_numpy(weights), bias, form=form) for e in envs]
    if form == "window":
        ndone = _lockstep(ref, envs, rolls, lambda obs: fo.policy_linear(obs, weights, bias), 7, 3, f"linear {form}")
    else:  # the oracle's restatement of the split sum, on the descriptors of the observation just returned
        L = P.shape[1]
        table, wsum = fo.policy_table(LR, weights, W)
        d = dict(row=ref.env_idx * L + ref.spot0, pos=None, pre=None)  # descriptors of the reset() observation

        def policy(obs):
            pos = obs[:, 0, 4::5].copy() if d["pos"] is None else d["pos"]
            return fo.policy_table_actions(table, wsum, bias, d["row"], pos)

        def before_step(r):
            d["pre"] = r.env_idx * L + r.spot0 + 1  # the returned (terminal on done) window

        def after_step(obs):
            d["row"], d["pos"] = d["pre"], obs[:, 0, 4::5].copy()

        ndone = _lockstep(ref, envs, rolls, policy, 7, 3, f"linear {form}", before_step=before_step, after_step=after_step)
    assert ndone > 0


@pytest.mark.parametrize("H,A,N,W,tiles,act,atol", [
    (32, 1, 3000, 8, (1, 33, 256), 1, 0.0),   # 256 = kBlock / A, above the default 128 (replace)
    (64, 1, 3000, 8, (1, 3), 1, 0.0),
    (128, 1, 3000, 8, (1, 7), 1, 0.0),
    (64, 3, 2100, 5, (1, 85), 1, 0.0),        # 85 = kBlock / A, above the default 42
    (64, 1, 3000, 8, (1,), 0, 2e-6),          # ELU
])
def test_mlp_rollout_tile_loop_equals_oracle(fe, fo, H, A, N, W, tiles, act, atol):
    """fe_rollout_mlp_kernel under set_launch(rollout_tile_envs=): tile 1 makes more tiles than kMaxGrid, so each workgroup
    walks several tiles with its W1 image loaded once; odd tiles; one tile above the default (up to 8 MFMA column blocks
    per workgroup).  ReLU bit for bit; ELU: actions within 2e-6 absolute (v_exp_f32 vs expm1f, as in
    test_mlp_rollout_gpu.py), the oracle stepped with the device's actions."""
    from finenvs_amd.rollout import FusedMLPRollout

    _, _, ref, envs = _rollout_envs(fe, fo, N, A, W, tiles, seed=3 * N + W + H)
    rng = np.random.default_rng(W + H)
    W1 = (rng.normal(0, 1.0, (5 * W, H)) * (12.0 / np.sqrt(W))).astype(np.float32)
    W1[4::5, :] = (rng.normal(0, 1.0, (W, H)) * (3.0 / W)).astype(np.float32)
    b1 = rng.normal(0, 0.3, H).astype(np.float32)
    W2 = (rng.normal(0, 1.0, H) * (0.9 / np.sqrt(H))).astype(np.float32)
    b2 = np.float32(0.03)
    w1t, wpos = fo.mlp_pack(W1, W)
    activation = {0: "elu", 1: "relu"}[act]
    rolls = [FusedMLPRollout(e, torch.from_numpy(W1), torch.from_numpy(b1), torch.from_numpy(W2), float(b2),
                             activation=activation) for e in envs]
    ndone = _lockstep(ref, envs, rolls, lambda obs: fo.policy_mlp(obs, w1t, wpos, b1, W2, b2, act=act), 5, 3,
                      f"mlp H={H} {activation}", atol=atol)  # tolerance: 2e-6 absolute (ELU), 0 (ReLU)
    assert ndone > 0


def _lstm_modules(H, seed, gain):
    torch.manual_seed(seed)
    lstm = torch.nn.LSTM(5, H, num_layers=1, batch_first=True)
    lin = torch.nn.Linear(H, 1)
    with torch.no_grad():
        lstm.weight_ih_l0[:, :4].mul_(gain * np.sqrt(H))
        lstm.weight_ih_l0[:, 4].mul_(4.0)
        lin.weight.mul_(6.0)
    return lstm, lin


@pytest.mark.parametrize("H,A,N,W,tiles,K,reps,split", [
    (32, 1, 4500, 4, (1, 7), 4, 3, False),     # 4500 single-env tiles: more than any resident grid
    (128, 1, 4500, 4, (1,), 2, 2, False),
    (32, 3, 4500, 4, (1,), 3, 2, False),       # one env = 3 pairs per tile
    (256, 1, 3000, 2, (1, 3), 2, 2, True),     # split LSTM: the accounting launch's tile loop
])
def test_lstm_rollout_tile_loop_equals_oracle(fe, fo, H, A, N, W, tiles, K, reps, split):
    """fe_rollout_lstm_kernel with set_launch(rollout_tile_envs=) shrinking the tile to 1 env: num_tiles exceeds the
    resident grid cus x per_cu of launch_lstm, so workgroups loop over tiles (h / c and descriptors reloaded per tile);
    fe_env_rollout_lstm_split (H = 256): its accounting kernel loops over more tiles than kMaxGrid.  Bit for bit against
    the oracle loop of test_lstm_rollout_equals_oracle_loop_bit_for_bit, over two or more launches."""
    from finenvs_amd.rollout import FusedLSTMRollout

    _, _, ref, envs = _rollout_envs(fe, fo, N, A, W, tiles, seed=N + H + A)
    if not split:
        assert _cdiv(N, 1) > 16 * _num_cus()
    lstm, lin = _lstm_modules(H, seed=W + H, gain=6.0 if H <= 128 else 2.0)
    whh, wx = fo.lstm_pack(t2n(lstm.weight_ih_l0), t2n(lstm.weight_hh_l0), t2n(lstm.bias_ih_l0), t2n(lstm.bias_hh_l0))
    wout, bout = t2n(lin.weight).reshape(-1).copy(), float(lin.bias.detach())
    rolls = [FusedLSTMRollout.from_modules(e, lstm, lin) for e in envs]
    for roll in rolls:
        roll.split = split
    seen = set()

    def policy(obs):
        a = _chunked(fo.policy_lstm, obs, whh, wx, wout, bout)
        seen.update(np.unique(np.round(a, 2)).tolist())
        return a

    _lockstep(ref, envs, rolls, policy, K, reps, f"lstm H={H} A={A}")
    assert len(seen) > 5, "the policy's outputs must vary across envs"


def test_evo_rollout_tile_loop_equals_oracle(fe, fo):
    """fe_evo_rollout_kernel at N = 40 000 (A = 1, W = 8, H = 32): 16-env tiles, so more tiles than kMaxGrid and every
    workgroup walks two -- no override needed.  Actions within 1e-5 of a plain f32 torch forward of each env's perturbed
    network (as in test_evo_rollout_gpu.py); fed to the oracle, rewards, dones, state and running returns bit for bit."""
    from finenvs_amd.data import synthetic
    from finenvs_amd.evo import FusedPopulationMLPRollout

    N, A, W, H = 40000, 1, 8, 32
    prices, day_id, _ = synthetic.synthetic_series(5, A, 20, 41, 0.0)
    P, LR, *_ = fo.tables_from_series(prices, day_id, W)
    idx = (np.arange(N) * 5 + 1) % P.shape[0]
    kw = dict(num_intervals=W, evaluate=False, starting_balance=2000)
    ref = fo.OracleEnv(P, LR, env_indices=idx, redraw_mode=1, seed=9, auto_emit=False, nthreads=8, **kw)
    ref.redraw_counter[0] = 1
    env = fe.TimeSeriesEnv(tables=(P, LR), env_indices=idx, redraw="device", seed=9, obs_buffers=0, **kw)
    pop = FusedPopulationMLPRollout(env, 4, H, 0.5, seed=4, action_noise_std=0.0, max_episodes=16)
    assert _cdiv(pop.num_pairs, 8) > 2048
    g = torch.Generator().manual_seed(H)
    W1 = torch.randn((5 * W, H), generator=g) * (12.0 / W ** 0.5)
    W1[4::5, :] = torch.randn((W, H), generator=g) * (3.0 / W)
    pop.set_parameters([W1, torch.randn((H, 1), generator=g) * (2.0 / H ** 0.5)],
                       [torch.randn((1, H), generator=g) * 0.3, torch.full((1, 1), 0.03)])
    h = pop.num_pairs
    z = pop.noise(torch.arange(h))
    e = z * torch.tensor(pop.noise_std_dev, dtype=torch.float32, device=z.device)
    w = pop.theta.unsqueeze(0).repeat(N, 1)
    w[:h] = w[:h] + e
    w[h:2 * h] = w[h:2 * h] - e
    O = 5 * W
    W1s, b1s = w[:, :O * H].reshape(N, O, H), w[:, O * H:O * H + H].reshape(N, 1, H)
    W2s, b2s = w[:, O * H + H:O * H + 2 * H].reshape(N, H, 1), w[:, O * H + 2 * H:].reshape(N, 1, 1)
    obs = ref.reset().copy()
    assert_bits(t2n(pop.observation()), obs, "initial obs")
    ret = np.zeros(N, dtype=np.float32)
    ndone = 0
    for rep, K in enumerate((3, 25)):
        acts, rews, dones = pop.run(K, record=True)
        for k in range(K):
            a_dev = t2n(acts[k])
            x = torch.as_tensor(obs, device=w.device).float().reshape(N, 1, O)
            a_ref = t2n(torch.tanh(torch.bmm(torch.tanh(torch.bmm(x, W1s) + b1s), W2s) + b2s).reshape(N, 1))
            np.testing.assert_allclose(a_dev, a_ref, rtol=0, atol=1e-5, err_msg=f"launch {rep} step {k} actions")  # tolerance: 1e-5
            obs, r_ref, d_ref, _ = ref.step(a_dev)
            obs = obs.copy()
            what = f"launch {rep} step {k}"
            assert_bits(t2n(rews[k]), r_ref, what + " rewards")
            assert_bits(t2n(dones[k]), d_ref, what + " dones")
            ret = (ret.astype(np.float64) + r_ref).astype(np.float32)
            ret[d_ref != 0] = 0.0
            ndone += int(d_ref.sum())
        assert_bits(t2n(env.cash), ref.cash, f"launch {rep} cash")
        assert_bits(t2n(env.margin), ref.margin, f"launch {rep} margin")
        assert_bits(t2n(env.env_indices), ref.env_idx, f"launch {rep} env_idx")
        assert_bits(t2n(env.env_spots[:, 0]), ref.spot0, f"launch {rep} spot0")
        assert_bits(t2n(pop.observation()), obs, f"launch {rep} observation()")
        assert_bits(t2n(pop.returns), ret, f"launch {rep} running returns")
    assert ndone > 0


def _evo2_tile_loop(fe, fo, N, A, W, H, num_eval, days, bars, chunks):
    """``_Lockstep`` of tests/test_evo2_rollout_gpu.py (member weights rebuilt from ``pop.noise``, ``_forward2`` in f64,
    ``ACTION_TOL``; rewards, dones, state, running returns, counters and episode slots bit for bit) at a tile count above
    kMaxGrid.  Returns the run and the tile count of fe_evo.hip's geometry."""
    from tests import test_evo2_rollout_gpu as te2

    run, _ = te2._case(fe, fo, N, A, W, H, num_eval, days, bars, stagger=True)
    pop = run.pop
    PB = max(1, min(8, 128 // A))
    tiles = _cdiv(pop.num_pairs, PB) + _cdiv(num_eval, 2 * PB)
    w = te2._member_weights(pop)
    for rep, K in enumerate(chunks):
        run.run(K, w, f"chunk {rep}")
    assert pop.num_finished() > 0 and run.total > 0
    run.report(f"evo2 tile loop (N, A, W, H) = ({N}, {A}, {W}, {H}), {tiles} tiles")
    return run, tiles, PB


def test_evo2_rollout_tile_loop_equals_oracle(fe, fo):
    """fe_evo2_rollout_kernel at N = 40 000 (A = 1, W = 8, H = 32), the shape of the one-layer case above: 2 501 tiles of
    16 envs for kMaxGrid workgroups, so 453 workgroups walk a second tile with theta loaded once and the per-wave exchange
    buffer of the second layer reused."""
    _, tiles, PB = _evo2_tile_loop(fe, fo, 40000, 1, 8, 32, 4, 5, 20, (3, 9))
    assert PB == 8 and tiles > 2048


def test_evo2_rollout_tile_loop_with_uneven_unit_counts(fe, fo):
    """A = 17: PB = 7 pairs, 14-env tiles, the waves of a tile run 2, 2, 2 and 1 units.  N = 28 663 is the smallest N with
    three evaluation envs whose tile count exceeds kMaxGrid (14 330 pairs = 2 047 full tiles + 1 of one pair, and one
    evaluation tile: 2 049), so one workgroup walks a second tile."""
    N, num_eval = 28663, 3
    _, tiles, PB = _evo2_tile_loop(fe, fo, N, 17, 4, 32, num_eval, 4, 11, (2, 5))
    assert PB == 7 and tiles == 2049
    assert _cdiv((N - 2 - num_eval) // 2, PB) + 1 <= 2048  # one pair fewer: no second tile


# ----------------------------------------------------------------------------- 2b. sampling rollouts in the tile loop
STATE = ("cash", "margin", "long_shares", "env_indices", "env_spots")


class _SampledMLP:
    """``FusedMLPRollout`` / ``FusedMLP2Rollout`` with a tanh output, ``run(noise=, std=, trajectory=)``."""
    outputs, std = ("actions", "means", "rewards", "dones"), 0.7

    def __init__(self, depth, H, W, activation, seed):
        from tests import test_mlp2_head_gpu as t2
        from tests import test_mlp_head_gpu as th

        self.t = th if depth == 1 else t2
        self.module = self.t._module(H, W, seed, activation, "tanh")

    def roll(self, env):
        return self.t._rollout(env, self.module, "tanh")

    def run(self, roll, K, noise, traj):
        a, r, d = roll.run(K, noise=noise, std=self.std, record_means=True, trajectory=traj)
        return dict(actions=a, means=roll.means, rewards=r, dones=d)

    def forward(self, roll, src, pos, noise):
        return dict(means=roll.forward(src, pos))

    def sampled(self, means, noise):  # fe_rollout_mlp_sampled_kernel's statement, exact in f32
        return (means + torch.tensor(self.std, dtype=torch.float32, device=means.device) * noise).clamp(-1.0, 1.0)

    def torch_means(self, pairs, dtype):
        with torch.no_grad():
            return copy.deepcopy(self.module).to(dtype)(pairs.to(dtype))


class _SacActor:
    """``FusedMLPSACRollout`` / ``FusedSACRollout`` (resident or streamed)."""
    outputs = ("actions", "means", "stds", "rewards", "dones")

    def __init__(self, lstm, H, W, activation, seed):
        from tests import test_mlp_sac_gpu as tms
        from tests import test_sac_rollout_gpu as tsr

        self.lstm, self.streamed = lstm, H > 128
        self.actor = tsr._actor(H, W, seed) if lstm else tms._rollout_actor(H, W, seed, activation)

    def roll(self, env):
        from finenvs_amd.mlp_sac import FusedMLPSACRollout
        from finenvs_amd.sac import FusedSACRollout

        if not self.lstm:
            return FusedMLPSACRollout(env, self.actor)
        roll = FusedSACRollout(env, self.actor, streamed=self.streamed)
        assert roll.streamed == self.streamed
        return roll

    def run(self, roll, K, noise, traj):
        a, r, d = roll.run(K, noise=noise, trajectory=traj, record_means=True, record_stds=True)
        return dict(actions=a, means=roll.means, stds=roll.stds, rewards=r, dones=d)

    def forward(self, roll, src, pos, noise):
        a, _, mu, sd = roll.forward(src, pos, noise)
        return dict(actions=a, means=mu, stds=sd)

    sampled = None

    def torch_means(self, pairs, dtype):
        with torch.no_grad():
            return copy.deepcopy(self.actor).to(dtype).get_distribution(pairs.to(dtype)).loc


def _sampled_tile_loop(fe, fo, fam, N, A, W, tiles, K, reps, seed, evaluate=False, stagger=False, what=""):
    """A rollout that takes a ``(K, N, A)`` noise tensor, on one oracle env, one automatic-geometry env and one env per
    ``rollout_tile_envs`` override.  Per launch, bit for bit: every override run equals the automatic one in every output,
    both trajectory descriptor arrays (K + 1 rows) and the env's state; ``forward`` on the last override run's trajectory
    rows returns what ``run`` recorded; the evaluation env (the last of a training-mode env) acts on its mean and every
    other env's action differs from its mean; the oracle env stepped with the device's actions gives the device's
    rewards, dones and state.  The means of the first step of the last launch against the f64 torch forward on the
    rendered trajectory state, within the family's yardstick."""
    from finenvs_amd.sac import pair_states
    from finenvs_amd.trajectory import TrajectoryBuffer
    from tests.test_mlp_sac_gpu import _bound

    _, _, ref, envs = _rollout_envs(fe, fo, N, A, W, tiles, seed=seed, evaluate=evaluate, stagger=stagger)
    assert all(int(e._eval_env) == (-1 if evaluate else N - 1) for e in envs)
    rolls = [fam.roll(e) for e in envs]
    obs = ref.reset().copy()
    for roll in rolls:
        assert_bits(t2n(roll.observation()), obs, what + " initial obs")
    gen = torch.Generator(device="cuda").manual_seed(seed)
    ndone = 0
    for rep in range(reps):
        noise = torch.randn((K, N, A), generator=gen, device="cuda")
        res = []
        for roll in rolls:
            traj = TrajectoryBuffer(K, N, A, states=True)
            out = fam.run(roll, K, noise, traj)
            out.update(src=traj.obs_src, pos=traj.obs_pos)
            assert tuple(traj.obs_src.shape) == (K + 1, N) and tuple(traj.obs_pos.shape) == (K + 1, N, A)
            res.append((out, traj))
        for j in range(1, len(rolls)):
            w = f"{what} launch {rep}: tile {tiles[j - 1]} against the automatic geometry:"
            for name in fam.outputs + ("src", "pos"):
                assert_bits(t2n(res[j][0][name]), t2n(res[0][0][name]), f"{w} {name}")
            for name in STATE:
                assert_bits(t2n(getattr(envs[j], name)), t2n(getattr(envs[0], name)), f"{w} {name}")
            assert_bits(t2n(rolls[j].observation()), t2n(rolls[0].observation()), f"{w} observation()")
        (out, traj), env, roll = res[-1], envs[-1], rolls[-1]
        acts, means = out["actions"], out["means"]
        w = f"{what} launch {rep}:"
        # forward on the trajectory's rows returns what run recorded
        fwd = fam.forward(roll, out["src"][:K].reshape(-1), out["pos"][:K].reshape(-1, A), noise.reshape(-1, A))
        assert_bits(t2n(fwd["means"].reshape(K, N, A)), t2n(means), f"{w} forward means == run means")
        if "stds" in fwd:
            assert_bits(t2n(fwd["stds"].reshape(K, N, A)), t2n(out["stds"]), f"{w} forward stds == run stds")
        sampled = fwd["actions"].reshape(K, N, A) if "actions" in fwd else fam.sampled(means, noise)
        # the evaluation env acts on its mean, every other env samples
        differ = acts != means
        if not evaluate:
            assert_bits(t2n(acts[:, -1]), t2n(means[:, -1]), f"{w} the evaluation env acts on its mean")
            assert_bits(t2n(acts[:, :-1]), t2n(sampled[:, :-1]), f"{w} the other envs' actions are the samples")
            differ = differ[:, :-1]
        else:
            assert_bits(t2n(acts), t2n(sampled), f"{w} every env's action is the sample")
        # The sample's own statement can return the mean (a draw that is exactly 0.0, a mean that tanh rounded to +-1.0
        # and a clamp): decided from the recorded means and the noise alone, and rare -- at most one element in 10 000.
        same = sampled == means
        same = same if evaluate else same[:, :-1]
        print(f"{w} {int((~differ).sum())} of {differ.numel()} sampled actions equal their means; the statement gives the "
              f"mean for {int(same.sum())} (noise there: {noise[:, :N if evaluate else N - 1][same].tolist()[:4]})")
        assert int(same.sum()) <= 1e-4 * same.numel(), f"{w} {int(same.sum())} samples equal their means by their statement"
        assert bool((differ | same).all()), f"{w} a sampled action equals its mean"
        if rep == reps - 1:  # a consistent but wrong policy: the f64 torch forward on the rendered trajectory state
            pairs = pair_states(traj.states(env, 0), A)
            x32, x64 = fam.torch_means(pairs.float(), torch.float32), fam.torch_means(pairs, torch.float64)
            assert float(x64.std()) > 1e-3, "the head must depend on the observation"
            _bound(means[0].reshape(-1, 1), x32, x64, f"{w} means of step 0 against f64 torch")  # 2e-5 max|x64| + 4 max|x32 - x64|
        # the oracle env stepped with the device's actions
        for k in range(K):
            assert_bits(t2n(traj.states(env, k)), obs, f"{w} step {k} trajectory state")
            obs, r_ref, d_ref, _ = ref.step(t2n(acts[k]))
            obs = obs.copy()
            ndone += int(d_ref.sum())
            assert_bits(t2n(out["rewards"][k]), r_ref, f"{w} step {k} rewards")
            assert_bits(t2n(out["dones"][k]), d_ref, f"{w} step {k} dones")
        assert_bits(t2n(traj.states(env, K)), obs, f"{w} last trajectory state")
        assert_bits(t2n(roll.observation()), obs, f"{w} observation()")
        assert_bits(t2n(env.cash), ref.cash, f"{w} cash")
        assert_bits(t2n(env.margin), ref.margin, f"{w} margin")
        assert_bits(t2n(env.long_shares), ref.long, f"{w} long")
        assert_bits(t2n(env.env_indices), ref.env_idx, f"{w} env_idx")
        assert_bits(t2n(env.env_spots[:, 0]), ref.spot0, f"{w} spot0")
        if evaluate and int(ref.n_terminated[0]) == N:  # as tests/test_sac_rollout_gpu.py: every env has finished
            for e in envs:
                e.reset_evaluation_metrics()
            ref.terminated[:] = 0
            ref.episode_returns[:] = 0
            ref.n_terminated[0] = 0
    assert ndone > 0, "the run must cross episode ends"


# kMaxGrid = 2048 (fe_env.hip): at rollout_tile_envs = 1 every case below has more tiles than workgroups.  A tile holds at
# most kBlock / A = 256 / A envs; the policy phase walks ``blk = wave; blk < nblk; blk += 4`` over blocks of 32 pairs, so a
# tile of more than 128 pairs (256 at A = 1, 85 at A = 3) gives every wavefront a second block.
SAMPLED_MLP_CASES = [
    # depth, H, A, N, W, tiles, activation, evaluate
    (1, 32, 1, 3000, 8, (1, 33, 256), "elu", False),   # > 2048 tiles; ragged tile; 8 column blocks, so each wave takes 2
    (1, 64, 3, 2100, 5, (1, 85), "tanh", False),       # 3 pairs per tile; 255 pairs per tile
    (1, 64, 3, 2100, 5, (1,), "relu", True),           # an evaluate-mode env: every env samples
    (2, 64, 1, 3000, 8, (1, 256), "elu", False),
    (2, 128, 3, 2100, 5, (1, 7), "tanh", False),       # the one-workgroup-per-CU instantiation
    (2, 64, 1, 3000, 8, (1,), "relu", True),
]


@pytest.mark.parametrize("depth,H,A,N,W,tiles,activation,evaluate", SAMPLED_MLP_CASES)
def test_sampled_mlp_rollout_tile_loop(fe, fo, depth, H, A, N, W, tiles, activation, evaluate):
    """fe_rollout_mlp_sampled_kernel / fe_rollout_mlp2_sampled_kernel under set_launch(rollout_tile_envs=): three launches
    of five steps on 14-bar days."""
    assert _cdiv(N, 1) > 2048
    fam = _SampledMLP(depth, H, W, activation, seed=N + H + depth)
    _sampled_tile_loop(fe, fo, fam, N, A, W, tiles, 5, 3, seed=3 * N + W + H + depth, evaluate=evaluate,
                       what=f"mlp{depth} sampled H={H} A={A}")


SAC_MLP_CASES = [
    # H, A, N, W, tiles, activation, evaluate
    (32, 1, 3000, 8, (1, 33, 256), "elu", False),
    (64, 3, 2100, 5, (1, 85), "tanh", False),
    (128, 1, 3000, 4, (1, 7), "relu", False),
    (64, 3, 2100, 5, (1,), "elu", True),
]


@pytest.mark.parametrize("H,A,N,W,tiles,activation,evaluate", SAC_MLP_CASES)
def test_sac_mlp_rollout_tile_loop(fe, fo, H, A, N, W, tiles, activation, evaluate):
    """fe_rollout_mlp_sac_kernel under set_launch(rollout_tile_envs=): mu, s and the action leave from inside the policy
    phase, indexed by ``(k, n0 + ee, aa)``; three launches of five steps on 14-bar days."""
    assert _cdiv(N, 1) > 2048
    fam = _SacActor(False, H, W, activation, seed=H + A)
    _sampled_tile_loop(fe, fo, fam, N, A, W, tiles, 5, 3, seed=3 * N + W + H, evaluate=evaluate, what=f"sac mlp H={H} A={A}")


SAC_LSTM_CASES = [
    # H, A, N, W, tiles, K, reps, evaluate -- K and reps of test_lstm_rollout_tile_loop_equals_oracle
    (32, 1, 4500, 4, (1, 7), 4, 3, False),     # shrink-only override, as the LSTM case
    (128, 3, 4500, 4, (1,), 3, 2, False),
    (256, 1, 3000, 2, (1, 3), 2, 2, False),    # streamed
    (32, 1, 4500, 4, (1,), 4, 3, True),
]


@pytest.mark.parametrize("H,A,N,W,tiles,K,reps,evaluate", SAC_LSTM_CASES)
def test_sac_lstm_rollout_tile_loop(fe, fo, H, A, N, W, tiles, K, reps, evaluate):
    """fe_rollout_sac_kernel / fe_rollout_sac_big_kernel (``streamed=True``, H = 256) with the tile shrunk to one env: more
    tiles than the resident grid, so workgroups loop over tiles with h / c, the descriptors and the noise index reloaded
    per tile.  The runs are a few steps long, so the envs start staggered near their days' ends."""
    if H <= 128:
        assert _cdiv(N, 1) > 16 * _num_cus()
    else:  # a workgroup has 512 threads, so at most 2048 / 512 = 4 are resident per CU: twice as many tiles as workgroups
        assert _cdiv(N, 1) >= 2 * 4 * _num_cus()
    fam = _SacActor(True, H, W, None, seed=W + H)
    _sampled_tile_loop(fe, fo, fam, N, A, W, tiles, K, reps, seed=N + H + A, evaluate=evaluate, stagger=True,
                       what=f"sac lstm H={H} A={A}")


# ----------------------------------------------------------------------------- 3. replay sampling in the tile loop
def test_replay_sample_tile_loop_equals_the_reference_buffer(fe, fo):
    """fe_replay_sample_kernel with more tiles than its 8 x CU grid: A = 255, W = 1 caps a tile at 2048 / (1 + A) = 8
    samples, so B = 17 000 gives 2 125 tiles and workgroups revisit tiles (descriptor LDS reused).  Every row of the
    mini-batch equals the torch restatement of the reference buffer (tests/test_replay_gpu.py), the last tile included."""
    from finenvs_amd.replay import KEYS, ReplayBuffer
    from finenvs_amd.data import synthetic

    N, A, W, Cap, B = 16, 255, 1, 300, 17000
    assert _cdiv(B, 2048 // (1 + A)) > 8 * _num_cus()
    prices, day_id, _ = synthetic.synthetic_series(4, A, 20, 5, 0.05)
    P, LR, *_ = fo.tables_from_series(prices, day_id, W)
    env = fe.TimeSeriesEnv(tables=(P, LR), env_indices=(np.arange(N) * 7 + 1) % P.shape[0], num_intervals=W,
                           starting_balance=1500, redraw="device", seed=3, obs_dtype=torch.float32)
    buf = ReplayBuffer(env, max_size=Cap)
    ref = {}
    g = torch.Generator(device="cuda").manual_seed(1)
    desc = [env.describe(), (torch.empty(N, dtype=torch.int64, device="cuda"),
                             torch.empty((N, A), dtype=torch.float64, device="cuda"))]
    obs = env.reset().clone()
    ndone = 0
    for t in range(30):  # 480 transitions: the ring of 300 wraps
        a = torch.rand((N, A), generator=g, device="cuda") * 2 - 1
        state, nxt = desc[t % 2], desc[(t + 1) % 2]
        new_obs, r, d, _ = env.step(a, descriptors_out=nxt)
        buf.store(state, a, r, nxt, d)
        for k, v in dict(states=obs, actions=a, rewards=r, next_states=new_obs, dones=d).items():
            v = v.reshape(-1, 1) if v.dim() < 2 else v
            ref[k] = (torch.cat([ref[k], v.float()]) if k in ref else v.float().clone())[-Cap:]
        obs = new_obs.clone()
        ndone += int(d.sum())
    assert ndone > 0 and buf.size() == Cap
    idx = torch.cat([torch.tensor([0, Cap - 1], device="cuda"), torch.randint(0, Cap, (B - 3,), generator=g, device="cuda"),
                     torch.tensor([Cap - 1], device="cuda")])
    got = buf.get_mini_batch(B, indices=idx, check=True)
    assert list(got) == list(KEYS)
    for k in KEYS:
        assert_bits(t2n(got[k]), t2n(torch.index_select(ref[k], 0, idx)), f"{k} (B = {B})")


# ----------------------------------------------------------------------------- 4. fe_traj_returns / fe_traj_store
def _traj_inputs(T, N, seed, last_step_done=0.2):
    rng = np.random.default_rng(seed)
    rew = rng.normal(0, 3.0, (T, N))
    done = (rng.random((T, N)) < 0.2).astype(np.int32)
    done[T - 1] = (rng.random(N) < last_step_done).astype(np.int32)
    values = rng.normal(0, 5.0, (T, N)).astype(np.float32)
    last = rng.normal(0, 5.0, N).astype(np.float32)
    return rew, done, values, last


def _traj_returns(rew, done, values, last, gamma, with_adv=True):
    from finenvs_amd import _lib

    lib = _lib.load()
    T, N = rew.shape
    d = [torch.from_numpy(x).cuda() for x in (rew, done, values, last)]
    ret = torch.full((T, N), -7.0, dtype=torch.float32, device="cuda")
    adv = torch.full((T, N), -7.0, dtype=torch.float32, device="cuda")
    _lib.check(lib.fe_traj_returns(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr() if with_adv else None, d[3].data_ptr(),
                                   T, N, float(gamma), ret.data_ptr(), adv.data_ptr() if with_adv else None,
                                   torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return t2n(ret), t2n(adv)


@pytest.mark.parametrize("T", [1, 2, 3, 5, 7])
@pytest.mark.parametrize("gamma", [0.99, 0.0, 1.0])
def test_traj_returns_unrolled_scan_every_tail_length(fe, fo, T, gamma):
    """fe_traj_returns_kernel<4> (N < 2^19): T = 1, 2, 3, 5, 7 reach every length of the unrolled loop's t < 0 tail;
    gamma 0 and 1.  Returns equal fo.discounted_returns bit for bit, advantages equal np.float32(returns - values)."""
    rew, done, values, last = _traj_inputs(T, 1000, seed=T)
    ret, adv = _traj_returns(rew, done, values, last, gamma)
    want = fo.discounted_returns(rew, done, last, gamma)
    assert_bits(ret, want, f"returns T={T} gamma={gamma}")
    assert_bits(adv, (want - values).astype(np.float32), f"advantages T={T} gamma={gamma}")


def test_traj_returns_single_step_instantiation_at_2_pow_19_envs(fe, fo):
    """fe_traj_returns_kernel<1>, which the host picks at N >= 2^19: N = 2^19 + 37, T = 5, half the envs done at t = T - 1."""
    rew, done, values, last = _traj_inputs(5, (1 << 19) + 37, seed=19, last_step_done=0.5)
    ret, adv = _traj_returns(rew, done, values, last, 0.99)
    want = fo.discounted_returns(rew, done, last, 0.99)
    assert_bits(ret, want, "returns (U = 1)")
    assert_bits(adv, (want - values).astype(np.float32), "advantages (U = 1)")


def test_traj_returns_without_advantages_and_traj_store_with_three_assets(fe, fo):
    """fe_traj_returns(values = NULL, advantages = NULL), which the C ABI allows: the returns are unchanged and the
    advantages buffer is not written.  fe_traj_store at A = 3 (N*A action elements, N rewards / dones) through
    TrajectoryBuffer.store: every slot equals its inputs bit for bit."""
    from finenvs_amd.trajectory import TrajectoryBuffer

    rew, done, values, last = _traj_inputs(6, 1000, seed=6)
    ret, adv = _traj_returns(rew, done, values, last, 0.95, with_adv=False)
    assert_bits(ret, fo.discounted_returns(rew, done, last, 0.95), "returns without advantages")
    assert (adv == np.float32(-7.0)).all(), "the advantages buffer must not be written"
    T, N, A = 4, 1000, 3
    buf = TrajectoryBuffer(T, N, A, device="cuda:0")
    rng = np.random.default_rng(3)
    acts = rng.normal(0, 1, (T, N, A)).astype(np.float32)
    for t in range(T):
        buf.store(torch.from_numpy(acts[t]).cuda(), torch.from_numpy(rew[t]).cuda(), torch.from_numpy(done[t]).cuda())
    assert_bits(t2n(buf.actions[:T]).reshape(T, N, A), acts, "stored actions")
    assert_bits(t2n(buf.rewards[:T]), rew[:T], "stored rewards")
    assert_bits(t2n(buf.dones[:T]), done[:T], "stored dones")


# ----------------------------------------------------------------------------- 5. multi-asset grid rule
def test_multi_asset_grid_rule_at_config_3(fe, fo):
    """configure_launch, A > 1 (the rule ADVICE.md asks a test for): at A = 30, N = 262 144, W = 64 the grid is k x the
    resident count -- a multiple of 8, every workgroup walks >= 2 tiles, at most 8 x 8 workgroups per CU;
    set_launch(grid=) takes effect and set_launch() restores the automatic geometry.  With fewer tiles than resident
    workgroups (N = 200 < the CU count) the grid is the tile count."""
    from finenvs_amd.data import synthetic

    cus = _num_cus()
    A, W = 30, 64
    prices, day_id, _ = synthetic.synthetic_series(3, A, 120, 1234)
    P, LR, *_ = fo.tables_from_series(prices, day_id, W)
    env = fe.TimeSeriesEnv(tables=(P, LR), num_intervals=W, num_envs=262144, redraw="device", obs_buffers=0)
    info = env.launch_info()
    grid, tile = info["grid"], info["tile_envs"]
    num_tiles = _cdiv(262144, tile)
    assert 1 <= tile <= 256 // A
    assert grid % 8 == 0, info
    assert num_tiles >= 2 * grid, info
    assert grid <= 8 * 8 * cus, info
    assert env.set_launch(grid=1000)["grid"] == 1000
    assert env.launch_info()["tile_envs"] == tile
    assert env.set_launch() == info
    small = fe.TimeSeriesEnv(tables=(P, LR), num_intervals=W, num_envs=200, redraw="device", obs_buffers=0)
    s = small.launch_info()
    assert s["grid"] == _cdiv(200, s["tile_envs"]), s
