"""GPU: the device replay ring (finenvs_amd/replay.py) against a torch restatement of the reference's off-policy buffer
(finenvs/agents/off_policy_buffer.py: torch.cat of every store, index_select of the newest max_size rows, .float()) fed
with the observations env.step actually returned.  Every field of every mini-batch must be equal bit for bit -- with
explicit indices and with the default draw under the same torch seed -- over f64 and f32 observation envs, one and three
assets, done steps (terminal windows as next states) and a capacity that is not a multiple of N, wrapped several times."""
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


class TorchBuffer:
    """The reference buffer's semantics restated in torch: fields forced to 2-D, concatenated per store as f32, the
    newest max_size rows kept; get_mini_batch draws torch.randint(0, size, (B,)) on the device and index_selects."""

    def __init__(self, max_size):
        self.max_size, self.c = max_size, {}

    def store(self, **fields):
        for k, v in fields.items():
            v = v.reshape(-1, 1) if v.dim() < 2 else v
            self.c[k] = (torch.cat([self.c[k], v.float()]) if k in self.c else v.float())[-self.max_size:]

    def size(self):
        return self.c["dones"].shape[0] if self.c else 0

    def get_mini_batch(self, size, indices=None):
        if indices is None:
            indices = torch.randint(0, self.size(), (size,), device="cuda:0")
        return {k: torch.index_select(v, 0, indices) for k, v in self.c.items()}


def _make(fe, fo, N, A, W, obs_dtype, seed, days=6, bars=40, **kw):
    from finenvs_amd.data import synthetic

    prices, day_id, _ = synthetic.synthetic_series(days, A, bars, seed, 0.05)
    P, LR, *_ = fo.tables_from_series(prices, day_id, W)
    idx = (np.arange(N) * 7 + 1) % P.shape[0]
    return fe.TimeSeriesEnv(tables=(P, LR), env_indices=idx, num_intervals=W, starting_balance=1500, redraw="device",
                            seed=seed, obs_dtype=obs_dtype, **kw)


def _compare(got, want, what):
    from finenvs_amd.replay import KEYS

    assert list(got) == list(KEYS)
    for k in KEYS:
        assert got[k].dtype == torch.float32, f"{what} {k} dtype"
        assert_bits(got[k].cpu().numpy(), want[k].cpu().numpy(), f"{what} {k}")


@pytest.mark.parametrize("N,A,W,obs_dtype,C,f64_actions", [
    (37, 1, 8, torch.float64, 250, False),
    (29, 3, 5, torch.float64, 101, True),    # f64 actions are stored as f32
    (40, 1, 6, torch.float32, 130, False),
    (23, 3, 4, torch.float32, 70, False),
])
def test_mini_batches_equal_the_reference_buffer(fe, fo, N, A, W, obs_dtype, C, f64_actions):
    from finenvs_amd.replay import ReplayBuffer

    env = _make(fe, fo, N, A, W, obs_dtype, seed=N + W)
    buf, ref = ReplayBuffer(env, max_size=C), TorchBuffer(C)
    g = torch.Generator(device="cuda").manual_seed(A)
    desc = [env.describe(), (torch.empty(N, dtype=torch.int64, device="cuda"),
                             torch.empty((N, A), dtype=torch.float64, device="cuda"))]
    obs = env.reset().clone()
    ndone, B = 0, 97
    for t in range(90):  # 40-bar days: every env passes day ends; 90 N transitions wrap the ring several times
        a = torch.rand((N, A), generator=g, device="cuda") * 2 - 1
        if f64_actions:
            a = a.double() + 1e-9
        state, nxt = desc[t % 2], desc[(t + 1) % 2]
        new_obs, r, d, _ = env.step(a, descriptors_out=nxt)
        buf.store(state, a, r, nxt, d)
        ref.store(states=obs, actions=a, rewards=r, next_states=new_obs, dones=d)
        obs = new_obs.clone()
        ndone += int(d.sum())
        assert buf.size() == ref.size() == len(buf)
        if t % 9 == 4 or t == 89:
            size = buf.size()
            idx = torch.cat([torch.tensor([0, size - 1], device="cuda"),
                             torch.randint(0, size, (B,), generator=g, device="cuda")])
            _compare(buf.get_mini_batch(idx.numel(), indices=idx, check=True), ref.get_mini_batch(0, indices=idx),
                     f"step {t} explicit")
            torch.manual_seed(1000 + t)
            got = buf.get_mini_batch(B)
            torch.manual_seed(1000 + t)
            _compare(got, ref.get_mini_batch(B), f"step {t} default draw")
    assert ndone > 0 and 90 * N > 2 * C
    # every retained transition, in the reference's row order
    size = buf.size()
    _compare(buf.get_mini_batch(size, indices=torch.arange(size, device="cuda")),
             ref.get_mini_batch(0, indices=torch.arange(size, device="cuda")), "whole ring")


def test_f64_observations_sample_as_their_float_cast(fe, fo):
    """On an f64-table env the sample equals .float() of the f64 observation render() produces."""
    from finenvs_amd.replay import ReplayBuffer

    N, A, W = 33, 2, 7
    env = _make(fe, fo, N, A, W, torch.float64, seed=3)
    buf = ReplayBuffer(env, max_size=100)
    s = env.describe()
    n = (torch.empty(N, dtype=torch.int64, device="cuda"), torch.empty((N, A), dtype=torch.float64, device="cuda"))
    for _ in range(3):
        _, r, d, _ = env.step(torch.rand((N, A), device="cuda") * 2 - 1, descriptors_out=n)
        buf.store(s, torch.zeros((N, A), device="cuda"), r, n, d)
        s = (n[0].clone(), n[1].clone())
    idx = torch.arange(buf.size(), device="cuda")
    b = buf.get_mini_batch(idx.numel(), indices=idx)
    assert_bits(b["states"].cpu().numpy(), env.render(buf.state_src[idx], buf.state_pos[idx]).float().cpu().numpy(), "states")
    assert_bits(b["next_states"].cpu().numpy(), env.render(buf.next_src[idx], buf.next_pos[idx]).float().cpu().numpy(),
                "next states")


@pytest.mark.parametrize("C", [300, 1000])
def test_extend_after_a_graphed_chunk_equals_per_step_stores(fe, fo, C):
    """extend(traj) of a GraphedRollout chunk leaves the ring exactly as K per-step stores on a twin env do -- also
    when the chunk (K N = 512 transitions) is larger than the ring (C = 300: its newest 300 are kept)."""
    from finenvs_amd.replay import ReplayBuffer
    from finenvs_amd.rollout import GraphedRollout
    from finenvs_amd.trajectory import TrajectoryBuffer

    N, A, W, K = 64, 2, 6, 8
    g = torch.Generator().manual_seed(1)
    ring = [(torch.rand((N, A), generator=g) * 2 - 1).float().cuda() for _ in range(K)]
    graphed = _make(fe, fo, N, A, W, torch.float64, seed=5, obs_buffers=2)
    eager = _make(fe, fo, N, A, W, torch.float64, seed=5, obs_buffers=2)
    traj = TrajectoryBuffer(K, N, A, states=True)
    roll = GraphedRollout(graphed, lambda obs, k: ring[k], K, trajectory=traj, warmup=0)
    rb_g, rb_e = ReplayBuffer(graphed, max_size=C), ReplayBuffer(eager, max_size=C)
    eager.reset()
    desc = [eager.describe(), (torch.empty(N, dtype=torch.int64, device="cuda"),
                               torch.empty((N, A), dtype=torch.float64, device="cuda"))]
    ndone, t = 0, 0
    for rep in range(6):  # 48 steps over 40-bar days: done steps inside the chunks
        roll.run()
        rb_g.extend(traj)
        for k in range(K):
            _, r, d, _ = eager.step(ring[k], descriptors_out=desc[(t + 1) % 2])
            rb_e.store(desc[t % 2], ring[k], r, desc[(t + 1) % 2], d)
            ndone += int(d.sum())
            t += 1
        assert (rb_g.head, rb_g.size()) == (rb_e.head, rb_e.size()), f"replay {rep}"
        for name in ("state_src", "state_pos", "next_src", "next_pos", "actions", "rewards", "dones"):
            assert_bits(getattr(rb_g, name).cpu().numpy(), getattr(rb_e, name).cpu().numpy(), f"replay {rep} {name}")
    assert ndone > 0


def test_out_of_range_indices_give_nan_rows_and_check_raises(fe, fo):
    from finenvs_amd.replay import KEYS, ReplayBuffer

    N, A, W = 20, 3, 4
    env = _make(fe, fo, N, A, W, torch.float32, seed=9)
    buf = ReplayBuffer(env, max_size=50)
    s = env.describe()
    n = (torch.empty(N, dtype=torch.int64, device="cuda"), torch.empty((N, A), dtype=torch.float64, device="cuda"))
    for _ in range(3):  # 60 transitions into 50 slots
        _, r, d, _ = env.step(torch.rand((N, A), device="cuda") * 2 - 1, descriptors_out=n)
        buf.store(s, torch.rand((N, A), device="cuda"), r, n, d)
        s = (n[0].clone(), n[1].clone())
    assert buf.size() == 50
    idx = torch.tensor([3, 50, -1, 49, 1 << 40, 0, -(1 << 40)], device="cuda")
    bad = torch.tensor([False, True, True, False, True, False, True])
    with pytest.raises(IndexError, match="4 of 7 sample indices"):
        buf.get_mini_batch(7, indices=idx, check=True)
    out = buf.get_mini_batch(7, indices=idx)  # unchecked: the same rows, no exception
    good = buf.get_mini_batch(3, indices=idx[~bad.cuda()], check=True)
    for k in KEYS:
        v = out[k].cpu()
        assert torch.isnan(v[bad]).all(), k
        assert_bits(v[~bad].numpy(), good[k].cpu().numpy(), k)
    with pytest.raises(ValueError, match="integer tensor"):
        buf.get_mini_batch(2, indices=torch.zeros(2, device="cuda"))


def test_refusals_on_the_device(fe, fo):
    from finenvs_amd.replay import ReplayBuffer
    from finenvs_amd.trajectory import TrajectoryBuffer

    N, A, W = 12, 1, 4
    env = _make(fe, fo, N, A, W, torch.float64, seed=2)
    buf = ReplayBuffer(env, max_size=30)
    with pytest.raises(ValueError, match="empty replay buffer"):
        buf.get_mini_batch(4)
    obs, r, d, _ = env.step(torch.zeros((N, A), device="cuda"))
    with pytest.raises(ValueError, match="descriptors_out"):
        buf.store(obs, torch.zeros((N, A), device="cuda"), r, obs, d)
    with pytest.raises(ValueError, match="TrajectoryBuffer\\(states=True\\)"):
        buf.extend(TrajectoryBuffer(4, N, A))
    with pytest.raises(ValueError, match="envs x"):
        buf.extend(TrajectoryBuffer(4, N + 1, A, states=True))
    with pytest.raises(ValueError, match="does not fit"):
        ReplayBuffer(env, max_size=N - 1)
    buf.store(env.describe(), torch.zeros((N, A), device="cuda"), r, env.describe(), d)
    assert len(buf) == N
    buf.clear()
    assert buf.size() == 0 and buf.head == 0


def test_example_trains_a_few_iterations(fe):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import td3_time_series
    finally:
        sys.path.pop(0)
    hist, _ = td3_time_series.main(num_envs=64, window=8, hidden=(32, 32), iterations=12, batch=128, max_size=300, days=6,
                                   bars=40, quiet=True)
    assert len(hist) >= 8 and hist[-1]["buffer_size"] == 300
    assert all(np.isfinite(h["critic_loss"]) for h in hist)
    assert any("actor_loss" in h for h in hist) and all(np.isfinite(h["actor_loss"]) for h in hist if "actor_loss" in h)
