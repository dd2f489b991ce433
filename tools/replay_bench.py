"""GPU box: the device replay ring (finenvs_amd.replay.ReplayBuffer) against a torch restatement of the reference's
off-policy buffer (finenvs/agents/off_policy_buffer.py: torch.cat of the whole container + index_select of the newest
max_size rows + .float(), rendered observations as states) on the same GPU, at N = 65 536 envs, W = 64, A = 1 (f64
observations, the reference's dtype).

    timeout -k 10 900 python tools/replay_bench.py [--envs 65536] [--capacity 1000000]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/replay_bench.py --profile 65536   (sample kernel only)
    python tools/replay_bench.py --kernel-stats DIR/.../run_kernel_stats.csv --batch 65536           (its bytes / time)

Arms: us per store at capacity (device ring: one fe_replay_append launch; restatement: five cat + index_select), us per
get_mini_batch end to end (default draw included) at B = 4 096 and 65 536, and device time per sample launch (20 launches
replayed from one hipGraph).  Prints one line per arm and a final JSON line.
"""
import argparse
import csv
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import finenvs_amd  # noqa: E402
from bench import make_series  # noqa: E402
from finenvs_amd.replay import ReplayBuffer  # noqa: E402

HBM_BYTES_PER_S = 8.0e12  # MI355X peak HBM bandwidth


def sample_bytes(B, W, A):
    """Bytes fe_replay_sample writes: two (B, W, 5A) f32 observations, (B, A) actions, rewards and dones."""
    return B * (2 * W * 5 * A * 4 + 4 * A + 8)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3  # us


class TorchBuffer:
    """The reference buffer restated: every store concatenates the whole container and keeps its newest rows."""

    def __init__(self, max_size):
        self.max_size, self.c = max_size, {}

    def store(self, **fields):
        for k, v in fields.items():
            v = v.reshape(-1, 1) if v.dim() < 2 else v
            c = torch.cat([self.c[k], v], dim=0).float() if k in self.c else v.float()
            if c.shape[0] > self.max_size:
                c = torch.index_select(c, 0, torch.arange(c.shape[0] - self.max_size, c.shape[0], device=c.device))
            self.c[k] = c

    def size(self):
        return self.c["dones"].shape[0] if self.c else 0

    def get_mini_batch(self, size):
        idx = torch.randint(0, self.size(), (size,), device="cuda:0")
        return {k: torch.index_select(v, 0, idx) for k, v in self.c.items()}


def make_env(N, W, A):
    prices, day_id, _ = make_series(A)
    return finenvs_amd.TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=W, num_envs=N, redraw="device", seed=0)


def fill(env, buf, steps):
    """`steps` env steps stored through double-buffered descriptors; returns the last step's tensors."""
    N, A = env.num_envs, env.num_assets
    desc = [env.describe(), (torch.empty(N, dtype=torch.int64, device="cuda"), torch.empty((N, A), dtype=torch.float64, device="cuda"))]
    a = torch.rand((N, A), device="cuda") * 2 - 1
    for t in range(steps):
        _, r, d, _ = env.step(a, descriptors_out=desc[(t + 1) % 2])
        buf.store(desc[t % 2], a, r, desc[(t + 1) % 2], d)
    return desc, a, r, d


def profile(args):
    env = make_env(args.envs, args.window, 1)
    buf = ReplayBuffer(env, max_size=args.capacity)
    fill(env, buf, -(-args.capacity // args.envs) + 1)
    idx = torch.randint(0, buf.size(), (args.profile,), device="cuda")
    for _ in range(60):
        buf.get_mini_batch(args.profile, indices=idx)
    torch.cuda.synchronize()


def report_stats(args):
    with open(args.kernel_stats) as f:
        rows = [r for r in csv.DictReader(f) if "fe_replay_sample_kernel" in r["Name"]]
    ns = float(rows[0]["AverageNs"])
    nb = sample_bytes(args.batch, args.window, 1)
    print(f"fe_replay_sample_kernel B = {args.batch:6d}: {ns / 1e3:8.2f} us (rocprofv3 average of {rows[0]['Calls']} calls), "
          f"{nb / 1e6:.1f} MB written, {nb / ns / 1e3:.2f} TB/s = {nb / ns / 1e3 / (HBM_BYTES_PER_S / 1e12):.1%} of 8 TB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--window", type=int, default=64)
    ap.add_argument("--capacity", type=int, default=1_000_000)
    ap.add_argument("--profile", type=int, default=0, help="only run sample launches of this batch size (for rocprofv3)")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 kernel_stats.csv of a --profile run")
    ap.add_argument("--batch", type=int, default=65536)
    args = ap.parse_args()
    if args.kernel_stats is not None:
        return report_stats(args)
    assert torch.cuda.is_available(), "replay_bench runs on the GPU"
    torch.manual_seed(0)
    if args.profile:
        return profile(args)
    N, W, C = args.envs, args.window, args.capacity
    res = {"envs": N, "window": W, "assets": 1, "capacity": C}

    env = make_env(N, W, 1)
    buf = ReplayBuffer(env, max_size=C)
    desc, a, r, d = fill(env, buf, -(-C // N) + 1)  # at capacity
    res["ring_store_us"] = timed(lambda: buf.store(desc[0], a, r, desc[1], d), 200)
    print(f"device ring store     : {res['ring_store_us']:10.1f} us  (N = {N}, capacity {C}, {buf.size()} retained)")
    for B in (4096, 65536):
        res[f"ring_sample_{B}_us"] = timed(lambda: buf.get_mini_batch(B), 100)
        idx = torch.randint(0, buf.size(), (B,), device="cuda")
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                buf.get_mini_batch(B, indices=idx)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(20):
                buf.get_mini_batch(B, indices=idx)
        res[f"ring_sample_{B}_graph_us"] = timed(g.replay, 20) / 20
        nb = sample_bytes(B, W, 1)
        res[f"ring_sample_{B}_bytes"] = nb
        print(f"device get_mini_batch : {res[f'ring_sample_{B}_us']:10.1f} us  (B = {B}, default draw, end to end); "
              f"{res[f'ring_sample_{B}_graph_us']:.1f} us device time per launch in a graph, {nb / 1e6:.1f} MB written "
              f"= {nb / res[f'ring_sample_{B}_graph_us'] / 1e6:.2f} TB/s")
    del buf
    torch.cuda.empty_cache()

    # the restatement: rendered observations; capacity as large as fits (2 x 1280 B per transition for the states alone)
    free = torch.cuda.mem_get_info()[0]
    per = 2 * W * 5 * 4 + 12
    Cref = min(C, int(free * 0.3 / per) // N * N)
    ref = TorchBuffer(Cref)
    obs = env.reset().clone()
    for _ in range(-(-Cref // N) + 1):
        nobs, r, d, _ = env.step(a)
        ref.store(states=obs, actions=a, rewards=r, next_states=nobs, dones=d)
        obs = nobs.clone()
    res["torch_capacity"] = Cref
    res["torch_store_us"] = timed(lambda: ref.store(states=obs, actions=a, rewards=r, next_states=nobs, dones=d), 10)
    print(f"torch restatement store: {res['torch_store_us']:10.1f} us  (capacity {Cref}, {ref.size()} retained)")
    for B in (4096, 65536):
        res[f"torch_sample_{B}_us"] = timed(lambda: ref.get_mini_batch(B), 50)
        print(f"torch get_mini_batch  : {res[f'torch_sample_{B}_us']:10.1f} us  (B = {B})")
    res["store_speedup"] = res["torch_store_us"] / res["ring_store_us"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
