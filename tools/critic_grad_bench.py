"""GPU box: time per critic update of SAC / TD3 (both critics: q, MSE, backward; SAC/critic.py:30-45) -- fused against
torch as examples/sac_time_series.py computes it -- and the example's whole training iteration with and without
--fused-critics.

  fused          FusedTwinCritic.critic_loss(buffer, idx, y).backward(): descriptor gather, fe_twin_q_forward, the MSE,
                 fe_twin_q_backward (transpose, backward through time, reduction), the un-permutation and the .grad
                 accumulation, incl. the per-call weight re-packs
  torch_eager    ReplayBuffer.get_mini_batch (renders the states) + two nn.LSTM critics + MSE + backward
  torch_graphed  the same captured once in a torch.cuda.graph and replayed (gradients accumulate in place)

Device-synchronised timing after a warm-up; the arms alternate within one process and every figure is the median of
--rounds rounds.  The kernel-only times come from a separate rocprofv3 --kernel-trace --stats run.

    timeout -k 10 900 python tools/critic_grad_bench.py [--batch 256 4096 65536] [--hidden 32 64 128] [--window 4]

Prints one line per (H, B, arm) and a final JSON line (profiles/critic_grad_bench.txt).
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "examples"))
import finenvs_amd  # noqa: E402
from bench import make_series  # noqa: E402
from finenvs_amd.critic import CriticLSTM, FusedTwinCritic  # noqa: E402
from finenvs_amd.replay import ReplayBuffer  # noqa: E402
from finenvs_amd.sac import FusedSACRollout, SACActorLSTM  # noqa: E402
from finenvs_amd.trajectory import TrajectoryBuffer  # noqa: E402


def timed(fn, reps=3):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[256, 4096, 65536])
    ap.add_argument("--hidden", type=int, nargs="+", default=[32, 64, 128])
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-example", action="store_true")
    a = ap.parse_args()
    W, N, K = a.window, 4096, 17
    prices, day_id, _ = make_series(1)
    env = finenvs_amd.TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=W, num_envs=N, redraw="device")
    out = {"window": W, "results": {}}
    for H in a.hidden:
        torch.manual_seed(H)
        roll = FusedSACRollout(env, SACActorLSTM(H=H, W=W).cuda())
        traj = TrajectoryBuffer(K, N, 1, device=env._dev, states=True)
        roll.run(K, noise=torch.randn((K, N, 1), device="cuda"), trajectory=traj)
        buffer = ReplayBuffer(env, max_size=K * N)
        buffer.extend(traj)
        c1, c2 = CriticLSTM(H, W).cuda(), CriticLSTM(H, W).cuda()
        t1, t2 = copy.deepcopy(c1), copy.deepcopy(c2)
        twin = FusedTwinCritic(env, c1, c2)
        for B in a.batch:
            idx = torch.randint(0, buffer.size(), (B,), device="cuda")
            y = torch.randn((B, 1), device="cuda")

            def fused():
                twin.critic_loss(buffer, idx, y).backward()

            def torch_update():
                b = buffer.get_mini_batch(B, indices=idx)
                s, act = b["states"], b["actions"]
                (F.mse_loss(t1(s, act), y) + F.mse_loss(t2(s, act), y)).backward()

            arms = {"fused": fused, "torch_eager": torch_update}
            try:
                torch_update()
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(2):
                        torch_update()
                torch.cuda.current_stream().wait_stream(side)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    torch_update()
                arms["torch_graphed"] = graph.replay
            except Exception as exc:  # noqa: BLE001  (reported, not hidden)
                print(f"H={H} B={B}: torch_graphed not capturable: {exc}", flush=True)
            for fn in arms.values():
                fn()
            times = {k: [] for k in arms}
            for _ in range(a.rounds):
                for k, fn in arms.items():
                    times[k].append(timed(fn))
            res = out["results"].setdefault(str(H), {}).setdefault(str(B), {})
            for k, ts in times.items():
                us = 1e6 * statistics.median(ts)
                res[k] = {"us_per_update": us}
                print(f"H={H:4d} B={B:6d} {k:14s}: {us:10.1f} us/critic update", flush=True)
            for k in arms:
                if k != "fused":
                    res[f"{k}_over_fused"] = res[k]["us_per_update"] / res["fused"]["us_per_update"]
            if "torch_graphed" in arms:
                del graph
        del roll, buffer, traj, twin
        torch.cuda.empty_cache()
    if not a.no_example:
        import sac_time_series

        kw = dict(num_envs=1024, chunk=8, batch=256, quiet=True)
        modes = {"plain": {}, "fused_targets": {"fused_targets": True},
                 "fused_targets_and_critics": {"fused_targets": True, "fused_critics": True},
                 "fused_critics": {"fused_critics": True}}
        it = {k: [] for k in modes}
        for m in modes.values():  # warm-up (library, kernels, allocator)
            sac_time_series.main(iterations=3, **kw, **m)
        for _ in range(3):
            for key, m in modes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sac_time_series.main(iterations=20, **kw, **m)
                torch.cuda.synchronize()
                it[key].append((time.perf_counter() - t0) / 20)
        out["example_iteration_ms"] = {k: 1e3 * statistics.median(v) for k, v in it.items()}
        print("example (1024 envs, chunk 8, batch 256, H 128) ms per iteration:", out["example_iteration_ms"], flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
