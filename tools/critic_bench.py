"""GPU box: time per mini-batch of SAC's target half (compute_targets, SAC_agent.py:200-227) -- fused against torch as
examples/sac_time_series.py computes it -- and the example's whole training iteration with and without fused targets.

  fused          FusedTwinCritic.sac_targets: descriptor gather, FusedSACRollout.forward (the actor), fe_twin_q_target
                 (both target critics, min, entropy term, Bellman combination), incl. the per-call weight re-packs
  torch_eager    ReplayBuffer.get_mini_batch (renders next_states), the actor, two nn.LSTM critics, the epilogue
  torch_graphed  the same captured once in a torch.cuda.graph and replayed

Device-synchronised timing after a warm-up; the arms alternate within one process and every figure is the median of
--reps rounds.  The MFMA rate below is from shapes, 2 * B * W * 4H * (H + 8) FLOP per critic, over the fused wall time
(actor and gather included); the kernel-only time comes from a separate rocprofv3 --kernel-trace --stats run.

    timeout -k 10 900 python tools/critic_bench.py [--batch 256 4096 65536] [--hidden 32 64 128] [--window 4]

Prints one line per (H, B, arm) and a final JSON line (profiles/critic_bench.txt).
"""
import argparse
import json
import math
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

GAMMA = 0.99
LOG_SQRT_2PI = 0.5 * math.log(2 * math.pi)


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
        actor = SACActorLSTM(H=H, W=W).cuda()
        c1, c2 = CriticLSTM(H, W).cuda(), CriticLSTM(H, W).cuda()
        roll = FusedSACRollout(env, actor)
        traj = TrajectoryBuffer(K, N, 1, device=env._dev, states=True)
        roll.run(K, noise=torch.randn((K, N, 1), device="cuda"), trajectory=traj)
        buffer = ReplayBuffer(env, max_size=K * N)
        buffer.extend(traj)
        twin = FusedTwinCritic(env, c1, c2)
        for B in a.batch:
            idx = torch.randint(0, buffer.size(), (B,), device="cuda")
            eps = torch.randn((B, 1), device="cuda")

            def fused():
                return twin.sac_targets(buffer, idx, roll, eps, GAMMA, actor.log_alpha)

            def torch_targets():  # the example's compute_targets, Normal's log_prob written out (no host sync: capturable)
                b = buffer.get_mini_batch(B, indices=idx)
                s2, r, d = b["next_states"], b["rewards"], b["dones"]
                with torch.no_grad():
                    z = actor(s2)
                    mu, sd = actor.mu_layer(z), F.softplus(actor.std_layer(z))
                    u = mu + eps * sd
                    a2 = torch.tanh(u)
                    lp = -((u - mu) ** 2) / (2 * sd * sd) - sd.log() - LOG_SQRT_2PI - torch.log(1 - a2.pow(2) + 1e-7)
                    q = torch.min(c1(s2, a2), c2(s2, a2))
                    return r + GAMMA * (1.0 - d) * (q - actor.log_alpha.exp() * lp)

            arms = {"fused": fused, "torch_eager": torch_targets}
            try:
                torch_targets()
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(2):
                        torch_targets()
                torch.cuda.current_stream().wait_stream(side)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    torch_targets()
                arms["torch_graphed"] = graph.replay
            except Exception as exc:  # noqa: BLE001  (reported, not hidden)
                print(f"H={H} B={B}: torch_graphed not capturable: {exc}", flush=True)
            for fn in arms.values():
                fn()
            times = {k: [] for k in arms}
            for _ in range(a.rounds):
                for k, fn in arms.items():
                    times[k].append(timed(fn))
            flop = 2 * 2 * B * W * 4 * H * (H + 8)
            res = out["results"].setdefault(str(H), {}).setdefault(str(B), {})
            for k, ts in times.items():
                us = 1e6 * statistics.median(ts)
                res[k] = {"us_per_batch": us}
                print(f"H={H:4d} B={B:6d} {k:14s}: {us:10.1f} us/mini-batch", flush=True)
            res["critic_tflops_over_fused_wall"] = flop / (res["fused"]["us_per_batch"] * 1e-6) / 1e12
            for k in arms:
                if k != "fused":
                    res[f"{k}_over_fused"] = res[k]["us_per_batch"] / res["fused"]["us_per_batch"]
            if "torch_graphed" in arms:
                del graph
        del roll, buffer, traj, twin
        torch.cuda.empty_cache()
    if not a.no_example:
        import sac_time_series

        kw = dict(num_envs=1024, chunk=8, batch=256, quiet=True)
        it = {"plain": [], "fused_targets": []}
        for fused in (False, True):  # warm-up (library, kernels, allocator)
            sac_time_series.main(iterations=3, fused_targets=fused, **kw)
        for _ in range(3):
            for key, fused in (("plain", False), ("fused_targets", True)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sac_time_series.main(iterations=20, fused_targets=fused, **kw)
                torch.cuda.synchronize()
                it[key].append((time.perf_counter() - t0) / 20)
        out["example_iteration_ms"] = {k: 1e3 * statistics.median(v) for k, v in it.items()}
        print("example (1024 envs, chunk 8, batch 256, H 128) ms per iteration:", out["example_iteration_ms"], flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
