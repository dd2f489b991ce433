"""GPU box: time per SAC actor update (sample, min of the twin critics, the actor loss, backward; SAC/actor.py:63-81) --
fused against torch as examples/sac_time_series.py computes it -- and the example's whole training iteration for the
combinations of --fused-targets / --fused-critics / --fused-actor.

  fused          FusedSACRollout.sample on the ring's state descriptors, torch.min(*FusedTwinCritic.q(...)), the loss
                 and backward(): descriptor gather, fe_sac_forward, fe_twin_q_forward, fe_twin_q_backward (dQ/da; the
                 critics are frozen, as an actor update needs none of their gradients), fe_sac_backward (transposes,
                 backward through time, reduction) and the .grad accumulation, incl. the per-call weight re-packs
  torch_eager    ReplayBuffer.get_mini_batch (renders the states) + the nn.LSTM actor + two nn.LSTM critics + the loss +
                 backward (critics frozen, too)
  torch_graphed  the same captured once in a torch.cuda.graph and replayed (gradients accumulate in place); captured
                 with torch.distributions' argument validation off, whose host read a capture does not permit

Device-synchronised timing after a warm-up; the arms alternate within one process and every figure is the median of
--rounds rounds.

    timeout -k 10 900 python tools/sac_grad_bench.py [--batch 256 4096 65536] [--hidden 32 64 128] [--window 4]

Prints one line per (H, B, arm) and a final JSON line (profiles/sac_grad_bench.txt).
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch
from torch.distributions import Distribution

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
        actor = SACActorLSTM(H=H, W=W).cuda()
        roll = FusedSACRollout(env, actor)
        traj = TrajectoryBuffer(K, N, 1, device=env._dev, states=True)
        roll.run(K, noise=torch.randn((K, N, 1), device="cuda"), trajectory=traj)
        buffer = ReplayBuffer(env, max_size=K * N)
        buffer.extend(traj)
        c1, c2 = CriticLSTM(H, W).cuda().requires_grad_(False), CriticLSTM(H, W).cuda().requires_grad_(False)
        t_actor, t1, t2 = copy.deepcopy(actor), copy.deepcopy(c1), copy.deepcopy(c2)
        twin = FusedTwinCritic(env, c1, c2)
        alpha = actor.log_alpha.detach().exp()
        for B in a.batch:
            idx = torch.randint(0, buffer.size(), (B,), device="cuda")
            eps = torch.randn((B, 1), device="cuda")

            def fused():
                slots = buffer.physical(idx)
                src, pos = buffer.state_src[slots], buffer.state_pos[slots]
                a_new, lp = roll.sample(src, pos, eps)
                q = torch.min(*twin.q(src, pos, a_new))
                (-(q - alpha * lp.mean(dim=1, keepdim=True)).mean()).backward()

            def torch_update():
                s = buffer.get_mini_batch(B, indices=idx)["states"]
                a_new, lp = t_actor.get_actions_and_log_probs(s, eps)
                q = torch.min(t1(s, a_new), t2(s, a_new))
                (-(q - alpha * lp.mean(dim=1, keepdim=True)).mean()).backward()

            arms = {"fused": fused, "torch_eager": torch_update}
            try:
                # Normal's argument validation reads a device value on the host, which a capture does not permit: the
                # graphed arm is captured without it (a replay runs no Python, so this touches the capture only)
                Distribution.set_default_validate_args(False)
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
            finally:
                Distribution.set_default_validate_args(True)
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
                print(f"H={H:4d} B={B:6d} {k:14s}: {us:10.1f} us/actor update", flush=True)
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
        modes = {"plain": {}, "fused_actor": {"fused_actor": True},
                 "fused_targets_and_critics": {"fused_targets": True, "fused_critics": True},
                 "fused_critics_and_actor": {"fused_critics": True, "fused_actor": True},
                 "all_three": {"fused_targets": True, "fused_critics": True, "fused_actor": True}}
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
