"""GPU box: TD3 with the reference's MLP networks (include/finenvs_amd_mlp_critic.h) against torch, in the manner of
tools/mlp_grad_bench.py: time per critic update (targets + both critics' loss and backward) and per delayed actor
update (Actor.compute_loss through critic 1 and backward) on a mini-batch of B transitions of a full replay ring.

  fused          on descriptors: FusedTwinMLPCritic.td3_targets (target actor fe_mlp2_forward, fe_twin_mlpq_target) and
                 critic_loss(...).backward() (fe_twin_mlpq_forward, fe_twin_mlpq_backward), every module re-packed on the
                 device per call; the actor update is td3_actor_loss(FusedMLP2Head, ..., twin).backward()
  torch_eager    ReplayBuffer.get_mini_batch (renders both states of every transition: the arm pays its own render) +
                 torch_td3_targets + the MLPCritic modules' loss and backward; the actor update renders again, as a
                 learner that keeps no mini-batch between the two would (TD3_agent.py:205-222 renders once per epoch:
                 `shared` below is the actor update on an already rendered mini-batch)
  torch_graphed  the same captured once in a torch.cuda.graph and replayed

No optimizer step in any arm.  Device-synchronised timing after a warm-up; the arms alternate within one process and
every figure is the median of --rounds rounds.  The replay memory both ways is stated too: 44 B per transition as
descriptors against 2 x 20 W + 12 B rendered in f32.

    timeout -k 10 900 python tools/mlp_critic_bench.py [--batch 256 4096 65536] [--hidden 32 64 128] [--window 4]

Prints one line per (W, H, B, update, arm) and a final JSON line (profiles/mlp_critic_bench.txt).
"""
import argparse
import copy
import json
import math
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import finenvs_amd  # noqa: E402
from bench import make_series  # noqa: E402
from finenvs_amd.critic import torch_td3_targets  # noqa: E402
from finenvs_amd.lstm_head import td3_actor_loss  # noqa: E402
from finenvs_amd.mlp2_head import FusedMLP2Head, MLP2Head  # noqa: E402
from finenvs_amd.mlp_critic import FusedTwinMLPCritic, MLPCritic, torch_mlp_critic_loss, torch_td3_actor_loss  # noqa: E402
from finenvs_amd.replay import ReplayBuffer  # noqa: E402
from finenvs_amd.trajectory import TrajectoryBuffer  # noqa: E402

GAMMA, STD, CLIP = 0.99, 0.2, 0.5


def timed(fn, reps=3):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def scaled(m, H, W):
    with torch.no_grad():  # log-returns are ~1e-3: scale their columns so that the hidden units see them
        m.network[0].weight[:, :5 * W].reshape(H, W, 5)[:, :, :4].mul_(100.0 / math.sqrt(W))
    return m


def graphed(fn):
    fn()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[256, 4096, 65536])
    ap.add_argument("--hidden", type=int, nargs="+", default=[32, 64, 128], choices=[32, 64, 128])
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    W, N, K = a.window, 4096, 16
    out = {"window": W, "transitions": N * K,
           "replay_bytes_per_transition": {"descriptors": 44, "rendered_f32": 2 * 20 * W + 12}, "updates": {}}
    prices, day_id, _ = make_series(1)
    env = finenvs_amd.TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=W, num_envs=N, redraw="device",
                                    obs_dtype=torch.float32)
    for H in a.hidden:
        torch.manual_seed(H)
        actor = scaled(MLP2Head(H, W, "elu", "tanh", device="cuda"), H, W)
        c1, c2 = (scaled(MLPCritic(H, W, device="cuda"), H, W) for _ in range(2))
        actor_t, c1t, c2t = copy.deepcopy(actor), copy.deepcopy(c1), copy.deepcopy(c2)
        t_actor, t_c1, t_c2 = copy.deepcopy(actor), copy.deepcopy(c1), copy.deepcopy(c2)  # the torch arms' own .grad
        head, head_t = FusedMLP2Head(env, actor), FusedMLP2Head(env, actor_t)
        twin, twin_t = FusedTwinMLPCritic(env, c1, c2), FusedTwinMLPCritic(env, c1t, c2t)
        buffer = ReplayBuffer(env, max_size=N * K)
        traj = TrajectoryBuffer(K, N, 1, device=env._dev, states=True)
        head.rollout.sync_from_env()
        head.rollout.run(K, noise=torch.randn((K, N, 1), device="cuda"), std=0.1, trajectory=traj)
        buffer.extend(traj)
        for B in a.batch:
            idx = torch.randint(0, buffer.size(), (B,), device="cuda")
            eps = torch.randn((B, 1), device="cuda")

            def fused_critic():
                y = twin_t.td3_targets(buffer, idx, head_t.rollout, eps, GAMMA, STD, CLIP)
                twin.critic_loss(buffer, idx, y).backward()

            def fused_actor():
                td3_actor_loss(head, buffer, idx, twin).backward()

            def torch_critic():
                b = buffer.get_mini_batch(B, indices=idx)
                y = torch_td3_targets(actor_t, c1t, c2t, b["rewards"], b["next_states"], b["dones"], eps, GAMMA, STD, CLIP)
                torch_mlp_critic_loss(t_c1, t_c2, b["states"].float(), b["actions"], y).backward()
                return b

            def torch_actor():
                b = buffer.get_mini_batch(B, indices=idx)
                torch_td3_actor_loss(t_actor, t_c1, b["states"].float()).backward()

            shared_states = buffer.get_mini_batch(B, indices=idx)["states"].float()

            def torch_actor_shared():
                torch_td3_actor_loss(t_actor, t_c1, shared_states).backward()

            arms = {"critic": {"fused": fused_critic, "torch_eager": torch_critic},
                    "actor": {"fused": fused_actor, "torch_eager": torch_actor, "torch_eager_shared": torch_actor_shared}}
            graphs = []
            for update, fn in (("critic", torch_critic), ("actor", torch_actor), ("actor_shared", torch_actor_shared)):
                try:
                    g = graphed(fn)
                    graphs.append(g)
                    key = "torch_graphed" + ("_shared" if update == "actor_shared" else "")
                    arms[update.split("_")[0]][key] = g.replay
                except Exception as exc:  # noqa: BLE001  (reported, not hidden)
                    print(f"W={W} H={H} B={B} {update}: torch_graphed not capturable: {exc}", flush=True)
            for update, by_arm in arms.items():
                for fn in by_arm.values():
                    fn()
                times = {k: [] for k in by_arm}
                for _ in range(a.rounds):
                    for k, fn in by_arm.items():
                        times[k].append(timed(fn))
                res = out["updates"].setdefault(str(H), {}).setdefault(str(B), {}).setdefault(update, {})
                for k, ts in times.items():
                    res[k] = {"us_per_update": 1e6 * statistics.median(ts)}
                    print(f"W={W:3d} H={H:4d} B={B:6d} {update:6s} {k:22s}: {res[k]['us_per_update']:10.1f} us", flush=True)
                for k in by_arm:
                    if k != "fused":
                        res[f"{k}_over_fused"] = res[k]["us_per_update"] / res["fused"]["us_per_update"]
            del graphs
        del head, head_t, twin, twin_t, buffer, traj
        torch.cuda.empty_cache()
    per = out["replay_bytes_per_transition"]
    print(f"replay memory per transition: {per['descriptors']} B as descriptors, {per['rendered_f32']} B rendered (f32, W = {W})")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
