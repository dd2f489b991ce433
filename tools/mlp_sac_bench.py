"""GPU box: SAC with the reference's MLP actor (include/finenvs_amd_mlp_sac.h) against the project's own MLP heads and
against torch, in the manner of tools/mlp_critic_bench.py and tools/mlp2_grad_bench.py.

  rollout   us per step of --envs envs, K = 16 steps per launch or replay, alternating in the same process:
            sac      FusedMLPSACRollout.run with noise, means, stds and descriptor rows (fe_env_rollout_mlp_sac: the folded head)
            sac_bare the same launch without the means / stds outputs
            sac_packed  the sac arm on weights packed once (the heads' rollouts keep packed weights; FusedMLPSACRollout
                     re-packs and re-folds per run(): one pack launch and a dozen small device copies)
            mlp1     FusedMLPRollout.run of a one-layer head of the same H and first layer (what the fold is meant to recover)
            mlp2     FusedMLP2Rollout.run of a two-layer head of the same H (what the actor would cost unfolded)
            torch    GraphedRollout: K x (SACActorMLP sample + env.step) captured in a graph
  actor     one actor update on a mini-batch of B transitions of a full replay ring: sample, min q through FROZEN critics,
            backward.  fused: FusedMLPSACRollout.actor_losses(...)[0].backward() on descriptors; torch_eager:
            ReplayBuffer.get_mini_batch (the arm pays its own render) + torch_sac_mlp_actor_losses + backward;
            torch_eager_shared: the same on an already rendered mini-batch; torch_graphed(_shared): captured and replayed
  targets   one sac_targets call at the same sizes: FusedTwinMLPCritic.sac_targets against torch_sac_targets on a rendered
            mini-batch, eager and graphed

No optimizer step in any arm.  Device-synchronised timing after a warm-up; the arms alternate within one process and
every figure is the median of --rounds rounds.

    timeout -k 10 900 python tools/mlp_sac_bench.py [--batch 256 4096 65536] [--hidden 32 64 128] [--window 4]

Prints one line per measurement and a final JSON line (profiles/mlp_sac_bench.txt).
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
from torch.distributions import Distribution

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import finenvs_amd  # noqa: E402
from bench import make_series  # noqa: E402
from finenvs_amd.critic import torch_sac_targets  # noqa: E402
from finenvs_amd.mlp_critic import FusedTwinMLPCritic, MLPCritic  # noqa: E402
from finenvs_amd.mlp_sac import FusedMLPSACRollout, SACActorMLP, torch_sac_mlp_actor_losses  # noqa: E402
from finenvs_amd.replay import ReplayBuffer  # noqa: E402
from finenvs_amd.rollout import FusedMLP2Rollout, FusedMLPRollout, GraphedRollout  # noqa: E402
from finenvs_amd.trajectory import TrajectoryBuffer  # noqa: E402

GAMMA = 0.99


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
    Distribution.set_default_validate_args(False)  # Normal's argument check reads the device: not capturable
    try:
        with torch.cuda.graph(graph):
            fn()
    finally:
        Distribution.set_default_validate_args(True)
    return graph


def measure(arms, rounds):
    for fn in arms.values():
        fn()
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            times[k].append(timed(fn))
    return {k: statistics.median(ts) for k, ts in times.items()}


def rollouts(a, W, out):
    N, K = a.envs, 16
    prices, day_id, _ = make_series(1)
    for H in a.hidden:
        torch.manual_seed(H)
        actor = scaled(SACActorMLP(H, W, device="cuda"), H, W)
        w1, b1 = actor.network[0].weight.detach(), actor.network[0].bias.detach()
        w2, b2 = actor.network[2].weight.detach(), actor.network[2].bias.detach()
        wmu, bmu = actor.mu_layer.weight.detach().reshape(H), float(actor.mu_layer.bias.detach())
        # one env per arm (a rollout object owns its env's descriptors); the same days, first layer and launch geometry
        envs = [finenvs_amd.TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=W, num_envs=N, redraw="device",
                                          obs_dtype=torch.float32, obs_buffers=2 * (i == 3)) for i in range(4)]  # the graph's ring
        sac = FusedMLPSACRollout(envs[0], actor)
        one = FusedMLPRollout(envs[1], w1.t(), b1, wmu, bmu, output_activation="tanh")
        two = FusedMLP2Rollout(envs[2], w1.t(), b1, w2, b2, wmu, bmu, output_activation="tanh")
        noise = torch.randn((K, N, 1), device="cuda")
        trajs = [TrajectoryBuffer(K, N, 1, device=envs[i]._dev, states=True) for i in range(3)]

        def run_sac():
            trajs[0].clear()
            sac.run(K, noise=noise, record_means=True, record_stds=True, trajectory=trajs[0])

        def run_sac_bare():  # the same launch without the means / stds outputs: what those two (K, N) stores cost
            trajs[0].clear()
            sac.run(K, noise=noise, trajectory=trajs[0])

        packed = sac._weights()  # (sac._packed keeps its buffers alive)

        def run_sac_packed():  # the same launch and outputs on weights packed ONCE: what run() spends re-packing per call
            sac._weights = lambda: packed
            try:
                run_sac()
            finally:
                del sac._weights

        def run_head(roll, traj):
            traj.clear()
            roll.run(K, noise=noise, std=0.5, record_means=True, trajectory=traj)

        def policy(obs, k):
            dist = actor.get_distribution(obs.reshape(N, 5 * W))
            return torch.tanh(dist.loc + noise[k] * dist.scale)

        Distribution.set_default_validate_args(False)  # (as in graphed(): the capture is inside the constructor)
        try:
            with torch.no_grad():
                torch_loop = GraphedRollout(envs[3], policy, K)
        finally:
            Distribution.set_default_validate_args(True)
        arms = {"sac": run_sac, "sac_bare": run_sac_bare, "sac_packed": run_sac_packed, "mlp1": lambda: run_head(one, trajs[1]), "mlp2": lambda: run_head(two, trajs[2]),
                "torch": torch_loop.run}
        res = out["rollout"].setdefault(str(H), {"envs": N, "steps_per_launch": K})
        for k, t in measure(arms, a.rounds).items():
            res[k] = {"env_steps_per_s": N * K / t, "us_per_env_step": 1e6 * t / K}
            print(f"W={W:3d} H={H:4d} rollout {k:10s}: {res[k]['env_steps_per_s'] / 1e9:7.3f} G env-steps/s, "
                  f"{res[k]['us_per_env_step']:8.1f} us per step of {N} envs", flush=True)
        for k in ("mlp1", "mlp2", "torch"):
            res[f"sac_over_{k}"] = res["sac"]["env_steps_per_s"] / res[k]["env_steps_per_s"]
        del sac, one, two, torch_loop, envs, trajs
        torch.cuda.empty_cache()


def updates(a, W, out):
    N, K = 4096, 16
    prices, day_id, _ = make_series(1)
    env = finenvs_amd.TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=W, num_envs=N, redraw="device",
                                    obs_dtype=torch.float32)
    for H in a.hidden:
        torch.manual_seed(H)
        actor = scaled(SACActorMLP(H, W, device="cuda"), H, W)
        c1, c2 = (scaled(MLPCritic(H, W, device="cuda"), H, W).requires_grad_(False) for _ in range(2))
        t_actor = copy.deepcopy(actor)  # the torch arms' own .grad
        roll, twin = FusedMLPSACRollout(env, actor), FusedTwinMLPCritic(env, c1, c2)
        buffer = ReplayBuffer(env, max_size=N * K)
        traj = TrajectoryBuffer(K, N, 1, device=env._dev, states=True)
        roll.sync_from_env()
        roll.run(K, noise=torch.randn((K, N, 1), device="cuda"), trajectory=traj)
        buffer.extend(traj)
        for B in a.batch:
            idx = torch.randint(0, buffer.size(), (B,), device="cuda")
            eps = torch.randn((B, 1), device="cuda")
            shared = buffer.get_mini_batch(B, indices=idx)
            shared_states = shared["states"].float()

            def fused_actor():
                roll.actor_losses(buffer, idx, twin, eps)[0].backward()

            def torch_actor():
                b = buffer.get_mini_batch(B, indices=idx)
                torch_sac_mlp_actor_losses(t_actor, c1, c2, b["states"].float(), eps)[0].backward()

            def torch_actor_shared():
                torch_sac_mlp_actor_losses(t_actor, c1, c2, shared_states, eps)[0].backward()

            def fused_targets():
                twin.sac_targets(buffer, idx, roll, eps, GAMMA, actor.log_alpha)

            def torch_targets():
                b = buffer.get_mini_batch(B, indices=idx)
                torch_sac_targets(t_actor, c1, c2, b["rewards"], b["next_states"].float(), b["dones"], eps, GAMMA)

            def torch_targets_shared():
                torch_sac_targets(t_actor, c1, c2, shared["rewards"], shared["next_states"].float(), shared["dones"], eps, GAMMA)

            groups = {"actor": {"fused": fused_actor, "torch_eager": torch_actor, "torch_eager_shared": torch_actor_shared},
                      "targets": {"fused": fused_targets, "torch_eager": torch_targets, "torch_eager_shared": torch_targets_shared}}
            graphs = []
            for update, by_arm in groups.items():
                for key in ("torch_eager", "torch_eager_shared"):
                    try:
                        g = graphed(by_arm[key])
                        graphs.append(g)
                        by_arm[key.replace("eager", "graphed")] = g.replay
                    except Exception as exc:  # noqa: BLE001  (reported, not hidden)
                        print(f"W={W} H={H} B={B} {update} {key}: not capturable: {exc}", flush=True)
            for update, by_arm in groups.items():
                res = out["updates"].setdefault(str(H), {}).setdefault(str(B), {}).setdefault(update, {})
                for k, t in measure(by_arm, a.rounds).items():
                    res[k] = {"us_per_call": 1e6 * t}
                    print(f"W={W:3d} H={H:4d} B={B:6d} {update:7s} {k:22s}: {res[k]['us_per_call']:10.1f} us", flush=True)
                for k in by_arm:
                    if k != "fused":
                        res[f"{k}_over_fused"] = res[k]["us_per_call"] / res["fused"]["us_per_call"]
            del graphs
        del roll, twin, buffer, traj
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[256, 4096, 65536])
    ap.add_argument("--hidden", type=int, nargs="+", default=[32, 64, 128], choices=[32, 64, 128])
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-rollout", action="store_true")
    ap.add_argument("--no-updates", action="store_true")
    a = ap.parse_args()
    out = {"window": a.window, "updates": {}, "rollout": {}}
    if not a.no_rollout:
        rollouts(a, a.window, out)
    if not a.no_updates:
        updates(a, a.window, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
