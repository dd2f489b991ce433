"""GPU box: the two-hidden-layer MLP head (include/finenvs_amd_mlp2_head.h) against torch, in the manner of
tools/mlp_grad_bench.py: time per PPO minibatch update of the (5W, H, H, 1) actor and critic (compute_actor_loss +
backward, compute_critic_loss + backward) and env-steps/s of the sampled rollout.

  fused          ppo_actor_loss and ppo_critic_loss of finenvs_amd/lstm_head.py with FusedMLP2Heads on the minibatch's
                 descriptors, each with backward(): descriptor gather, twice fe_mlp_pack + five copies + fe_mlp2_forward,
                 twice fe_mlp2_backward (six launches) and the .grad accumulation
  torch_eager    TrajectoryBuffer.minibatch_states (renders the states: the arm pays its own render) + the MLP2Head actor
                 and critic + both losses + both backward passes
  torch_graphed  the same captured once in a torch.cuda.graph and replayed; captured with torch.distributions' argument
                 validation off, whose host read a capture does not permit

No optimizer step in any arm.  Device-synchronised timing after a warm-up; the arms alternate within one process and
every figure is the median of --rounds rounds.

  rollout        env-steps/s at --envs envs, K = 16 steps per launch or replay, alternating in the same process:
                 mlp2     FusedMLP2Rollout.run with noise, means and descriptor rows (fe_env_rollout_mlp2_sampled)
                 mlp1     FusedMLPRollout.run of the one-layer head of the same H, the same outputs
                 torch    GraphedRollout: K x (MLP2Head(obs) + std * noise, clamped, env.step) captured in a graph

    timeout -k 10 900 python tools/mlp2_grad_bench.py [--batch 256 4096 65536] [--hidden 32 64 128] [--window 4]

Prints one line per (W, H, B, arm) and a final JSON line (profiles/mlp2_grad_bench.txt).
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
from finenvs_amd.lstm_head import ppo_actor_loss, ppo_critic_loss, torch_ppo_actor_loss, torch_ppo_critic_loss  # noqa: E402
from finenvs_amd.mlp2_head import FusedMLP2Head, MLP2Head, mlp2_head_parameters  # noqa: E402
from finenvs_amd.rollout import FusedMLP2Rollout, FusedMLPRollout, GraphedRollout  # noqa: E402
from finenvs_amd.trajectory import TrajectoryBuffer  # noqa: E402


def timed(fn, reps=3):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def head(H, W, output):
    m = MLP2Head(H, W, "elu", output, device="cuda")
    with torch.no_grad():  # log-returns are ~1e-3: scale their columns so that the hidden units see them
        m.network[0].weight.reshape(H, W, 5)[:, :, :4].mul_(100.0 / math.sqrt(W))
    return m


def updates(a, W, out):
    N, K = 4096, 16
    prices, day_id, _ = make_series(1)
    env = finenvs_amd.TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=W, num_envs=N, redraw="device",
                                    obs_dtype=torch.float32)
    for H in a.hidden:
        torch.manual_seed(H)
        actor, critic = head(H, W, "tanh"), head(H, W, "none")
        actor_head, critic_head = FusedMLP2Head(env, actor), FusedMLP2Head(env, critic)
        t_actor, t_critic = copy.deepcopy(actor), copy.deepcopy(critic)
        log_std = torch.full((1, 1), math.log(0.5), device="cuda", requires_grad=True)
        t_log_std = log_std.detach().clone().requires_grad_(True)
        traj = TrajectoryBuffer(K, N, 1, device=env._dev, states=True)
        noise = torch.randn((K, N, 1), device="cuda")
        actor_head.rollout.sync_from_env()
        actions, _, _ = actor_head.rollout.run(K, noise=noise, std=0.5, record_means=True, trajectory=traj)
        flat = lambda x: x.reshape(K, N).t().reshape(K * N, 1)  # noqa: E731
        with torch.no_grad():
            f_act = flat(actions)
            f_logp = flat(torch.distributions.Normal(actor_head.rollout.means, 0.5).log_prob(actions)) - 0.05
            f_adv, f_ret = torch.randn((K * N, 1), device="cuda"), torch.randn((K * N, 1), device="cuda")
        for B in a.batch:
            mb = torch.randint(0, K * N, (B,), device="cuda")
            act, logp, adv, ret = f_act[mb], f_logp[mb], f_adv[mb], f_ret[mb]

            def fused():
                src, pos = traj.minibatch_descriptors(mb)
                ppo_actor_loss(actor_head, log_std, src, pos, act, logp, adv, 0.2, 0.01).backward()
                ppo_critic_loss(critic_head, src, pos, ret).backward()

            def torch_update():
                s = traj.minibatch_states(env, mb)
                torch_ppo_actor_loss(t_actor(s), t_log_std, act, logp, adv, 0.2, 0.01).backward()
                torch_ppo_critic_loss(t_critic(s), ret).backward()

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
                print(f"W={W} H={H} B={B}: torch_graphed not capturable: {exc}", flush=True)
            finally:
                Distribution.set_default_validate_args(True)
            for fn in arms.values():
                fn()
            times = {k: [] for k in arms}
            for _ in range(a.rounds):
                for k, fn in arms.items():
                    times[k].append(timed(fn))
            res = out["updates"].setdefault(str(W), {}).setdefault(str(H), {}).setdefault(str(B), {})
            for k, ts in times.items():
                us = 1e6 * statistics.median(ts)
                res[k] = {"us_per_update": us}
                print(f"W={W:3d} H={H:4d} B={B:6d} {k:14s}: {us:10.1f} us/actor + critic update", flush=True)
            for k in arms:
                if k != "fused":
                    res[f"{k}_over_fused"] = res[k]["us_per_update"] / res["fused"]["us_per_update"]
            if "torch_graphed" in arms:
                del graph
        del actor_head, critic_head, traj
        torch.cuda.empty_cache()


def rollouts(a, W, out):
    N, K = a.envs, 16
    prices, day_id, _ = make_series(1)
    for H in a.hidden:
        torch.manual_seed(H)
        module = head(H, W, "tanh")
        w1, b1, w2, b2, w3, b3 = (p.detach() for p in mlp2_head_parameters(module))
        # one env per arm (a rollout object owns its env's descriptors); the same days, first layer and launch geometry
        envs = [finenvs_amd.TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=W, num_envs=N, redraw="device",
                                          obs_dtype=torch.float32, obs_buffers=2 * (i == 2)) for i in range(3)]  # the graph's ring
        two = FusedMLP2Rollout(envs[0], w1.t(), b1, w2, b2, w3, float(b3), output_activation="tanh")
        one = FusedMLPRollout(envs[1], w1.t(), b1, w3, float(b3), output_activation="tanh")
        noise = torch.randn((K, N, 1), device="cuda")
        trajs = [TrajectoryBuffer(K, N, 1, device=envs[i]._dev, states=True) for i in range(2)]

        def run(roll, traj):
            traj.clear()
            roll.run(K, noise=noise, std=0.5, record_means=True, trajectory=traj)

        with torch.no_grad():
            graphed = GraphedRollout(envs[2], lambda obs, k: (module(obs) + 0.5 * noise[k]).clamp(-1.0, 1.0), K)
        arms = {"mlp2": lambda: run(two, trajs[0]), "mlp1": lambda: run(one, trajs[1]), "torch": graphed.run}
        for fn in arms.values():
            fn()
        times = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, fn in arms.items():
                times[k].append(timed(fn))
        res = out["rollout"].setdefault(str(W), {}).setdefault(str(H), {"envs": N, "steps_per_launch": K})
        for k, ts in times.items():
            t = statistics.median(ts)
            res[k] = {"env_steps_per_s": N * K / t, "us_per_env_step": 1e6 * t / K}
            print(f"W={W:3d} H={H:4d} rollout {k:6s}: {res[k]['env_steps_per_s'] / 1e9:7.3f} G env-steps/s, "
                  f"{res[k]['us_per_env_step']:8.1f} us per step of {N} envs", flush=True)
        res["mlp2_over_mlp1"] = res["mlp2"]["env_steps_per_s"] / res["mlp1"]["env_steps_per_s"]
        res["mlp2_over_torch"] = res["mlp2"]["env_steps_per_s"] / res["torch"]["env_steps_per_s"]
        del two, one, graphed, envs, trajs
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[256, 4096, 65536])
    ap.add_argument("--hidden", type=int, nargs="+", default=[32, 64, 128], choices=[32, 64, 128])
    ap.add_argument("--window", type=int, nargs="+", default=[4])
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-rollout", action="store_true")
    a = ap.parse_args()
    out = {"updates": {}, "rollout": {}}
    for W in a.window:
        updates(a, W, out)
        if not a.no_rollout:
            rollouts(a, W, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
