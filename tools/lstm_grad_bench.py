"""GPU box: time per PPO minibatch update of the LSTM actor and the LSTM critic (compute_actor_loss + backward,
compute_critic_loss + backward; PPO/continuous_actor.py:59-78, PPO/critic.py:26-32) -- fused against torch as
examples/ppo_lstm_fused.py computes it -- and the example's whole training iteration with and without --fused-update.

  fused          ppo_actor_loss and ppo_critic_loss of finenvs_amd/lstm_head.py on the minibatch's descriptors, each with
                 backward(): descriptor gather, twice fe_lstm_forward, twice fe_lstm_backward (transpose, backward
                 through time, reduction) and the .grad accumulation, incl. the per-call weight re-packs and the two
                 4-byte bias copies to the host
  torch_eager    TrajectoryBuffer.minibatch_states (renders the states) + the nn.LSTM actor and critic + both losses +
                 both backward passes
  torch_graphed  the same captured once in a torch.cuda.graph and replayed (gradients accumulate in place); captured
                 with torch.distributions' argument validation off, whose host read a capture does not permit

No optimizer step in any arm (it is the same in all).  Device-synchronised timing after a warm-up; the arms alternate
within one process and every figure is the median of --rounds rounds.

    timeout -k 10 900 python tools/lstm_grad_bench.py [--batch 256 4096 65536] [--hidden 32 64 128] [--window 4]
    timeout -k 10 900 python tools/lstm_grad_bench.py --hidden 256 512 1024 --example-hidden 1024

Prints one line per (H, B, arm) and a final JSON line (profiles/lstm_grad_bench.txt; the large sizes:
profiles/lstm_grad_streamed_bench.txt).
"""
import argparse
import copy
import importlib.util
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
from finenvs_amd.lstm_head import (FusedLSTMHead, LSTMHead, ppo_actor_loss, ppo_critic_loss,  # noqa: E402
                                   torch_ppo_actor_loss, torch_ppo_critic_loss)
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
    ap.add_argument("--hidden", type=int, nargs="+", default=[32, 64, 128], choices=[32, 64, 128, 256, 512, 1024])
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-example", action="store_true")
    ap.add_argument("--example-hidden", type=int, default=64, choices=[32, 64, 128, 256, 512, 1024])
    ap.add_argument("--example-iters", type=int, default=5)
    a = ap.parse_args()
    W, N, K = a.window, 4096, 16
    prices, day_id, _ = make_series(1)
    env = finenvs_amd.TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=W, num_envs=N, redraw="device",
                                    obs_dtype=torch.float32)
    out = {"window": W, "results": {}}
    for H in a.hidden:
        torch.manual_seed(H)
        actor, critic = LSTMHead(H, W, "tanh", device="cuda"), LSTMHead(H, W, "none", device="cuda")
        actor_head = FusedLSTMHead(env, actor, streamed=H > 128)
        critic_head = FusedLSTMHead(env, critic, streamed=H > 128)
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
                print(f"H={H:4d} B={B:6d} {k:14s}: {us:10.1f} us/actor + critic update", flush=True)
            for k in arms:
                if k != "fused":
                    res[f"{k}_over_fused"] = res[k]["us_per_update"] / res["fused"]["us_per_update"]
            if "torch_graphed" in arms:
                del graph
        del actor_head, critic_head, traj
        torch.cuda.empty_cache()
    if not a.no_example:
        spec = importlib.util.spec_from_file_location("ppo_lstm_fused", os.path.join(REPO, "examples", "ppo_lstm_fused.py"))
        example = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(example)
        modes = {"plain": {}, "fused_update": {"fused_update": True}}
        it = {k: [] for k in modes}
        EH, iters = a.example_hidden, a.example_iters
        for m in modes.values():  # warm-up (library, kernels, allocator)
            example.main(iters=2, hidden=EH, quiet=True, **m)
        for _ in range(3):
            for key, m in modes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                example.main(iters=iters, hidden=EH, quiet=True, **m)
                torch.cuda.synchronize()
                it[key].append((time.perf_counter() - t0) / iters)
        out["example_hidden"] = EH
        out["example_iteration_ms"] = {k: 1e3 * statistics.median(v) for k, v in it.items()}
        print(f"example (defaults: 4096 envs, 16 steps, 2 epochs x 4 minibatches; H {EH}) ms per iteration:",
              out["example_iteration_ms"], flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
