"""GPU box: env-steps/s of the fused SAC rollout (finenvs_amd.sac.FusedSACRollout: K steps per launch, the SAC actor's
head in the kernel) against FusedLSTMRollout with noise at the same H, and against the unfused loop -- SACActorLSTM +
rsample + tanh + env.step, eager and captured in a GraphedRollout -- on the same GPU.

    timeout -k 10 900 python tools/sac_bench.py [--envs 65536] [--window 4] [--steps 32] [--hidden 32 64 128]

Prints one line per (H, arm) and a final JSON line (profiles/sac_bench.txt).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import finenvs_amd  # noqa: E402
from bench import make_series  # noqa: E402
from finenvs_amd.rollout import FusedLSTMRollout, GraphedRollout  # noqa: E402
from finenvs_amd.sac import FusedSACRollout, SACActorLSTM  # noqa: E402


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--hidden", type=int, nargs="+", default=[32, 64, 128])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    N, W, K = a.envs, a.window, a.steps
    prices, day_id, _ = make_series(1)

    def make_env():
        return finenvs_amd.TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=W, num_envs=N, redraw="device",
                                         obs_buffers=2)

    out = {"envs": N, "window": W, "steps_per_launch": K, "results": {}}

    def report(H, arm, ms_per_step):
        r = out["results"].setdefault(str(H), {})
        r[arm] = {"us_per_step": 1e3 * ms_per_step, "env_steps_per_s": N / (ms_per_step * 1e-3)}
        print(f"H={H:4d} {arm:22s}: {1e3 * ms_per_step:10.1f} us/step  {N / (ms_per_step * 1e-3):.3e} env-steps/s", flush=True)

    for H in a.hidden:
        torch.manual_seed(H)
        actor = SACActorLSTM(H=H, W=W).cuda()
        gen = torch.Generator(device="cuda").manual_seed(0)
        noise = torch.randn((K, N, 1), generator=gen, device="cuda")
        # ---- fused SAC
        env = make_env()
        roll = FusedSACRollout(env, actor)
        report(H, "fused_sac", timed(lambda: roll.run(K, noise=noise), a.reps) / K)
        # ---- fused LSTM actor (PPO's head) with noise, same H
        env = make_env()
        lin = torch.nn.Linear(H, 1)
        lroll = FusedLSTMRollout.from_modules(env, actor.lstm, lin)
        report(H, "fused_lstm", timed(lambda: lroll.run(K, noise=noise, std=0.5), a.reps) / K)
        del env, roll, lroll

        # ---- unfused: SACActorLSTM + rsample + tanh + env.step (SACAgent.step, the eval env on the mean)
        def policy(obs, k):  # get_distribution + rsample, without Normal's argument check (a host sync: not capturable)
            with torch.no_grad():
                z = actor(obs.float())
                mu, sd = actor.mu_layer(z), torch.nn.functional.softplus(actor.std_layer(z))
                actions = torch.tanh(mu + torch.randn_like(mu) * sd)
                actions[-1, :] = mu[-1, :]
            return actions

        env = make_env()
        state = {"obs": env.reset()}

        def eager():
            for k in range(K):
                state["obs"], _, _, _ = env.step(policy(state["obs"], k))

        report(H, "unfused_eager", timed(eager, max(1, a.reps // 2)) / K)
        del env
        env = make_env()
        env.reset()
        graphed = GraphedRollout(env, policy, K)
        report(H, "unfused_graphed", timed(graphed.run, a.reps) / K)
        del env, graphed
        r = out["results"][str(H)]
        r["sac_vs_lstm"] = r["fused_sac"]["us_per_step"] / r["fused_lstm"]["us_per_step"]
        r["speedup_vs_graphed"] = r["unfused_graphed"]["us_per_step"] / r["fused_sac"]["us_per_step"]
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
