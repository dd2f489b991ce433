"""GPU box: env-steps/s of the fused ES population (finenvs_amd.evo, one launch per K steps, noise generated in the
kernel) against a torch restatement of the reference's loop on the same GPU: ParallelMLP's per-env weight copies and
batched matmul (parallel_mlp.py:84-156) + env.step, with and without EvoAgent.store's per-step nonzero() / .item()
(evo_agent.py:96-112).

    timeout -k 10 600 python tools/evo_bench.py [--envs 16384] [--window 16] [--hidden 64] [--steps 32] [--assets 1]
                                                [--hidden-layers 2] [--streamed [--rounds 3] [--no-torch]]

``--hidden-layers 2``: the two-hidden-layer population (fe_evo2_rollout) against a three-layer ParallelMLP restated in
torch, and against the one-layer kernel at the same H where that exists (H = 32 / 64).

``--streamed``: the two-hidden-layer population with theta read through L2 (fe_evo2_rollout_streamed, H = 32 / 64 / 128 /
256) and, at H <= 128, the LDS-resident one on the same env in the same process; the arms alternate ``--rounds`` times
(at least 3) and each reports its median and its spread (max - min).  The torch ParallelMLP loop follows at the same
shape, with the bytes of its per-env weight copies (``--no-torch`` skips it).

Prints one line per arm and a final JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import finenvs_amd  # noqa: E402
from bench import make_series  # noqa: E402
from finenvs_amd.evo import FusedEvoAgent  # noqa: E402


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


def streamed_arms(a, make_env, out):
    """The streamed population and, at H <= 128, the resident one on the same env, alternating."""
    from finenvs_amd.evo import FusedPopulationMLP2Rollout

    N, W, H, K, A, E = a.envs, a.window, a.hidden, a.steps, a.assets, a.eval_envs
    rounds = max(3, a.rounds)
    env = make_env()
    arms = {}

    def population(streamed):
        agent = FusedEvoAgent(env, hidden_dim=H, hidden_layers=2, num_eval_envs=E, max_episodes=64, streamed=streamed)
        assert agent.population.streamed is streamed
        return agent.population

    arms["streamed"] = population(True)
    fits = H <= 128 and 0 < env._lib.fe_evo2_lds_bytes(W, A, H) <= FusedPopulationMLP2Rollout.LDS_BYTES
    if fits:
        arms["resident"] = population(False)
    times = {name: [] for name in arms}
    for _ in range(rounds):
        for name, pop in arms.items():
            pop.sync_from_env()      # the arms of one env take turns: each looks at the state the other left
            pop.next_generation()    # and starts from empty episode slots
            times[name].append(1e3 * timed(lambda: pop.run(K), a.reps) / K)
    out["rounds"], out["lds_bytes_streamed"] = rounds, int(env._lib.fe_evo2_streamed_lds_bytes(W, A, H))
    for name, t in times.items():
        med, spread = statistics.median(t), max(t) - min(t)
        out[name + "_us_per_step"], out[name + "_spread_us"] = med, spread
        print(f"{name:21s}: {med:9.1f} us/step  spread {spread:6.1f}  {N / (med * 1e-6):.3e} env-steps/s  "
              f"({', '.join(f'{x:.1f}' for x in t)})")
    out["theta_bytes"] = 4 * arms["streamed"].num_params
    return out["streamed_us_per_step"] * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--window", type=int, default=16)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--assets", type=int, default=1)
    ap.add_argument("--eval-envs", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--hidden-layers", type=int, default=1, choices=(1, 2))
    ap.add_argument("--streamed", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="with --streamed: skip the torch loop (its weights take N * P floats)")
    a = ap.parse_args()
    if a.streamed:
        a.hidden_layers = 2
    N, W, H, K, A, E = a.envs, a.window, a.hidden, a.steps, a.assets, a.eval_envs
    prices, day_id, _ = make_series(A)

    def make_env():
        return finenvs_amd.TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=W, num_envs=N, redraw="device",
                                         obs_buffers=2)

    L = a.hidden_layers
    out = {"envs": N, "window": W, "hidden": H, "steps_per_launch": K, "assets": A}
    if L == 2:
        out["hidden_layers"] = 2
        if H in (32, 64) and not a.streamed:  # the one-layer kernel at the same H, in the same process
            env = make_env()
            one = FusedEvoAgent(env, hidden_dim=H, num_eval_envs=E, max_episodes=64).population
            out["one_layer_us_per_step"] = 1e3 * timed(lambda: one.run(K), a.reps) / K
            print(f"one-layer population : {out['one_layer_us_per_step']:9.1f} us/step")
            del one, env
            torch.cuda.empty_cache()
    # ---- fused
    if a.streamed:
        fused_ms = streamed_arms(a, make_env, out)
        torch.cuda.empty_cache()
        if a.no_torch:
            print(json.dumps(out))
            return
    else:
        env = make_env()
        agent = FusedEvoAgent(env, hidden_dim=H, hidden_layers=L, num_eval_envs=E, max_episodes=64)
        pop = agent.population
        fused_ms = timed(lambda: pop.run(K), a.reps) / K
        out["fused_us_per_step"] = 1e3 * fused_ms
        out["fused_env_steps_per_s"] = N / (fused_ms * 1e-3)
        print(f"fused population     : {1e3 * fused_ms:9.1f} us/step  {out['fused_env_steps_per_s']:.3e} env-steps/s")
        gz = torch.randn((pop.num_pairs,), device=env._dev)
        out["gradient_ms"] = timed(lambda: pop.gradient(gz), 3)
        print(f"gradient kernel      : {out['gradient_ms']:9.3f} ms per generation")
        del agent, pop, env
        torch.cuda.empty_cache()

    # ---- torch restatement of ParallelMLP + env.step (+ EvoAgent.store)
    env = make_env()
    dev = env._dev
    n_train, half = N - E, (N - E) // 2
    torch.manual_seed(0)
    shapes = [(5 * W, H), (H, 1)] if L == 1 else [(5 * W, H), (H, H), (H, 1)]
    layers = [(torch.randn(s, device=dev) * (2 / s[0]) ** 0.5, torch.randn((1, s[1]), device=dev) * (2 / s[0]) ** 0.5) for s in shapes]

    def perturb():
        pw = []
        for w, b in layers:
            eps_w = torch.normal(0, 0.02, (half, *w.shape), device=dev)
            eps_b = torch.normal(0, 0.02, (half, *b.shape), device=dev)
            zw, zb = torch.zeros((E, *w.shape), device=dev), torch.zeros((E, *b.shape), device=dev)
            pw.append((w.repeat((N, 1, 1)) + torch.cat([eps_w, -eps_w, zw]), b.repeat((N, 1, 1)) + torch.cat([eps_b, -eps_b, zb])))
        return pw

    pw = perturb()
    out["torch_weight_bytes"] = sum(w.numel() * 4 + b.numel() * 4 for w, b in pw)
    print(f"torch per-env weights: {out['torch_weight_bytes'] / 1e9:9.2f} GB")
    state = {"obs": env.reset()}
    cur_ret = torch.zeros((N,), device=dev)
    cur_ts = torch.zeros((N,), device=dev)

    def torch_steps(store):
        with torch.no_grad():
            for _ in range(K):
                x = state["obs"].float()
                acts = []
                for aa in range(A):
                    c = x[:, :, 5 * aa:5 * aa + 5].reshape(N, 1, 5 * W)
                    for (w, b) in pw:
                        c = torch.tanh(torch.matmul(c, w) + b)
                    acts.append(c.reshape(N))
                act = torch.stack(acts, 1)
                noise = torch.normal(0, 0.01, act.shape, device=dev)
                noise[-E:, :] = 0
                act.add_(noise)
                state["obs"], rew, done, _ = env.step(act)
                if store:
                    cur_ts.add_(1)
                    cur_ret.add_(rew)
                    idx = torch.squeeze(done.nonzero(), 1)
                    _ = cur_ts[idx].sum().item()
                    cur_ret[idx] = 0
                    cur_ts[idx] = 0

    t_ms = timed(lambda: torch_steps(False), max(1, a.reps // 2)) / K
    out["torch_us_per_step"] = 1e3 * t_ms
    print(f"torch ParallelMLP    : {1e3 * t_ms:9.1f} us/step  {N / (t_ms * 1e-3):.3e} env-steps/s")
    ts_ms = timed(lambda: torch_steps(True), max(1, a.reps // 2)) / K
    out["torch_store_us_per_step"] = 1e3 * ts_ms
    print(f"torch + agent.store  : {1e3 * ts_ms:9.1f} us/step  {N / (ts_ms * 1e-3):.3e} env-steps/s")
    out["perturb_ms"] = timed(perturb, 3)
    print(f"torch perturb (once per generation): {out['perturb_ms']:.3f} ms")
    out["speedup_vs_torch"] = t_ms / fused_ms
    out["speedup_vs_torch_store"] = ts_ms / fused_ms
    if "one_layer_us_per_step" in out:
        out["ratio_to_one_layer"] = out["fused_us_per_step"] / out["one_layer_us_per_step"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
