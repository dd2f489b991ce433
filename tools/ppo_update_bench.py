#!/usr/bin/env python3
"""One PPO ``train()`` -- values, returns, 4 epochs x 4 mini-batches of an actor and a critic step -- on a full
trajectory chunk of T = 64 steps (W = 4), four ways:

    python tools/ppo_update_bench.py [--out FILE]   (default: ppo_update_bench.txt under profiles/) [--envs 1024 16384] [--hidden 128 1024] [--counts]

* ``eager_loop``   the loop of examples/ppo_lstm_fused.py --fused-optim: ``torch.randperm`` per epoch, six fancy-index
                   gathers per mini-batch, the torch loss expressions, FusedAdam (the parent commit's path: the yardstick)
* ``ppo_update``   ``PPOUpdate.train`` eager: device shuffle and gather, fused losses
* ``graphed``      the same ``train`` under ``GraphedUpdate``: one hipGraph launch
* ``torch_graph``  torch modules on states rendered once outside the timed call, ``torch.optim.Adam(capturable=True)``,
                   the whole update captured; its permutations are static tensors (a captured ``randperm`` would repeat)

All arms live in ONE process, each on its own env and networks of the same seed, and advance alternately, one
``train()`` at a time, timed on the host between two device synchronisations after ``--settle`` untimed calls each;
``--alternations`` blocks of ``--rounds`` calls: the median of the block medians and their min .. max.  H = 1024 runs
the streamed backward.  ``--counts``: kernel launches per ``train()`` of the first three arms, one ``rocprofv3
--kernel-trace --stats`` run per arm and length (this script as the profiled program after ``--``), the difference of
two run lengths."""
import argparse
import csv
import glob
import math
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, W, EPOCHS, MINIBATCHES = 64, 4, 4, 4
CLIP, ENT, GAMMA = 0.2, 0.01, 0.99
ARMS = ("eager_loop", "ppo_update", "graphed", "torch_graph")


def build(name, N, H, seed=0):
    """A callable that runs one train() of arm `name` on a filled chunk."""
    import torch
    from torch.distributions import Normal

    from finenvs_amd import TimeSeriesEnv
    from finenvs_amd.data import synthetic
    from finenvs_amd.graphed import GraphedUpdate
    from finenvs_amd.lstm_head import FusedLSTMHead, LSTMHead, ppo_actor_loss, ppo_critic_loss, torch_ppo_actor_loss, \
        torch_ppo_critic_loss
    from finenvs_amd.optim import FusedAdam
    from finenvs_amd.ppo import PPOUpdate, no_distribution_checks
    from finenvs_amd.trajectory import TrajectoryBuffer

    dev = "cuda:0"
    torch.manual_seed(seed)
    prices, day_id, _ = synthetic.synthetic_series(12, 1, 390, 1234)
    env = TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=W, num_envs=N, redraw="device", seed=seed,
                        obs_dtype=torch.float32)
    actor, critic = LSTMHead(H, W, "tanh", device=dev), LSTMHead(H, W, "none", device=dev)
    log_std = torch.nn.Parameter(torch.full((1,), math.log(0.5), device=dev))
    opt_a, opt_c = FusedAdam(lr=3e-4), FusedAdam(lr=3e-4)
    opt_a.add(actor)
    opt_a.add_tensor(log_std)
    opt_c.add(critic)
    streamed = {"streamed": True} if H > 128 else {}
    actor_head = FusedLSTMHead(env, actor, weights=opt_a, **streamed)
    critic_head = FusedLSTMHead(env, critic, weights=opt_c, **streamed)
    traj = TrajectoryBuffer(T, N, 1, states=True)
    roll = actor_head.rollout
    noise = torch.randn((T, N, 1), device=dev)
    roll.run(T, noise=noise, std=0.5, record_means=True, trajectory=traj)
    means, total = roll.means, T * N
    flat = lambda x: x.reshape(T, N).t().reshape(total)  # noqa: E731

    if name == "eager_loop":
        def train():
            with torch.no_grad():
                old_logp = Normal(means, log_std.exp()).log_prob(traj.actions)
                values = critic_head.rollout.forward(traj.obs_src, traj.obs_pos).reshape(T + 1, N)
                returns, advantages = traj.returns_and_advantages(values[:T], values[T], GAMMA)
            f_act, f_logp, f_adv, f_ret = flat(traj.actions), flat(old_logp), flat(advantages), flat(returns)
            for _ in range(EPOCHS):
                perm = torch.randperm(total, device=dev)
                for mb in perm.chunk(MINIBATCHES):
                    src, pos = traj.minibatch_descriptors(mb)
                    ppo_actor_loss(actor_head, log_std, src, pos, f_act[mb], f_logp[mb], f_adv[mb], CLIP, ENT).backward()
                    opt_a.step()
                    ppo_critic_loss(critic_head, src, pos, f_ret[mb]).backward()
                    opt_c.step()
        return train
    if name in ("ppo_update", "graphed"):
        update = PPOUpdate(env, traj, actor_head, critic_head, log_std, opt_a, opt_c, epochs=EPOCHS, minibatches=MINIBATCHES,
                           clip_epsilon=CLIP, entropy_coefficient=ENT, gamma=GAMMA, seed=seed)
        update.load_means(means)
        if name == "ppo_update":
            return update.train
        return GraphedUpdate(update.train, warmup=1).replay
    # torch_graph: plain modules on rendered states
    states = env.render(traj.obs_src.reshape(-1), traj.obs_pos.reshape(-1, 1)).float().reshape(T + 1, N, W, 5)
    env_major = states[:T].permute(1, 0, 2, 3).reshape(total, W, 5).contiguous()
    params_a = list(actor.parameters()) + [log_std]
    adam_a = torch.optim.Adam(params_a, 3e-4, capturable=True)
    adam_c = torch.optim.Adam(critic.parameters(), 3e-4, capturable=True)
    perms = [torch.randperm(total, device=dev) for _ in range(EPOCHS)]

    def torch_train():  # (torch's argument validation waits for the device: not capturable, so it is off inside this arm)
        with no_distribution_checks():
            torch_update()

    def torch_update():
        with torch.no_grad():
            old_logp = Normal(means, log_std.exp()).log_prob(traj.actions)
            values = critic(states.reshape(-1, W, 5)).reshape(T + 1, N)
            returns, advantages = traj.returns_and_advantages(values[:T], values[T], GAMMA)
        f_act, f_logp, f_adv, f_ret = flat(traj.actions), flat(old_logp), flat(advantages), flat(returns)
        for perm in perms:
            for mb in perm.chunk(MINIBATCHES):
                s = env_major[mb]
                adam_a.zero_grad(set_to_none=False)
                torch_ppo_actor_loss(actor(s), log_std, f_act[mb].reshape(-1, 1), f_logp[mb].reshape(-1, 1),
                                     f_adv[mb].reshape(-1, 1), CLIP, ENT).backward()
                adam_a.step()
                adam_c.zero_grad(set_to_none=False)
                torch_ppo_critic_loss(critic(s), f_ret[mb].reshape(-1, 1)).backward()
                adam_c.step()

    for p in params_a + list(critic.parameters()):
        p.grad = torch.zeros_like(p)
    return GraphedUpdate(torch_train, warmup=2).replay


def interleaved(N, H, arms, settle, rounds, alternations):
    import torch

    fns = {name: build(name, N, H) for name in arms}
    for _ in range(settle):
        for fn in fns.values():
            fn()
    blocks = {name: [] for name in fns}
    for _ in range(alternations):
        times = {name: [] for name in fns}
        for _ in range(rounds):
            for name, fn in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
        for name in fns:
            blocks[name].append(statistics.median(times[name]))
    return blocks


def count_arm(name, N, H, calls):
    import torch

    fn = build(name, N, H)
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()


def kernel_launches(name, N, H, calls):
    out = tempfile.mkdtemp(prefix="ppo_update_bench_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable,
               os.path.abspath(__file__), "--count-arm", name, "--envs", str(N), "--hidden", str(H), "--calls", str(calls)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
        files = glob.glob(os.path.join(out, "**", "*_kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no kernel statistics")
        return sum(int(r["Calls"]) for r in csv.DictReader(open(max(files, key=os.path.getmtime))))
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_update_bench.txt"))
    ap.add_argument("--envs", type=int, nargs="+", default=[1024, 16384])
    ap.add_argument("--hidden", type=int, nargs="+", default=[128, 1024])
    ap.add_argument("--arms", nargs="+", default=list(ARMS), choices=ARMS)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--settle", type=int, default=5)
    ap.add_argument("--budget-ms", type=float, default=2000.0,
                    help="a configuration whose settle calls average more than this runs rounds = 1")
    ap.add_argument("--counts", action="store_true")
    ap.add_argument("--count-arm", choices=ARMS, default=None)
    ap.add_argument("--calls", type=int, default=0)
    a = ap.parse_args()
    if a.count_arm:
        count_arm(a.count_arm, a.envs[0], a.hidden[0], a.calls)
        return
    import torch

    if not torch.cuda.is_available():
        sys.exit("ppo_update_bench needs the GPU: no device is visible")
    if a.alternations < 5:
        ap.error("--alternations must be at least 5: the spread is the run-to-run figure")
    lines = [f"# python tools/ppo_update_bench.py   (MI355X; one train(): T = {T}, W = {W}, {EPOCHS} epochs x {MINIBATCHES} "
             "mini-batches, actor + critic step each)",
             f"# all arms in one process, alternating one train() at a time after {a.settle} untimed calls each; host time "
             f"between two synchronisations; {a.alternations} blocks: median of the block medians [min .. max], ms",
             "# eager_loop: the example's --fused-optim loop (randperm, fancy-index gathers, torch loss expressions)",
             "# ppo_update: PPOUpdate.train eager   graphed: the same under GraphedUpdate   torch_graph: captured torch "
             "update on rendered states"]
    for H in a.hidden:
        for N in a.envs:
            rounds = a.rounds
            probe = build("ppo_update", N, H)
            probe()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            probe()
            torch.cuda.synchronize()
            if (time.perf_counter() - t0) * 1e3 > a.budget_ms:
                rounds = 1
            del probe
            blocks = interleaved(N, H, a.arms, a.settle if rounds > 1 else 1, rounds, a.alternations)
            med = {}
            for name, xs in blocks.items():
                med[name] = statistics.median(xs)
                lines.append(f"H={H:4d} N={N:6d} B={T * N // MINIBATCHES:7d} {name:11s}: {med[name]:10.3f} ms/train  "
                             f"[{min(xs):.3f} .. {max(xs):.3f}]  (rounds {rounds})")
            if "eager_loop" in med:
                lines.append(f"H={H:4d} N={N:6d} eager_loop / x: " + "  ".join(
                    f"{k} {med['eager_loop'] / v:.2f}" for k, v in med.items() if k != "eager_loop"))
            print("\n".join(lines[-(len(blocks) + 1):]), flush=True)
    if a.counts:
        N, H = a.envs[0], a.hidden[0]
        lines.append(f"# kernels per train() at H = {H}, N = {N}: rocprofv3 --kernel-trace --stats, (launches of 6 calls - "
                     "launches of 3) / 3")
        for name in ARMS[:3]:
            n1, n2 = kernel_launches(name, N, H, 3), kernel_launches(name, N, H, 6)
            lines.append(f"{name:11s}: {(n2 - n1) / 3.0:7.1f} kernels/train")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
