"""GPU box: the streamed twin LSTM critics (H = 256 / 512 / 1024, ``FusedTwinCritic(..., streamed=True)``) against
torch on rendered mini-batches, for the two passes a TD3 / SAC learner makes through its critics:

  update   one critic update without the optimizer step (it is the same in all arms): TD3's targets from the target
           critics, then MSE(q1, y) + MSE(q2, y) and its backward to both critics' parameters
  dqda     one ``q()`` + ``dQ/da`` pass: -q1.mean() back to the actions through frozen critics (TD3's actor loss as the
           critics see it; the second critic does not run)

  fused          ``td3_targets`` + ``critic_loss(...).backward()`` / ``q()`` + ``backward()`` on the ring's descriptors,
                 incl. the per-call weight re-packs
  torch_eager    ``ReplayBuffer.get_mini_batch`` (renders states and next states) + ``torch_td3_targets`` + the nn.LSTM
                 critics + backward
  torch_graphed  the same captured once in a torch.cuda.graph and replayed (gradients accumulate in place)

The target actor's actions are computed outside the timed region in every arm (they are an input of the critics' half).
Device-synchronised timing after a warm-up; the arms alternate within one process and every figure is the median of
--rounds rounds.  One H per process keeps a step short; each step under its own time limit, chained:

    timeout -k 10 600 python tools/critic_streamed_bench.py --hidden 256 --out profiles/critic_streamed_bench.txt && \\
    timeout -k 10 600 python tools/critic_streamed_bench.py --hidden 512 --out profiles/critic_streamed_bench.txt --append && \\
    timeout -k 10 900 python tools/critic_streamed_bench.py --hidden 1024 --out profiles/critic_streamed_bench.txt --append

Prints one line per (H, B, pass, arm) and a final JSON line; ``--out`` writes the same lines to a file.
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
import finenvs_amd  # noqa: E402
from bench import make_series  # noqa: E402
from finenvs_amd.critic import CriticLSTM, FusedTwinCritic, torch_td3_targets  # noqa: E402
from finenvs_amd.lstm_head import LSTMHead  # noqa: E402
from finenvs_amd.replay import ReplayBuffer  # noqa: E402
from finenvs_amd.rollout import FusedLSTMRollout  # noqa: E402
from finenvs_amd.trajectory import TrajectoryBuffer  # noqa: E402

GAMMA, STD, CLIP = 0.99, 0.2, 0.5


def timed(fn, reps=3):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def graphed(fn):
    """``fn`` captured after two warm-up calls on a side stream; None (and a printed reason) if it cannot be."""
    try:
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
    except Exception as exc:  # noqa: BLE001  (reported, not hidden)
        print(f"torch_graphed not capturable: {exc}", flush=True)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[256, 4096, 65536])
    ap.add_argument("--hidden", type=int, nargs="+", default=[256, 512, 1024], choices=[256, 512, 1024])
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    W, N, K = a.window, 4096, 16
    prices, day_id, _ = make_series(1)
    env = finenvs_amd.TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=W, num_envs=N, redraw="device",
                                    obs_dtype=torch.float32)
    torch.manual_seed(0)
    actor = LSTMHead(128, W, "tanh", device="cuda")  # fills the ring and gives the next actions: not what is measured
    roll = FusedLSTMRollout.from_modules(env, actor.lstm, actor.last_layer[0], output_activation="tanh")
    traj = TrajectoryBuffer(K, N, 1, device=env._dev, states=True)
    roll.sync_from_env()
    roll.run(K, noise=torch.randn((K, N, 1), device="cuda"), std=0.5, trajectory=traj)
    buffer = ReplayBuffer(env, max_size=K * N)
    buffer.extend(traj)
    out = {"window": W, "results": {}}
    say(f"# tools/critic_streamed_bench.py: W = {W}, ring of {K * N} transitions, median of {a.rounds} rounds x 3 calls; "
        "us per pass")
    for H in a.hidden:
        torch.manual_seed(H)
        nets = [CriticLSTM(H, W, device="cuda") for _ in range(4)]  # critics 1, 2 and their targets
        frozen = [copy.deepcopy(c).requires_grad_(False) for c in nets[:2]]
        twin, twin_t = FusedTwinCritic(env, *nets[:2], streamed=True), FusedTwinCritic(env, *nets[2:], streamed=True)
        twin_f = FusedTwinCritic(env, *frozen, streamed=True)
        t_nets = [copy.deepcopy(c) for c in nets]
        t_frozen = [copy.deepcopy(c) for c in frozen]
        for B in a.batch:
            idx = torch.randint(0, buffer.size(), (B,), device="cuda")
            eps = torch.randn((B, 1), device="cuda")
            slots = buffer.physical(idx)
            with torch.no_grad():
                next_actions = roll.forward(buffer.next_src[slots], buffer.next_pos[slots])
            probe = (torch.rand((B, 1), device="cuda") * 2 - 1).requires_grad_()
            t_probe = probe.detach().clone().requires_grad_()

            def fused_update():
                y = twin_t._targets(buffer, idx, next_actions, eps.reshape(B), STD, CLIP, None, None, GAMMA, 1.0)
                twin.critic_loss(buffer, idx, y).backward()

            def torch_update():
                b = buffer.get_mini_batch(B, indices=idx)
                y = torch_td3_targets(lambda s: next_actions, t_nets[2], t_nets[3], b["rewards"], b["next_states"],
                                      b["dones"], eps, GAMMA, STD, CLIP)
                (F.mse_loss(t_nets[0](b["states"], b["actions"]), y)
                 + F.mse_loss(t_nets[1](b["states"], b["actions"]), y)).backward()

            def fused_dqda():
                s = buffer.physical(idx)
                q1, _ = twin_f.q(buffer.state_src[s], buffer.state_pos[s].reshape(B), probe)
                (-q1.mean()).backward()

            def torch_dqda():
                b = buffer.get_mini_batch(B, indices=idx)
                (-t_frozen[0](b["states"], t_probe).mean()).backward()

            for name, f_fn, t_fn in (("update", fused_update, torch_update), ("dqda", fused_dqda, torch_dqda)):
                arms = {"fused": f_fn, "torch_eager": t_fn}
                t_fn()
                graph = graphed(t_fn)
                if graph is not None:
                    arms["torch_graphed"] = graph.replay
                for fn in arms.values():
                    fn()
                times = {k: [] for k in arms}
                for _ in range(a.rounds):
                    for k, fn in arms.items():
                        times[k].append(timed(fn))
                res = out["results"].setdefault(str(H), {}).setdefault(str(B), {}).setdefault(name, {})
                for k, ts in times.items():
                    res[k] = 1e6 * statistics.median(ts)
                best = min(res, key=res.get)
                for k in arms:
                    say(f"H={H:4d} B={B:6d} {name:6s} {k:14s}: {res[k]:11.1f} us"
                        + (f"  ({res[k] / res['fused']:.2f} x fused)" if k != "fused" else "")
                        + ("  <- fastest" if k == best else ""))
                del graph
                torch.cuda.empty_cache()
        del twin, twin_t, twin_f
        torch.cuda.empty_cache()
    say(json.dumps(out))
    if a.out:
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
