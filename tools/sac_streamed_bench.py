"""GPU box: the streamed SAC LSTM actor (H = 256 / 512 / 1024, ``FusedSACRollout(..., streamed=True)``) against torch,
for the two things a SAC learner does with its actor:

  update   one actor update without the optimizer step (it is the same in all arms): ``sample`` on the mini-batch's
           states, ``min(q1, q2)`` of the sampled actions through frozen streamed critics, and the backward of
           -(q - alpha log_prob).mean() to the actor's ten parameters
             fused          ``FusedSACRollout.sample`` + ``FusedTwinCritic(streamed=True).q`` on the ring's descriptors,
                            incl. the per-call weight re-packs
             torch_eager    ``ReplayBuffer.get_mini_batch`` (renders the states) + the nn.LSTM actor and critics + backward
             torch_graphed  the same captured once in a torch.cuda.graph and replayed (gradients accumulate in place)
  run      K env steps at --envs envs: ``FusedSACRollout.run`` (one launch; the fused kernel at every env count, there is no
           split-by-time-step form for SAC) against SACActorLSTM + rsample + tanh + env.step captured in a GraphedRollout

``--regress PARENT_LIB``: instead, ``fe_env_rollout_lstm`` (the kernel whose body the acting kernel shares as text) at
H = 256 and 1024, --envs envs, A = 1, with the parent commit's library and this one in one process, the arms
parent / parent again / new interleaved; the rule of NOTES.md: new - parent <= max(|parent again - parent|, max - min of
the parent arm's rounds).

Device-synchronised timing after a warm-up; the arms alternate within one process and every figure is the median of
--rounds rounds.  One H per process keeps a step short; each step under its own time limit, chained:

    timeout -k 10 600 python tools/sac_streamed_bench.py --hidden 256 --out profiles/sac_streamed_bench.txt && \\
    timeout -k 10 600 python tools/sac_streamed_bench.py --hidden 512 --out profiles/sac_streamed_bench.txt --append && \\
    timeout -k 10 900 python tools/sac_streamed_bench.py --hidden 1024 --out profiles/sac_streamed_bench.txt --append

Prints one line per figure and a final JSON line; ``--out`` writes the same lines to a file.
"""
import argparse
import copy
import ctypes as C
import json
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
from finenvs_amd import _lib  # noqa: E402
from finenvs_amd.critic import CriticLSTM, FusedTwinCritic  # noqa: E402
from finenvs_amd.replay import ReplayBuffer  # noqa: E402
from finenvs_amd.rollout import FusedLSTMRollout, GraphedRollout  # noqa: E402
from finenvs_amd.sac import FusedSACRollout, SACActorLSTM  # noqa: E402
from finenvs_amd.trajectory import TrajectoryBuffer  # noqa: E402


def timed(fn, reps=3):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def graphed(fn):
    """``fn`` captured after two warm-up calls on a side stream; None (and a printed reason) if it cannot be.  Normal's
    argument validation reads a device value on the host, which a capture does not permit: captured without it."""
    try:
        Distribution.set_default_validate_args(False)
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
    finally:
        Distribution.set_default_validate_args(True)


def interleaved(arms, rounds):
    for fn in arms.values():
        fn()
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            times[k].append(timed(fn))
    return times


def load_older(path):
    """A library of an older commit: it lacks the newest exports, so every name it HAS is bound, not every name."""
    lib = C.CDLL(path)
    for table in (getattr(_lib, k) for k in dir(_lib) if k.endswith("SIGNATURES")):
        for name, (res, args) in table.items():
            fn = getattr(lib, name, None)
            if fn is not None:
                fn.restype, fn.argtypes = res, args
    return lib


def regress(a, say, out):
    """fe_env_rollout_lstm through the parent's library and this one: parent / parent again / new, interleaved."""
    W, N, K = a.window, a.envs, a.steps
    prices, day_id, _ = make_series(1)
    libs = {"parent": load_older(a.regress), "parent_again": load_older(a.regress), "new": _lib.load()}
    for H in a.hidden:
        torch.manual_seed(H)
        lstm, lin = torch.nn.LSTM(5, H, batch_first=True).cuda(), torch.nn.Linear(H, 1).cuda()
        noise = torch.randn((K, N, 1), device="cuda")
        arms = {}
        for name, lib in libs.items():
            env = finenvs_amd.TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=W, num_envs=N, redraw="device",
                                            obs_buffers=2, _native=lib)
            roll = FusedLSTMRollout.from_modules(env, lstm, lin)
            arms[name] = (lambda r: lambda: r.run(K, noise=noise, std=0.5))(roll)
        times = interleaved(arms, a.rounds)
        med = {k: 1e6 * statistics.median(v) / K for k, v in times.items()}
        spread = 1e6 * (max(times["parent"]) - min(times["parent"])) / K
        allowed = max(abs(med["parent_again"] - med["parent"]), spread)
        ok = med["new"] - med["parent"] <= allowed
        out["results"].setdefault(str(H), {})["fe_env_rollout_lstm"] = {**med, "allowed": allowed, "ok": ok}
        say(f"H={H:4d} N={N:6d} fe_env_rollout_lstm us/step: parent {med['parent']:.1f}  parent again {med['parent_again']:.1f}  "
            f"new {med['new']:.1f}  new - parent {med['new'] - med['parent']:+.1f} (allowed {allowed:.1f}): "
            + ("no regression" if ok else "REGRESSION"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[256, 4096, 65536])
    ap.add_argument("--hidden", type=int, nargs="+", default=[256, 512, 1024], choices=[256, 512, 1024])
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--no-run", action="store_true")
    ap.add_argument("--regress", default=None, metavar="PARENT_LIB")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def finish(out):
        say(json.dumps(out))
        if a.out:
            with open(a.out, "a" if a.append else "w") as f:
                f.write("\n".join(lines) + "\n")

    W = a.window
    out = {"window": W, "results": {}}
    if a.regress:
        say(f"# tools/sac_streamed_bench.py --regress: W = {W}, {a.envs} envs, A = 1, K = {a.steps}, median of {a.rounds} "
            "rounds x 3 calls, interleaved")
        regress(a, say, out)
        return finish(out)
    N, K = 4096, 16
    prices, day_id, _ = make_series(1)
    env = finenvs_amd.TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=W, num_envs=N, redraw="device",
                                    obs_dtype=torch.float32)
    torch.manual_seed(0)
    filler = FusedSACRollout(env, SACActorLSTM(H=128, W=W).cuda())  # fills the ring: not what is measured
    traj = TrajectoryBuffer(K, N, 1, device=env._dev, states=True)
    filler.run(K, noise=torch.randn((K, N, 1), device="cuda"), trajectory=traj)
    buffer = ReplayBuffer(env, max_size=K * N)
    buffer.extend(traj)
    say(f"# tools/sac_streamed_bench.py: W = {W}, ring of {K * N} transitions, median of {a.rounds} rounds x 3 calls")
    for H in a.hidden:
        torch.manual_seed(H)
        actor = SACActorLSTM(H=H, W=W).cuda()
        c1, c2 = CriticLSTM(H, W).cuda().requires_grad_(False), CriticLSTM(H, W).cuda().requires_grad_(False)
        t_actor, t1, t2 = copy.deepcopy(actor), copy.deepcopy(c1), copy.deepcopy(c2)
        roll = FusedSACRollout(env, actor, streamed=True)
        roll.sync_from_env()
        twin = FusedTwinCritic(env, c1, c2, streamed=True)
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
            torch_update()
            graph = graphed(torch_update)
            if graph is not None:
                arms["torch_graphed"] = graph.replay
            times = interleaved(arms, a.rounds)
            res = out["results"].setdefault(str(H), {}).setdefault(str(B), {})
            for k, ts in times.items():
                res[k] = 1e6 * statistics.median(ts)
            best = min(res, key=res.get)
            for k in arms:
                say(f"H={H:4d} B={B:6d} update {k:14s}: {res[k]:11.1f} us"
                    + (f"  ({res[k] / res['fused']:.2f} x fused)" if k != "fused" else "")
                    + ("  <- fastest" if k == best else ""))
            del graph
            torch.cuda.empty_cache()
        del roll, twin
        torch.cuda.empty_cache()
        if a.no_run:
            continue
        # ---- acting: K steps at a.envs envs
        NE, KS = a.envs, a.steps

        def make_env():
            return finenvs_amd.TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=W, num_envs=NE, redraw="device",
                                             obs_buffers=2)

        noise = torch.randn((KS, NE, 1), device="cuda")
        big = make_env()
        act = FusedSACRollout(big, actor, streamed=True)

        def policy(obs, k):  # get_distribution + rsample, without Normal's argument check (a host sync: not capturable)
            with torch.no_grad():
                z = actor(obs.float())
                mu, sd = actor.mu_layer(z), torch.nn.functional.softplus(actor.std_layer(z))
                actions = torch.tanh(mu + torch.randn_like(mu) * sd)
                actions[-1, :] = mu[-1, :]
            return actions

        other = make_env()
        other.reset()
        loop = GraphedRollout(other, policy, KS)
        times = interleaved({"fused": lambda: act.run(KS, noise=noise), "torch_graphed": loop.run}, a.rounds)
        res = out["results"][str(H)].setdefault("run", {})
        for k, ts in times.items():
            res[k] = 1e6 * statistics.median(ts) / KS
        for k in res:
            say(f"H={H:4d} N={NE:6d} run    {k:14s}: {res[k]:11.1f} us/step"
                + (f"  ({res[k] / res['fused']:.2f} x fused)" if k != "fused" else ""))
        del big, act, other, loop
        torch.cuda.empty_cache()
    finish(out)


if __name__ == "__main__":
    main()
