#!/usr/bin/env python3
"""What ``--fused-optim`` does to the SAC example's training iteration (examples/sac_time_series.py at its defaults:
1024 envs, H = 128, W = 4, chunk 8, with ``--fused-targets --fused-critics --fused-actor``), at B = 100 and B = 256.

    python tools/optim_bench.py [--out profiles/optim_bench.txt] [--batch 100 256] [--rounds 200]

* iteration time: both arms (with and without ``--fused-optim``) live in ONE process, each a generator of the example's
  loop on its own env; after ``--settle`` untimed iterations of each, the arms advance alternately, one iteration at a
  time, and every iteration is timed on the host between two device synchronisations (the example itself reads its
  losses back once per iteration, so an iteration ends synchronised anyway).  Median and quartiles of ``--rounds``.
* kernels per iteration: one ``rocprofv3 --kernel-trace --stats`` run per arm (this script again, ``--count-arm``, as the
  profiled program after ``--``; no counters are collected), the difference of the launch totals of two run lengths
  divided by the difference in iterations, so that construction and warm-up cancel.
* beside them, the graphed-torch figures of the existing benches at the same H and B: ``tools/critic_grad_bench.py``
  (one critic update) and ``tools/sac_grad_bench.py`` (one actor update), each a child process.
"""
import argparse
import csv
import glob
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

FLAGS = dict(fused_targets=True, fused_critics=True, fused_actor=True)
ARMS = {"torch_optim": False, "fused_optim": True}


def arm(batch, fused_optim, iterations, seed=0):
    import sac_time_series

    return sac_time_series.iterate(iterations=iterations, batch=batch, seed=seed, fused_optim=fused_optim, **FLAGS)


def interleaved(batch, settle, rounds):
    """µs per iteration of both arms, alternating, after `settle` untimed iterations of each."""
    import torch

    gens = {name: arm(batch, fused, settle + rounds + 1) for name, fused in ARMS.items()}
    for _ in range(settle):
        for g in gens.values():
            next(g)
    times = {name: [] for name in gens}
    for _ in range(rounds):
        for name, g in gens.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            next(g)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e6)
    return times


def count_arm(name, batch, iterations):
    """The profiled program: `iterations` iterations of one arm, nothing else."""
    import torch

    for _ in arm(batch, ARMS[name], iterations):
        pass
    torch.cuda.synchronize()


def kernel_launches(name, batch, iterations):
    """Total kernel launches of `count_arm` under rocprofv3 --kernel-trace --stats."""
    out = tempfile.mkdtemp(prefix="optim_bench_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable,
               os.path.abspath(__file__), "--count-arm", name, "--batch", str(batch), "--iterations", str(iterations)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        files = glob.glob(os.path.join(out, "**", "*_kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no kernel statistics")
        rows = list(csv.DictReader(open(max(files, key=os.path.getmtime))))
        return sum(int(r["Calls"]) for r in rows), {r["Name"]: int(r["Calls"]) for r in rows}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def graphed_torch(tool, batches, hidden):
    """The torch_graphed (and fused) lines of an existing bench at the same sizes, from a child process."""
    cmd = [sys.executable, os.path.join(ROOT, "tools", tool), "--batch", *map(str, batches), "--hidden", str(hidden),
           "--no-example"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    keep = [ln for ln in res.stdout.splitlines() if ln.startswith("H=") and ("torch_graphed" in ln or " fused " in ln)]
    return keep or [f"({tool} printed no figures: exit {res.returncode})"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, nargs="+", default=[100, 256])
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--settle", type=int, default=40)  # x 2 arms x several ms: well past the clock transient after idling
    ap.add_argument("--iterations", type=int, default=0)
    ap.add_argument("--count-arm", choices=sorted(ARMS), default=None)
    ap.add_argument("--no-counts", action="store_true")
    ap.add_argument("--no-graphed", action="store_true")
    a = ap.parse_args()
    if a.count_arm:
        count_arm(a.count_arm, a.batch[0], a.iterations)
        return
    lines = ["# python tools/optim_bench.py   (MI355X; examples/sac_time_series.py at its defaults -- 1024 envs, H = 128, W = 4, "
             "chunk 8 -- with --fused-targets --fused-critics --fused-actor)",
             f"# iteration: both arms in one process, alternating one iteration at a time after {a.settle} untimed iterations each; "
             f"host time between two synchronisations, median [quartiles] of {a.rounds}",
             "# torch_optim: three torch.optim.Adam + four soft_update loops, modules re-packed at every fused call, the actor's "
             "biases copied to the host",
             "# fused_optim: two FusedAdam.step (fe_net_update) + one zero_grad launch, resident packed weights (weights=)"]
    for B in a.batch:
        t = interleaved(B, a.settle, a.rounds)
        med = {}
        for name, xs in t.items():
            q = statistics.quantiles(xs, n=4)
            med[name] = statistics.median(xs)
            lines.append(f"B={B:4d} {name:12s}: {med[name]:9.1f} us/iteration  [{q[0]:.1f} .. {q[2]:.1f}]")
        lines.append(f"B={B:4d} torch_optim / fused_optim = {med['torch_optim'] / med['fused_optim']:.2f}")
        print("\n".join(lines[-3:]), flush=True)
    if not a.no_counts:
        lines.append("# kernels per iteration: rocprofv3 --kernel-trace --stats, one run per arm and length, "
                     "(launches of 40 iterations - launches of 20) / 20")
        for B in a.batch:
            for name in ARMS:
                (n1, _), (n2, by) = kernel_launches(name, B, 20), kernel_launches(name, B, 40)
                lines.append(f"B={B:4d} {name:12s}: {(n2 - n1) / 20.0:7.1f} kernels/iteration")
                own = {k: v for k, v in by.items() if "fe_net_update" in k}
                if own:
                    lines.append(f"B={B:4d} {name:12s}: of those fe_net_update_kernel {sum(own.values()) / 40.0:.1f}")
                print(lines[-1], flush=True)
    if not a.no_graphed:
        lines.append("# the existing benches at the same sizes (us per update; torch_graphed = the torch path captured in one graph)")
        for tool in ("critic_grad_bench.py", "sac_grad_bench.py"):
            lines += [f"{tool}: {ln}" for ln in graphed_torch(tool, a.batch, 128)]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
