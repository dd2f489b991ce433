#!/usr/bin/env python3
"""What ``--graph-update`` does to the SAC example's training iteration (examples/sac_time_series.py at its defaults:
1024 envs, H = 128, W = 4, chunk 8), at B = 100 and B = 256.

    python tools/graph_update_bench.py [--out FILE] [--batch 100 256] [--rounds 40] [--counts]

* iteration time: both arms live in ONE process, each a generator of the example's loop on its own env --
  ``eager_fused`` with ``--fused-targets --fused-critics --fused-actor --fused-optim`` (the baseline: about 160 launches
  per iteration from the host) and ``graph_update`` with ``--graph-update`` (the same update captured once, one graph
  launch per iteration; rollout and ``buffer.extend`` stay outside the graph in both).  After ``--settle`` untimed
  iterations of each, the arms advance alternately, one iteration at a time; every iteration is timed on the host
  between two device synchronisations.  ``--alternations`` such blocks of ``--rounds`` iterations: per arm the median
  of every block, and their spread (min .. max of the block medians) as the run-to-run figure.
* beside them, the graphed-torch figures of the existing benches at the same H and B: ``tools/critic_grad_bench.py``
  (one critic update) and ``tools/sac_grad_bench.py`` (one actor update), each a child process.
* kernels per iteration (``--counts``): one ``rocprofv3 --kernel-trace --stats`` run per arm (this script again,
  ``--count-arm``, as the profiled program after ``--``; no counters are collected), the difference of the launch
  totals of two run lengths divided by the difference in iterations, so that construction and warm-up cancel.
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

ARMS = {"eager_fused": dict(fused_targets=True, fused_critics=True, fused_actor=True, fused_optim=True),
        "graph_update": dict(graph_update=True, log_every=1 << 30)}  # the graphed arm reads no loss back


def arm(name, batch, iterations, seed=0):
    import sac_time_series

    return sac_time_series.iterate(iterations=iterations, batch=batch, seed=seed, **ARMS[name])


def interleaved(batch, settle, rounds, alternations):
    """µs per iteration of both arms: `alternations` blocks of `rounds` alternating iterations after `settle` untimed ones."""
    import torch

    gens = {name: arm(name, batch, settle + rounds * alternations + 1) for name in ARMS}
    for _ in range(settle):
        for g in gens.values():
            next(g)
    blocks = {name: [] for name in gens}
    for _ in range(alternations):
        times = {name: [] for name in gens}
        for _ in range(rounds):
            for name, g in gens.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                next(g)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e6)
        for name in gens:
            blocks[name].append(statistics.median(times[name]))
    return blocks


def count_arm(name, batch, iterations):
    """The profiled program: `iterations` iterations of one arm, nothing else."""
    import torch

    for _ in arm(name, batch, iterations):
        pass
    torch.cuda.synchronize()


def kernel_launches(name, batch, iterations):
    """Total kernel launches of `count_arm` under rocprofv3 --kernel-trace --stats."""
    out = tempfile.mkdtemp(prefix="graph_update_bench_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable,
               os.path.abspath(__file__), "--count-arm", name, "--batch", str(batch), "--iterations", str(iterations)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
        files = glob.glob(os.path.join(out, "**", "*_kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no kernel statistics")
        rows = list(csv.DictReader(open(max(files, key=os.path.getmtime))))
        return sum(int(r["Calls"]) for r in rows)
    finally:
        shutil.rmtree(out, ignore_errors=True)


def graphed_torch(tool, batches, hidden):
    """The torch_graphed (and fused) lines of an existing bench at the same sizes, from a child process."""
    cmd = [sys.executable, os.path.join(ROOT, "tools", tool), "--batch", *map(str, batches), "--hidden", str(hidden),
           "--no-example"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    keep = [ln for ln in res.stdout.splitlines() if ln.startswith("H=") and ("torch_graphed" in ln or " fused " in ln)]
    return keep or [f"({tool} printed no figures: exit {res.returncode})"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, nargs="+", default=[100, 256])
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--settle", type=int, default=40)  # x 2 arms x several ms: well past the clock transient after idling
    ap.add_argument("--iterations", type=int, default=0)
    ap.add_argument("--count-arm", choices=sorted(ARMS), default=None)
    ap.add_argument("--counts", action="store_true")
    ap.add_argument("--no-graphed", action="store_true")
    a = ap.parse_args()
    if a.count_arm:
        count_arm(a.count_arm, a.batch[0], a.iterations)
        return
    if a.alternations < 5:
        ap.error("--alternations must be at least 5: the spread is the run-to-run figure")
    lines = ["# python tools/graph_update_bench.py   (MI355X; examples/sac_time_series.py at its defaults -- 1024 envs, H = 128, "
             "W = 4, chunk 8)",
             f"# iteration: both arms in one process, alternating one iteration at a time after {a.settle} untimed iterations "
             f"each; host time between two synchronisations; {a.alternations} blocks of {a.rounds} iterations: median of the "
             "block medians [min .. max of the block medians]",
             "# eager_fused : --fused-targets --fused-critics --fused-actor --fused-optim (every launch issued from the host)",
             "# graph_update: --graph-update (draw from the device cursor; the update is one hipGraph launch; rollout and "
             "extend outside it)"]
    for B in a.batch:
        blocks = interleaved(B, a.settle, a.rounds, a.alternations)
        med = {}
        for name, xs in blocks.items():
            med[name] = statistics.median(xs)
            lines.append(f"B={B:4d} {name:12s}: {med[name]:9.1f} us/iteration  [{min(xs):.1f} .. {max(xs):.1f}]")
        lines.append(f"B={B:4d} eager_fused / graph_update = {med['eager_fused'] / med['graph_update']:.2f}")
        print("\n".join(lines[-3:]), flush=True)
    if not a.no_graphed:
        lines.append("# the existing benches at the same sizes (us per update of ONE network; torch_graphed = the torch path "
                     "captured in one graph)")
        for tool in ("critic_grad_bench.py", "sac_grad_bench.py"):
            lines += [f"{tool}: {ln}" for ln in graphed_torch(tool, a.batch, 128)]
            print("\n".join(lines[-4:]), flush=True)
    if a.counts:
        lines.append("# kernels per iteration: rocprofv3 --kernel-trace --stats, one run per arm and length, "
                     "(launches of 30 iterations - launches of 15) / 15")
        for B in a.batch:
            for name in ARMS:
                n1, n2 = kernel_launches(name, B, 15), kernel_launches(name, B, 30)
                lines.append(f"B={B:4d} {name:12s}: {(n2 - n1) / 15.0:7.1f} kernels/iteration")
                print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
