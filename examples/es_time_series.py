#!/usr/bin/env python3
"""The reference's ES training loop (ES_MLP_Isaac_Gym.py of its examples: agent.step -> env.step -> agent.store until a
batch of episodes has finished, then agent.train()) on the time-series env with synthetic bars, through the fused
population (finenvs_amd.evo): K env steps of every perturbed member per launch, one host read per launch.

    python examples/es_time_series.py [--envs 4096] [--eval-envs 12] [--window 16] [--hidden 64] [--generations 5]
                                      [--hidden-layers 2] [--streamed]

``--hidden-layers 2`` is the reference's default network shape (hidden_dims = (H, H)); it admits ``--hidden 128``, the
widest theta that fits the LDS, and ``--hidden 256``, the reference's own width, which reads theta through L2 (the streamed
population).  ``--streamed`` takes the streamed population at the smaller widths too.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from finenvs_amd import TimeSeriesEnv  # noqa: E402
from finenvs_amd.data import synthetic  # noqa: E402
from finenvs_amd.evo import FusedEvoAgent  # noqa: E402


def main(num_envs=4096, num_eval_envs=12, window=16, hidden=64, generations=5, episodes_per_batch=None, days=40,
         bars=120, assets=1, chunk=32, seed=0, quiet=False, hidden_layers=1, streamed=None):
    prices, day_id, _ = synthetic.synthetic_series(days, assets, bars, 1234 + seed)
    env = TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=window, num_envs=num_envs, redraw="device", seed=seed)
    agent = FusedEvoAgent(env, hidden_dim=hidden, hidden_layers=hidden_layers, learning_rate=0.01, noise_std_dev=0.02, l2_coefficient=0.005,
                          num_eval_envs=num_eval_envs, seed=seed, max_episodes=8, streamed=streamed)
    # about two episodes per env and generation (the reference asks for 10 000 of 4 096 envs)
    batch = episodes_per_batch if episodes_per_batch is not None else 2 * num_envs
    history = []
    for g in range(generations):
        t0 = time.perf_counter()
        agent.collect(batch, chunk=chunk)
        agent.train()
        p = agent.log_progress(print_line=not quiet)
        p["seconds"] = time.perf_counter() - t0
        history.append(p)
    return history


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--eval-envs", type=int, default=12)
    ap.add_argument("--window", type=int, default=16)
    ap.add_argument("--hidden", type=int, default=64, choices=(32, 64, 128, 256))
    ap.add_argument("--hidden-layers", type=int, default=1, choices=(1, 2))
    ap.add_argument("--generations", type=int, default=5)
    ap.add_argument("--streamed", action="store_true", help="theta read through L2 (two hidden layers)")
    a = ap.parse_args()
    if a.hidden >= 128 and a.hidden_layers != 2:
        ap.error(f"--hidden {a.hidden} needs --hidden-layers 2 (the one-layer population runs H = 32 / 64)")
    if a.streamed and a.hidden_layers != 2:
        ap.error("--streamed needs --hidden-layers 2")
    main(a.envs, a.eval_envs, a.window, a.hidden, a.generations, hidden_layers=a.hidden_layers,
         streamed=True if a.streamed else None)
