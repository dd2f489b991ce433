#!/usr/bin/env python3
"""Write tests/golden/evo_update.npz by RUNNING THE REFERENCE's ES update (test infrastructure, not the product).

Runs only where a checkout of the reference is available: its Python is imported the way oracle/make_goldens.py does it
(setup_reference: a scratch copy of its package put on sys.path; nothing of it is written here).  The fixture holds arrays only:
  inputs   theta0 (P) = W1, b1, W2, b2 flattened; eps (pairs, P) the positive perturbations the update sees (after
           reconstruct_perturbations); dones / returns of the finished episodes in the order they finished
  outputs  final_ranks (N) of EvoAgent.perform_rank_transformation, theta1 (P) after ParallelMLP.update_parameters

    python tools/make_evo_golden.py <reference checkout>
"""
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
N, NUM_EVAL, W, H = 40, 2, 4, 32
SIGMA, LR, L2 = 0.02, 0.01, 0.005
EPISODES = 150


def flat(weights, biases):
    return torch.cat([weights[0].reshape(-1), biases[0].reshape(-1), weights[1].reshape(-1), biases[1].reshape(-1)])


def setup_reference(ref: str) -> None:
    """A scratch copy of the reference's package on sys.path (its Python writes caches next to its sources)."""
    sys.dont_write_bytecode = True
    work = tempfile.mkdtemp(prefix="fe_evo_golden_")
    shutil.copytree(os.path.join(ref, "finenvs"), os.path.join(work, "finenvs"),
                    ignore=shutil.ignore_patterns("isaac_gym_envs", "__pycache__", "data"))
    sys.path.insert(0, work)


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "finenvs")):
        sys.exit("usage: python tools/make_evo_golden.py <reference checkout>")
    setup_reference(sys.argv[1])
    from finenvs.agents.ES.evo_agent import EvoAgent

    torch.manual_seed(7)
    env_args = {"env_name": "golden", "num_envs": N, "num_eval_envs": NUM_EVAL, "num_observations": 5 * W, "num_actions": 1}
    agent = EvoAgent(env_args, hidden_dims=(H,), learning_rate=LR, noise_std_dev=SIGMA, l2_coefficient=L2,
                     write_to_csv=False, device_id=-1)
    net = agent.network
    theta0 = flat(net.weight_layers, net.bias_layers).clone()
    rng = np.random.default_rng(11)
    dones = torch.from_numpy(rng.integers(0, N, EPISODES)).long()
    returns = torch.from_numpy(rng.normal(0.0, 40.0, EPISODES).astype(np.float32))
    agent.dones, agent.finished_returns = dones, returns
    net.reconstruct_perturbations()
    half = (N - NUM_EVAL) // 2
    eps = torch.cat(
        [net.perturbed_weights[0][:half].reshape(half, -1), net.perturbed_biases[0][:half].reshape(half, -1),
         net.perturbed_weights[1][:half].reshape(half, -1), net.perturbed_biases[1][:half].reshape(half, -1)], dim=1)
    agent.perform_rank_transformation()
    final_ranks = agent.final_ranks.clone()
    net.update_parameters(agent.final_ranks)
    theta1 = flat(net.weight_layers, net.bias_layers)
    out = os.path.join(REPO, "tests", "golden", "evo_update.npz")
    np.savez_compressed(out, theta0=theta0.numpy(), eps=eps.numpy(), dones=dones.numpy(), returns=returns.numpy(),
                        final_ranks=final_ranks.numpy(), theta1=theta1.numpy(),
                        meta=np.array([N, NUM_EVAL, W, H], dtype=np.int64), hyper=np.array([SIGMA, LR, L2], dtype=np.float64))
    print("wrote", out)


if __name__ == "__main__":
    main()
