#!/usr/bin/env python3
"""Write tests/golden/evo2_update.npz by RUNNING THE REFERENCE's two-hidden-layer ES network and update (test
infrastructure, not the product).

Runs only where a checkout of the reference is available; its Python is imported as tools/make_evo_golden.py does it
(a scratch copy of its package on sys.path; nothing of it is written here).  The fixture holds arrays only:
  inputs   theta0 (P) = W1, b1, W2, b2, W3, b3 flattened; eps (pairs, P) the positive perturbations the update sees (after
           reconstruct_perturbations); obs (N, 5W) a batch of observations; dones / returns of the finished episodes in
           the order they finished
  outputs  actions (N, 1): ParallelMLP.forward on obs with the perturbed members, the action noise switched off here
           (add_action_noise replaced by a no-op: it is the only random draw of forward); final_ranks (N) of
           EvoAgent.perform_rank_transformation; theta1 (P) after ParallelMLP.update_parameters

    python tools/make_evo2_golden.py <reference checkout>
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
N, NUM_EVAL, W, H = 24, 2, 4, 32
SIGMA, LR, L2 = 0.02, 0.01, 0.005
EPISODES = 90


def flat(weights, biases):
    return torch.cat([t.reshape(-1) for pair in zip(weights, biases) for t in pair])


def main():
    from make_evo_golden import setup_reference

    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "finenvs")):
        sys.exit("usage: python tools/make_evo2_golden.py <reference checkout>")
    setup_reference(sys.argv[1])
    from finenvs.agents.ES.evo_agent import EvoAgent

    torch.manual_seed(13)
    env_args = {"env_name": "golden", "num_envs": N, "num_eval_envs": NUM_EVAL, "num_observations": 5 * W, "num_actions": 1}
    agent = EvoAgent(env_args, hidden_dims=(H, H), learning_rate=LR, noise_std_dev=SIGMA, l2_coefficient=L2,
                     write_to_csv=False, device_id=-1)
    net = agent.network
    assert [tuple(w.shape) for w in net.weight_layers] == [(5 * W, H), (H, H), (H, 1)]
    theta0 = flat(net.weight_layers, net.bias_layers).clone()
    rng = np.random.default_rng(17)
    # log-return-sized columns and a position column, as the env's observations are
    obs = rng.normal(0.0, 0.02, (N, W, 5)).astype(np.float32)
    obs[:, :, 4] = rng.integers(-3, 4, (N, 1)).astype(np.float32)
    obs = torch.from_numpy(obs.reshape(N, 5 * W))
    net.add_action_noise = lambda outputs, std_dev: None
    actions = net.forward(obs).clone()
    dones = torch.from_numpy(rng.integers(0, N, EPISODES)).long()
    returns = torch.from_numpy(rng.normal(0.0, 40.0, EPISODES).astype(np.float32))
    agent.dones, agent.finished_returns = dones, returns
    net.reconstruct_perturbations()
    half = (N - NUM_EVAL) // 2
    eps = torch.cat([t[:half].reshape(half, -1) for pair in zip(net.perturbed_weights, net.perturbed_biases) for t in pair],
                    dim=1)
    agent.perform_rank_transformation()
    final_ranks = agent.final_ranks.clone()
    net.update_parameters(agent.final_ranks)
    theta1 = flat(net.weight_layers, net.bias_layers)
    out = os.path.join(REPO, "tests", "golden", "evo2_update.npz")
    np.savez_compressed(out, theta0=theta0.numpy(), eps=eps.numpy(), obs=obs.numpy(), actions=actions.numpy(),
                        dones=dones.numpy(), returns=returns.numpy(), final_ranks=final_ranks.numpy(), theta1=theta1.numpy(),
                        meta=np.array([N, NUM_EVAL, W, H], dtype=np.int64), hyper=np.array([SIGMA, LR, L2], dtype=np.float64))
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
