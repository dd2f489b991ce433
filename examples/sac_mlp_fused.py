#!/usr/bin/env python3
"""SAC with the reference's default MLP networks (``SACAgentMLP``, SAC_agent.py:244-279: an ``ActorMLP`` whose
``MLPNetwork((5W, H, H), ELU, Identity)`` feeds ``mu_layer`` / ``std_layer``, and two ``CriticMLP((5W + 1, H, H, 1))``
critics, each with its target) on the time-series env with synthetic bars -- on observation descriptors only: no state
of the rollout or of a mini-batch is ever rendered.

* acting: ``FusedMLPSACRollout.run`` steps the env ``chunk`` times per launch with the actor in the kernel (the H x H
  layer folded into the head) and the caller's standard normals, writing the transitions' descriptors into a
  ``TrajectoryBuffer`` that ``ReplayBuffer.extend`` stores;
* targets: ``FusedTwinMLPCritic.sac_targets`` -- the actor on the ring's next-state descriptors, both target critics and
  the entropy-regularised Bellman target;
* critics: ``FusedTwinMLPCritic.critic_loss`` on the ring's state descriptors and stored actions;
* actor and temperature: ``FusedMLPSACRollout.actor_losses``, ``-(min Q - alpha log_prob)`` chained through both
  critics' ``dQ/da``, and the temperature's loss.

The optimizers are torch's Adam and the soft update is torch's.

    python examples/sac_mlp_fused.py [--hidden 128] [--envs 1024] [--window 4] [--batch 256] [--iterations 100]
"""
import argparse
import copy
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from finenvs_amd import TimeSeriesEnv  # noqa: E402
from finenvs_amd.data import synthetic  # noqa: E402
from finenvs_amd.mlp_critic import FusedTwinMLPCritic, MLPCritic  # noqa: E402
from finenvs_amd.mlp_sac import FusedMLPSACRollout, SACActorMLP  # noqa: E402
from finenvs_amd.replay import ReplayBuffer  # noqa: E402
from finenvs_amd.trajectory import TrajectoryBuffer  # noqa: E402


def soft_update(target, source, rho):
    with torch.no_grad():
        for t, s in zip(target.parameters(), source.parameters()):
            t.mul_(1.0 - rho).add_(s, alpha=rho)


def main(num_envs=1024, window=4, hidden=128, iterations=100, chunk=4, batch=256, max_size=1_000_000, days=40, bars=120,
         gamma=0.99, rho=0.005, lr=3e-4, starting_alpha=0.2, reward_scale=0.01, seed=0, quiet=False, log_every=10):
    """Returns (history, nets): one log entry per iteration that trained, and the modules by name with their initial
    ``state_dict``s under ``"initial"``."""
    torch.manual_seed(seed)
    prices, day_id, _ = synthetic.synthetic_series(days, 1, bars, 1234 + seed)
    env = TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=window, num_envs=num_envs, redraw="device", seed=seed)
    dev, N = env.device, num_envs
    buffer = ReplayBuffer(env, max_size=max(max_size, chunk * N), seed=seed)
    actor = SACActorMLP(hidden, window, "elu", starting_alpha=starting_alpha).to(dev)
    critic_1, critic_2 = MLPCritic(hidden, window).to(dev), MLPCritic(hidden, window).to(dev)
    critic_1t, critic_2t = copy.deepcopy(critic_1), copy.deepcopy(critic_2)
    nets = {"actor": actor, "critic_1": critic_1, "critic_2": critic_2, "critic_1t": critic_1t, "critic_2t": critic_2t}
    nets["initial"] = {k: copy.deepcopy(m.state_dict()) for k, m in nets.items()}
    actor_opt = torch.optim.Adam(actor.parameters(), lr=lr)
    alpha_opt = torch.optim.Adam([actor.log_alpha], lr=lr)
    critic_opt = torch.optim.Adam(list(critic_1.parameters()) + list(critic_2.parameters()), lr=lr)
    roll = FusedMLPSACRollout(env, actor)  # re-packs (and re-folds) the actor's parameters at every call
    twin, twin_t = FusedTwinMLPCritic(env, critic_1, critic_2), FusedTwinMLPCritic(env, critic_1t, critic_2t)
    gen = torch.Generator(device=dev).manual_seed(seed)
    history = []
    for it in range(iterations):
        traj = TrajectoryBuffer(chunk, N, 1, device=dev, states=True)
        roll.run(chunk, noise=torch.randn((chunk, N, 1), generator=gen, device=dev), trajectory=traj)
        buffer.extend(traj)
        if buffer.size() < batch:
            continue
        entry = {"iteration": it, "buffer_size": buffer.size()}
        idx = torch.randint(0, buffer.size(), (batch,), device=dev)
        y = twin_t.sac_targets(buffer, idx, roll, None, gamma, actor.log_alpha, reward_scale)
        critic_loss = twin.critic_loss(buffer, idx, y)
        critic_opt.zero_grad()  # (the actor loss's backward left values in the critics' gradients)
        critic_loss.backward()
        critic_opt.step()
        actor_loss, alpha_loss = roll.actor_losses(buffer, idx, twin)
        actor_opt.zero_grad()
        actor_loss.backward()
        actor_opt.step()
        alpha_opt.zero_grad()  # (the actor loss's backward left mean(log_probs) * alpha there; the reference discards it)
        alpha_loss.backward()
        alpha_opt.step()
        soft_update(critic_1t, critic_1, rho)
        soft_update(critic_2t, critic_2, rho)
        entry.update(critic_loss=critic_loss.item(), actor_loss=actor_loss.item(), alpha_loss=alpha_loss.item(),
                     alpha=actor.log_alpha.detach().exp().item())
        history.append(entry)
        if not quiet and it % log_every == 0:
            print(f"iter {it:5d}  buffer {entry['buffer_size']:8d}  critic {entry['critic_loss']:.4g}  "
                  f"actor {entry['actor_loss']:.4g}  alpha {entry['alpha']:.4g}")
    return history, nets


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iterations", type=int, default=100)
    a = ap.parse_args()
    main(a.envs, a.window, a.hidden, a.iterations, batch=a.batch)
