#!/usr/bin/env python3
"""TD3 (Fujimoto, van Hoof and Meger, "Addressing Function Approximation Error in Actor-Critic Methods", 2018: twin
critics, target policy smoothing, delayed actor and target updates) on the time-series env with synthetic bars, trained
from the device replay ring (finenvs_amd.replay.ReplayBuffer).  Plain torch MLPs on flattened observations.

Every env step stores all N transitions as descriptors (the env writes them through double-buffered descriptors_out);
each training step samples a mini-batch whose states and next states are rendered in one launch.  The last env acts
deterministically (no exploration noise): it is the evaluation env.

With ``--fused-optim`` every optimizer step is one launch of ``FusedAdam`` (finenvs_amd/optim.py): Adam on all of a
network's tensors and, on the delayed iterations, the soft update of their targets in the same pass.  These MLPs have no
packed form, so their tensors are registered with ``add_tensor``.  With the same seed the losses agree with the default
path up to f32 rounding.

With ``--graph-update`` (which implies ``--fused-optim``) the update part of an iteration is ONE hipGraph launch: the
mini-batch is drawn on the device from the replay ring's cursor (``ReplayBuffer(cursor=True).draw``), rendered from that
``ReplayDraw`` (``get_mini_batch(indices=draw)``: head and size are read on the device), and ``GraphedUpdate``
(finenvs_amd/graphed.py) captures the whole update.  The delayed actor update is a host-side alternation, so two graphs
are captured, one with and one without the actor step; each capture runs one warm-up update (a real one) first.  The
env steps and ``buffer.store`` stay outside the graphs; the losses are read only for iterations that are logged.

    python examples/td3_time_series.py [--envs 1024] [--window 16] [--iterations 200] [--batch 256] [--fused-optim]
                                       [--graph-update]
"""
import argparse
import copy
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from finenvs_amd import TimeSeriesEnv  # noqa: E402
from finenvs_amd.data import synthetic  # noqa: E402
from finenvs_amd.graphed import GraphedUpdate  # noqa: E402
from finenvs_amd.optim import FusedAdam  # noqa: E402
from finenvs_amd.replay import ReplayBuffer  # noqa: E402


def mlp(inputs, outputs, hidden, out_act=None):
    layers, d = [], inputs
    for h in hidden:
        layers += [nn.Linear(d, h), nn.ReLU()]
        d = h
    layers.append(nn.Linear(d, outputs))
    if out_act is not None:
        layers.append(out_act)
    return nn.Sequential(*layers)


class Critic(nn.Module):
    def __init__(self, obs_dim, act_dim, hidden):
        super().__init__()
        self.q = mlp(obs_dim + act_dim, 1, hidden)

    def forward(self, s, a):
        return self.q(torch.cat([s, a], dim=1))


def soft_update(target, source, rho):
    with torch.no_grad():
        for t, s in zip(target.parameters(), source.parameters()):
            t.mul_(1.0 - rho).add_(s, alpha=rho)


def main(num_envs=1024, window=16, hidden=(256, 256), iterations=200, batch=256, max_size=1_000_000, days=40, bars=120,
         assets=1, gamma=0.99, rho=0.005, lr=3e-4, exploration_std=0.1, policy_std=0.2, policy_clip=0.5, policy_delay=2,
         reward_scale=0.01, seed=0, quiet=False, fused_optim=False, graph_update=False, log_every=20):
    fused_optim = fused_optim or graph_update
    torch.manual_seed(seed)
    prices, day_id, _ = synthetic.synthetic_series(days, assets, bars, 1234 + seed)
    env = TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=window, num_envs=num_envs, redraw="device", seed=seed)
    dev, N, A = env.device, num_envs, assets
    buffer = ReplayBuffer(env, max_size=max(max_size, N), cursor=graph_update, seed=seed)
    obs_dim = window * 5 * A
    actor = mlp(obs_dim, A, hidden, nn.Tanh()).to(dev)
    critic_1, critic_2 = Critic(obs_dim, A, hidden).to(dev), Critic(obs_dim, A, hidden).to(dev)
    actor_t, critic_1t, critic_2t = copy.deepcopy(actor), copy.deepcopy(critic_1), copy.deepcopy(critic_2)
    if fused_optim:
        actor_opt, critic_opt = FusedAdam(lr=lr), FusedAdam(lr=lr)
        for p, t in zip(actor.parameters(), actor_t.parameters()):
            actor_opt.add_tensor(p, target=t, rho=rho)
        for net, net_t in ((critic_1, critic_1t), (critic_2, critic_2t)):
            for p, t in zip(net.parameters(), net_t.parameters()):
                critic_opt.add_tensor(p, target=t, rho=rho)
    else:
        actor_opt = torch.optim.Adam(actor.parameters(), lr=lr)
        critic_opt = torch.optim.Adam(list(critic_1.parameters()) + list(critic_2.parameters()), lr=lr)
    explore = torch.full((N, 1), exploration_std, device=dev)
    explore[-1] = 0.0  # the evaluation env acts deterministically

    # double-buffered descriptors: the state of step t is what step t - 1 returned
    descriptors = [env.describe(), (torch.empty((N,), dtype=torch.int64, device=dev),
                                    torch.empty((N, A), dtype=torch.float64, device=dev))]
    obs = env.reset()
    eval_return, eval_returns, history = 0.0, [], []
    draw = buffer.new_draw(batch) if graph_update else None
    graphs = {}

    def update(delayed):  # what GraphedUpdate captures: no host integer of the ring, no .item()
        b = buffer.get_mini_batch(batch, indices=buffer.draw(batch, out=draw))
        s, s2 = b["states"].flatten(1), b["next_states"].flatten(1)
        r, d = b["rewards"] * reward_scale, b["dones"]
        with torch.no_grad():
            noise = (torch.randn_like(b["actions"]) * policy_std).clamp(-policy_clip, policy_clip)
            a2 = (actor_t(s2) + noise).clamp(-1.0, 1.0)
            y = r + gamma * (1.0 - d) * torch.min(critic_1t(s2, a2), critic_2t(s2, a2))
        critic_loss = F.mse_loss(critic_1(s, b["actions"]), y) + F.mse_loss(critic_2(s, b["actions"]), y)
        critic_opt.zero_grad()
        critic_loss.backward()
        critic_opt.step(soft_update=delayed)
        if not delayed:
            return (critic_loss.detach(),)
        actor_loss = -critic_1(s, actor(s)).mean()
        actor_loss.backward()
        actor_opt.step()
        return critic_loss.detach(), actor_loss.detach()

    for it in range(iterations):
        with torch.no_grad():
            actions = (actor(obs.float().flatten(1)) + torch.randn((N, A), device=dev) * explore).clamp(-1.0, 1.0)
        state, next_state = descriptors[it % 2], descriptors[(it + 1) % 2]
        obs, rewards, dones, _ = env.step(actions, descriptors_out=next_state)
        buffer.store(state, actions, rewards, next_state, dones)
        eval_return += float(rewards[-1])
        if int(dones[-1]):
            eval_returns.append(eval_return)
            eval_return = 0.0
        if buffer.size() < batch:
            continue
        if graph_update:
            delayed = it % policy_delay == 0
            if delayed not in graphs:  # one warm-up update (a real one) on this ring state, then the capture
                graphs[delayed] = GraphedUpdate(lambda delayed=delayed: update(delayed), warmup=1)
            losses = graphs[delayed].replay()
            entry = {"iteration": it, "buffer_size": buffer.size()}
            if it % log_every == 0 or it == iterations - 1:
                entry.update(zip(("critic_loss", "actor_loss"), (float(x) for x in losses)))
                if not quiet:
                    print(f"iter {it:5d}  buffer {buffer.size():8d}  critic {entry['critic_loss']:.4g}  "
                          f"actor {entry.get('actor_loss', float('nan')):.4g}  eval episodes {len(eval_returns)}")
            history.append(entry)
            continue
        b = buffer.get_mini_batch(batch)
        s, s2 = b["states"].flatten(1), b["next_states"].flatten(1)
        r, d = b["rewards"] * reward_scale, b["dones"]
        with torch.no_grad():  # target policy smoothing, clipped double-Q target
            noise = (torch.randn_like(b["actions"]) * policy_std).clamp(-policy_clip, policy_clip)
            a2 = (actor_t(s2) + noise).clamp(-1.0, 1.0)
            y = r + gamma * (1.0 - d) * torch.min(critic_1t(s2, a2), critic_2t(s2, a2))
        critic_loss = F.mse_loss(critic_1(s, b["actions"]), y) + F.mse_loss(critic_2(s, b["actions"]), y)
        delayed = it % policy_delay == 0  # delayed actor and target updates
        critic_opt.zero_grad()  # (the actor loss's backward left values in the first critic's gradients)
        critic_loss.backward()
        if fused_optim:  # the critics' targets follow in the same launch: the critics do not change before soft_update below
            critic_opt.step(soft_update=delayed)
        else:
            critic_opt.step()
        entry = {"iteration": it, "critic_loss": critic_loss.item(), "buffer_size": buffer.size()}
        if delayed:
            actor_loss = -critic_1(s, actor(s)).mean()
            if not fused_optim:  # FusedAdam.step() leaves the gradients zeroed, and nothing else reaches the actor's
                actor_opt.zero_grad()
            actor_loss.backward()
            actor_opt.step()
            if not fused_optim:
                soft_update(actor_t, actor, rho)
                soft_update(critic_1t, critic_1, rho)
                soft_update(critic_2t, critic_2, rho)
            entry["actor_loss"] = actor_loss.item()
        history.append(entry)
        if not quiet and it % 20 == 0:
            print(f"iter {it:5d}  buffer {buffer.size():8d}  critic {entry['critic_loss']:.4g}  "
                  f"actor {entry.get('actor_loss', float('nan')):.4g}  eval episodes {len(eval_returns)}")
    return history, eval_returns


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--window", type=int, default=16)
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--max-size", type=int, default=1_000_000)
    ap.add_argument("--fused-optim", action="store_true")
    ap.add_argument("--graph-update", action="store_true")
    a = ap.parse_args()
    main(a.envs, a.window, iterations=a.iterations, batch=a.batch, max_size=a.max_size, fused_optim=a.fused_optim,
         graph_update=a.graph_update)
