#!/usr/bin/env python3
"""TD3 with the reference's LSTM networks (``TD3AgentLSTM``: an ``LSTMNetwork((5, H, 1), W, Tanh)`` actor and two
``CriticLSTM((6, H, 1), W)`` critics, each with its target) on the time-series env with synthetic bars -- on observation
descriptors only: no state of the rollout or of a mini-batch is ever rendered.

* acting: ``FusedLSTMHead.rollout.run`` steps the env ``chunk`` times per launch with the actor in the kernel and
  Gaussian exploration noise, writing the transitions' descriptors into a ``TrajectoryBuffer`` that
  ``ReplayBuffer.extend`` stores;
* targets: ``FusedTwinCritic.td3_targets`` -- the target actor on the ring's next-state descriptors, the smoothed
  action, both target critics and the Bellman target;
* critics: ``FusedTwinCritic.critic_loss`` on the ring's state descriptors and stored actions;
* the delayed actor step: ``td3_actor_loss``, ``-Q_1(s, mu(s))`` chained through the first critic's ``dQ/da``.

``--hidden`` 32 / 64 / 128 runs the register-resident kernels; 256 / 512 / 1024 (the reference trains
``hidden_dim=1024``) the streamed ones (``streamed=True`` on both front ends: their backward's workspace grows with the
batch).  With ``--fused-optim`` every optimizer step is one ``FusedAdam`` launch that also soft-updates the targets and
keeps the packed weights the kernels read; with ``--graph-update`` (which implies it) the update is ONE hipGraph launch,
two graphs being captured for the delayed actor step as examples/td3_time_series.py does.

    python examples/td3_lstm_fused.py [--hidden 128] [--envs 1024] [--window 4] [--batch 256] [--iterations 100]
                                      [--fused-optim] [--graph-update]
"""
import argparse
import copy
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from finenvs_amd import TimeSeriesEnv  # noqa: E402
from finenvs_amd.critic import CriticLSTM, FusedTwinCritic  # noqa: E402
from finenvs_amd.data import synthetic  # noqa: E402
from finenvs_amd.graphed import GraphedUpdate  # noqa: E402
from finenvs_amd.lstm_head import FusedLSTMHead, LSTMHead, td3_actor_loss  # noqa: E402
from finenvs_amd.optim import FusedAdam  # noqa: E402
from finenvs_amd.replay import ReplayBuffer  # noqa: E402
from finenvs_amd.trajectory import TrajectoryBuffer  # noqa: E402


def soft_update(target, source, rho):
    with torch.no_grad():
        for t, s in zip(target.parameters(), source.parameters()):
            t.mul_(1.0 - rho).add_(s, alpha=rho)


def main(num_envs=1024, window=4, hidden=128, iterations=100, chunk=4, batch=256, max_size=1_000_000, days=40, bars=120,
         gamma=0.99, rho=0.005, lr=3e-4, exploration_std=0.1, policy_std=0.2, policy_clip=0.5, policy_delay=2,
         reward_scale=0.01, seed=0, quiet=False, fused_optim=False, graph_update=False, log_every=10):
    """Returns (history, nets): one log entry per iteration that trained (with ``graph_update`` the losses only every
    ``log_every`` iterations and at the last one: reading them waits for the device), and the modules by name with their
    initial ``state_dict``s under ``"initial"``."""
    fused_optim = fused_optim or graph_update
    torch.manual_seed(seed)
    prices, day_id, _ = synthetic.synthetic_series(days, 1, bars, 1234 + seed)
    env = TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=window, num_envs=num_envs, redraw="device", seed=seed)
    dev, N = env.device, num_envs
    buffer = ReplayBuffer(env, max_size=max(max_size, chunk * N), cursor=graph_update, seed=seed)
    actor = LSTMHead(hidden, window, "tanh").to(dev)
    critic_1, critic_2 = CriticLSTM(hidden, window).to(dev), CriticLSTM(hidden, window).to(dev)
    actor_t, critic_1t, critic_2t = copy.deepcopy(actor), copy.deepcopy(critic_1), copy.deepcopy(critic_2)
    nets = {"actor": actor, "critic_1": critic_1, "critic_2": critic_2, "actor_t": actor_t, "critic_1t": critic_1t,
            "critic_2t": critic_2t}
    nets["initial"] = {k: copy.deepcopy(m.state_dict()) for k, m in nets.items()}
    streamed = hidden > 128
    if fused_optim:  # one launch per step: Adam, the soft updates and the packed forms the front ends read
        actor_opt, critic_opt = FusedAdam(lr=lr), FusedAdam(lr=lr)
        actor_opt.add(actor, target=actor_t, rho=rho)
        critic_opt.add(critic_1, target=critic_1t, rho=rho)
        critic_opt.add(critic_2, target=critic_2t, rho=rho)
        resident_a, resident_c = {"weights": actor_opt}, {"weights": critic_opt}
    else:
        actor_opt = torch.optim.Adam(actor.parameters(), lr=lr)
        critic_opt = torch.optim.Adam(list(critic_1.parameters()) + list(critic_2.parameters()), lr=lr)
        resident_a = resident_c = {}
    head = FusedLSTMHead(env, actor, streamed=streamed, **resident_a)
    head_t = FusedLSTMHead(env, actor_t, streamed=streamed, **resident_a)
    twin = FusedTwinCritic(env, critic_1, critic_2, streamed=streamed, **resident_c)
    twin_t = FusedTwinCritic(env, critic_1t, critic_2t, streamed=streamed, **resident_c)
    gen = torch.Generator(device=dev).manual_seed(seed)
    draw = buffer.new_draw(batch) if graph_update else None
    graphs, history = {}, []

    def update(delayed):  # what GraphedUpdate captures: no host integer of the ring, no .item()
        buffer.draw(batch, out=draw)
        y = twin_t.td3_targets(buffer, draw, head_t.rollout, torch.randn((batch, 1), device=dev), gamma, policy_std,
                               policy_clip, reward_scale)
        critic_loss = twin.critic_loss(buffer, draw, y)
        critic_opt.zero_grad()  # (the actor loss's backward left values in the first critic's gradients)
        critic_loss.backward()
        critic_opt.step(soft_update=delayed)
        if not delayed:
            return (critic_loss.detach(),)
        actor_loss = td3_actor_loss(head, buffer, draw, twin)
        actor_loss.backward()
        actor_opt.step()
        return critic_loss.detach(), actor_loss.detach()

    for it in range(iterations):
        traj = TrajectoryBuffer(chunk, N, 1, device=dev, states=True)
        head.refresh()  # the actor's current parameters into the acting kernel (nothing to do with resident weights)
        head.rollout.run(chunk, noise=torch.randn((chunk, N, 1), generator=gen, device=dev), std=exploration_std,
                         trajectory=traj)
        buffer.extend(traj)
        if buffer.size() < batch:
            continue
        delayed = it % policy_delay == 0  # delayed actor and target updates
        entry = {"iteration": it, "buffer_size": buffer.size()}
        if graph_update:
            if delayed not in graphs:  # one warm-up update (a real one) on this ring state, then the capture
                graphs[delayed] = GraphedUpdate(lambda delayed=delayed: update(delayed), warmup=1)
            losses = graphs[delayed].replay()
            if it % log_every == 0 or it == iterations - 1:
                entry.update(zip(("critic_loss", "actor_loss"), (float(x) for x in losses)))
        elif fused_optim:
            idx = torch.randint(0, buffer.size(), (batch,), device=dev)
            y = twin_t.td3_targets(buffer, idx, head_t.rollout, None, gamma, policy_std, policy_clip, reward_scale)
            critic_loss = twin.critic_loss(buffer, idx, y)
            critic_opt.zero_grad()
            critic_loss.backward()
            critic_opt.step(soft_update=delayed)  # the critics' targets follow in the same launch
            entry["critic_loss"] = critic_loss.item()
            if delayed:
                actor_loss = td3_actor_loss(head, buffer, idx, twin)
                actor_loss.backward()
                actor_opt.step()
                entry["actor_loss"] = actor_loss.item()
        else:
            idx = torch.randint(0, buffer.size(), (batch,), device=dev)
            head_t.refresh()  # the soft-updated target actor into its kernel
            y = twin_t.td3_targets(buffer, idx, head_t.rollout, None, gamma, policy_std, policy_clip, reward_scale)
            critic_loss = twin.critic_loss(buffer, idx, y)
            critic_opt.zero_grad()
            critic_loss.backward()
            critic_opt.step()
            entry["critic_loss"] = critic_loss.item()
            if delayed:
                actor_loss = td3_actor_loss(head, buffer, idx, twin)
                actor_opt.zero_grad()
                actor_loss.backward()
                actor_opt.step()
                soft_update(actor_t, actor, rho)
                soft_update(critic_1t, critic_1, rho)
                soft_update(critic_2t, critic_2, rho)
                entry["actor_loss"] = actor_loss.item()
        history.append(entry)
        if not quiet and "critic_loss" in entry and it % log_every == 0:
            print(f"iter {it:5d}  buffer {entry['buffer_size']:8d}  critic {entry['critic_loss']:.4g}  "
                  f"actor {entry.get('actor_loss', float('nan')):.4g}")
    return history, nets


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--fused-optim", action="store_true")
    ap.add_argument("--graph-update", action="store_true")
    a = ap.parse_args()
    main(a.envs, a.window, a.hidden, a.iterations, batch=a.batch, fused_optim=a.fused_optim, graph_update=a.graph_update)
