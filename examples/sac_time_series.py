#!/usr/bin/env python3
"""SAC (Haarnoja et al., "Soft Actor-Critic", 2018: twin critics, entropy-regularised targets, learned temperature) on
the time-series env with synthetic bars, in the structure of the reference's SACAgentLSTM: actor
``SACActorLSTM(H=128, W=4)``, twin LSTM critics on ``[states | actions repeated over the window]``
(finenvs/agents/agent_utils.py:5-14), target critics with soft updates.

Rollout chunks come from ``FusedSACRollout.run(K, noise, trajectory=)`` -- K env steps with the actor in the kernel --
and go into the device replay ring with one ``ReplayBuffer.extend``; every training step samples a mini-batch whose
states and next states are rendered in one launch.  The last env is the evaluation env: it acts on the mean.

With ``--fused-targets`` the no-grad target half of every training step runs on the replayed descriptors instead: the
actor in ``FusedSACRollout.forward`` and both target critics plus the Bellman combination in
``FusedTwinCritic.sac_targets`` (the next states are never rendered).  It draws the same indices and normals as the
default path, so with the same seed both compute the same targets up to fp32 rounding.

With ``--fused-critics`` the gradient half of the critics runs on the replayed descriptors too: the critic update is
``FusedTwinCritic.critic_loss`` (both critics' forward and backward through time in HIP, nothing rendered) and the
actor update takes ``min(q1, q2)`` from ``FusedTwinCritic.q`` on the sampled state descriptors, so ``dQ/da`` reaches the
torch actor (which still runs on the rendered states) through the fused backward.

With ``--fused-actor`` the actor's own update runs on the replayed state descriptors as well: ``FusedSACRollout.sample``
gives the actions and log-probabilities with a HIP backward through the head and the recurrence, with the normals drawn
where ``rsample`` drew them.  ``q`` comes from ``FusedTwinCritic.q`` with ``--fused-critics`` (``dQ/da`` then goes from one
fused backward into the other) and from the torch critics on the rendered states otherwise.  With all three flags a
training step renders no observation at all: ``get_mini_batch`` is not called.

With ``--fused-optim`` the parameter side is one launch per optimizer step: ``FusedAdam`` (finenvs_amd/optim.py) runs
Adam on both critics, soft-updates both targets and writes all four packed forms in ``fe_net_update``, and another
does the actor and the temperature.  The fused front ends read those packed buffers (``weights=``) instead of
re-packing the modules at every call, and the actor's two output biases stay on the device.  The arithmetic is
torch's, one f32 rounding per operation: with the same seed the losses agree with the default path up to f32 rounding.

With ``--graph-update`` (which implies the four flags above) the update part of an iteration is ONE hipGraph launch:
the mini-batch is drawn on the device from the replay ring's cursor (``ReplayBuffer(cursor=True).draw``), every fused
front end takes that ``ReplayDraw``, and ``GraphedUpdate`` (finenvs_amd/graphed.py) captures draw, targets, both
backward passes and both optimizer steps once and replays them.  The rollout and ``buffer.extend`` stay outside the
graph.  The first iteration that trains also runs the capture's three warm-up updates (real ones), and the losses are
read from the device only for iterations that are logged.  The draws differ from the other paths' (Philox on the
device instead of ``torch.randint``), so the losses are comparable in distribution, not number for number.

With ``--hidden`` above 128 (256, 512 or 1024; the reference trains ``hidden_dim=1024``) the actor's rollout and
every fused front end the flags above select are built with ``streamed=True``: the kernels whose recurrent weights
stream from L2 (include/finenvs_amd_sac_streamed.h, include/finenvs_amd_critic_streamed.h).

    python examples/sac_time_series.py [--envs 1024] [--hidden 128] [--iterations 100] [--chunk 8] [--batch 256]
                                       [--fused-targets] [--fused-critics] [--fused-actor] [--fused-optim]
                                       [--graph-update]
"""
import argparse
import copy
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from finenvs_amd import TimeSeriesEnv  # noqa: E402
from finenvs_amd.critic import CriticLSTM, FusedTwinCritic  # noqa: E402
from finenvs_amd.data import synthetic  # noqa: E402
from finenvs_amd.graphed import GraphedUpdate  # noqa: E402
from finenvs_amd.optim import FusedAdam  # noqa: E402
from finenvs_amd.replay import ReplayBuffer  # noqa: E402
from finenvs_amd.sac import FusedSACRollout, SACActorLSTM  # noqa: E402
from finenvs_amd.trajectory import TrajectoryBuffer  # noqa: E402


def soft_update(target, source, rho):
    with torch.no_grad():
        for t, s in zip(target.parameters(), source.parameters()):
            t.mul_(1.0 - rho).add_(s, alpha=rho)


def iterate(num_envs=1024, window=4, hidden=128, iterations=100, chunk=8, batch=256, updates_per_chunk=1, max_size=1_000_000,
            days=40, bars=120, gamma=0.99, rho=0.005, lr=3e-4, reward_scale=0.01, seed=0, fused_targets=False,
            fused_critics=False, fused_actor=False, fused_optim=False, graph_update=False, log_every=1):
    """The training loop as a generator: one log entry per iteration that trained (tools/optim_bench.py steps two of
    these alternately).  With ``graph_update`` an entry carries the losses only every ``log_every`` iterations and at
    the last one: reading them waits for the device."""
    if graph_update:
        fused_targets = fused_critics = fused_actor = fused_optim = True
    torch.manual_seed(seed)
    prices, day_id, _ = synthetic.synthetic_series(days, 1, bars, 1234 + seed)
    env = TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=window, num_envs=num_envs, redraw="device", seed=seed)
    dev, N, A = env.device, num_envs, 1
    buffer = ReplayBuffer(env, max_size=max(max_size, chunk * N), cursor=graph_update, seed=seed)
    actor = SACActorLSTM(H=hidden, W=window).to(dev)
    critic_1, critic_2 = CriticLSTM(hidden, window).to(dev), CriticLSTM(hidden, window).to(dev)
    critic_1t, critic_2t = copy.deepcopy(critic_1), copy.deepcopy(critic_2)
    if fused_optim:  # one launch per step: Adam, the soft updates and the packed forms the front ends read
        actor_opt, critic_opt = FusedAdam(lr=lr), FusedAdam(lr=lr)
        actor_opt.add(actor)
        actor_opt.add_tensor(actor.log_alpha)
        critic_opt.add(critic_1, target=critic_1t, rho=rho)
        critic_opt.add(critic_2, target=critic_2t, rho=rho)
        resident_a, resident_c = {"weights": actor_opt}, {"weights": critic_opt}
    else:
        actor_opt = torch.optim.Adam(actor.parameters(), lr=lr)
        alpha_opt = torch.optim.Adam([actor.log_alpha], lr=lr)
        critic_opt = torch.optim.Adam(list(critic_1.parameters()) + list(critic_2.parameters()), lr=lr)
        resident_a = resident_c = {}
    # without weights= the front ends re-pack their modules at every call: updates are seen right away either way
    streamed = {"streamed": True} if hidden > 128 else {}  # the kernels of H = 256 / 512 / 1024 are an opt-in
    roll = FusedSACRollout(env, actor, **resident_a, **streamed)
    twin = FusedTwinCritic(env, critic_1t, critic_2t, **resident_c, **streamed) if fused_targets else None
    twin_online = FusedTwinCritic(env, critic_1, critic_2, **resident_c, **streamed) if fused_critics else None
    gen = torch.Generator(device=dev).manual_seed(seed)
    render = not (fused_critics and fused_actor)  # somebody still reads the rendered states
    graphed, draw = None, buffer.new_draw(batch) if graph_update else None

    def update():  # what GraphedUpdate captures: no host integer of the ring, no .item()
        for _ in range(updates_per_chunk):
            buffer.draw(batch, out=draw)
            y = twin.sac_targets(buffer, draw, roll, torch.randn((batch, 1), device=dev), gamma, actor.log_alpha,
                                 reward_scale=reward_scale)
            critic_loss = twin_online.critic_loss(buffer, draw, y)
            critic_opt.zero_grad()
            critic_loss.backward()
            critic_opt.step()
            a_new, lp = roll.sample(draw.state_src, draw.state_pos, torch.randn((batch, 1), device=dev))
            mean_lp = lp.mean(dim=1, keepdim=True)
            q = torch.min(*twin_online.q(draw.state_src, draw.state_pos, a_new))
            actor_loss = -(q - actor.log_alpha.exp().detach() * mean_lp).mean()
            alpha_loss = (-actor.log_alpha.exp() * (mean_lp + actor.target_entropy).detach()).mean()
            actor_loss.backward()
            alpha_loss.backward()
            actor_opt.step()
        return critic_loss.detach(), actor_loss.detach(), alpha_loss.detach(), actor.log_alpha.detach().exp()

    for it in range(iterations):
        traj = TrajectoryBuffer(chunk, N, A, device=dev, states=True)
        noise = torch.randn((chunk, N, A), generator=gen, device=dev)
        roll.run(chunk, noise=noise, trajectory=traj)
        buffer.extend(traj)
        if buffer.size() < batch:
            continue
        if graph_update:
            if graphed is None:  # three warm-up updates (real ones) on this ring state, then the capture
                graphed = GraphedUpdate(update, warmup=3)
            losses = graphed.replay()
            entry = {"iteration": it, "buffer_size": buffer.size()}
            if it % log_every == 0 or it == iterations - 1:
                entry.update(zip(("critic_loss", "actor_loss", "alpha_loss", "alpha"), (float(x) for x in losses)))
            yield entry
            continue
        for _ in range(updates_per_chunk):
            if fused_targets:  # the same draws as below: get_mini_batch's indices, then rsample's normals
                idx = torch.randint(0, buffer.size(), (batch,), device=dev)
                if render:
                    b = buffer.get_mini_batch(batch, indices=idx)
                    s, a = b["states"], b["actions"]
                eps = torch.randn((batch, 1), device=dev)
                y = twin.sac_targets(buffer, idx, roll, eps, gamma, actor.log_alpha, reward_scale=reward_scale)
            else:
                idx = torch.randint(0, buffer.size(), (batch,), device=dev) if fused_critics or fused_actor else None
                b = buffer.get_mini_batch(batch, indices=idx)
                s, a, s2 = b["states"], b["actions"], b["next_states"]
                r, d = b["rewards"] * reward_scale, b["dones"]
                with torch.no_grad():  # compute_targets (SAC_agent.py:200-225)
                    a2, lp2 = actor.get_actions_and_log_probs(s2)
                    q2 = torch.min(critic_1t(s2, a2), critic_2t(s2, a2))
                    y = r + gamma * (1.0 - d) * (q2 - actor.log_alpha.exp() * lp2.mean(dim=1, keepdim=True))
            if fused_critics:  # the ring's state descriptors and stored actions of the same transitions
                critic_loss = twin_online.critic_loss(buffer, idx, y)
            else:
                critic_loss = F.mse_loss(critic_1(s, a), y) + F.mse_loss(critic_2(s, a), y)
            critic_opt.zero_grad()  # (the actor loss's backward left values in the critics' gradients)
            critic_loss.backward()
            # fused: the targets follow here, not after the actor's update -- the critics do not change in between
            critic_opt.step()
            if fused_critics or fused_actor:
                slots = buffer.physical(idx)
            if fused_actor:  # SAC/actor.py:63-85 on the descriptors, the normals drawn where rsample draws them
                a_new, lp = roll.sample(buffer.state_src[slots], buffer.state_pos[slots], torch.randn((batch, 1), device=dev))
            else:
                a_new, lp = actor.get_actions_and_log_probs(s)  # SAC/actor.py:63-85
            mean_lp = lp.mean(dim=1, keepdim=True)
            if fused_critics:
                q = torch.min(*twin_online.q(buffer.state_src[slots], buffer.state_pos[slots], a_new))
            else:
                q = torch.min(critic_1(s, a_new), critic_2(s, a_new))
            actor_loss = -(q - actor.log_alpha.exp().detach() * mean_lp).mean()
            alpha_loss = (-actor.log_alpha.exp() * (mean_lp + actor.target_entropy).detach()).mean()
            if fused_optim:  # the two losses share no parameter: one step takes both (and zeroes their gradients)
                actor_loss.backward()
                alpha_loss.backward()
                actor_opt.step()
                continue
            actor_opt.zero_grad()
            actor_loss.backward()
            actor_opt.step()
            alpha_opt.zero_grad()
            alpha_loss.backward()
            alpha_opt.step()
            soft_update(critic_1t, critic_1, rho)
            soft_update(critic_2t, critic_2, rho)
        yield {"iteration": it, "critic_loss": critic_loss.item(), "actor_loss": actor_loss.item(),
               "alpha_loss": alpha_loss.item(), "alpha": float(actor.log_alpha.detach().exp()), "buffer_size": buffer.size()}


def main(num_envs=1024, window=4, hidden=128, iterations=100, chunk=8, batch=256, updates_per_chunk=1, max_size=1_000_000,
         days=40, bars=120, gamma=0.99, rho=0.005, lr=3e-4, reward_scale=0.01, seed=0, quiet=False, fused_targets=False,
         fused_critics=False, fused_actor=False, fused_optim=False, graph_update=False, log_every=10):
    history = []
    for entry in iterate(num_envs, window, hidden, iterations, chunk, batch, updates_per_chunk, max_size, days, bars, gamma,
                         rho, lr, reward_scale, seed, fused_targets, fused_critics, fused_actor, fused_optim, graph_update,
                         log_every):
        history.append(entry)
        if not quiet and entry["iteration"] % 10 == 0 and "critic_loss" in entry:
            print(f"iter {entry['iteration']:5d}  buffer {entry['buffer_size']:8d}  critic {entry['critic_loss']:.4g}  "
                  f"actor {entry['actor_loss']:.4g}  alpha {entry['alpha']:.4g}")
    return history


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--fused-targets", action="store_true")
    ap.add_argument("--fused-critics", action="store_true")
    ap.add_argument("--fused-actor", action="store_true")
    ap.add_argument("--fused-optim", action="store_true")
    ap.add_argument("--graph-update", action="store_true")
    a = ap.parse_args()
    main(a.envs, hidden=a.hidden, iterations=a.iterations, chunk=a.chunk, batch=a.batch, fused_targets=a.fused_targets,
         fused_critics=a.fused_critics, fused_actor=a.fused_actor, fused_optim=a.fused_optim,
         graph_update=a.graph_update)
