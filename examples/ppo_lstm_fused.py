#!/usr/bin/env python3
"""PPO with the reference's LSTM actor on the fused rollout: the loop of
/root/reference/examples/time_series/PPO_LSTM_training_SPY.py:22-30 with the K env steps between two ``agent.train``
calls done by ONE kernel launch (actor evaluated in the kernel, actions sampled from the caller's noise, agent.store's
fields written into a trajectory chunk whose ``states`` are 16-byte descriptors).  The learner is plain PyTorch-ROCm
user code (agents are out of this repo's scope): clipped-surrogate PPO with an LSTM actor and an LSTM critic, shaped
like finenvs/agents/PPO/{PPO_agent,continuous_actor,critic}.py.

    python examples/ppo_lstm_fused.py [--envs 4096] [--steps 16] [--iters 5] [--hidden 64] [--window 4] [--fused-update]
                                      [--fused-optim] [--graph-update]

What runs where:
    rollout   : FusedLSTMRollout.run(K, noise, std, trajectory)       one launch per K steps, nothing written but
                                                                       actions / rewards / dones / descriptors
    values    : FusedLSTMRollout(..., "none").forward(descriptors)    all (K + 1) x N states in one launch, no observations
    returns   : TrajectoryBuffer.returns_and_advantages               one reverse-scan kernel (buffer.py:80-100)
    update    : torch autograd on minibatches rendered from descriptors (PPO_agent.py:175-196)
                --fused-update: ppo_actor_loss / ppo_critic_loss of finenvs_amd/lstm_head.py on the minibatches'
                descriptors (fe_lstm_forward / fe_lstm_backward; fe_lstm_backward_streamed at H >= 256): nothing is
                rendered, and the updated parameters reach the rollout kernel without a trip through the host
                --fused-optim (implies --fused-update): FusedAdam of finenvs_amd/optim.py -- Adam and the packing of a
                head in one launch per step (fe_net_update); the heads and their rollouts read its packed buffers and
                its output bias on the device, so nothing is re-packed per call and refresh() has nothing to do
                --graph-update (implies --fused-optim): PPOUpdate of finenvs_amd/ppo.py -- values, returns, the epochs'
                shuffles drawn and gathered on the device (fe_ppo_minibatch), both losses with their gradients one
                launch each, every optimizer step -- captured once by GraphedUpdate and replayed as one hipGraph
                launch per iteration (the first iteration's update is the eager warm-up call)
"""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from finenvs_amd import TimeSeriesEnv  # noqa: E402
from finenvs_amd.data import synthetic  # noqa: E402
from finenvs_amd.lstm_head import FusedLSTMHead, ppo_actor_loss, ppo_critic_loss  # noqa: E402
from finenvs_amd.lstm_head import LSTMHead as TrainableLSTMHead  # noqa: E402
from finenvs_amd.graphed import GraphedUpdate  # noqa: E402
from finenvs_amd.optim import FusedAdam  # noqa: E402
from finenvs_amd.ppo import PPOUpdate  # noqa: E402
from finenvs_amd.rollout import FusedLSTMRollout  # noqa: E402
from finenvs_amd.stats import EpisodeStats  # noqa: E402
from finenvs_amd.trajectory import TrajectoryBuffer  # noqa: E402


class LSTMHead(torch.nn.Module):
    """LSTM(5, H) over the window, Linear(H, 1) on the last hidden state (the shape of the reference's LSTMNetwork)."""

    def __init__(self, hidden: int, squash: bool):
        super().__init__()
        self.lstm = torch.nn.LSTM(5, hidden, num_layers=1, batch_first=True)
        self.last = torch.nn.Linear(hidden, 1)
        self.squash = squash

    def forward(self, states: torch.Tensor) -> torch.Tensor:
        out = self.last(self.lstm(states)[0][:, -1, :])
        return torch.tanh(out) if self.squash else out


def main(envs=4096, steps=16, iters=5, hidden=64, window=4, epochs=2, minibatches=4, seed=0, quiet=False,
         fused_update=False, fused_optim=False, graph_update=False):
    fused_optim = fused_optim or graph_update
    fused_update = fused_update or fused_optim
    torch.manual_seed(seed)
    dev = "cuda:0"
    prices, day_id, _ = synthetic.synthetic_series(12, 1, 390, 1234)
    env = TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=window, num_envs=envs, redraw="device", seed=seed,
                        obs_dtype=torch.float32)  # the learner consumes states.float() (PPO_agent.py:101)
    if fused_update:
        actor = TrainableLSTMHead(hidden, window, "tanh", device=dev)
        critic = TrainableLSTMHead(hidden, window, "none", device=dev)
    else:
        actor, critic = LSTMHead(hidden, True).to(dev), LSTMHead(hidden, False).to(dev)
    log_std = torch.nn.Parameter(torch.full((1,), math.log(0.5), device=dev))
    if fused_optim:
        opt_a, opt_c = FusedAdam(lr=3e-4), FusedAdam(lr=3e-4)
        opt_a.add(actor)
        opt_a.add_tensor(log_std)
        opt_c.add(critic)
    else:
        opt_a = torch.optim.Adam(list(actor.parameters()) + [log_std], 3e-4)
        opt_c = torch.optim.Adam(critic.parameters(), 3e-4)
    traj = TrajectoryBuffer(steps, envs, 1, states=True)
    stats = EpisodeStats(env)
    if fused_update:  # the heads train on descriptors; each owns the rollout object that runs its parameters
        streamed = {"streamed": True} if hidden > 128 else {}  # H >= 256: the chunked backward, an opt-in of the head
        resident_a, resident_c = ({"weights": opt_a}, {"weights": opt_c}) if fused_optim else ({}, {})
        actor_head = FusedLSTMHead(env, actor, **streamed, **resident_a)
        critic_head = FusedLSTMHead(env, critic, **streamed, **resident_c)
        roll, value_head = actor_head.rollout, critic_head.rollout
    else:
        roll = FusedLSTMRollout.from_modules(env, actor.lstm, actor.last)
        value_head = FusedLSTMRollout.from_modules(env, critic.lstm, critic.last, output_activation="none")
    gen = torch.Generator(device=dev).manual_seed(seed)
    clip, ent_coef, gamma = 0.2, 0.01, 0.99
    update = graph = None
    if graph_update:  # the whole train() as one object: captured after its first (eager) call, replayed from then on
        update = PPOUpdate(env, traj, actor_head, critic_head, log_std, opt_a, opt_c, epochs=epochs, minibatches=minibatches,
                           clip_epsilon=clip, entropy_coefficient=ent_coef, gamma=gamma, seed=seed)
    history = []

    def finish(it, loss_c, rewards, std):  # the end of an iteration: the chunk handed back, the episode log read
        traj.clear()
        log = stats.read(reset=True)
        history.append((float(loss_c.detach()), float(rewards.mean()), log))
        if not quiet:
            print(f"iter {it}: critic loss {history[-1][0]:.4f}  mean step reward {history[-1][1]:+.5f}  std {std:.3f}  "
                  f"finished episodes {log['num_training_episodes']}", flush=True)

    t0 = time.perf_counter()
    for it in range(iters):
        # ---- rollout: K env steps, one launch (agent.step + env.step + agent.store, K times) ----
        std = float(log_std.detach().exp())
        noise = torch.randn((steps, envs, 1), generator=gen, device=dev)
        actions, rewards, dones = roll.run(steps, noise=noise, std=std, record_means=True, trajectory=traj)
        if graph_update:
            update.load_means(roll.means)
            if graph is None:  # one real update (the warm-up call), then the capture, which executes nothing
                calls = []

                def train():
                    calls.append(update.train())
                    return calls[-1]

                graph = GraphedUpdate(train, warmup=1)
                loss_c = calls[0][1]  # the warm-up call's loss; calls[1] are the static outputs the replays fill
            else:
                loss_c = graph.replay()[1]
            finish(it, loss_c, rewards, std)
            continue
        with torch.no_grad():
            old_logp = torch.distributions.Normal(roll.means, std).log_prob(actions)           # (K, N, 1)
            # ---- values of the K stored states and of the bootstrap state: the critic on their descriptors ----
            values = value_head.forward(traj.obs_src, traj.obs_pos).reshape(steps + 1, envs)          # (K+1, N)
            returns, advantages = traj.returns_and_advantages(values[:steps], values[steps], gamma)     # (K, N) f32
        # ---- update: minibatches rendered from the descriptors (sample = env * steps + step, buffer.py:102-109) ----
        total = envs * steps
        flat = lambda x: x.reshape(steps, envs).t().reshape(total)  # (K, N[,1]) -> env-major samples
        f_act, f_logp, f_adv, f_ret = flat(actions), flat(old_logp), flat(advantages), flat(returns)
        for _ in range(epochs):
            perm = torch.randperm(total, device=dev)
            for mb in perm.chunk(minibatches):
                if fused_update:  # the same two updates on the minibatch's descriptors (16 bytes per state)
                    src, pos = traj.minibatch_descriptors(mb)
                    loss_a = ppo_actor_loss(actor_head, log_std, src, pos, f_act[mb], f_logp[mb], f_adv[mb], clip, ent_coef)
                    if not fused_optim:  # FusedAdam.step() leaves the gradients zeroed
                        opt_a.zero_grad()
                    loss_a.backward()
                    opt_a.step()
                    loss_c = ppo_critic_loss(critic_head, src, pos, f_ret[mb])
                    if not fused_optim:
                        opt_c.zero_grad()
                    loss_c.backward()
                    opt_c.step()
                    continue
                states = traj.minibatch_states(env, mb)  # (B, W, 5) f32, rendered now
                dist = torch.distributions.Normal(actor(states).squeeze(-1), log_std.exp())
                ratio = (dist.log_prob(f_act[mb]) - f_logp[mb]).exp()
                adv = f_adv[mb]
                surrogate = torch.minimum(ratio * adv, ratio.clamp(1 - clip, 1 + clip) * adv).mean()
                loss_a = -(surrogate + ent_coef * dist.entropy().mean())
                opt_a.zero_grad()
                loss_a.backward()
                opt_a.step()
                loss_c = ((f_ret[mb] - critic(states).squeeze(-1)) ** 2).mean()
                opt_c.zero_grad()
                loss_c.backward()
                opt_c.step()
        if fused_update:  # the last optimizer steps, packed on the device
            actor_head.refresh()
            critic_head.refresh()
        else:
            for head, net in ((roll, actor), (value_head, critic)):  # the updated networks go back into the kernels
                head.set_weights(net.lstm.weight_ih_l0, net.lstm.weight_hh_l0, net.lstm.bias_ih_l0, net.lstm.bias_hh_l0,
                                 net.last.weight, float(net.last.bias.detach()))
        finish(it, loss_c, rewards, std)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if not quiet:
        print(f"{iters} iterations of {steps} steps x {envs} envs in {dt:.2f} s ({iters * steps * envs / dt / 1e6:.2f} M env-steps/s "
              f"including the learner)")
    return history


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--hidden", type=int, default=64, choices=[32, 64, 128, 256, 512, 1024])
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--fused-optim", action="store_true",
                    help="with --fused-update: one launch per optimizer step, packed weights resident on the device")
    ap.add_argument("--fused-update", action="store_true",
                    help="train both heads on descriptors with the fused backward (every --hidden; the chunked "
                         "streamed-weight backward at 256 and above)")
    ap.add_argument("--graph-update", action="store_true",
                    help="implies --fused-optim: the whole update (device shuffle, fused losses, optimizer steps) captured "
                         "once and replayed as one graph launch per iteration")
    a = ap.parse_args()
    main(a.envs, a.steps, a.iters, a.hidden, a.window, fused_update=a.fused_update, fused_optim=a.fused_optim,
         graph_update=a.graph_update)
