#!/usr/bin/env python3
"""PPO with the reference's MLP actor on the fused rollout: examples/ppo_lstm_fused.py for ``PPOAgentMLP``
(finenvs/agents/PPO/PPO_agent.py:209-243) with one hidden layer -- ``ContinuousActorMLP((5W, H, 1))`` (ELU, Tanh) and
``CriticMLP((5W, H, 1))`` (ELU, Identity) -- or, with ``--hidden-layers 2``, with the reference's default of two:
``(5W, H, H, 1)`` (finenvs_amd/mlp2_head.py, include/finenvs_amd_mlp2_head.h).  The K env steps between two ``agent.train`` calls are ONE kernel launch
(actor evaluated in the kernel on the matrix cores, actions sampled from the caller's noise, agent.store's fields written
into a trajectory chunk whose ``states`` are 16-byte descriptors).

    python examples/ppo_mlp_fused.py [--envs 4096] [--steps 16] [--iters 5] [--hidden 64] [--window 4] [--fused-update]
                                     [--fused-optim] [--hidden-layers {1,2}]

What runs where:
    rollout   : FusedMLPRollout.run(K, noise, std, trajectory)        one launch per K steps (fe_env_rollout_mlp_sampled),
                                                                       nothing written but actions / rewards / dones /
                                                                       descriptors
    values    : FusedMLPRollout(..., "none").forward(descriptors)     all (K + 1) x N states in one launch, no observations
    returns   : TrajectoryBuffer.returns_and_advantages               one reverse-scan kernel (buffer.py:80-100)
    update    : torch autograd on minibatches rendered from descriptors (PPO_agent.py:175-196)
                --fused-update: ppo_actor_loss / ppo_critic_loss of finenvs_amd/lstm_head.py with the FusedMLPHead of
                finenvs_amd/mlp_head.py on the minibatches' descriptors (fe_mlp_forward / fe_mlp_backward): nothing is
                rendered, and the updated parameters reach the rollout kernel without a trip through the host
                --fused-optim (implies --fused-update): FusedAdam of finenvs_amd/optim.py with the four parameters of each
                head and log_std registered as plain tensors (add_tensor): one launch per optimizer step.  (Packed MLP
                weights resident in the optimizer are out of scope: the heads re-pack on the device, fe_mlp_pack.)
                --hidden-layers 2: the same with MLP2Head / FusedMLP2Head / FusedMLP2Rollout (fe_env_rollout_mlp2_sampled,
                fe_mlp2_forward / fe_mlp2_backward) and six parameters per head
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
from finenvs_amd.lstm_head import ppo_actor_loss, ppo_critic_loss  # noqa: E402
from finenvs_amd.mlp2_head import FusedMLP2Head, MLP2Head, mlp2_head_parameters  # noqa: E402
from finenvs_amd.mlp_head import FusedMLPHead, MLPHead, mlp_head_parameters  # noqa: E402
from finenvs_amd.optim import FusedAdam  # noqa: E402
from finenvs_amd.rollout import FusedMLP2Rollout, FusedMLPRollout  # noqa: E402
from finenvs_amd.stats import EpisodeStats  # noqa: E402
from finenvs_amd.trajectory import TrajectoryBuffer  # noqa: E402


def _rollout_weights(net):
    """``FusedMLPRollout``'s constructor arguments of an ``MLPHead``: W1 (5W, H), b1, W2, b2."""
    w1, b1, w2, b2 = mlp_head_parameters(net)
    return w1.detach().t(), b1.detach(), w2.detach(), float(b2.detach())


def _rollout2_weights(net):
    """``FusedMLP2Rollout``'s constructor arguments of an ``MLP2Head``: W1 (5W, H), b1, W2 (H, H), b2, W3, b3."""
    w1, b1, w2, b2, w3, b3 = mlp2_head_parameters(net)
    return w1.detach().t(), b1.detach(), w2.detach(), b2.detach(), w3.detach(), float(b3.detach())


def main(envs=4096, steps=16, iters=5, hidden=64, window=4, epochs=2, minibatches=4, seed=0, quiet=False,
         fused_update=False, fused_optim=False, hidden_layers=1):
    fused_update = fused_update or fused_optim
    if hidden_layers not in (1, 2):
        raise ValueError(f"hidden_layers must be 1 or 2 (got {hidden_layers})")
    # the module, its parameters in gradient order, the fused head, the rollout object and its constructor arguments
    Head, parameters, FusedHead, Rollout, rollout_weights = (
        (MLPHead, mlp_head_parameters, FusedMLPHead, FusedMLPRollout, _rollout_weights) if hidden_layers == 1 else
        (MLP2Head, mlp2_head_parameters, FusedMLP2Head, FusedMLP2Rollout, _rollout2_weights))
    torch.manual_seed(seed)
    dev = "cuda:0"
    prices, day_id, _ = synthetic.synthetic_series(12, 1, 390, 1234)
    env = TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=window, num_envs=envs, redraw="device", seed=seed,
                        obs_dtype=torch.float32)  # the learner consumes states.float() (PPO_agent.py:101)
    actor = Head(hidden, window, "elu", "tanh", device=dev)
    critic = Head(hidden, window, "elu", "none", device=dev)
    with torch.no_grad():  # log-returns are ~1e-3: scale their columns so that the hidden units see them
        for net in (actor, critic):
            net.network[0].weight.reshape(hidden, window, 5)[:, :, :4].mul_(100.0)
    log_std = torch.nn.Parameter(torch.full((1,), math.log(0.5), device=dev))
    if fused_optim:
        opt_a, opt_c = FusedAdam(lr=3e-4), FusedAdam(lr=3e-4)
        for p in list(parameters(actor)) + [log_std]:
            opt_a.add_tensor(p)
        for p in parameters(critic):
            opt_c.add_tensor(p)
    else:
        opt_a = torch.optim.Adam(list(actor.parameters()) + [log_std], 3e-4)
        opt_c = torch.optim.Adam(critic.parameters(), 3e-4)
    traj = TrajectoryBuffer(steps, envs, 1, states=True)
    stats = EpisodeStats(env)
    if fused_update:  # the heads train on descriptors; each owns the rollout object that runs its parameters
        actor_head, critic_head = FusedHead(env, actor), FusedHead(env, critic)
        roll, value_head = actor_head.rollout, critic_head.rollout
    else:
        roll = Rollout(env, *rollout_weights(actor), activation="elu", output_activation="tanh")
        value_head = Rollout(env, *rollout_weights(critic), activation="elu", output_activation="none")
    gen = torch.Generator(device=dev).manual_seed(seed)
    clip, ent_coef, gamma = 0.2, 0.01, 0.99
    history = []
    t0 = time.perf_counter()
    for it in range(iters):
        # ---- rollout: K env steps, one launch (agent.step + env.step + agent.store, K times) ----
        std = float(log_std.detach().exp())
        noise = torch.randn((steps, envs, 1), generator=gen, device=dev)
        actions, rewards, dones = roll.run(steps, noise=noise, std=std, record_means=True, trajectory=traj)
        with torch.no_grad():
            old_logp = torch.distributions.Normal(roll.means, std).log_prob(actions)           # (K, N, 1)
            # ---- values of the K stored states and of the bootstrap state: the critic on their descriptors ----
            values = value_head.forward(traj.obs_src, traj.obs_pos).reshape(steps + 1, envs)          # (K+1, N)
            returns, advantages = traj.returns_and_advantages(values[:steps], values[steps], gamma)     # (K, N) f32
        # ---- update: minibatches of the descriptors (sample = env * steps + step, buffer.py:102-109) ----
        total = envs * steps
        flat = lambda x: x.reshape(steps, envs).t().reshape(total)  # (K, N[,1]) -> env-major samples
        f_act, f_logp, f_adv, f_ret = flat(actions), flat(old_logp), flat(advantages), flat(returns)
        for _ in range(epochs):
            perm = torch.randperm(total, device=dev)
            for mb in perm.chunk(minibatches):
                if fused_update:  # the two updates on the minibatch's descriptors (16 bytes per state)
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
            roll.set_weights(*rollout_weights(actor))  # the updated networks go back into the kernels
            value_head.set_weights(*rollout_weights(critic))
        traj.clear()
        log = stats.read(reset=True)
        history.append((float(loss_c.detach()), float(rewards.mean()), log))
        if not quiet:
            print(f"iter {it}: critic loss {history[-1][0]:.4f}  mean step reward {history[-1][1]:+.5f}  std {std:.3f}  "
                  f"finished episodes {log['num_training_episodes']}", flush=True)
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
    ap.add_argument("--hidden", type=int, default=64, choices=[32, 64, 128])
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--fused-optim", action="store_true",
                    help="with --fused-update: one launch per optimizer step (FusedAdam on the heads' tensors)")
    ap.add_argument("--fused-update", action="store_true", help="train both heads on descriptors with the fused backward")
    ap.add_argument("--hidden-layers", type=int, default=1, choices=[1, 2],
                    help="2: the reference's default MLP of two hidden layers (H, H)")
    a = ap.parse_args()
    main(a.envs, a.steps, a.iters, a.hidden, a.window, fused_update=a.fused_update, fused_optim=a.fused_optim,
         hidden_layers=a.hidden_layers)
