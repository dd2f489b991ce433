#!/usr/bin/env python3
"""Write tests/golden/lstm_head_grads.npz by RUNNING THE REFERENCE's PPO and TD3 losses on its one-output LSTM networks
and their backward (test infrastructure, not the product).

Runs only where a checkout of the reference is available: its Python is imported from a scratch copy of its package, as
tools/make_critic_golden.py does it (nothing of it is written here).  On CPU, f32 states (B, W, 5) with realistic
log-return scales:
  PPO actor   ``ContinuousActorLSTM((5, H, 1), W)`` and ``compute_actor_loss(states, actions, log_probs, advantages)``
              (PPO/continuous_actor.py:59-78); the actions are draws of the actor's own policy, the old log-probs those
              of a perturbed copy of it, so that the ratios spread around 1 and a part of them is clipped;
  PPO critic  ``CriticLSTM((5, H, 1), W)`` and ``compute_critic_loss(states, returns)`` (PPO/critic.py:26-32);
  TD3 actor   ``ActorLSTM((5, H, 1), W)`` and ``compute_loss(states, critic)`` with one TD3 ``CriticLSTM((6, H, 1), W)``
              (TD3/actor.py:50-56);
each followed by ``backward()``.  Arrays only:
  inputs   state_dicts (``ppo_actor.<key>``, ``ppo_critic.<key>``, ``td3_critic.<key>``; TD3's actor has the PPO actor's
           ``lstm.*`` and ``last_layer.*``),
           states (B, W, 5), actions, old_log_probs, advantages, returns (B, 1), clip_epsilon, entropy_coefficient,
           meta (B, W, H)
  outputs  ``loss.<net>`` (scalars) and ``g.<net>.<key>``: every parameter's .grad of the three trained networks

    python tools/make_lstm_grad_golden.py <reference checkout>
"""
import copy
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
B, W, H = 80, 4, 32


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "finenvs")):
        sys.exit("usage: python tools/make_lstm_grad_golden.py <reference checkout>")
    from make_critic_golden import setup_reference

    setup_reference(sys.argv[1])
    from finenvs.agents.PPO.continuous_actor import ContinuousActorLSTM
    from finenvs.agents.PPO.critic import CriticLSTM as PPOCriticLSTM
    from finenvs.agents.TD3.actor import ActorLSTM as TD3ActorLSTM
    from finenvs.agents.TD3.critic import CriticLSTM as TD3CriticLSTM

    torch.manual_seed(31)
    ppo_actor = ContinuousActorLSTM((5, H, 1), sequence_length=W, starting_std_dev=0.5, device_id=-1)
    ppo_critic = PPOCriticLSTM((5, H, 1), sequence_length=W, device_id=-1)
    td3_actor = TD3ActorLSTM((5, H, 1), W, device_id=-1)
    td3_critic = TD3CriticLSTM((6, H, 1), W, device_id=-1)
    nets = {"ppo_actor": ppo_actor, "ppo_critic": ppo_critic, "td3_actor": td3_actor, "td3_critic": td3_critic}
    with torch.no_grad():  # inputs of log-return size must move the gates: scale the input weights up
        for net in nets.values():
            net.lstm.weight_ih_l0[:, :4].mul_(6.0 * np.sqrt(H))
        td3_critic.lstm.weight_ih_l0[:, 5].mul_(3.0)
        # TD3's actor is the same network as PPO's (LSTMNetwork((5, H, 1), W, Tanh)): the fixture holds its weights once
        td3_actor.load_state_dict({k: v for k, v in ppo_actor.state_dict().items() if k != "log_standard_deviation"})
        for net in nets.values():  # weights on a grid of 1 / 128 (exact in f32): their arrays compress to a quarter
            for q in net.parameters():
                q.copy_(torch.round(q * 128.0) / 128.0)
    rng = np.random.default_rng(17)
    states = np.concatenate([rng.normal(0.0, 2e-3, (B, W, 4)), rng.uniform(-1.0, 1.0, (B, W, 1))], axis=2).astype(np.float32)
    states[:, :, 4] = states[:, :1, 4]  # the position feature is constant over the window
    s = torch.from_numpy(states)

    with torch.no_grad():
        for net in (ppo_actor, ppo_critic, td3_actor):  # not saturated: p is the last layer's output before the activation
            p = net.last_layer[0](net.lstm(s)[0][:, -1, :])
            assert float(p.abs().max()) < 4.0, float(p.abs().max())
        old = copy.deepcopy(ppo_actor)
        gen = torch.Generator().manual_seed(5)
        for q in old.parameters():
            q.add_(0.4 * q.abs().mean() * torch.randn(q.shape, generator=gen))
        dist = ppo_actor.get_distribution(s)
        actions = dist.loc + dist.scale * torch.randn((B, 1), generator=gen)
        old_log_probs = old.get_distribution(s).log_prob(actions)
        advantages = torch.randn((B, 1), generator=gen)
        returns = ppo_critic.forward(s) + 0.3 * torch.randn((B, 1), generator=gen)
        ratios = torch.exp(dist.log_prob(actions) - old_log_probs)
        clip = ppo_actor.clip_epsilon
        for edge in (1 - clip, 1 + clip):  # a ratio on the edge of the clip is a discontinuity of the gradient
            assert float((ratios - edge).abs().min()) > 1e-4, float((ratios - edge).abs().min())
        clipped = ((ratios < 1 - clip) & (advantages < 0)) | ((ratios > 1 + clip) & (advantages > 0))
        assert 0 < int(clipped.sum()) < B // 2, int(clipped.sum())

    losses, grads = {}, {}

    def record(tag, net, loss):
        loss.backward()
        losses[f"loss.{tag}"] = np.float32(loss.detach())
        for k, p in net.named_parameters():
            grads[f"g.{tag}.{k}"] = p.grad.detach().numpy().copy()

    for net in nets.values():
        net.zero_grad()
    record("ppo_actor", ppo_actor, ppo_actor.compute_actor_loss(s, actions, old_log_probs, advantages))
    record("ppo_critic", ppo_critic, ppo_critic.compute_critic_loss(s, returns))
    record("td3_actor", td3_actor, td3_actor.compute_loss(s, td3_critic))
    assert all(np.abs(g).max() > 0 for g in grads.values()), "a gradient of the fixture is identically zero"

    arrays = {}
    for tag, net in nets.items():
        if tag == "td3_actor":
            continue
        arrays.update({f"{tag}.{k}": v.detach().numpy().copy() for k, v in net.state_dict().items()})
    out = os.path.join(REPO, "tests", "golden", "lstm_head_grads.npz")
    np.savez_compressed(out, states=states, actions=actions.numpy(), old_log_probs=old_log_probs.numpy(),
                        advantages=advantages.numpy(), returns=returns.numpy(), meta=np.array([B, W, H], dtype=np.int64),
                        clip_epsilon=np.float32(clip), entropy_coefficient=np.float32(ppo_actor.entropy_coefficient),
                        **losses, **grads, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
