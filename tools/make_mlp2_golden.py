#!/usr/bin/env python3
"""Write tests/golden/mlp2_head.npz by RUNNING THE REFERENCE's PPO losses on its two-hidden-layer MLP networks and their
backward (test infrastructure, not the product).

Runs only where a checkout of the reference is available: its Python is imported from a scratch copy of its package, as
tools/make_critic_golden.py does it (nothing of it is written here).  On CPU, flattened f32 states (B, 5W) with realistic
log-return scales, the position feature constant over the window:
  PPO actor   ``ContinuousActorMLP((5W, H, H, 1))`` (ELU, Tanh) and ``compute_actor_loss(states, actions, log_probs,
              advantages)`` (PPO/continuous_actor.py:59-78); the actions are draws of the actor's own policy, the old
              log-probs those of a perturbed copy of it, so that the ratios spread around 1 and a part of them is clipped;
  PPO critic  ``CriticMLP((5W, H, H, 1))`` (ELU, Identity) and ``compute_critic_loss(states, returns)`` (PPO/critic.py:26-32);
each followed by ``backward()``.  Arrays only:
  inputs   state_dicts (``ppo_actor.<key>``, ``ppo_critic.<key>``), states (B, 5W), actions, old_log_probs, advantages,
           returns (B, 1), clip_epsilon, entropy_coefficient, meta (B, W, H)
  outputs  ``out.<net>`` (B, 1), ``loss.<net>`` (scalars) and ``g.<net>.<key>``: every parameter's .grad

    python tools/make_mlp2_golden.py <reference checkout>
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
        sys.exit("usage: python tools/make_mlp2_golden.py <reference checkout>")
    from make_critic_golden import setup_reference

    setup_reference(sys.argv[1])
    from finenvs.agents.PPO.continuous_actor import ContinuousActorMLP
    from finenvs.agents.PPO.critic import CriticMLP

    torch.manual_seed(37)
    actor = ContinuousActorMLP((5 * W, H, H, 1), starting_std_dev=0.5, device_id=-1)
    critic = CriticMLP((5 * W, H, H, 1), device_id=-1)
    nets = {"ppo_actor": actor, "ppo_critic": critic}
    with torch.no_grad():  # inputs of log-return size must move the hidden units: scale their weights up
        for net in nets.values():
            w1 = net.network[0].weight.reshape(H, W, 5)
            w1[:, :, :4].mul_(120.0)
            net.network[2].weight.mul_(3.0)
            net.network[4].weight.mul_(3.0)
        for net in nets.values():  # weights on a grid of 1 / 128 (exact in f32): their arrays compress to a quarter
            for q in net.parameters():
                q.copy_(torch.round(q * 128.0) / 128.0)
    rng = np.random.default_rng(19)
    states = np.concatenate([rng.normal(0.0, 2e-3, (B, W, 4)), rng.uniform(-1.0, 1.0, (B, W, 1))], axis=2).astype(np.float32)
    states[:, :, 4] = states[:, :1, 4]  # the position feature is constant over the window
    s = torch.from_numpy(states.reshape(B, 5 * W))

    with torch.no_grad():
        for net in nets.values():  # not saturated: p is the last layer's output before the activation
            p = net.network[:5](s)
            assert float(p.abs().max()) < 4.0, float(p.abs().max())
            for pre in (net.network[0](s), net.network[:3](s)):  # both hidden layers work on both sides of zero
                assert 0.2 < float((pre < 0).float().mean()) < 0.8, float((pre < 0).float().mean())
        old = copy.deepcopy(actor)
        gen = torch.Generator().manual_seed(5)
        for q in old.parameters():
            q.add_(0.2 * q.abs().mean() * torch.randn(q.shape, generator=gen))
        dist = actor.get_distribution(s)
        actions = dist.loc + dist.scale * torch.randn((B, 1), generator=gen)
        old_log_probs = old.get_distribution(s).log_prob(actions)
        advantages = torch.randn((B, 1), generator=gen)
        returns = critic.forward(s) + 0.3 * torch.randn((B, 1), generator=gen)
        ratios = torch.exp(dist.log_prob(actions) - old_log_probs)
        clip = actor.clip_epsilon
        for edge in (1 - clip, 1 + clip):  # a ratio on the edge of the clip is a discontinuity of the gradient
            assert float((ratios - edge).abs().min()) > 1e-4, float((ratios - edge).abs().min())
        clipped = ((ratios < 1 - clip) & (advantages < 0)) | ((ratios > 1 + clip) & (advantages > 0))
        assert 0 < int(clipped.sum()) < B // 2, int(clipped.sum())
        outs = {f"out.{tag}": net.forward(s).numpy().copy() for tag, net in nets.items()}

    losses, grads = {}, {}

    def record(tag, net, loss):
        loss.backward()
        losses[f"loss.{tag}"] = np.float32(loss.detach())
        for k, p in net.named_parameters():
            grads[f"g.{tag}.{k}"] = p.grad.detach().numpy().copy()

    for net in nets.values():
        net.zero_grad()
    record("ppo_actor", actor, actor.compute_actor_loss(s, actions, old_log_probs, advantages))
    record("ppo_critic", critic, critic.compute_critic_loss(s, returns))
    assert all(np.abs(g).max() > 0 for g in grads.values()), "a gradient of the fixture is identically zero"

    arrays = {}
    for tag, net in nets.items():
        arrays.update({f"{tag}.{k}": v.detach().numpy().copy() for k, v in net.state_dict().items()})
    out = os.path.join(REPO, "tests", "golden", "mlp2_head.npz")
    np.savez_compressed(out, states=s.numpy(), actions=actions.numpy(), old_log_probs=old_log_probs.numpy(),
                        advantages=advantages.numpy(), returns=returns.numpy(), meta=np.array([B, W, H], dtype=np.int64),
                        clip_epsilon=np.float32(clip), entropy_coefficient=np.float32(actor.entropy_coefficient),
                        **outs, **losses, **grads, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
