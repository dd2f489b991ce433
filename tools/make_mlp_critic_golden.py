#!/usr/bin/env python3
"""Write tests/golden/mlp_critic.npz by RUNNING THE REFERENCE's TD3 MLP networks, their losses with backward() and
``TD3Agent.compute_targets`` (test infrastructure, not the product).

Runs only where a checkout of the reference is available: its Python is imported from a scratch copy of its package, as
tools/make_critic_golden.py does it (nothing of it is written here).  On CPU, flattened f32 states (B, 5W) with realistic
log-return scales, the position feature constant over the window, weights on a grid of 1 / 128:
  critics   ``CriticMLP((5W + 1, H, H, 1))`` x 2 (TD3/critic.py:49-64) on (states, actions): q1, q2, and
            ``Critic.compute_loss(states, actions, targets)`` (TD3/critic.py:31-39) with ``backward()`` for both;
  actor     the tanh ``ActorMLP((5W, H, H, 1))`` (TD3/actor.py:64-80) and ``Actor.compute_loss(states, critic_1)``
            (TD3/actor.py:50-56) with ``backward()``: the actor's and critic 1's .grad;
  targets   ``TD3Agent.compute_targets(rewards, next_states, dones)`` (TD3_agent.py:231-251) with the standard normals it
            draws recorded (torch.manual_seed, then randn in the same shape).
Arrays only:
  inputs   state_dicts (``c1.<key>``, ``c2.<key>``, ``actor.<key>``), states, next_states (B, 5W), actions, rewards,
           dones, targets (B, 1), td3_eps (B, 1), meta (B, W, H), params (gamma, std, clip)
  outputs  q1, q2 (B, 1); loss.c1, loss.c2, loss.actor; g.c1.<key>, g.c2.<key> (critic loss), g.actor.<key> and
           g.actor_c1.<key> (actor loss); td3_targets (B, 1)

    python tools/make_mlp_critic_golden.py <reference checkout>
"""
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
B, W, H = 80, 4, 32
GAMMA, STD, CLIP = 0.99, 0.2, 0.5


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "finenvs")):
        sys.exit("usage: python tools/make_mlp_critic_golden.py <reference checkout>")
    from make_critic_golden import setup_reference

    setup_reference(sys.argv[1])
    from finenvs.agents.TD3.actor import ActorMLP
    from finenvs.agents.TD3.critic import CriticMLP
    from finenvs.agents.TD3.TD3_agent import TD3Agent

    torch.manual_seed(43)
    c1 = CriticMLP((5 * W + 1, H, H, 1), device_id=-1)
    c2 = CriticMLP((5 * W + 1, H, H, 1), device_id=-1)
    actor = ActorMLP((5 * W, H, H, 1), device_id=-1)
    nets = {"c1": c1, "c2": c2, "actor": actor}
    with torch.no_grad():  # inputs of log-return size must move the hidden units: scale their weights up
        for net in nets.values():
            w1 = net.network[0].weight[:, :5 * W].reshape(H, W, 5)
            w1[:, :, :4].mul_(120.0)
            net.network[2].weight.mul_(3.0)
            net.network[4].weight.mul_(3.0)
        for net in (c1, c2):
            net.network[0].weight[:, 5 * W].mul_(3.0)
        for net in nets.values():  # weights on a grid of 1 / 128 (exact in f32): their arrays compress to a quarter
            for q in net.parameters():
                q.copy_(torch.round(q * 128.0) / 128.0)
    rng = np.random.default_rng(23)

    def draw_states():
        x = np.concatenate([rng.normal(0.0, 2e-3, (B, W, 4)), rng.uniform(-1.0, 1.0, (B, W, 1))], axis=2).astype(np.float32)
        x[:, :, 4] = x[:, :1, 4]  # the position feature is constant over the window
        return torch.from_numpy(x.reshape(B, 5 * W))

    s, s_next = draw_states(), draw_states()
    a = torch.from_numpy(rng.uniform(-1.0, 1.0, (B, 1)).astype(np.float32))
    r = torch.from_numpy(rng.normal(0.0, 1.0, (B, 1)).astype(np.float32))
    d = torch.from_numpy((rng.uniform(0.0, 1.0, (B, 1)) < 0.2).astype(np.float32))

    with torch.no_grad():
        x = torch.cat([s, a], dim=1)
        q1, q2 = c1.forward(x), c2.forward(x)
        gen = torch.Generator().manual_seed(5)
        targets = 0.5 * (q1 + q2) + 0.3 * torch.randn((B, 1), generator=gen)
        agent = types.SimpleNamespace(target_actor=actor, target_critic_1=c1, target_critic_2=c2, gamma=GAMMA,
                                      training_std_dev=STD, traning_clip=CLIP, device="cpu")
        torch.manual_seed(12)
        td3_y = TD3Agent.compute_targets(agent, r, s_next, d)
        torch.manual_seed(12)
        td3_eps = torch.randn((B, 1))
        # the f64 side: both hidden layers of every network work on both sides of zero
        for net, inputs in ((c1, x), (c2, x), (actor, s), (c1, torch.cat([s, actor.forward(s)], dim=1))):
            n64 = [m.double() for m in (torch.nn.Linear(*net.network[0].weight.shape[::-1]), torch.nn.Linear(H, H))]
            n64[0].load_state_dict({k: v.double() for k, v in net.network[0].state_dict().items()})
            n64[1].load_state_dict({k: v.double() for k, v in net.network[2].state_dict().items()})
            z1 = n64[0](inputs.double())
            z2 = n64[1](torch.nn.functional.elu(z1))
            for z in (z1, z2):
                assert 0.2 < float((z < 0).double().mean()) < 0.8, float((z < 0).double().mean())

    losses, grads = {}, {}

    def record(tag, loss, named):
        for net in nets.values():
            net.zero_grad()
        loss.backward()
        losses[f"loss.{tag}"] = np.float32(loss.detach())
        for prefix, net in named.items():
            for k, p in net.named_parameters():
                grads[f"g.{prefix}.{k}"] = p.grad.detach().numpy().copy()

    record("c1", c1.compute_loss(s, a, targets), {"c1": c1})
    record("c2", c2.compute_loss(s, a, targets), {"c2": c2})
    record("actor", actor.compute_loss(s, c1), {"actor": actor, "actor_c1": c1})
    # ... and no gradient is identically zero (f64 of the recorded f32: the same zeros)
    assert all(np.abs(g.astype(np.float64)).max() > 0 for g in grads.values()), "a gradient of the fixture is identically zero"

    arrays = {}
    for tag, net in nets.items():
        arrays.update({f"{tag}.{k}": v.detach().numpy().copy() for k, v in net.state_dict().items()})
    out = os.path.join(REPO, "tests", "golden", "mlp_critic.npz")
    np.savez_compressed(out, states=s.numpy(), next_states=s_next.numpy(), actions=a.numpy(), rewards=r.numpy(),
                        dones=d.numpy(), targets=targets.numpy(), td3_eps=td3_eps.numpy(), q1=q1.numpy(), q2=q2.numpy(),
                        td3_targets=td3_y.numpy(), meta=np.array([B, W, H], dtype=np.int64),
                        params=np.array([GAMMA, STD, CLIP], dtype=np.float64), **losses, **grads, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
