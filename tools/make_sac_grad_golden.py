#!/usr/bin/env python3
"""Write tests/golden/sac_actor_grads.npz by RUNNING THE REFERENCE's SAC actor losses and their backward (test
infrastructure, not the product).

Runs only where a checkout of the reference is available: its Python is imported from a scratch copy of its package, as
tools/make_critic_grad_golden.py does it (nothing of it is written here).  On CPU, f32 states (B, W, 5) with realistic
log-return scales, the reference's ``ActorLSTM((5, H, 1), W)`` and two ``CriticLSTM((6, H, 1), W)``, then
``actor.compute_losses(states, critic_1, critic_2)`` (SAC/actor.py:63-81) after ``torch.manual_seed(SEED)`` and
``loss.backward()``.  ``eps`` is ``torch.manual_seed(SEED); torch.randn(B, 1)``: the tool asserts that the loss
recomputed through the reference's own modules with ``u = loc + eps * scale`` equals the one ``rsample`` gave, so the
fixture's normals are the ones the gradients belong to.  Arrays only:
  inputs   state_dicts (``actor.<key>``, ``c1.<key>``, ``c2.<key>``), log_alpha, target_entropy, states (B, W, 5),
           eps (B, 1), meta (B, W, H)
  outputs  loss, alpha_loss (scalars); ``g.<key>`` every actor parameter's .grad

    python tools/make_sac_grad_golden.py <reference checkout>
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
B, W, H, SEED = 80, 4, 32, 23


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "finenvs")):
        sys.exit("usage: python tools/make_sac_grad_golden.py <reference checkout>")
    from make_critic_golden import setup_reference

    setup_reference(sys.argv[1])
    from finenvs.agents.agent_utils import match_actions_dim_with_states
    from finenvs.agents.SAC.actor import ActorLSTM
    from finenvs.agents.SAC.critic import CriticLSTM

    torch.manual_seed(29)
    actor = ActorLSTM((5, H, 1), sequence_length=W, starting_alpha=0.7, device_id=-1)
    c1 = CriticLSTM((6, H, 1), W, device_id=-1)
    c2 = CriticLSTM((6, H, 1), W, device_id=-1)
    with torch.no_grad():  # inputs of log-return size must move the gates: scale the input weights up
        actor.lstm.weight_ih_l0[:, :4].mul_(6.0 * np.sqrt(H))
        actor.std_layer.bias.add_(-0.5)
        for net in (c1, c2):
            net.lstm.weight_ih_l0[:, :4].mul_(6.0 * np.sqrt(H))
            net.lstm.weight_ih_l0[:, 5].mul_(3.0)
    rng = np.random.default_rng(13)
    states = np.concatenate([rng.normal(0.0, 2e-3, (B, W, 4)), rng.uniform(-1.0, 1.0, (B, W, 1))], axis=2).astype(np.float32)
    states[:, :, 4] = states[:, :1, 4]  # the position feature is constant over the window
    s = torch.from_numpy(states)

    actor.zero_grad()
    torch.manual_seed(SEED)
    loss, alpha_loss = actor.compute_losses(s, c1, c2)
    loss.backward()
    grads = {f"g.{k}": p.grad.detach().numpy().copy() for k, p in actor.named_parameters()}

    # the normals rsample drew: the loss again through the reference's own modules with the draw made by hand
    torch.manual_seed(SEED)
    eps = torch.randn(B, 1)
    with torch.no_grad():
        dist = actor.get_distribution(s)
        u = dist.loc + eps * dist.scale
        a = torch.tanh(u)
        lp = (dist.log_prob(u) - torch.log(1 - a.pow(2) + 1e-7)).mean(dim=1, keepdim=True)
        ar, dim = match_actions_dim_with_states(s, a)
        sa = torch.cat([s, ar], dim=dim)
        again = -(torch.min(c1.forward(sa), c2.forward(sa)) - actor.log_alpha.exp() * lp).mean()
    assert abs(float(again) - float(loss.detach())) <= 1e-6 * max(1.0, abs(float(again))), (float(again), float(loss))
    assert all(np.abs(g).max() > 0 for g in grads.values()), "a gradient of the fixture is identically zero"

    arrays = {}
    for tag, net in (("actor", actor), ("c1", c1), ("c2", c2)):
        arrays.update({f"{tag}.{k}": v.detach().numpy().copy() for k, v in net.state_dict().items()})
    out = os.path.join(REPO, "tests", "golden", "sac_actor_grads.npz")
    np.savez_compressed(out, states=states, eps=eps.numpy(), meta=np.array([B, W, H], dtype=np.int64),
                        log_alpha=np.float32(actor.log_alpha.detach()), target_entropy=np.float32(actor.target_entropy),
                        loss=np.float32(loss.detach()), alpha_loss=np.float32(alpha_loss.detach()), **grads, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
