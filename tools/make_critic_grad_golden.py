#!/usr/bin/env python3
"""Write tests/golden/critic_grads.npz by RUNNING THE REFERENCE's critic loss and its backward (test infrastructure, not
the product).

Runs only where a checkout of the reference is available: its Python is imported from a scratch copy of its package, as
tools/make_critic_golden.py does it (nothing of it is written here).  On CPU, f32 states (B, W, 5) with realistic
log-return scales, two of the reference's ``CriticLSTM((6, H, 1), W)`` and, for each, ``compute_loss(states, actions,
targets).backward()`` (SAC/critic.py:30-45) with the actions requiring a gradient.  Arrays only:
  inputs   state_dicts (``c1.<key>``, ``c2.<key>``), states (B, W, 5), actions (B, 1), targets (B, 1), meta (B, W, H)
  outputs  loss1, loss2 (scalars); ``g1.<key>`` / ``g2.<key>`` every parameter's .grad; d_actions (B, 1) = the
           actions' .grad after both backward calls

    python tools/make_critic_grad_golden.py <reference checkout>
"""
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
        sys.exit("usage: python tools/make_critic_grad_golden.py <reference checkout>")
    from make_critic_golden import setup_reference

    setup_reference(sys.argv[1])
    from finenvs.agents.SAC.critic import CriticLSTM

    torch.manual_seed(17)
    c1 = CriticLSTM((6, H, 1), W, device_id=-1)
    c2 = CriticLSTM((6, H, 1), W, device_id=-1)
    with torch.no_grad():  # inputs of log-return size must move the gates: scale the input weights up
        for net in (c1, c2):
            net.lstm.weight_ih_l0[:, :4].mul_(6.0 * np.sqrt(H))
            net.lstm.weight_ih_l0[:, 5].mul_(3.0)
    rng = np.random.default_rng(9)
    states = np.concatenate([rng.normal(0.0, 2e-3, (B, W, 4)), rng.uniform(-1.0, 1.0, (B, W, 1))], axis=2).astype(np.float32)
    states[:, :, 4] = states[:, :1, 4]  # the position feature is constant over the window
    actions = rng.uniform(-1.0, 1.0, (B, 1)).astype(np.float32)
    targets = rng.normal(0.0, 1.0, (B, 1)).astype(np.float32)
    s, y = torch.from_numpy(states), torch.from_numpy(targets)
    a = torch.from_numpy(actions.copy()).requires_grad_()
    arrays = {}
    for tag, net in (("c1", c1), ("c2", c2)):
        arrays.update({f"{tag}.{k}": v.detach().numpy().copy() for k, v in net.state_dict().items()})
    losses = []
    for tag, net in (("g1", c1), ("g2", c2)):
        net.zero_grad()
        loss = net.compute_loss(s, a, y)
        loss.backward()
        losses.append(float(loss.detach()))
        arrays.update({f"{tag}.{k}": p.grad.detach().numpy().copy() for k, p in net.named_parameters()})
    out = os.path.join(REPO, "tests", "golden", "critic_grads.npz")
    np.savez_compressed(out, states=states, actions=actions, targets=targets, meta=np.array([B, W, H], dtype=np.int64),
                        loss1=np.float32(losses[0]), loss2=np.float32(losses[1]), d_actions=a.grad.numpy(), **arrays)
    print("wrote", out)


if __name__ == "__main__":
    main()
