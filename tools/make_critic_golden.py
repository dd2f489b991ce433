#!/usr/bin/env python3
"""Write tests/golden/critic_targets.npz by RUNNING THE REFERENCE's twin critics and both compute_targets (test
infrastructure, not the product).

Runs only where a checkout of the reference is available: its Python is imported from a scratch copy of its package, as
tools/make_sac_golden.py does it (nothing of it is written here).  On CPU, f32 next states (B, W, 5) with realistic
log-return scales: the reference's ``CriticLSTM((6, H, 1), W)`` x 2 on (states, actions), ``SACAgent.compute_targets``
with its ``ActorLSTM((5, H, 1), W)`` and ``TD3Agent.compute_targets`` with its tanh ``ActorLSTM((5, H, 1), W)``, each
with the standard normals it draws recorded (torch.manual_seed, then randn in the same shape).  Arrays only:
  inputs   state_dicts (``c1.<key>``, ``c2.<key>``, ``sac.<key>``, ``td3.<key>``), states (B, W, 5), actions (B, 1),
           rewards (B, 1), dones (B, 1), sac_eps (B, 1), td3_eps (B, 1), meta (B, W, H), params (gamma, log_alpha,
           std, clip)
  outputs  q1, q2 (B, 1) of the critics on (states, actions); sac_targets, td3_targets (B, 1)

    python tools/make_critic_golden.py <reference checkout>
"""
import math
import os
import shutil
import sys
import tempfile
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
B, W, H = 80, 4, 32
GAMMA, LOG_ALPHA, STD, CLIP = 0.99, math.log(0.2), 0.2, 0.5


def setup_reference(ref: str) -> None:
    """A scratch copy of the reference's package on sys.path (its Python writes caches next to its sources)."""
    sys.dont_write_bytecode = True
    work = tempfile.mkdtemp(prefix="fe_critic_golden_")
    shutil.copytree(os.path.join(ref, "finenvs"), os.path.join(work, "finenvs"),
                    ignore=shutil.ignore_patterns("isaac_gym_envs", "__pycache__", "data"))
    sys.path.insert(0, work)


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "finenvs")):
        sys.exit("usage: python tools/make_critic_golden.py <reference checkout>")
    setup_reference(sys.argv[1])
    from finenvs.agents.SAC.actor import ActorLSTM as SACActorLSTM
    from finenvs.agents.SAC.critic import CriticLSTM
    from finenvs.agents.SAC.SAC_agent import SACAgent
    from finenvs.agents.TD3.actor import ActorLSTM as TD3ActorLSTM
    from finenvs.agents.TD3.TD3_agent import TD3Agent

    torch.manual_seed(7)
    c1 = CriticLSTM((6, H, 1), W, device_id=-1)
    c2 = CriticLSTM((6, H, 1), W, device_id=-1)
    sac = SACActorLSTM((5, H, 1), sequence_length=W, device_id=-1)
    td3 = TD3ActorLSTM((5, H, 1), W, device_id=-1)
    with torch.no_grad():  # inputs of log-return size must move the gates: scale the input weights up
        for net in (c1, c2, sac, td3):
            net.lstm.weight_ih_l0[:, :4].mul_(6.0 * np.sqrt(H))
        for net in (c1, c2):
            net.lstm.weight_ih_l0[:, 5].mul_(3.0)
        sac.log_alpha.fill_(LOG_ALPHA)
    rng = np.random.default_rng(4)
    states = np.concatenate([rng.normal(0.0, 2e-3, (B, W, 4)), rng.uniform(-1.0, 1.0, (B, W, 1))], axis=2).astype(np.float32)
    states[:, :, 4] = states[:, :1, 4]  # the position feature is constant over the window
    actions = rng.uniform(-1.0, 1.0, (B, 1)).astype(np.float32)
    rewards = rng.normal(0.0, 1.0, (B, 1)).astype(np.float32)
    dones = (rng.uniform(0.0, 1.0, (B, 1)) < 0.2).astype(np.float32)
    s, a, r, d = (torch.from_numpy(x) for x in (states, actions, rewards, dones))

    with torch.no_grad():
        x = torch.cat([s, a.unsqueeze(1).repeat(1, W, 1)], dim=2)
        q1, q2 = c1.forward(x), c2.forward(x)
        agent = types.SimpleNamespace(actor=sac, target_critic_1=c1, target_critic_2=c2, gamma=GAMMA)
        torch.manual_seed(11)
        sac_y = SACAgent.compute_targets(agent, r, s, d)
        torch.manual_seed(11)
        sac_eps = torch.randn((B, 1))
        agent = types.SimpleNamespace(target_actor=td3, target_critic_1=c1, target_critic_2=c2, gamma=GAMMA,
                                      training_std_dev=STD, traning_clip=CLIP, device="cpu")
        torch.manual_seed(12)
        td3_y = TD3Agent.compute_targets(agent, r, s, d)
        torch.manual_seed(12)
        td3_eps = torch.randn((B, 1))
    arrays = {}
    for tag, net in (("c1", c1), ("c2", c2), ("sac", sac), ("td3", td3)):
        arrays.update({f"{tag}.{k}": v.detach().numpy() for k, v in net.state_dict().items()})
    out = os.path.join(REPO, "tests", "golden", "critic_targets.npz")
    np.savez_compressed(out, states=states, actions=actions, rewards=rewards, dones=dones, sac_eps=sac_eps.numpy(),
                        td3_eps=td3_eps.numpy(), q1=q1.numpy(), q2=q2.numpy(), sac_targets=sac_y.numpy(),
                        td3_targets=td3_y.numpy(), meta=np.array([B, W, H], dtype=np.int64),
                        params=np.array([GAMMA, LOG_ALPHA, STD, CLIP], dtype=np.float64), **arrays)
    print("wrote", out)


if __name__ == "__main__":
    main()
