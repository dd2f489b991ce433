#!/usr/bin/env python3
"""Write tests/golden/sac_actor.npz by RUNNING THE REFERENCE's SAC LSTM actor (test infrastructure, not the product).

Runs only where a checkout of the reference is available: its Python is imported from a scratch copy of its package, as
tools/make_evo_golden.py does it (nothing of it is written here).  The reference's ``ActorLSTM((5, H, 1), W)`` on CPU,
f32 observations (B, W, 5) with realistic log-return scales, its own ``rsample`` with the standard normals recorded.
The fixture holds arrays only:
  inputs   the actor's state_dict (one array per key, ``sd.<key>``), obs (B, W, 5), eps (B, 1)
  outputs  loc, scale of get_distribution; actions = tanh(u) and log_probs of get_actions_and_log_probs;
           step_actions of SACAgent.step (tanh(u) with the last row overwritten by loc)

    python tools/make_sac_golden.py <reference checkout>
"""
import os
import shutil
import sys
import tempfile
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
B, W, H = 96, 4, 32


def setup_reference(ref: str) -> None:
    """A scratch copy of the reference's package on sys.path (its Python writes caches next to its sources)."""
    sys.dont_write_bytecode = True
    work = tempfile.mkdtemp(prefix="fe_sac_golden_")
    shutil.copytree(os.path.join(ref, "finenvs"), os.path.join(work, "finenvs"),
                    ignore=shutil.ignore_patterns("isaac_gym_envs", "__pycache__", "data"))
    sys.path.insert(0, work)


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "finenvs")):
        sys.exit("usage: python tools/make_sac_golden.py <reference checkout>")
    setup_reference(sys.argv[1])
    from torch.distributions import Normal

    from finenvs.agents.SAC.actor import ActorLSTM
    from finenvs.agents.SAC.SAC_agent import SACAgent

    torch.manual_seed(5)
    actor = ActorLSTM((5, H, 1), sequence_length=W, device_id=-1)
    with torch.no_grad():  # inputs of log-return size must move the gates: scale the input weights up
        actor.lstm.weight_ih_l0[:, :4].mul_(6.0 * np.sqrt(H))
        actor.std_layer.bias.add_(-0.5)
    rng = np.random.default_rng(3)
    obs = np.concatenate([rng.normal(0.0, 2e-3, (B, W, 4)), rng.uniform(-1.0, 1.0, (B, W, 1))], axis=2).astype(np.float32)
    obs[:, :, 4] = obs[:, :1, 4]  # the position feature is constant over the window
    states = torch.from_numpy(obs)

    drawn = []
    rsample = Normal.rsample

    def recording_rsample(self, sample_shape=torch.Size()):  # Normal.rsample with its standard normals kept
        out = rsample(self, sample_shape)
        drawn.append(((out - self.loc) / self.scale).detach().clone())
        return out

    Normal.rsample = recording_rsample
    with torch.no_grad():
        dist = actor.get_distribution(states)
        g = torch.Generator().manual_seed(11)
        eps = torch.randn(dist.loc.shape, generator=g)
        torch.manual_seed(11)
        actions, log_probs = actor.get_actions_and_log_probs(states)
        torch.manual_seed(11)
        step_actions = SACAgent.step(types.SimpleNamespace(actor=actor), states)
    Normal.rsample = rsample
    # the recorded draws are the generator's own normals: torch.manual_seed(11) then randn in the same shape
    assert torch.allclose(drawn[0], eps, atol=1e-5), "rsample did not draw torch.randn's normals"
    out = os.path.join(REPO, "tests", "golden", "sac_actor.npz")
    arrays = {f"sd.{k}": v.detach().numpy() for k, v in actor.state_dict().items()}
    np.savez_compressed(out, obs=obs, eps=eps.numpy(), loc=dist.loc.numpy(), scale=dist.scale.numpy(),
                        actions=actions.numpy(), log_probs=log_probs.numpy(), step_actions=step_actions.numpy(),
                        meta=np.array([B, W, H], dtype=np.int64), **arrays)
    print("wrote", out)


if __name__ == "__main__":
    main()
