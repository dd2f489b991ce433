#!/usr/bin/env python3
"""Measured errors of the fused PPO losses (fe_ppo_actor_loss / fe_ppo_value_loss, include/finenvs_amd_ppo.h) against
torch autograd in float64, beside the errors of the same torch expressions in float32 on the same inputs.

    python tools/ppo_loss_check.py [--out profiles/ppo_loss_check.txt] [--batch 61 4096 262144]

Inputs as tests/test_ppo_update_gpu.py builds them: probability ratios from {0.5, 0.7, 0.9, 1.0, 1.1, 1.3, 2.0} (none
within 1e-3 of a clip boundary, so every precision takes the same branch), advantages of both signs.  Error = max
absolute difference to the float64 result; the test's bound is 4 x the float32 torch error."""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RATIOS = (0.5, 0.7, 0.9, 1.0, 1.1, 1.3, 2.0)
CLIP, ENT = 0.2, 0.01


def case(B, seed=99):
    from torch.distributions import Normal

    gen = torch.Generator(device="cuda").manual_seed(seed)
    means = torch.tanh(torch.randn((B, 1), generator=gen, device="cuda"))
    actions = (means + 0.5 * torch.randn((B, 1), generator=gen, device="cuda")).clamp(-1, 1)
    log_std = torch.full((1,), math.log(0.5), device="cuda")
    new_lp = Normal(means.double(), log_std.double().exp()).log_prob(actions.double())
    b = torch.arange(B, device="cuda")
    target = torch.tensor(RATIOS, dtype=torch.float64, device="cuda")[b % 7].reshape(B, 1)
    old_lp = (new_lp - target.log()).float()
    sign = torch.where((b // 7) % 2 == 0, 1.0, -1.0).reshape(B, 1).float()
    advantages = sign * (0.1 + torch.rand((B, 1), generator=gen, device="cuda"))
    values = torch.randn((B, 1), generator=gen, device="cuda")
    returns = values + torch.randn((B, 1), generator=gen, device="cuda")
    ratio = (new_lp - old_lp.double()).exp()
    margin = float(torch.minimum((ratio - (1 - CLIP)).abs(), (ratio - (1 + CLIP)).abs()).min())
    return dict(means=means, actions=actions, log_std=log_std, old_lp=old_lp, advantages=advantages, values=values,
                returns=returns), margin


def actor(c, dtype, fused=False):
    from finenvs_amd.lstm_head import fused_ppo_actor_loss, torch_ppo_actor_loss

    means = c["means"].detach().to(dtype).clone().requires_grad_(True)
    log_std = c["log_std"].detach().to(dtype).clone().requires_grad_(True)
    fn = fused_ppo_actor_loss if fused else torch_ppo_actor_loss
    loss = fn(means, log_std, c["actions"].to(dtype), c["old_lp"].to(dtype), c["advantages"].to(dtype), CLIP, ENT)
    loss.backward()
    return [t.double().reshape(-1) for t in (loss.detach(), means.grad, log_std.grad)]


def critic(c, dtype, fused=False):
    from finenvs_amd.lstm_head import fused_ppo_critic_loss, torch_ppo_critic_loss

    values = c["values"].detach().to(dtype).clone().requires_grad_(True)
    loss = (fused_ppo_critic_loss if fused else torch_ppo_critic_loss)(values, c["returns"].to(dtype))
    loss.backward()
    return [t.double().reshape(-1) for t in (loss.detach(), values.grad)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_loss_check.txt"))
    ap.add_argument("--batch", type=int, nargs="+", default=[61, 4096, 262144])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ppo_loss_check needs the GPU: no device is visible")
    lines = ["# python tools/ppo_loss_check.py   (MI355X; max |x - float64 torch| of the fused kernel and of the float32 torch "
             "expression, same inputs)"]
    for B in a.batch:
        c, margin = case(B)
        lines.append(f"B={B}: closest ratio to a clip boundary {margin:.3e}")
        for what, fn, names in (("actor", actor, ("loss", "g_means", "g_log_std")), ("critic", critic, ("loss", "g_values"))):
            want, f32, got = fn(c, torch.float64), fn(c, torch.float32), fn(c, torch.float32, fused=True)
            for n, w, x, g in zip(names, want, f32, got):
                ek, e32 = float((g - w).abs().max()), float((x - w).abs().max())
                lines.append(f"B={B} {what:6s} {n:9s}: kernel {ek:.3e}   torch f32 {e32:.3e}   |f64| max {float(w.abs().max()):.3e}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
