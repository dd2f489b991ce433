"""What the CPU and the GPU tests of the fused PPO losses' edges share (tests/test_ppo_loss_edges_host.py,
tests/test_ppo_loss_edges_gpu.py): the cases, built on the CPU from a CPU generator so that their conditions can be decided
without a GPU, the float64 torch reference on the same float32 inputs, and the bound.  No kernel runs in this file.

The bound is derived, not measured.  ``fe_ppo_actor_loss`` / ``fe_ppo_value_loss`` evaluate every sample in f64 and round
each output to f32 once (include/finenvs_amd_ppo.h), so against torch autograd in f64

* a per-sample gradient is within ``2^-23 |want|``: one f32 ulp, half of it the rounding, half a rounding flipped by the
  few f64 ulps by which two ``exp`` / ``log`` and two orders of the same products differ;
* a sum (the loss, ``g_log_std``) is within ``2^-23 |want| + 1e-12 sum|terms|``, the second term for the order of an f64
  summation.

A result below the f32 normal range may be flushed to zero: the cases keep every expected gradient that is not exactly
zero above 1e-30 in magnitude (``smallest_nonzero``), and the host tests assert it."""
import functools
import math

import torch
from torch.distributions import Normal

F32, F64 = torch.float32, torch.float64
CLIP, ENT = 0.2, 0.01
ULP = 2.0 ** -23
SUM_SLACK = 1e-12
RATIOS = (0.5, 0.7, 0.9, 1.0, 1.1, 1.3, 2.0)
# one sample; a full workgroup; two workgroups, the smallest launch whose ticket publishes a partial; the largest launch
# without a stride (256 workgroups); the first strided sample
EDGE_SIZES = (1, 256, 257, 65536, 65537)
BOUNDARY_B = 4096
SMALL_B = 257
LOG_STDS = (-5.0, 0.0, 2.0)
NEAR, FAR, MARGIN = 1e-7, 1e-5, 1e-9  # a boundary population's distance from its boundary, relative; nobody's below MARGIN


def _new_log_probs(means, log_std, actions):
    return Normal(means.double(), log_std.double().exp()).log_prob(actions.double())


def ratios(c):
    """The probability ratios in f64 from the case's f32 inputs, (B,)."""
    return (_new_log_probs(c["means"], c["log_std"], c["actions"]) - c["old_lp"].double()).exp().reshape(-1)


def _draw(B, seed, log_std, targets=RATIOS):
    """B samples whose ratios are ``targets`` in turn, advantages of both signs under each target; values and returns."""
    gen = torch.Generator().manual_seed(seed)
    std = math.exp(log_std)
    means = torch.tanh(torch.randn((B, 1), generator=gen))
    actions = means + std * torch.randn((B, 1), generator=gen)
    if std <= 1.0:
        actions = actions.clamp(-1, 1)
    log_std_t = torch.full((1,), log_std, dtype=F32)
    b = torch.arange(B)
    target = torch.tensor(targets, dtype=F64)[b % len(targets)].reshape(B, 1)
    old_lp = (_new_log_probs(means, log_std_t, actions) - target.log()).float()
    sign = torch.where((b // len(targets)) % 2 == 0, 1.0, -1.0).float().reshape(B, 1)
    advantages = sign * (0.1 + torch.rand((B, 1), generator=gen))
    values = torch.randn((B, 1), generator=gen)
    returns = values + torch.randn((B, 1), generator=gen)
    return dict(B=B, clip=CLIP, means=means, actions=actions, log_std=log_std_t, old_lp=old_lp, advantages=advantages,
                values=values, returns=returns)


@functools.lru_cache(maxsize=None)
def size_case(B):
    return _draw(B, 1000 + B, math.log(0.5))


def boundary_populations(c):
    """{(boundary name, advantage positive, ratio above the boundary): sample indices} of the samples whose f64 ratio lies
    within [NEAR, FAR] relative of a clip boundary."""
    ratio, adv = ratios(c), c["advantages"].double().reshape(-1)
    out = {}
    for name, edge in (("lo", 1.0 - c["clip"]), ("hi", 1.0 + c["clip"])):
        rel = ratio / edge - 1.0
        for positive in (True, False):
            for above in (True, False):
                side = rel if above else -rel
                out[name, positive, above] = torch.nonzero((side >= NEAR) & (side <= FAR) & ((adv > 0) == positive)).reshape(-1)
    return out


def boundary_distance(c):
    """The smallest relative distance of any sample's f64 ratio from a clip boundary."""
    ratio = ratios(c)
    return float(torch.minimum((ratio / (1.0 - c["clip"]) - 1.0).abs(), (ratio / (1.0 + c["clip"]) - 1.0).abs()).min())


@functools.lru_cache(maxsize=None)
def boundary_case():
    """B = 4 096.  Sample b aims at population b % 8 (boundary, sign of the advantage, side): its ``old_lp`` is solved in
    f64 for a ratio of ``edge (1 +- delta)``, delta log-uniform in [2e-7, 5e-6], and rounded to f32.  The rounding moves
    the ratio by up to 2^-24 |old_lp|, so a sample whose realised f64 ratio left [NEAR, FAR] or its side is given one of
    RATIOS instead, far from both boundaries."""
    B = BOUNDARY_B
    c = _draw(B, 4242, math.log(0.5))
    gen = torch.Generator().manual_seed(4243)
    b = torch.arange(B)
    edge = torch.where(b % 2 == 0, 1.0 - CLIP, 1.0 + CLIP).double()
    above = (b // 2) % 2 == 0
    positive = (b // 4) % 2 == 0
    delta = torch.exp(torch.empty(B, dtype=F64).uniform_(math.log(2e-7), math.log(5e-6), generator=gen))
    target = edge * torch.where(above, 1.0 + delta, 1.0 - delta)
    new_lp = _new_log_probs(c["means"], c["log_std"], c["actions"]).reshape(-1)
    aimed = (new_lp - target.log()).float()
    adv = c["advantages"].reshape(-1).abs() * torch.where(positive, 1.0, -1.0).float()
    realised = (new_lp - aimed.double()).exp() / edge - 1.0
    side = torch.where(above, realised, -realised)
    keep = (side >= NEAR) & (side <= FAR)
    c = dict(c)
    c["old_lp"] = torch.where(keep, aimed, c["old_lp"].reshape(-1)).reshape(B, 1)
    c["advantages"] = adv.reshape(B, 1)
    return c


# +0.0 under each of RATIOS in turn, then -0.0 under each, and the last sample (the second workgroup's only one)
ZERO_ADVANTAGES = {**{i: 0.0 for i in range(14, 21)}, **{i: -0.0 for i in range(21, 28)}, 256: -0.0}
NAN_ADVANTAGE = 130


@functools.lru_cache(maxsize=None)
def ties_case():
    """B = 257 (two workgroups).  Fifteen samples have an advantage of exactly +0.0 or -0.0 (both terms of the minimum
    are zeros: a tie), each sign at ratios 0.9, 1.0 and 1.1 (inside the clamp) and 0.5, 0.7, 1.3, 2.0 (outside); sample 130
    has a NaN advantage."""
    c = dict(_draw(SMALL_B, 77, math.log(0.5)))
    adv = c["advantages"].clone()
    for i, z in ZERO_ADVANTAGES.items():
        adv[i, 0] = z
    adv[NAN_ADVANTAGE, 0] = float("nan")
    c["advantages"] = adv
    return c


@functools.lru_cache(maxsize=None)
def clip_zero_case():
    """``clip_epsilon = 0``: both boundaries are 1 and no ratio is inside.  The ratios are RATIOS with 1.00001 for 1.0."""
    c = dict(_draw(SMALL_B, 78, math.log(0.5), tuple(1.00001 if r == 1.0 else r for r in RATIOS)))
    c["clip"] = 0.0
    return c


EXACT = 8  # the first samples of exact_boundary_case


@functools.lru_cache(maxsize=None)
def exact_boundary_case():
    """Ratios of exactly 1.0 = lo = hi under ``clip_epsilon = 0``: the one place where ``ratio >= lo`` and ``ratio > lo``
    differ.  With ``log_std = 0`` the standard deviation, the variance and ``log std`` are 1, 1 and 0 exactly, so
    ``lp = fl(fl(-(d d) / 2) - log sqrt(2 pi))``, d = action - mean, in the kernel's order and in ``Normal.log_prob``'s.
    The two do not hold the same constant: csrc/fe_ppo_kernels.h writes the correctly rounded 0.91893853320467274178,
    ``Normal.log_prob`` evaluates ``math.log(math.sqrt(2 * math.pi))``, one f64 ulp (2^-53) below it.  Where |lp| >= 1 an
    ulp of ``lp`` is 2^-52, so for half of all ``d`` both subtractions round to the same number.  The first EXACT samples
    are searched (plain f64) for a mean and an action whose ``lp`` is, under both constants, the same f32 number; with that
    number as ``old_lp`` the difference is exactly 0 and the ratio ``exp(0)`` in the kernel and in the reference.
    Advantages of both signs; the other samples are ``clip_zero_case``'s rule at ``log_std = 0``."""
    import numpy as np

    K_TORCH, K_KERNEL = math.log(math.sqrt(2 * math.pi)), float("0.91893853320467274178")
    assert K_KERNEL - K_TORCH == 2.0 ** -53
    hits = []
    for k in range(1, 1 << 16):  # old_lp = -(1 + k 2^-23), the f32 numbers below -1
        old = -(1.0 + k * 2.0 ** -23)
        d = math.sqrt(2.0 * (-old - K_TORCH))  # about 0.40: an action's f32 spacing there is 3e-8, so the mean carries the
        action = np.float32(d)                  # fine part, and only below 2^-29, where its own spacing is at most 2^-53
        if float(action) < d:                   # (d d / 2 then moves by 4e-17 a step), is it fine enough
            action = np.nextafter(action, np.float32(1))
        if not 2.0 ** -32 < float(action) - d < 2.0 ** -29:
            continue
        mean = np.float32(float(action) - d)
        for _ in range(16):
            mean = np.nextafter(mean, np.float32(-1))
        for _ in range(48):
            diff = float(action) - float(mean)  # exact in f64: the two span 52 bits
            half_square = -(diff * diff) / 2.0 - 0.0
            if half_square - K_TORCH == old and half_square - K_KERNEL == old:
                hits.append((float(mean), float(action), old))
                break
            mean = np.nextafter(mean, np.float32(1))
        if len(hits) == EXACT:
            break
    assert len(hits) >= EXACT, len(hits)
    B = 64
    c = dict(_draw(B, 79, 0.0, tuple(1.00001 if r == 1.0 else r for r in RATIOS)))
    c["clip"] = 0.0
    for k in ("means", "actions", "old_lp", "advantages"):
        c[k] = c[k].clone()
    for i, (mean, action, old_lp) in enumerate(hits[:EXACT]):
        c["means"][i, 0], c["actions"][i, 0], c["old_lp"][i, 0] = mean, action, old_lp
        c["advantages"][i, 0] = (0.5 + 0.1 * i) * (1.0 if i % 2 == 0 else -1.0)
    return c


@functools.lru_cache(maxsize=None)
def log_std_case(log_std):
    """B = 257 at another ``log_std``.  Three samples of five are a policy that moved: their ``old_lp`` is the log-prob of a
    standard deviation of 0.5 around a mean 0.3 to 1.0 away from the action.  At ``log_std = -5`` (std 0.0067) that is
    more than 44 standard deviations: the ratio underflows to exactly 0 in f64, and so does the gradient.  The other two
    samples' actions lie within three standard deviations of their means and their ratios are those of RATIOS."""
    B = SMALL_B
    c = dict(_draw(B, 500 + int(log_std), log_std))
    gen = torch.Generator().manual_seed(600 + int(log_std))
    b = torch.arange(B)
    moved = (b % 5 < 3).reshape(B, 1)
    std = math.exp(log_std)
    near = (c["means"] + std * torch.empty((B, 1)).uniform_(-3.0, 3.0, generator=gen))
    gap = torch.empty((B, 1)).uniform_(0.3, 1.0, generator=gen)
    far = c["means"] - torch.sign(c["means"]) * gap  # towards zero: inside (-1, 1)
    far = torch.where(c["means"] == 0, gap, far)
    c["actions"] = torch.where(moved, far, near)
    new_lp = _new_log_probs(c["means"], c["log_std"], c["actions"])
    target = torch.tensor(RATIOS, dtype=F64)[b % len(RATIOS)].reshape(B, 1)
    old_moved = Normal(c["means"].double(), 0.5).log_prob(c["actions"].double())
    c["old_lp"] = torch.where(moved, old_moved, new_lp - target.log()).float()
    return c


# ---------------------------------------------------------------- the reference and the bound
def reference_actor(c):
    """torch autograd in f64 on the case's f32 inputs: ``loss``, ``g_means`` (B,), ``g_log_std``, and the sums of the
    absolute per-sample terms of the two sums (``loss_terms``, ``g_log_std_terms``) the bound's slack is scaled by."""
    from finenvs_amd.lstm_head import torch_ppo_actor_loss

    args = [c[k].double() for k in ("actions", "old_lp", "advantages")]
    means = c["means"].double().clone().requires_grad_(True)
    log_std = c["log_std"].double().clone().requires_grad_(True)
    loss = torch_ppo_actor_loss(means, log_std, *args, c["clip"], ENT)
    loss.backward()
    # the same expression with one log_std per sample: its gradient is the per-sample term of d loss / d log_std
    per_sample = c["log_std"].double().expand(c["B"], 1).clone().requires_grad_(True)
    torch_ppo_actor_loss(c["means"].double(), per_sample, *args, c["clip"], ENT).backward()
    ratio, adv = ratios(c).reshape(-1, 1), args[2]
    surrogate = torch.minimum(ratio * adv, ratio.clamp(1 - c["clip"], 1 + c["clip"]) * adv)
    entropy = 0.5 + 0.5 * math.log(2 * math.pi) + float(c["log_std"])
    return dict(loss=loss.detach(), g_means=means.grad.reshape(-1), g_log_std=log_std.grad.reshape(()),
                loss_terms=float(surrogate.abs().mean()) + abs(ENT * entropy), g_log_std_terms=float(per_sample.grad.abs().sum()))


def reference_critic(c):
    from finenvs_amd.lstm_head import torch_ppo_critic_loss

    values = c["values"].double().clone().requires_grad_(True)
    loss = torch_ppo_critic_loss(values, c["returns"].double())
    loss.backward()
    return dict(loss=loss.detach(), g_values=values.grad.reshape(-1), loss_terms=float(loss.detach()))  # squares: |terms| = terms


def smallest_nonzero(x):
    """The smallest magnitude among the finite entries of ``x`` that are not exactly zero (inf if there is none)."""
    x = x.double().reshape(-1).abs()
    x = x[torch.isfinite(x) & (x > 0)]
    return float(x.min()) if x.numel() else math.inf


def assert_within(got, want, what, terms=0.0):
    """``|got - want| <= 2^-23 |want| + 1e-12 terms`` element for element, NaN exactly where ``want`` is NaN; returns the
    worst ``err / (2^-23 |want|)`` over the finite entries with ``want != 0`` (0 if there is none)."""
    got, want = got.detach().double().cpu().reshape(-1), want.detach().double().cpu().reshape(-1)
    assert got.shape == want.shape, f"{what}: {tuple(got.shape)} against {tuple(want.shape)}"
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN at {torch.nonzero(torch.isnan(got)).reshape(-1).tolist()[:8]}, " \
                                               f"the reference's at {torch.nonzero(nan).reshape(-1).tolist()[:8]}"
    got, want = got[~nan], want[~nan]
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    err, tol = (got - want).abs(), ULP * want.abs() + SUM_SLACK * terms
    bad = torch.nonzero(err > tol).reshape(-1)
    assert bad.numel() == 0, (f"{what}: {bad.numel()} beyond the bound, first at {int(bad[0])}: {float(got[bad[0]])!r} against "
                              f"{float(want[bad[0]])!r} (error {float(err[bad[0]]):.3e}, allowed {float(tol[bad[0]]):.3e})")
    scale = want != 0
    return float((err[scale] / (ULP * want[scale].abs())).max()) if bool(scale.any()) else 0.0
