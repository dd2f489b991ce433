"""CPU: the conditions of the fused PPO losses' edge cases (tests/ppo_loss_cases.py), decided without a GPU from the
float64 torch reference: what tests/test_ppo_loss_edges_gpu.py runs on the device is what its docstrings say it is."""
import math
import os

import pytest
import torch

from tests import ppo_loss_cases as cases

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _no_denormal_gradient(c, ref):
    """No expected gradient lies in (0, 1e-30): the kernel's f32 result is a normal number or exactly zero."""
    for k in ("g_means", "g_log_std", "g_values"):
        if k in ref:
            assert cases.smallest_nonzero(ref[k]) > 1e-30, k


@pytest.mark.parametrize("B", cases.EDGE_SIZES)
def test_size_cases(B):
    c = cases.size_case(B)
    assert c["means"].shape == (B, 1) and c["means"].dtype is torch.float32 and c["means"].device.type == "cpu"
    ratio = cases.ratios(c)
    assert cases.boundary_distance(c) > 1e-3  # the ratios are those of RATIOS, up to old_lp's rounding
    assert float((ratio - torch.tensor(cases.RATIOS, dtype=torch.float64)[torch.arange(B) % 7]).abs().max()) < 1e-5
    actor, critic = cases.reference_actor(c), cases.reference_critic(c)
    for ref in (actor, critic):
        assert all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in ref.values())
        _no_denormal_gradient(c, ref)
    if B >= 256:  # every branch of the clip occurs
        adv = c["advantages"].double().reshape(-1)
        for low, high in ((0, 0.8), (0.8, 1.2), (1.2, 9)):
            for positive in (True, False):
                assert bool(((ratio > low) & (ratio < high) & ((adv > 0) == positive)).any()), (low, high, positive)
        assert int((actor["g_means"] == 0).sum()) > B // 8  # the clipped samples' gradients are exact zeros


def test_boundary_case_has_its_eight_populations():
    """For each boundary, sign of the advantage and side, at least eight samples within [1e-7, 1e-5] relative of the
    boundary; no sample within 1e-9.  Measured: all 512 aimed at each population stayed in it, the closest sample 1.4e-7 away."""
    c = cases.boundary_case()
    pops = cases.boundary_populations(c)
    assert len(pops) == 8
    print({k: int(v.numel()) for k, v in pops.items()}, "closest", cases.boundary_distance(c))
    for key, members in pops.items():
        assert members.numel() >= 8, key
    assert cases.boundary_distance(c) >= cases.MARGIN
    ref = cases.reference_actor(c)
    _no_denormal_gradient(c, ref)
    # the populations are where the branch decides: below lo with a negative advantage and above hi with a positive one the
    # minimum takes the clamped term (gradient exactly zero); on the other side, and under the other sign, it flows
    g = ref["g_means"]
    for (name, positive, above), members in pops.items():
        clamped = (name == "lo" and not above and not positive) or (name == "hi" and above and positive)
        assert bool((g[members] == 0).all()) if clamped else bool((g[members] != 0).all()), (name, positive, above)


def test_ties_case():
    c = cases.ties_case()
    adv, ratio = c["advantages"].reshape(-1), cases.ratios(c)
    zeros = sorted(cases.ZERO_ADVANTAGES)
    assert all(float(adv[i]) == 0.0 for i in zeros)
    signs = [math.copysign(1.0, float(adv[i])) for i in zeros]
    inside = [(0.8 < float(ratio[i]) < 1.2) for i in zeros]
    for sign in (1.0, -1.0):
        for where in (True, False):
            assert (sign, where) in set(zip(signs, inside)), (sign, where)
    assert int(torch.isnan(adv).sum()) == 1 and math.isnan(float(adv[cases.NAN_ADVANTAGE]))
    assert cases.boundary_distance(c) > 1e-3
    ref = cases.reference_actor(c)
    assert math.isnan(float(ref["loss"])) and math.isnan(float(ref["g_log_std"]))
    g = ref["g_means"]
    assert torch.nonzero(torch.isnan(g)).reshape(-1).tolist() == [cases.NAN_ADVANTAGE]
    assert all(float(g[i]) == 0.0 for i in zeros)
    _no_denormal_gradient(c, ref)


def test_clip_zero_case():
    c = cases.clip_zero_case()
    assert c["clip"] == 0.0
    assert float((cases.ratios(c) - 1.0).abs().min()) >= 1e-6
    assert cases.boundary_distance(c) >= 1e-6
    ref = cases.reference_actor(c)
    assert math.isfinite(float(ref["loss"]))
    _no_denormal_gradient(c, ref)
    g, ratio, adv = ref["g_means"], cases.ratios(c), c["advantages"].double().reshape(-1)
    assert torch.equal(g != 0, (ratio < 1) == (adv > 0))  # only where min() takes the unclipped term (no mean equals its action)


def test_exact_boundary_case():
    """The first eight ratios are exactly 1.0 = lo = hi, under advantages of both signs; the reference passes the whole
    gradient there (clamp's closed interval, a tie of the minimum), none of them is zero."""
    c = cases.exact_boundary_case()
    assert c["clip"] == 0.0 and float(c["log_std"]) == 0.0
    ratio, adv = cases.ratios(c), c["advantages"].double().reshape(-1)
    exact = slice(0, cases.EXACT)
    assert bool((ratio[exact] == 1.0).all()) and float((ratio[cases.EXACT:] - 1.0).abs().min()) >= 1e-6
    assert bool((adv[exact] > 0).any()) and bool((adv[exact] < 0).any())
    ref = cases.reference_actor(c)
    _no_denormal_gradient(c, ref)
    diff = (c["actions"].double() - c["means"].double()).reshape(-1)
    # the kernel's statement with the kernel's constant (one f64 ulp above Normal.log_prob's) gives old_lp exactly, too
    literal = "0.91893853320467274178"
    assert f"kHalfLog2Pi = {literal};" in open(os.path.join(REPO, "finenvs_amd", "csrc", "fe_ppo_kernels.h")).read()
    assert float(literal) - math.log(math.sqrt(2 * math.pi)) == 2.0 ** -53
    kernel_lp = -(diff * diff) / (2.0 * 1.0) - 0.0 - float(literal)
    assert torch.equal(kernel_lp[exact], c["old_lp"].double().reshape(-1)[exact])
    want = -adv * diff / c["B"]  # d_ratio = adv, ratio = 1, var = 1
    assert float((ref["g_means"][exact] / want[exact] - 1.0).abs().max()) < 1e-12
    assert float(ref["g_means"][exact].abs().min()) > 1e-7


@pytest.mark.parametrize("log_std", cases.LOG_STDS)
def test_log_std_cases(log_std):
    """At ``log_std = -5`` the moved samples' ratios underflow to exactly 0 in f64; two samples of five keep a ratio of
    RATIOS, and at least a quarter of all samples a gradient that is not zero."""
    c = cases.log_std_case(log_std)
    B = c["B"]
    assert float(c["log_std"]) == log_std
    assert cases.boundary_distance(c) >= cases.MARGIN
    ref = cases.reference_actor(c)
    assert math.isfinite(float(ref["loss"])) and math.isfinite(float(ref["g_log_std"]))
    _no_denormal_gradient(c, ref)
    ratio = cases.ratios(c)
    share = float((ref["g_means"] != 0).double().mean())
    print(f"log_std = {log_std}: {int((ratio == 0).sum())} of {B} ratios are 0, {share:.3f} of the gradients are not")
    assert share >= 0.25
    if log_std == -5.0:
        moved = torch.arange(B) % 5 < 3
        assert bool((ratio[moved] == 0).all()) and int((ratio == 0).sum()) > B // 2
        assert cases.smallest_nonzero(ratio) > 0.4  # nothing between an underflow and RATIOS
