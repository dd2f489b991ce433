"""GPU: ``fe_ppo_actor_loss`` / ``fe_ppo_value_loss`` (include/finenvs_amd_ppo.h) at their edges, against torch autograd in
float64 under the derived bound of tests/ppo_loss_cases.py (one f32 ulp per gradient; one f32 ulp plus the order of an
f64 summation for the two sums).  tests/test_ppo_update_gpu.py keeps its ``4 x f32 torch`` comparison at B = 61, 4 096 and
70 001 with every ratio 1e-3 away from a clip boundary; here

* B = 1, 256, 257 (the smallest launch whose ticket publishes a partial), 65 536 and 65 537 (the first strided sample);
* ratios within [1e-7, 1e-5] of ``1 - clip`` and ``1 + clip``, on both sides, under both signs of the advantage;
* advantages of exactly +0.0 and -0.0 (a tie of the minimum) inside and outside the clamp, one NaN advantage;
* ``clip_epsilon = 0``; ``log_std`` in {-5, 0, 2};
* a ``grad_output`` that is not 1; ``means`` as (B,), ``actions`` as a non-contiguous view.

The cases are built on the CPU (tests/ppo_loss_cases.py); tests/test_ppo_loss_edges_host.py decides their conditions."""
import math

import pytest
import torch

from tests import ppo_loss_cases as cases
from tests.helpers import assert_bits
from tests.test_ppo_update_gpu import _kept_workspace, _workspace_left_clean

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fe():
    import finenvs_amd

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return finenvs_amd


def _on_device(c):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


def _fused_actor(d, workspace=None, scale=None, means=None, actions=None):
    """(loss, g_means, g_log_std) of the fused actor loss on the device case ``d``; ``scale * loss`` is differentiated if
    given; ``means`` / ``actions`` replace the case's (another shape or stride of the same values)."""
    from finenvs_amd.lstm_head import fused_ppo_actor_loss

    means = (d["means"] if means is None else means).detach().clone().requires_grad_(True)
    log_std = d["log_std"].detach().clone().requires_grad_(True)
    loss = fused_ppo_actor_loss(means, log_std, d["actions"] if actions is None else actions, d["old_lp"], d["advantages"],
                                d["clip"], cases.ENT, workspace=workspace)
    (loss if scale is None else scale * loss).backward()
    return loss.detach(), means.grad, log_std.grad


def _fused_critic(d, workspace=None, scale=None):
    from finenvs_amd.lstm_head import fused_ppo_critic_loss

    values = d["values"].detach().clone().requires_grad_(True)
    loss = fused_ppo_critic_loss(values, d["returns"], workspace=workspace)
    (loss if scale is None else scale * loss).backward()
    return loss.detach(), values.grad


def _actor_within_bound(got, ref, what):
    worst = (cases.assert_within(got[0], ref["loss"], f"{what}: loss", ref["loss_terms"]),
             cases.assert_within(got[1], ref["g_means"], f"{what}: g_means"),
             cases.assert_within(got[2], ref["g_log_std"], f"{what}: g_log_std", ref["g_log_std_terms"]))
    print(f"{what}: actor loss / g_means / g_log_std errors in f32 ulps of the reference: " + " / ".join(f"{w:.3f}" for w in worst))


@pytest.mark.parametrize("B", cases.EDGE_SIZES)
def test_actor_loss_sizes(fe, B):
    c = cases.size_case(B)
    d, ref = _on_device(c), cases.reference_actor(c)
    big, ws = _kept_workspace(B)
    got = _fused_actor(d, ws)
    _workspace_left_clean(big, ws)
    assert got[1].shape == (B, 1) and got[2].shape == (1,) and got[0].shape == ()
    _actor_within_bound(got, ref, f"B = {B}")
    again = _fused_actor(d, ws)  # the same workspace: the ticket the first launch reset
    _workspace_left_clean(big, ws)
    for name, a, b in zip(("loss", "g_means", "g_log_std"), got, again):
        assert_bits(a.cpu().numpy(), b.cpu().numpy(), f"{name}: two launches")


@pytest.mark.parametrize("B", cases.EDGE_SIZES)
def test_value_loss_sizes(fe, B):
    c = cases.size_case(B)
    d, ref = _on_device(c), cases.reference_critic(c)
    big, ws = _kept_workspace(B)
    got = _fused_critic(d, ws)
    _workspace_left_clean(big, ws)
    worst = (cases.assert_within(got[0], ref["loss"], f"B = {B}: loss", ref["loss_terms"]),
             cases.assert_within(got[1], ref["g_values"], f"B = {B}: g_values"))
    print(f"B = {B}: value loss / g_values errors in f32 ulps of the reference: {worst[0]:.3f} / {worst[1]:.3f}")
    again = _fused_critic(d, ws)
    _workspace_left_clean(big, ws)
    for name, a, b in zip(("loss", "g_values"), got, again):
        assert_bits(a.cpu().numpy(), b.cpu().numpy(), f"{name}: two launches")


def test_actor_loss_next_to_the_clip_boundaries(fe):
    """512 samples in each of the eight populations (boundary, sign of the advantage, side), 1e-7 to 1e-5 from their
    boundary: a wrong comparison or tie weight there changes a gradient by its full size, the bound is one ulp of it."""
    c = cases.boundary_case()
    d, ref = _on_device(c), cases.reference_actor(c)
    got = _fused_actor(d)
    _actor_within_bound(got, ref, "boundaries")
    g = got[1].reshape(-1).cpu()
    for key, members in cases.boundary_populations(c).items():
        assert torch.equal(g[members] == 0, ref["g_means"][members] == 0), key  # clipped exactly where the reference clips


def test_actor_loss_ties_and_a_nan_advantage(fe):
    c = cases.ties_case()
    d, ref = _on_device(c), cases.reference_actor(c)
    big, ws = _kept_workspace(c["B"])
    got = _fused_actor(d, ws)
    _workspace_left_clean(big, ws)
    assert math.isnan(float(got[0])) and math.isnan(float(got[2]))
    g = got[1].reshape(-1).cpu()
    assert torch.nonzero(torch.isnan(g)).reshape(-1).tolist() == [cases.NAN_ADVANTAGE]
    _actor_within_bound(got, ref, "ties")  # NaN where the reference's is, every other gradient finite and within the bound
    zeros = sorted(cases.ZERO_ADVANTAGES)
    assert all(float(g[i]) == 0.0 for i in zeros) and all(float(ref["g_means"][i]) == 0.0 for i in zeros)
    print("signs of the zero gradients, kernel / reference:",
          [(math.copysign(1, float(g[i])), math.copysign(1, float(ref["g_means"][i]))) for i in zeros])


def test_actor_loss_with_no_clip_range(fe):
    c = cases.clip_zero_case()
    got = _fused_actor(_on_device(c))
    _actor_within_bound(got, cases.reference_actor(c), "clip_epsilon = 0")


def test_actor_loss_on_the_boundary_itself(fe):
    """Eight ratios of exactly 1.0 = lo = hi (``clip_epsilon = 0``): clamp's interval is closed, so the whole gradient flows;
    ``ratio > lo`` for ``ratio >= lo`` would halve it."""
    c = cases.exact_boundary_case()
    ref = cases.reference_actor(c)
    got = _fused_actor(_on_device(c))
    _actor_within_bound(got, ref, "ratio = lo = hi")
    assert float(got[1].reshape(-1)[:cases.EXACT].abs().min()) > 0


@pytest.mark.parametrize("log_std", cases.LOG_STDS)
def test_actor_loss_at_other_log_stds(fe, log_std):
    c = cases.log_std_case(log_std)
    ref = cases.reference_actor(c)
    got = _fused_actor(_on_device(c))
    _actor_within_bound(got, ref, f"log_std = {log_std}")
    assert torch.equal(got[1].reshape(-1).cpu() == 0, ref["g_means"] == 0)  # the underflowed ratios' gradients: exact zeros


def test_backward_scales_by_grad_output(fe):
    """``(0.37 * loss).backward()`` gives ``g * 0.37`` in f32, bit for bit, for both losses."""
    d = _on_device(cases.size_case(257))
    plain, scaled = _fused_actor(d), _fused_actor(d, scale=0.37)
    assert_bits(scaled[0].cpu().numpy(), plain[0].cpu().numpy(), "actor loss")
    for name, g, s in zip(("g_means", "g_log_std"), plain[1:], scaled[1:]):
        assert float(g.abs().max()) > 0
        assert_bits(s.cpu().numpy(), (g * 0.37).cpu().numpy(), name)
    plain, scaled = _fused_critic(d), _fused_critic(d, scale=0.37)
    assert_bits(scaled[0].cpu().numpy(), plain[0].cpu().numpy(), "critic loss")
    assert float(plain[1].abs().max()) > 0
    assert_bits(scaled[1].cpu().numpy(), (plain[1] * 0.37).cpu().numpy(), "g_values")


def test_shapes_and_strides_give_the_same_bits(fe):
    """``means`` as (B,) and as (B, 1), ``actions`` as every other element of a wider tensor and as a column of a matrix."""
    d = _on_device(cases.size_case(257))
    B = 257
    base = _fused_actor(d)
    assert base[1].shape == (B, 1)
    flat = _fused_actor(d, means=d["means"].reshape(B))
    assert flat[1].shape == (B,)
    wide = torch.full((B, 2), -3.0, device="cuda")
    wide[:, 0:1] = d["actions"]
    column = wide[:, 0:1]
    every_other = torch.full((2 * B,), -3.0, device="cuda")
    every_other[::2] = d["actions"].reshape(B)
    assert not column.is_contiguous() and not every_other[::2].is_contiguous()
    for what, got in (("means (B,)", flat), ("actions as a matrix column", _fused_actor(d, actions=column)),
                      ("actions[::2]", _fused_actor(d, actions=every_other[::2]))):
        for name, a, b in zip(("loss", "g_means", "g_log_std"), got, base):
            assert_bits(a.reshape(-1).cpu().numpy(), b.reshape(-1).cpu().numpy(), f"{what}: {name}")
