"""CPU: the conditions the hot cases of tests/test_saturated_gpu.py rest on, checked without a GPU.

Every case of ``HOT`` is built by the family's own builder (inside ``tests/helpers.py::modules_on_cpu``), heated with its
gate and output scale and evaluated in f64 on the case's crafted batch, rendered from the oracle's log-return table
(``cpu_states``): the saturated shares of ``hot_shares`` must hold, so that a change to a builder, to the descriptor
generator or to the synthetic series cannot quietly empty the saturated share the GPU cases are there for.
"""
import pytest
import torch

from tests import test_saturated_gpu as S
from tests.helpers import cpu_states, heat, hot_preactivations, hot_shares, modules_on_cpu


def _states(H, W, B):
    src, pos = S.descriptors(H, W, B)
    states, (D, L) = cpu_states(S.DAYS, S.BARS, W, S.TABLE_SEED, src, pos)
    assert (D, L) == (S.DAYS - 1, S.BARS + W)  # the table ``descriptors`` drew its windows for
    assert tuple(states.shape) == (B, W, 5) and states.dtype is torch.float64
    return states


def test_every_family_and_shape_has_a_hot_case():
    for family, variants in (("head", ("tanh", "none")), ("critics", (None,)), ("sac", (None,)), ("mlp", S.ACTIVATIONS),
                             ("mlp2", S.ACTIVATIONS), ("mlp critics", S.ACTIVATIONS)):
        shapes = S.SHAPES + ([S.STREAMED] if family in ("head", "critics", "sac") else [])
        for v in variants:
            for shape in shapes:
                if shape == (64, 7, 257) and (family, v) in (("head", "tanh"), ("sac", None)):
                    shape = (64, 5, 257)  # SHORTENED in tests/test_saturated_gpu.py: b_out / b_mu / b_std are not resolvable at W = 7
                gate, out, seed = S.HOT[(family, v) + shape]
                assert 20 <= gate <= 100, (family, v, shape)


@pytest.mark.parametrize("case", list(S.HOT), ids=str)
def test_hot_case_meets_the_saturated_shares(case):
    family, variant, H, W, B = case
    states = _states(H, W, B)
    with modules_on_cpu():
        fam, mods, aux, cs = S.hot_case(case, states, "cpu")
    assert all(p.device.type == "cpu" for m in mods for p in m.parameters())
    sh, kink = S.shares(fam, mods, states, aux)  # asserts them
    assert len(sh) == len(mods) and int(kink.sum()) <= 0.02 * B
    if family == "sac":  # enough pairs keep their log-probability's upstream gradient
        u = fam.preacts(mods, states, aux)[0][1]
        assert float((u.abs() <= S.SAC_GUARD_U).double().mean()) >= 0.3


@pytest.mark.parametrize("H,W,B,hot", S.CHAINED)
def test_the_chained_sac_actor_keeps_hot_gates_after_its_output_scale_is_halved(H, W, B, hot):
    states = _states(H, W, B)
    with modules_on_cpu():
        fam, mods, aux, _ = S.hot_case(("sac", None, H, W, B), states, "cpu", 20)  # the seed the chained test starts from
    for _ in range(12):
        if float(fam.preacts(mods, states, aux)[0][1].abs().max()) <= S.SAC_GUARD_U:
            break
        heat(mods[0], 1.0, 0.5)
    z, u = fam.preacts(mods, states, aux)[0]
    assert float(u.abs().max()) <= S.SAC_GUARD_U
    hot_shares(z, None, True, False)


def test_heat_scales_the_layers_it_names_and_no_other():
    with modules_on_cpu():
        for build, gates, out, rest in (
                (lambda: S.tl._module(32, 4, 1), ("lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0"),
                 ("last_layer.0.weight", "last_layer.0.bias"), ()),
                (lambda: S.tsac._actor(32, 4, 1), ("lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0"),
                 ("mu_layer.weight", "mu_layer.bias"), ("last_layer.0.weight", "last_layer.0.bias", "std_layer.weight", "std_layer.bias")),
                (lambda: S.t2._module(32, 4, 1), ("network.0.weight", "network.0.bias"), ("network.4.weight", "network.4.bias"),
                 ("network.2.weight", "network.2.bias"))):
            a, b = build(), heat(build(), 7.0, 3.0)
            pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
            for n in gates:
                assert torch.equal(pb[n], pa[n] * 7.0), n
            for n in out:
                assert torch.equal(pb[n], pa[n] * 3.0), n
            for n in rest:
                assert torch.equal(pb[n], pa[n]), n
            assert set(gates) | set(out) | set(rest) == set(pa)


def test_hot_preactivations_of_an_unheated_head_are_the_modules_own():
    states = _states(32, 4, 33)
    with modules_on_cpu():
        m = S.tl._module(32, 4, 20, "tanh")
        q = S.th._module(32, 4, 20, "elu", "tanh")
    z, p = hot_preactivations(m, states)
    assert tuple(z.shape) == (33, 4, 128) and float((torch.tanh(p) - m.double()(states).detach()).abs().max()) < 1e-12
    z, p = hot_preactivations(q, states)
    assert tuple(z.shape) == (33, 32) and float((torch.tanh(p) - q.double()(states).detach()).abs().max()) < 1e-12
    with pytest.raises(AssertionError):
        hot_shares(z, p, False, True)  # an ordinary module is not hot
