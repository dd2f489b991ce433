"""CPU: the conditions the contract cases of tests/test_mlp_sac_contract_gpu.py rest on, checked without a GPU.

``contract_case`` builds the SAC MLP actor with the family's own builder (inside ``tests/helpers.py::modules_on_cpu``), shifts
and scales its ``std_layer`` and draws 97 crafted descriptors rendered from the oracle's log-return table (``cpu_states``).
Its conditions are decided here, from the f64 copy alone, so that a change to the builder, to the descriptor generator or
to the synthetic series cannot quietly empty the ranges the GPU cases are there for: q spans [-15, 100] with at least five
rows in each band of ``_sac_bands``, at most 3 rows within 1e-3 of softplus's threshold, at least 10 rows on either side
of ``|u| = 4``, between 5 and 96 actions at exactly +-1.0 in f32 torch, stds from below 4e-7 to above 99.
"""
import pytest
import torch

from tests import test_mlp_sac_contract_gpu as G
from tests import test_saturated_gpu as S


@pytest.mark.parametrize("H,activation", G.SHAPES)
def test_contract_case_meets_its_conditions_at_the_recorded_seed(H, activation):
    case = G.contract_case(H, activation)
    actor, states, noise = case["actor"], case["states"], case["noise"]
    assert all(p.device.type == "cpu" for p in actor.parameters())
    assert actor.hidden_size == H and actor.activation == activation and actor.sequence_length == G.W
    assert tuple(states.shape) == (G.COUNT, G.W, 5) and states.dtype is torch.float64
    assert case["seed"] == G.SEEDS[H], "the first module seed that meets the conditions has moved: record it in SEEDS"
    figures = G.conditions(actor, states, noise)  # asserts them
    assert figures == case["figures"]
    print(f"H = {H} {activation}: seed {case['seed']} {figures}")
    # the noise's prefix, and descriptors the env's check admits: multiples of 4 inside the table
    assert noise[:15, 0].tolist() == list(S.SPECIAL_NOISE) * 3
    D, L = G.cases.DAYS - 1, G.cases.bars(G.W) + G.W
    src = case["src"]
    assert bool((src % 4 == 0).all()) and int(src.min()) >= 0 and int(src.max()) // 4 + G.W <= D * L
    assert bool((case["pos"] != 0).all())


def test_both_first_layer_variants_and_two_activations_run():
    assert sorted(H for H, _ in G.SHAPES) == [32, 64, 128]
    assert {a for _, a in G.SHAPES} == {"elu", "tanh"} and dict(G.SHAPES)[64] == "tanh"
    assert G.COUNT == 97 and G.W == 4


def test_the_grid_reaches_the_edges_the_backward_guards():
    """``GRID_ACTIONS`` holds +-1.0 (om = 0: the guard alone keeps the quotient finite) and the two f32 neighbours below it;
    ``GRID_STDS`` goes down to 1e-6 (``gl / s`` of 1e6)."""
    acts = torch.tensor(S.GRID_ACTIONS, dtype=torch.float64).float()
    assert int((acts.abs() == 1.0).sum()) == 2
    assert float(acts.abs()[acts.abs() < 1].max()) == 1 - 2.0 ** -24
    assert min(S.GRID_STDS) == 1e-6 and max(S.GRID_STDS) == 25.0
    assert len(S.GRID_ACTIONS) * len(S.GRID_STDS) <= G.COUNT
