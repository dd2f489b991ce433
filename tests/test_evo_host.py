"""CPU: the ES update of finenvs_amd/evo.py against the reference's own outputs (tests/golden/evo_update.npz, written by
tools/make_evo_golden.py from the reference's EvoAgent / ParallelMLP), and the argument checks that need no device."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.helpers import load_golden


@pytest.fixture(scope="module")
def gold():
    return load_golden("evo_update.npz")


def _slots(gold):
    """The finished episodes of the fixture (reference order: by step, env order within a step) as the population keeps
    them: per env, in finishing order."""
    N = int(gold["meta"][0])
    dones, returns = gold["dones"], gold["returns"]
    M = int(np.bincount(dones, minlength=N).max())
    table = np.zeros((N, M), dtype=np.float32)
    counts = np.zeros(N, dtype=np.int32)
    for n, r in zip(dones, returns):
        table[n, counts[n]] = r
        counts[n] += 1
    return torch.from_numpy(table), torch.from_numpy(counts)


def test_final_ranks_equal_the_reference_exactly(gold):
    from finenvs_amd import evo

    table, counts = _slots(gold)
    got = evo.final_ranks(table, counts).numpy()
    assert got.dtype == np.float32
    assert got.tobytes() == gold["final_ranks"].tobytes()


def test_centered_ranks_match_the_reference_formula_and_break_ties_stably():
    from finenvs_amd import evo

    r = torch.tensor([3.0, -1.0, 3.0, 0.5, -1.0], dtype=torch.float32)
    got = evo.centered_ranks(r)
    # stable order: -1 (idx 1), -1 (idx 4), 0.5, 3 (idx 0), 3 (idx 2)
    want = torch.tensor([3, 0, 4, 2, 1], dtype=torch.float32) / 4 - 0.5
    assert torch.equal(got, want)


def test_adam_update_equals_the_reference(gold):
    from finenvs_amd import evo

    N, num_eval, W, H = (int(x) for x in gold["meta"])
    sigma, lr, l2 = (float(x) for x in gold["hyper"])
    table, counts = _slots(gold)
    ranks = evo.final_ranks(table, counts)
    diffed = evo.fitness(ranks, N - num_eval)
    assert diffed.shape == ((N - num_eval) // 2,)
    z = torch.from_numpy(gold["eps"]).double() / sigma
    zsum = (diffed.double().unsqueeze(1) * z).sum(dim=0)
    theta0 = torch.from_numpy(gold["theta0"])
    assert theta0.numel() == 5 * W * H + 2 * H + 1
    grad = evo.es_gradient(zsum, diffed.numel(), theta0, l2)
    m = torch.zeros_like(theta0)
    theta1, m1, v1 = evo.adam_step(theta0, grad, m, m.clone(), 1, lr)
    np.testing.assert_allclose(theta1.numpy(), gold["theta1"], rtol=1e-6, atol=1e-8)
    assert not np.array_equal(gold["theta1"], gold["theta0"])


def test_init_parameters_have_parallel_mlp_shapes_and_scales():
    from finenvs_amd import evo

    w, b = evo.init_parameters(80, 64, torch.Generator().manual_seed(0))
    assert [tuple(t.shape) for t in w] == [(80, 64), (64, 1)]
    assert [tuple(t.shape) for t in b] == [(1, 64), (1, 1)]
    assert abs(float(w[0].std()) - np.sqrt(2 / 80)) < 0.02


def test_evo_entry_points_reject_bad_arguments_without_a_gpu():
    from finenvs_amd import _lib

    lib = _lib.load()
    for name in _lib.EVO_SIGNATURES:
        assert hasattr(lib, name)
    assert not set(_lib.EVO_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES))
    pop = _lib.FeEvoPopulation()
    assert lib.fe_evo_rollout(None, C.byref(pop), 4, None, None, None, None, None) == _lib.FE_ERR_ARG
    assert b"bad argument" in lib.fe_last_error()
    assert lib.fe_evo_gradient(0, 0, 0, 10, None, None, None, None) == _lib.FE_ERR_ARG
    assert lib.fe_evo_noise(0, 0, None, 1, 10, None, None) == _lib.FE_ERR_ARG
    assert lib.fe_evo_gradient_workspace_doubles(100, 10) == 2 * 10
    assert lib.fe_evo_gradient_workspace_doubles(0, 10) == 0


def test_header_declares_exactly_the_evo_signatures():
    import os
    import re

    from finenvs_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "finenvs_amd_evo.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(fe_[a-z0-9_]+)\s*\(", text))) == sorted(_lib.EVO_SIGNATURES)
