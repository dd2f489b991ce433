"""CPU: the two-hidden-layer ES population's host side (finenvs_amd/evo.py, include/finenvs_amd_evo2.h) against the
reference's own outputs (tests/golden/evo2_update.npz, written by tools/make_evo2_golden.py from the reference's EvoAgent /
ParallelMLP with hidden_dims = (32, 32)), and the pieces that need no device.

``_forward2`` is the plain torch restatement of the per-env three-layer forward that tests/test_evo2_rollout_gpu.py holds
the kernel to.  On the fixture it reproduces ParallelMLP.forward to ``FORWARD_BOUND``: measured here, 24 members x 1 action,
the largest difference was 8.94e-08 (1.5 ulp of an output in [0.5, 1): the negative members' weights are rebuilt as
``theta - eps`` from the perturbation the update sees, which can differ from the reference's own by an ulp, and the batched
product may sum in another order).  The bound is two of those ulps rounded up.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests.helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORWARD_BOUND = 2e-7  # see the module docstring; well under 1e-6, where a wrong weight would start to hide


@pytest.fixture(scope="module")
def gold():
    return load_golden("evo2_update.npz")


def _forward2(w, obs, W, H):
    """Every env's own network on every asset: ``w`` (N, P) member weights in the layout of include/finenvs_amd_evo2.h,
    ``obs`` (N, W, 5A); returns (N, A) in ``w``'s dtype: tanh(tanh(tanh(x W1 + b1) W2 + b2) W3 + b3)."""
    N, O = w.shape[0], 5 * W
    A = obs.shape[2] // 5
    o = 0
    parts = []
    for rows, cols in ((O, H), (1, H), (H, H), (1, H), (H, 1), (1, 1)):
        parts.append(w[:, o:o + rows * cols].reshape(N, rows, cols))
        o += rows * cols
    assert o == w.shape[1]
    W1, b1, W2, b2, W3, b3 = parts
    x = torch.as_tensor(obs, device=w.device).to(w.dtype)
    out = []
    for a in range(A):
        xa = x[:, :, 5 * a:5 * a + 5].reshape(N, 1, O)
        h1 = torch.tanh(torch.bmm(xa, W1) + b1)
        h2 = torch.tanh(torch.bmm(h1, W2) + b2)
        out.append(torch.tanh(torch.bmm(h2, W3) + b3).reshape(N))
    return torch.stack(out, 1)


def _slots(gold):
    N = int(gold["meta"][0])
    dones, returns = gold["dones"], gold["returns"]
    M = int(np.bincount(dones, minlength=N).max())
    table = np.zeros((N, M), dtype=np.float32)
    counts = np.zeros(N, dtype=np.int32)
    for n, r in zip(dones, returns):
        table[n, counts[n]] = r
        counts[n] += 1
    return torch.from_numpy(table), torch.from_numpy(counts)


def test_flat_layout_offsets_and_parameter_count():
    from finenvs_amd import _lib, evo

    lib = _lib.load()
    for W, H in ((1, 32), (3, 64), (8, 128), (16, 64), (4, 32)):
        lay = evo.evo2_layout(5 * W, H)
        assert list(lay) == ["W1", "b1", "W2", "b2", "W3", "b3"]  # the reference's layer order
        O = 5 * W
        assert [lay[k][0] for k in lay] == [0, O * H, O * H + H, O * H + H + H * H, O * H + 2 * H + H * H, O * H + 3 * H + H * H]
        assert all(off % 4 == 0 for off, _ in lay.values())
        assert [lay[k][1] for k in lay] == [(O, H), (1, H), (H, H), (1, H), (H, 1), (1, 1)]
        P = 5 * W * H + H * H + 3 * H + 1
        assert evo.FusedPopulationMLP2Rollout._count_params(O, H) == P == lib.fe_evo2_num_params(W, H)
    assert lib.fe_evo2_num_params(8, 256) == -1 and lib.fe_evo2_num_params(0, 32) == -1
    assert evo.FusedPopulationMLP2Rollout.HIDDEN == (32, 64, 128)
    # the one-layer class is what it was
    assert evo.FusedPopulationMLPRollout.HIDDEN == (32, 64)
    assert evo.FusedPopulationMLPRollout._count_params(40, 64) == 40 * 64 + 2 * 64 + 1


def test_lds_rule_counts_theta_and_the_exchange_buffer():
    from finenvs_amd import _lib

    lib = _lib.load()
    for H in (32, 64, 128):
        for A in (1, 3, 17, 100, 128):
            b0, b1 = lib.fe_evo2_lds_bytes(8, A, H), lib.fe_evo2_lds_bytes(9, A, H)
            assert b1 - b0 == 5 * H * 4  # one more window row: five rows of W1
            P = lib.fe_evo2_num_params(8, H)
            assert b0 >= 4 * P + 4 * 2 * H * 4  # theta, and 2H floats per wavefront for the middle layer's exchange
            assert b0 % 16 == 0
    assert lib.fe_evo2_lds_bytes(8, 1, 128) > 64 * 1024  # the big-LDS launch even at W = 8
    assert lib.fe_evo2_lds_bytes(8, 129, 32) == -1 and lib.fe_evo2_lds_bytes(8, 0, 32) == -1
    assert lib.fe_evo2_lds_bytes(8, 1, 256) == -1 and lib.fe_evo2_lds_bytes(0, 1, 32) == -1


def test_flatten_refuses_wrong_shapes_and_non_finite_entries_and_views_round_trip():
    from finenvs_amd import evo

    O, H = 15, 32
    g = torch.Generator().manual_seed(0)
    w, b = evo.init_parameters(O, H, g, hidden_layers=2)
    theta = evo.evo2_flatten(w, b, O, H)
    assert theta.dtype == torch.float32 and theta.numel() == O * H + H * H + 3 * H + 1
    vw, vb = evo.evo2_views(theta, O, H)
    for got, want in zip(vw + vb, w + b):
        assert torch.equal(got, want)
    assert vw[1].data_ptr() == theta.data_ptr() + 4 * (O * H + H)  # views, not copies
    with pytest.raises(ValueError, match="three weight"):
        evo.evo2_flatten(w[:2], b[:2], O, H)
    for i, bad in ((0, torch.zeros(O, H + 1)), (1, torch.zeros(H, 1)), (2, torch.zeros(H, 2))):
        ww = list(w)
        ww[i] = bad
        with pytest.raises(ValueError, match="expected"):
            evo.evo2_flatten(ww, b, O, H)
    bb = list(b)
    bb[1] = torch.zeros(H)
    with pytest.raises(ValueError, match="expected"):
        evo.evo2_flatten(w, bb, O, H)
    for value in (float("nan"), float("inf")):
        ww = [t.clone() for t in w]
        ww[1][3, 5] = value
        with pytest.raises(ValueError, match="non-finite"):
            evo.evo2_flatten(ww, b, O, H)


def test_init_parameters_two_layers_equal_a_restated_draw():
    from finenvs_amd import evo

    O, H = 80, 64
    w, b = evo.init_parameters(O, H, torch.Generator().manual_seed(5), hidden_layers=2)
    g = torch.Generator().manual_seed(5)
    for i, (fan_in, fan_out) in enumerate(((O, H), (H, H), (H, 1))):  # W1, b1, W2, b2, W3, b3
        std = float(np.sqrt(2 / fan_in))
        assert torch.equal(w[i], torch.normal(0.0, std, (fan_in, fan_out), generator=g))
        assert torch.equal(b[i], torch.normal(0.0, std, (1, fan_out), generator=g))
    assert len(w) == len(b) == 3
    # the one-layer form is what it was, with and without the new argument
    w1, b1 = evo.init_parameters(O, H, torch.Generator().manual_seed(5))
    w1k, _ = evo.init_parameters(O, H, torch.Generator().manual_seed(5), hidden_layers=1)
    assert [tuple(t.shape) for t in w1] == [(O, H), (H, 1)] and torch.equal(w1[0], w[0]) and torch.equal(w1[1], w1k[1])
    with pytest.raises(ValueError):
        evo.init_parameters(O, H, g, hidden_layers=3)


def test_forward2_reproduces_the_reference_forward(gold):
    N, num_eval, W, H = (int(x) for x in gold["meta"])
    half = (N - num_eval) // 2
    theta0, eps = torch.from_numpy(gold["theta0"]), torch.from_numpy(gold["eps"])
    assert theta0.numel() == 5 * W * H + H * H + 3 * H + 1 and eps.shape == (half, theta0.numel())
    w = theta0.unsqueeze(0).repeat(N, 1)
    w[:half] += eps
    w[half:2 * half] -= eps
    obs = torch.from_numpy(gold["obs"]).reshape(N, W, 5)
    got = _forward2(w, obs, W, H).numpy()
    want = gold["actions"]
    assert got.shape == want.shape == (N, 1) and got.dtype == np.float32
    worst = float(np.abs(got.astype(np.float64) - want).max())
    print(f"worst |_forward2 - ParallelMLP.forward| {worst:.3g}")
    assert worst <= FORWARD_BOUND
    assert np.array_equal(got[2 * half:], _forward2(theta0.unsqueeze(0).repeat(N, 1), obs, W, H).numpy()[2 * half:])
    assert float(np.abs(want[:half] - want[half:2 * half]).max()) > 1e-3  # the members differ
    assert float(np.abs(want).max()) < 0.999  # not saturated: an error in a weight would show


def test_final_ranks_and_adam_update_equal_the_reference(gold):
    from finenvs_amd import evo

    N, num_eval, W, H = (int(x) for x in gold["meta"])
    sigma, lr, l2 = (float(x) for x in gold["hyper"])
    table, counts = _slots(gold)
    ranks = evo.final_ranks(table, counts)
    assert ranks.numpy().tobytes() == gold["final_ranks"].tobytes()
    diffed = evo.fitness(ranks, N - num_eval)
    z = torch.from_numpy(gold["eps"]).double() / sigma
    zsum = (diffed.double().unsqueeze(1) * z).sum(dim=0)
    theta0 = torch.from_numpy(gold["theta0"])
    grad = evo.es_gradient(zsum, diffed.numel(), theta0, l2)
    m = torch.zeros_like(theta0)
    theta1, _, _ = evo.adam_step(theta0, grad, m, m.clone(), 1, lr)
    np.testing.assert_allclose(theta1.numpy(), gold["theta1"], rtol=1e-6, atol=1e-8)
    assert not np.array_equal(gold["theta1"], gold["theta0"])


def test_fixture_is_small_and_holds_arrays_only():
    path = os.path.join(ROOT, "tests", "golden", "evo2_update.npz")
    assert os.path.getsize(path) < 100_000
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == sorted(["theta0", "eps", "obs", "actions", "dones", "returns", "final_ranks", "theta1",
                                          "meta", "hyper"])


def test_entry_points_reject_bad_arguments_without_a_gpu_and_the_header_declares_them():
    from finenvs_amd import _lib

    lib = _lib.load()
    for name in _lib.EVO2_SIGNATURES:
        assert hasattr(lib, name)
    pop = _lib.FeEvoPopulation()
    assert lib.fe_evo2_rollout(None, C.byref(pop), 4, None, None, None, None, None) == _lib.FE_ERR_ARG
    assert b"fe_evo2_rollout: bad argument" in lib.fe_last_error()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "finenvs_amd_evo2.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(fe_[a-z0-9_]+)\s*\(", text))) == sorted(_lib.EVO2_SIGNATURES)
    from finenvs_amd.csrc import build

    assert "fe_evo.hip" in build.SOURCES and "fe_evo_kernels.h" in build.HEADERS
