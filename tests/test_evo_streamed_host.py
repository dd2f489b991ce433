"""CPU: the host side of the streamed two-hidden-layer ES population (include/finenvs_amd_evo2_streamed.h,
finenvs_amd/csrc/fe_evo_streamed.hip, ``FusedPopulationMLP2Rollout(..., streamed=True)``): the two size functions, the
refusal of the entry without a GPU, the build lists, and the reference's default shape (hidden_dims = (256, 256),
finenvs/agents/ES/evo_agent.py:17) in ``evo_layout`` / ``init_parameters``.
"""
import ctypes as C
import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (32, 64, 128, 256)


def test_num_params_is_the_formula_at_the_four_widths():
    from finenvs_amd import _lib, evo

    lib = _lib.load()
    for H in WIDTHS:
        for W in (1, 3, 8, 16, 64, 300):
            P = 5 * W * H + H * H + 3 * H + 1
            assert lib.fe_evo2_streamed_num_params(W, H) == P
            assert evo.FusedPopulationMLP2Rollout._count_params(5 * W, H) == P
    for H in (48, 512, 0, -32, 16):
        assert lib.fe_evo2_streamed_num_params(8, H) == -1
    assert lib.fe_evo2_streamed_num_params(0, 256) == -1 and lib.fe_evo2_streamed_num_params(-1, 32) == -1
    # the resident entry's functions are what they were
    assert lib.fe_evo2_num_params(8, 256) == -1 and lib.fe_evo2_lds_bytes(8, 1, 256) == -1
    assert evo.FusedPopulationMLP2Rollout.HIDDEN == (32, 64, 128)
    assert evo.FusedPopulationMLP2Rollout.STREAMED_HIDDEN == WIDTHS


def test_lds_bytes_hold_no_theta_and_do_not_grow_with_the_window():
    from finenvs_amd import _lib

    lib = _lib.load()
    for H in WIDTHS:
        for A in (1, 3, 17, 100, 128):
            b = lib.fe_evo2_streamed_lds_bytes(1, A, H)
            assert all(lib.fe_evo2_streamed_lds_bytes(W, A, H) == b for W in (2, 8, 36, 64, 1000))
            xchg = 4 * 2 * H * 4  # four wavefronts, members A and B, H floats each
            assert b % 16 == 0 and xchg < b <= xchg + 16 * 1024
            if H < 256:  # the resident launch is this one plus theta, up to theta's alignment
                P = lib.fe_evo2_num_params(8, H)
                assert 0 <= lib.fe_evo2_lds_bytes(8, A, H) - b - 4 * P < 16
    assert lib.fe_evo2_streamed_lds_bytes(8, 1, 256) <= 9 * 1024  # "8 KiB at H = 256": the exchange buffer and one tile
    for W, A, H in ((8, 1, 48), (8, 1, 512), (0, 1, 256), (8, 0, 256), (8, 129, 256), (8, 129, 32)):
        assert lib.fe_evo2_streamed_lds_bytes(W, A, H) == -1


def test_entry_rejects_bad_arguments_without_a_gpu_and_the_header_declares_the_three():
    from finenvs_amd import _lib

    lib = _lib.load()
    assert sorted(_lib.EVO2_STREAMED_SIGNATURES) == ["fe_evo2_rollout_streamed", "fe_evo2_streamed_lds_bytes",
                                                     "fe_evo2_streamed_num_params"]
    for name in _lib.EVO2_STREAMED_SIGNATURES:
        assert hasattr(lib, name)
    pop = _lib.FeEvoPopulation()
    assert lib.fe_evo2_rollout_streamed(None, C.byref(pop), 4, None, None, None, None, None) == _lib.FE_ERR_ARG
    assert b"fe_evo2_rollout_streamed: bad argument" in lib.fe_last_error()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "finenvs_amd_evo2_streamed.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(fe_[a-z0-9_]+)\s*\(", text))) == sorted(_lib.EVO2_STREAMED_SIGNATURES)


def test_build_lists_name_the_new_files():
    from finenvs_amd.csrc import build

    assert "fe_evo_streamed.hip" in build.SOURCES and "fe_evo.hip" in build.SOURCES
    assert "fe_evo_host.h" in build.HEADERS and "fe_evo_kernels.h" in build.HEADERS
    for name in build.SOURCES + build.HEADERS:
        assert os.path.exists(os.path.join(build.HERE, name)), name
    assert "finenvs_amd_evo2_streamed.h" in open(os.path.join(build.HERE, "build.py")).read()  # a dependency of the library
    assert os.path.exists(os.path.join(ROOT, "include", "finenvs_amd_evo2_streamed.h"))


def test_the_reference_default_shape_in_layout_and_initialisation():
    """EvoAgent's default ParallelMLP: shape (5W, 256, 256, 1), weights (in, out), biases (1, out), ~ N(0, sqrt(2 / in))."""
    from finenvs_amd import evo

    W, H = 16, 256
    O = 5 * W
    P = O * H + H * H + 3 * H + 1
    lay = evo.evo_layout(O, H, 2)
    assert list(lay) == ["W1", "b1", "W2", "b2", "W3", "b3"]
    assert [lay[k][1] for k in lay] == [(O, H), (1, H), (H, H), (1, H), (H, 1), (1, 1)]
    assert [lay[k][0] for k in lay] == [0, O * H, O * H + H, O * H + H + H * H, O * H + 2 * H + H * H, P - 1]
    assert all(off % 4 == 0 for off, _ in lay.values())
    w, b = evo.init_parameters(O, H, torch.Generator().manual_seed(7), hidden_layers=2)
    assert [tuple(t.shape) for t in w] == [(O, H), (H, H), (H, 1)] and [tuple(t.shape) for t in b] == [(1, H), (1, H), (1, 1)]
    g = torch.Generator().manual_seed(7)
    for i, (fan_in, fan_out) in enumerate(((O, H), (H, H), (H, 1))):
        std = float(np.sqrt(2 / fan_in))
        assert torch.equal(w[i], torch.normal(0.0, std, (fan_in, fan_out), generator=g))
        assert torch.equal(b[i], torch.normal(0.0, std, (1, fan_out), generator=g))
    theta = evo.evo_flatten(w, b, O, H, 2)
    assert theta.numel() == P == 86785
    vw, vb = evo.evo_views(theta, O, H, 2)
    for got, want in zip(vw + vb, w + b):
        assert torch.equal(got, want)
