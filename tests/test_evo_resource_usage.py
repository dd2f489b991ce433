"""CPU (cross-compile only): the fe_evo_* kernels of finenvs_amd/csrc/fe_evo.hip have no scratch memory and no VGPR spills
(tools/resource_usage.py).  The unit's whole kernel set and its committed table are tests/test_evo2_resource_usage.py's."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def table():
    import resource_usage

    from finenvs_amd.csrc import build as hip_build

    if not os.path.exists(hip_build.HIPCC):
        pytest.skip("hipcc not available")
    return resource_usage.kernel_table(source="fe_evo.hip")


def test_evo_kernels_use_no_scratch(table):
    import finenvs_amd.evo  # noqa: F401  (the Python side of these kernels)

    evo = [r for r in table if r["name"].startswith("fe_evo_")]
    # rollout: (single / multi asset) x (H = 32, 64); gradient: two passes; noise render
    assert len([r for r in evo if r["name"].startswith("fe_evo_rollout_kernel")]) == 4
    assert {r["name"] for r in evo if not r["name"].startswith("fe_evo_rollout_kernel")} == {
        "fe_evo_gradient_partial_kernel", "fe_evo_gradient_reduce_kernel", "fe_evo_noise_kernel"}
    bad = [(r["name"], r["scratch"], r["vgpr_spill"]) for r in evo if r["scratch"] != 0 or r["vgpr_spill"] != 0]
    assert not bad, f"scratch / VGPR spills in the ES kernels: {bad}"
    assert all(r["occupancy"] >= 2 for r in evo if r["name"].startswith("fe_evo_rollout_kernel"))  # __launch_bounds__(256, 2)
