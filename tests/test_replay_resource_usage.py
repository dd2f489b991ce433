"""CPU (cross-compile only): the fe_replay_* kernels have no scratch memory and no VGPR spills (tools/resource_usage.py)."""
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
    return resource_usage.kernel_table()


def test_replay_kernels_use_no_scratch(table):
    import finenvs_amd.replay  # noqa: F401  (the Python side of these kernels)

    rows = [r for r in table if r["name"].startswith("fe_replay_")]
    # append: (single / multi asset) x (f32 / f64 actions); sample: (16-, 8-, 4-byte stores) x (single / multi asset)
    assert len([r for r in rows if r["name"].startswith("fe_replay_append_kernel<")]) == 4
    assert len([r for r in rows if r["name"].startswith("fe_replay_sample_kernel<")]) == 6
    assert len(rows) == 10
    bad = [(r["name"], r["scratch"], r["vgpr_spill"]) for r in rows if r["scratch"] != 0 or r["vgpr_spill"] != 0]
    assert not bad, f"scratch / VGPR spills in the replay kernels: {bad}"
