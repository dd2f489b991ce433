"""CPU (cross-compile only): fe_ring_draw_kernel exists and has no scratch memory and no VGPR spills
(tools/resource_usage.py)."""
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


def test_ring_draw_kernel_uses_no_scratch(table):
    import finenvs_amd.replay  # noqa: F401  (the Python side of this kernel)

    rows = [r for r in table if r["name"].startswith("fe_ring_draw_kernel")]
    assert len(rows) == 1, [r["name"] for r in rows]  # one kernel for every A: no instantiations
    bad = [(r["name"], r["scratch"], r["vgpr_spill"]) for r in rows if r["scratch"] != 0 or r["vgpr_spill"] != 0]
    assert not bad, f"scratch / VGPR spills in the ring draw kernel: {bad}"
    # the draw is no replay-ring kernel by name: tests/test_replay_resource_usage.py counts those
    assert not [r["name"] for r in table if r["name"].startswith("fe_replay_") and "draw" in r["name"]]
