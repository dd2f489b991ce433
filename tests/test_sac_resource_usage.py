"""CPU (cross-compile only): the SAC head's kernels keep the occupancy of the LSTM kernels they extend and use no more
scratch (tools/resource_usage.py; the table is profiles/sac_resource_usage.txt)."""
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
    return {r["name"]: r for r in resource_usage.kernel_table()}


@pytest.mark.parametrize("single", ["true", "false"])
@pytest.mark.parametrize("nt", [1, 2, 4])  # H = 32, 64, 128
def test_sac_kernel_keeps_the_lstm_kernels_occupancy_and_scratch(table, single, nt):
    sac = table[f"fe_rollout_sac_kernel<{single}, {nt}>"]
    lstm = table[f"fe_rollout_lstm_kernel<{single}, {nt}>"]
    assert sac["occupancy"] >= lstm["occupancy"], (sac, lstm)
    assert sac["scratch"] <= lstm["scratch"], (sac, lstm)


def test_no_sac_kernel_for_the_streamed_sizes(table):
    assert len([n for n in table if n.startswith("fe_rollout_sac_kernel")]) == 6
