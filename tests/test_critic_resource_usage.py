"""CPU (cross-compile only): the twin critic's kernels keep the occupancy of the LSTM kernel whose recurrence they share
and use no more scratch; the target epilogue uses none (tools/resource_usage.py; the table is
profiles/critic_resource_usage.txt)."""
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


@pytest.mark.parametrize("nt", [1, 2, 4])  # H = 32, 64, 128
def test_twin_q_kernel_keeps_the_lstm_kernels_occupancy_and_scratch(table, nt):
    q = table[f"fe_twin_q_kernel<{nt}>"]
    lstm = table[f"fe_rollout_lstm_kernel<true, {nt}>"]
    assert q["occupancy"] >= lstm["occupancy"], (q, lstm)
    assert q["scratch"] <= lstm["scratch"], (q, lstm)


def test_three_critic_instantiations_and_a_scratch_free_epilogue(table):
    assert sorted(n for n in table if n.startswith("fe_twin_q_kernel")) == [f"fe_twin_q_kernel<{nt}>" for nt in (1, 2, 4)]
    assert table["fe_twin_q_target_kernel"]["scratch"] == 0
