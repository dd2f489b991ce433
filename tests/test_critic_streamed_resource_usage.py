"""CPU (cross-compile only): the streamed twin-critic kernels of fe_critic_streamed_kernels.h -- the exact kernel list
(three H instantiations of each form of the recurrence, the d_actions kernel and the six-column final kernel), no scratch
and no VGPR spill outside the recurrence, the recurrence's scratch and occupancy against the forward it mirrors
(``fe_rollout_lstm_big_kernel<true, RTW>``), and every row as committed in profiles/critic_streamed_resource_usage.txt
(tools/resource_usage.py).  The kernels this feature launches but does not own are counted, not touched."""
import os
import sys

import pytest

from tests.test_lstm_grad_streamed_resource_usage import _committed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
PROFILE = "critic_streamed_resource_usage.txt"
SCRATCH_FREE = ("da", "final")
FORWARD = [f"fe_critic_sgrad_forward_kernel<{rtw}, {stash}>" for rtw in (4, 8, 16) for stash in ("false", "true")]
KERNELS = sorted([f"fe_critic_sgrad_{k}_kernel" for k in SCRATCH_FREE] + FORWARD)


@pytest.fixture(scope="module")
def table():
    import resource_usage

    from finenvs_amd.csrc import build as hip_build

    if not os.path.exists(hip_build.HIPCC):
        pytest.skip("hipcc not available")
    return {r["name"]: r for r in resource_usage.kernel_table()}


def test_the_streamed_critic_kernels_exist_and_the_shared_ones_are_undisturbed(table):
    assert sorted(n for n in table if n.startswith("fe_critic_sgrad_")) == KERNELS
    assert sorted(_committed(PROFILE)) == KERNELS
    # the kernels the new host code launches, and the register-resident critics, keep their instantiations
    assert len([n for n in table if n.startswith("fe_lstm_sgrad_")]) == 9
    assert len([n for n in table if n.startswith("fe_lstm_sgrad_forward_kernel<")]) == 3
    assert sorted(n for n in table if n.startswith("fe_twin_q_kernel")) == [f"fe_twin_q_kernel<{nt}>" for nt in (1, 2, 4)]
    assert len([n for n in table if n.startswith("fe_rollout_lstm_big_kernel<")]) == 6
    # ... and their committed rows
    committed = _committed("lstm_grad_streamed_resource_usage.txt")
    for name, row in committed.items():
        assert (table[name]["vgpr"], table[name]["scratch"], table[name]["occupancy"]) == \
            (row["vgpr"], row["scratch"], row["occupancy"]), (name, table[name], row)


@pytest.mark.parametrize("kernel", SCRATCH_FREE)
def test_d_actions_and_final_use_no_scratch(table, kernel):
    row = table[f"fe_critic_sgrad_{kernel}_kernel"]
    assert row["scratch"] == 0 and row["vgpr_spill"] == 0, row


@pytest.mark.parametrize("stash", ["false", "true"])
@pytest.mark.parametrize("rtw", [4, 8, 16])  # H = 256, 512, 1024
def test_the_recurrence_keeps_no_more_in_scratch_than_the_forward_it_mirrors(table, rtw, stash):
    row, forward = table[f"fe_critic_sgrad_forward_kernel<{rtw}, {stash}>"], table[f"fe_rollout_lstm_big_kernel<true, {rtw}>"]
    assert row["vgpr_spill"] == 0, row
    assert row["scratch"] <= forward["scratch"], (row, forward)
    assert row["occupancy"] >= forward["occupancy"], (row, forward)


@pytest.mark.parametrize("name", KERNELS)
def test_every_row_matches_the_committed_table(table, name):
    committed = _committed(PROFILE)
    assert table[name]["scratch"] == committed[name]["scratch"], (table[name], committed[name])
    assert table[name]["vgpr"] == committed[name]["vgpr"], (table[name], committed[name])
    assert table[name]["occupancy"] >= committed[name]["occupancy"], (table[name], committed[name])
