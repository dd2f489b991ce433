"""CPU (cross-compile only): the streamed SAC actor kernels of fe_sac_streamed_kernels.h -- the exact kernel list (six
instantiations of the acting kernel, the six stages of the backward's head), no scratch and no VGPR spill outside the
recurrence, the acting kernel's spills, scratch and occupancy against the kernel whose body it shares
(``fe_rollout_lstm_big_kernel<SINGLE, RTW>``), and every row as committed in profiles/sac_streamed_resource_usage.txt
(tools/resource_usage.py).  The kernels this feature launches but does not own are counted, not touched."""
import os
import sys

import pytest

from tests.test_lstm_grad_streamed_resource_usage import _committed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
PROFILE = "sac_streamed_resource_usage.txt"
SCRATCH_FREE = ("pack", "z", "head", "dh", "wl", "final")
ROLLOUT = [f"fe_rollout_sac_big_kernel<{single}, {rtw}>" for single in ("false", "true") for rtw in (4, 8, 16)]
KERNELS = sorted([f"fe_sac_sgrad_{k}_kernel" for k in SCRATCH_FREE] + ROLLOUT)


@pytest.fixture(scope="module")
def table():
    import resource_usage

    from finenvs_amd.csrc import build as hip_build

    if not os.path.exists(hip_build.HIPCC):
        pytest.skip("hipcc not available")
    return {r["name"]: r for r in resource_usage.kernel_table()}


def test_the_streamed_sac_kernels_exist_and_the_shared_ones_are_undisturbed(table):
    assert sorted(n for n in table if n.startswith("fe_sac_sgrad_") or n.startswith("fe_rollout_sac_big_kernel<")) == KERNELS
    assert sorted(_committed(PROFILE)) == KERNELS
    # the kernels the new host code launches, and the families other tests count, keep their instantiations
    assert len([n for n in table if n.startswith("fe_lstm_sgrad_")]) == 9
    assert len([n for n in table if n.startswith("fe_critic_sgrad_")]) == 8
    assert len([n for n in table if n.startswith("fe_rollout_lstm_big_kernel<")]) == 6
    assert len([n for n in table if n.startswith("fe_rollout_sac_kernel")]) == 6
    assert len([n for n in table if n.startswith("fe_sac_grad_kernel")]) == 3
    # ... and their committed rows
    for profile in ("lstm_grad_streamed_resource_usage.txt", "critic_streamed_resource_usage.txt"):
        for name, row in _committed(profile).items():
            assert (table[name]["vgpr"], table[name]["scratch"], table[name]["occupancy"]) == \
                (row["vgpr"], row["scratch"], row["occupancy"]), (name, table[name], row)


@pytest.mark.parametrize("kernel", SCRATCH_FREE)
def test_everything_but_the_recurrence_uses_no_scratch(table, kernel):
    row = table[f"fe_sac_sgrad_{kernel}_kernel"]
    assert row["scratch"] == 0 and row["vgpr_spill"] == 0, row


@pytest.mark.parametrize("single", ["false", "true"])
@pytest.mark.parametrize("rtw", [4, 8, 16])  # H = 256, 512, 1024
def test_the_acting_kernel_keeps_no_more_in_scratch_than_the_kernel_whose_body_it_shares(table, rtw, single):
    row, lstm = table[f"fe_rollout_sac_big_kernel<{single}, {rtw}>"], table[f"fe_rollout_lstm_big_kernel<{single}, {rtw}>"]
    assert row["vgpr_spill"] == 0, row
    assert row["scratch"] <= lstm["scratch"], (row, lstm)
    assert row["occupancy"] >= lstm["occupancy"], (row, lstm)


@pytest.mark.parametrize("name", KERNELS)
def test_every_row_matches_the_committed_table(table, name):
    committed = _committed(PROFILE)
    assert table[name]["scratch"] == committed[name]["scratch"], (table[name], committed[name])
    assert table[name]["vgpr"] == committed[name]["vgpr"], (table[name], committed[name])
    assert table[name]["occupancy"] >= committed[name]["occupancy"], (table[name], committed[name])
