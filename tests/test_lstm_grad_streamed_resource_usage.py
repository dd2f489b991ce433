"""CPU (cross-compile only): the streamed LSTM head gradient kernels of fe_lstm_grad_streamed_kernels.h -- three H
instantiations of the recompute kernel, scratch-free elementwise / transpose / head / contraction / final kernels, and
every kernel's scratch and occupancy as committed in profiles/lstm_grad_streamed_resource_usage.txt
(tools/resource_usage.py).  The recompute kernel keeps c_t and the pending h_t in per-lane scratch as
fe_rollout_lstm_big_kernel does, and no more than it."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
SCRATCH_FREE = ("dz", "pack", "head", "dh", "wgrad", "final")
KERNELS = sorted([f"fe_lstm_sgrad_{k}_kernel" for k in SCRATCH_FREE]
                 + [f"fe_lstm_sgrad_forward_kernel<{rtw}>" for rtw in (4, 8, 16)])


@pytest.fixture(scope="module")
def table():
    import resource_usage

    from finenvs_amd.csrc import build as hip_build

    if not os.path.exists(hip_build.HIPCC):
        pytest.skip("hipcc not available")
    return {r["name"]: r for r in resource_usage.kernel_table()}


def _committed(name):
    rows = {}
    for line in open(os.path.join(ROOT, "profiles", name)):
        if line.startswith("#") or line.startswith("kernel"):
            continue
        m = re.match(r"(\S+(?:<[^>]*>)?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)", line.strip())
        if m:
            rows[m.group(1)] = {"vgpr": int(m.group(2)), "scratch": int(m.group(5)), "occupancy": int(m.group(8))}
    return rows


def test_the_streamed_gradient_kernels_exist(table):
    assert sorted(n for n in table if n.startswith("fe_lstm_sgrad_")) == KERNELS
    assert sorted(_committed("lstm_grad_streamed_resource_usage.txt")) == KERNELS
    # the count of the register-resident backward's instantiations is not disturbed
    assert len([n for n in table if n.startswith("fe_lstm_grad_kernel")]) == 3


@pytest.mark.parametrize("kernel", SCRATCH_FREE)
def test_everything_but_the_recurrence_uses_no_scratch(table, kernel):
    row = table[f"fe_lstm_sgrad_{kernel}_kernel"]
    assert row["scratch"] == 0 and row["vgpr_spill"] == 0, row


@pytest.mark.parametrize("rtw", [4, 8, 16])  # H = 256, 512, 1024
def test_the_recurrence_keeps_no_more_in_scratch_than_the_forward_it_mirrors(table, rtw):
    row, forward = table[f"fe_lstm_sgrad_forward_kernel<{rtw}>"], table[f"fe_rollout_lstm_big_kernel<true, {rtw}>"]
    assert row["vgpr_spill"] == 0, row
    assert row["scratch"] <= forward["scratch"], (row, forward)
    assert row["occupancy"] >= forward["occupancy"], (row, forward)


@pytest.mark.parametrize("name", KERNELS)
def test_scratch_and_occupancy_match_the_committed_table(table, name):
    committed = _committed("lstm_grad_streamed_resource_usage.txt")
    assert table[name]["scratch"] == committed[name]["scratch"], (table[name], committed[name])
    assert table[name]["occupancy"] >= committed[name]["occupancy"], (table[name], committed[name])
