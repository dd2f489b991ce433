"""CPU (cross-compile only): the LSTM head gradient kernels of fe_lstm_grad_kernels.h -- three H instantiations of the
backward kernel, a scratch-free transpose and reduction, and the backward kernel's scratch and occupancy as committed in
profiles/lstm_grad_resource_usage.txt (tools/resource_usage.py); its occupancy is at least the SAC actor backward's at
the same H, whose superset of work it does with more LDS."""
import os
import re
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


def _committed(name):
    rows = {}
    for line in open(os.path.join(ROOT, "profiles", name)):
        if line.startswith("#") or line.startswith("kernel"):
            continue
        m = re.match(r"(\S+(?:<[^>]*>)?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)", line.strip())
        if m:
            rows[m.group(1)] = {"vgpr": int(m.group(2)), "scratch": int(m.group(5)), "occupancy": int(m.group(8))}
    return rows


def test_three_backward_instantiations(table):
    assert sorted(n for n in table if n.startswith("fe_lstm_grad_kernel")) == [f"fe_lstm_grad_kernel<{nt}>" for nt in (1, 2, 4)]


def test_the_reduction_and_the_transpose_use_no_scratch(table):
    assert table["fe_lstm_grad_reduce_kernel"]["scratch"] == 0
    assert table["fe_lstm_grad_pack_kernel"]["scratch"] == 0


@pytest.mark.parametrize("nt", [1, 2, 4])  # H = 32, 64, 128
def test_backward_scratch_and_occupancy_match_the_committed_table(table, nt):
    name = f"fe_lstm_grad_kernel<{nt}>"
    committed = _committed("lstm_grad_resource_usage.txt")
    assert name in committed, sorted(committed)
    assert committed[name]["scratch"] == 0
    assert table[name]["scratch"] == committed[name]["scratch"], (table[name], committed[name])
    assert table[name]["occupancy"] >= committed[name]["occupancy"], (table[name], committed[name])
    # at least the SAC actor backward's waves per SIMD at the same H (2 / 2 / 1)
    sac = _committed("sac_grad_resource_usage.txt")[f"fe_sac_grad_kernel<{nt}>"]
    assert sac["occupancy"] == {1: 2, 2: 2, 4: 1}[nt]
    assert committed[name]["occupancy"] >= sac["occupancy"] and table[name]["occupancy"] >= sac["occupancy"]
