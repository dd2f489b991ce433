"""CPU (cross-compile only): registers and scratch of the library's fifth translation unit,
finenvs_amd/csrc/fe_evo_streamed.hip (include/finenvs_amd_evo2_streamed.h).

* the unit holds exactly the eight ``fe_evo2_streamed_rollout_kernel<SINGLE, H>`` instantiations (one and many assets at
  H = 32 / 64 / 128 / 256) and, re-emitted from the headers it includes as in the other small units, the two gradient
  kernels, the noise kernel and ``fe_policy_table_kernel`` (nobody launches them from this unit); every kernel once;
* none of the eight uses scratch memory or spills a VGPR, and each reaches two waves per SIMD: with theta out of the LDS,
  what is resident is set by these registers;
* the table of this build is committed as profiles/evo_streamed_resource_usage.txt.
fe_evo.hip's own table staying what it was is tests/test_evo2_resource_usage.py's.
"""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
PROFILE = os.path.join(ROOT, "profiles", "evo_streamed_resource_usage.txt")
KERNELS = {"fe_evo2_streamed_rollout_kernel": 8, "fe_evo_gradient_partial_kernel": 1, "fe_evo_gradient_reduce_kernel": 1,
           "fe_evo_noise_kernel": 1, "fe_policy_table_kernel": 1}
COLUMNS = ("vgpr", "agpr", "sgpr", "scratch", "vgpr_spill", "sgpr_spill", "occupancy", "lds")


@pytest.fixture(scope="module")
def table():
    import resource_usage

    from finenvs_amd.csrc import build as hip_build

    if not os.path.exists(hip_build.HIPCC):
        pytest.skip("hipcc not available")
    return resource_usage.kernel_table(source="fe_evo_streamed.hip")


def test_the_unit_holds_the_eight_streamed_instantiations(table):
    counts = {}
    for r in table:
        family = re.sub(r"<.*", "", r["name"])
        counts[family] = counts.get(family, 0) + 1
    assert counts == KERNELS
    streamed = {r["name"] for r in table if r["name"].startswith("fe_evo2_streamed_rollout_kernel")}
    assert streamed == {f"fe_evo2_streamed_rollout_kernel<{s}, {h}>" for s in ("true", "false") for h in (32, 64, 128, 256)}
    assert len({r["name"] for r in table}) == len(table) == sum(KERNELS.values())  # each kernel once


def test_no_scratch_no_vgpr_spill_and_two_waves_per_simd(table):
    checked = 0
    for r in table:
        if r["name"].startswith("fe_evo2_streamed_rollout_kernel"):
            assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (r["name"], r["scratch"], r["vgpr_spill"])
            assert r["occupancy"] >= 2, (r["name"], r["occupancy"])
            assert r["lds"] == 0, (r["name"], r["lds"])  # the LDS is the launch's (fe_evo2_streamed_lds_bytes), none static
            checked += 1
    assert checked == 8
    bad = [(r["name"], r["scratch"], r["vgpr_spill"]) for r in table if r["scratch"] != 0 or r["vgpr_spill"] != 0]
    assert not bad, f"scratch / VGPR spills in the streamed ES unit: {bad}"


def test_committed_table_matches_this_build(table):
    committed = []
    for line in open(PROFILE).read().splitlines():
        if line.startswith("fe_"):
            committed.append((line[:58].strip(),) + tuple(int(c) for c in line[58:].split()))
    mine = [(r["name"][:58].strip(),) + tuple(r[c] for c in COLUMNS) for r in table]
    assert sorted(committed) == sorted(mine), "regenerate profiles/evo_streamed_resource_usage.txt (tools/resource_usage.py " \
                                              "--source fe_evo_streamed.hip --out ...)"
