"""CPU (cross-compile only): registers and scratch of the library's fourth translation unit,
finenvs_amd/csrc/fe_evo.hip (include/finenvs_amd_evo.h, include/finenvs_amd_evo2.h).

* the unit holds exactly the four ``fe_evo_rollout_kernel<SINGLE, H>`` instantiations (one and many assets at H = 32 / 64),
  the six ``fe_evo2_rollout_kernel<SINGLE, H>`` instantiations (H = 32 / 64 / 128), the two gradient kernels, the noise
  kernel and, because ``fe_evo_kernels.h`` includes ``fe_rollout_kernels.h`` as the other small units do, that header's
  ``fe_policy_table_kernel`` (nobody launches it from this unit); every kernel once;
* no kernel uses scratch memory or spills a VGPR;
* every rollout instantiation, H = 128 included, is compiled for ``__launch_bounds__(256, 2)`` and reaches two waves per
  SIMD (what is resident at H = 128 is set by theta's LDS, not by registers);
* the table of this build is committed as profiles/evo_resource_usage.txt.
The other units' tables staying what they were is tests/test_resource_usage.py's, tests/test_mlp_critic_resource_usage.py's
and tests/test_mlp_sac_resource_usage.py's.
"""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
PROFILE = os.path.join(ROOT, "profiles", "evo_resource_usage.txt")
KERNELS = {"fe_evo_rollout_kernel": 4, "fe_evo2_rollout_kernel": 6, "fe_evo_gradient_partial_kernel": 1, "fe_evo_gradient_reduce_kernel": 1,
           "fe_evo_noise_kernel": 1, "fe_policy_table_kernel": 1}
COLUMNS = ("vgpr", "agpr", "sgpr", "scratch", "vgpr_spill", "sgpr_spill", "occupancy", "lds")


@pytest.fixture(scope="module")
def table():
    import resource_usage

    from finenvs_amd.csrc import build as hip_build

    if not os.path.exists(hip_build.HIPCC):
        pytest.skip("hipcc not available")
    return resource_usage.kernel_table(source="fe_evo.hip")


def test_the_unit_holds_these_kernels_and_none_uses_scratch_or_spills_a_vgpr(table):
    counts = {}
    for r in table:
        family = re.sub(r"<.*", "", r["name"])
        counts[family] = counts.get(family, 0) + 1
    assert counts == KERNELS
    rollouts = {r["name"] for r in table if r["name"].startswith("fe_evo2_rollout_kernel")}
    assert rollouts == {f"fe_evo2_rollout_kernel<{s}, {h}>" for s in ("true", "false") for h in (32, 64, 128)}
    one = {r["name"] for r in table if r["name"].startswith("fe_evo_rollout_kernel")}
    assert one == {f"fe_evo_rollout_kernel<{s}, {h}>" for s in ("true", "false") for h in (32, 64)}
    assert len({r["name"] for r in table}) == len(table) == sum(KERNELS.values())  # each kernel once
    bad = [(r["name"], r["scratch"], r["vgpr_spill"]) for r in table if r["scratch"] != 0 or r["vgpr_spill"] != 0]
    assert not bad, f"scratch / VGPR spills in the ES unit: {bad}"


def test_the_rollout_instantiations_keep_two_waves_per_simd(table):
    checked = 0
    for r in table:
        if r["name"].startswith(("fe_evo_rollout_kernel", "fe_evo2_rollout_kernel")):
            assert r["occupancy"] >= 2, (r["name"], r["occupancy"])
            checked += 1
    assert checked == 10


def test_committed_table_matches_this_build(table):
    committed = []
    for line in open(PROFILE).read().splitlines():
        if line.startswith("fe_"):
            committed.append((line[:58].strip(),) + tuple(int(c) for c in line[58:].split()))
    mine = [(r["name"][:58].strip(),) + tuple(r[c] for c in COLUMNS) for r in table]
    assert sorted(committed) == sorted(mine), "regenerate profiles/evo_resource_usage.txt (tools/resource_usage.py " \
                                              "--source fe_evo.hip --out ...)"
