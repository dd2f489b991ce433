"""CPU (cross-compile only): registers and scratch of the library's second translation unit,
finenvs_amd/csrc/fe_mlp_critic.hip (include/finenvs_amd_mlp_critic.h).

* every kernel of the unit -- the ``fe_mlpq_*`` kernels, the ``fe_mlp2_wgrad2_kernel`` instantiations it launches and the
  four non-template kernels the MLP headers emit a second time -- uses no scratch memory and spills no VGPR;
* the H = 32 / 64 instantiations reach at least two waves per SIMD.  No floor is asked of H = 128, as for the two-layer
  head: 66 KiB of LDS for W2 alone leave one workgroup per CU;
* the table of this build is committed as profiles/mlp_critic_resource_usage.txt.
fe_env.hip's own table staying what it was is tests/test_mlp2_head_resource_usage.py's and tests/test_resource_usage.py's.
"""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
PROFILE = os.path.join(ROOT, "profiles", "mlp_critic_resource_usage.txt")
# family: instantiations
KERNELS = {"fe_mlpq_forward_kernel": 3, "fe_mlpq_grad_kernel": 3, "fe_mlpq_dgrad_kernel": 3, "fe_mlpq_wgrad_kernel": 3,
           "fe_mlpq_grad_reduce_kernel": 1, "fe_mlpq_target_kernel": 1, "fe_mlp2_wgrad2_kernel": 3,
           "fe_policy_table_kernel": 1, "fe_mlp_pack_kernel": 1, "fe_mlp_grad_reduce_kernel": 1, "fe_mlp2_grad_reduce_kernel": 1}
COLUMNS = ("vgpr", "agpr", "sgpr", "scratch", "vgpr_spill", "sgpr_spill", "occupancy", "lds")


@pytest.fixture(scope="module")
def table():
    import resource_usage

    from finenvs_amd.csrc import build as hip_build

    if not os.path.exists(hip_build.HIPCC):
        pytest.skip("hipcc not available")
    return resource_usage.kernel_table(source="fe_mlp_critic.hip")


def _family(name):
    return re.sub(r"<.*", "", name)


def test_the_unit_holds_these_kernels_and_none_uses_scratch_or_spills_a_vgpr(table):
    counts = {}
    for r in table:
        counts[_family(r["name"])] = counts.get(_family(r["name"]), 0) + 1
    assert counts == KERNELS
    assert not [f for f in KERNELS if "mlp2" in f and f.startswith("fe_mlpq")]  # the new kernels' names carry no "mlp2"
    bad = [(r["name"], r["scratch"], r["vgpr_spill"]) for r in table if r["scratch"] != 0 or r["vgpr_spill"] != 0]
    assert not bad, f"scratch / VGPR spills in the MLP critic unit: {bad}"


def test_the_32_and_64_wide_instantiations_keep_two_waves_per_simd(table):
    checked = 0
    for r in table:
        if r["name"].endswith("<1>") or r["name"].endswith("<2>"):
            assert r["occupancy"] >= 2, (r["name"], r["occupancy"])
            checked += 1
    assert checked == 10


def test_committed_table_matches_this_build(table):
    committed = []
    for line in open(PROFILE).read().splitlines():
        if line.startswith("fe_"):
            committed.append((line[:58].strip(),) + tuple(int(c) for c in line[58:].split()))
    mine = [(r["name"][:58].strip(),) + tuple(r[c] for c in COLUMNS) for r in table]
    assert sorted(committed) == sorted(mine), "regenerate profiles/mlp_critic_resource_usage.txt (tools/resource_usage.py " \
                                              "--source fe_mlp_critic.hip --out ...)"
