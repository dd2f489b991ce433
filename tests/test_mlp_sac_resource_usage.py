"""CPU (cross-compile only): registers and scratch of the library's third translation unit,
finenvs_amd/csrc/fe_mlp_sac.hip (include/finenvs_amd_mlp_sac.h).

* the unit holds exactly the five new kernel families (sampled rollout and forward at <SINGLE, NT>, the backward's first
  kernel at <NT>, the fold / pack kernel, the reduce + epilogue kernel), the ``fe_mlp_wgrad_kernel`` instantiations the
  backward launches, and the three non-template kernels ``fe_mlp_head_kernels.h`` emits again;
* no kernel uses scratch memory or spills a VGPR;
* the H = 32 / 64 instantiations reach at least two waves per SIMD.  No floor is asked of H = 128: the backward's first
  kernel keeps 128 accumulators of [A_mu | A_q] next to the first layer's 64 and runs one wave per SIMD;
* the table of this build is committed as profiles/mlp_sac_resource_usage.txt.
The other units' tables staying what they were is tests/test_mlp2_head_resource_usage.py's, tests/test_resource_usage.py's
and tests/test_mlp_critic_resource_usage.py's.
"""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
PROFILE = os.path.join(ROOT, "profiles", "mlp_sac_resource_usage.txt")
# family: instantiations
KERNELS = {"fe_rollout_mlp_sac_kernel": 6, "fe_mlp_sac_forward_kernel": 6, "fe_mlp_sac_grad_kernel": 3,
           "fe_mlp_sac_pack_kernel": 1, "fe_mlp_sac_grad_reduce_kernel": 1, "fe_mlp_wgrad_kernel": 3,
           "fe_policy_table_kernel": 1, "fe_mlp_pack_kernel": 1, "fe_mlp_grad_reduce_kernel": 1}
COLUMNS = ("vgpr", "agpr", "sgpr", "scratch", "vgpr_spill", "sgpr_spill", "occupancy", "lds")


@pytest.fixture(scope="module")
def table():
    import resource_usage

    from finenvs_amd.csrc import build as hip_build

    if not os.path.exists(hip_build.HIPCC):
        pytest.skip("hipcc not available")
    return resource_usage.kernel_table(source="fe_mlp_sac.hip")


def _family(name):
    return re.sub(r"<.*", "", name)


def test_the_unit_holds_these_kernels_and_none_uses_scratch_or_spills_a_vgpr(table):
    counts = {}
    for r in table:
        counts[_family(r["name"])] = counts.get(_family(r["name"]), 0) + 1
    assert counts == KERNELS
    bad = [(r["name"], r["scratch"], r["vgpr_spill"]) for r in table if r["scratch"] != 0 or r["vgpr_spill"] != 0]
    assert not bad, f"scratch / VGPR spills in the SAC MLP unit: {bad}"


def test_the_32_and_64_wide_instantiations_keep_two_waves_per_simd(table):
    checked = 0
    for r in table:
        if re.search(r"[<, ][12]>$", r["name"]):
            assert r["occupancy"] >= 2, (r["name"], r["occupancy"])
            checked += 1
    assert checked == 4 + 4 + 2 + 2  # rollout and forward at both SINGLE, the backward's kernel, the weight gradient


def test_committed_table_matches_this_build(table):
    committed = []
    for line in open(PROFILE).read().splitlines():
        if line.startswith("fe_"):
            committed.append((line[:58].strip(),) + tuple(int(c) for c in line[58:].split()))
    mine = [(r["name"][:58].strip(),) + tuple(r[c] for c in COLUMNS) for r in table]
    assert sorted(committed) == sorted(mine), "regenerate profiles/mlp_sac_resource_usage.txt (tools/resource_usage.py " \
                                              "--source fe_mlp_sac.hip --out ...)"
