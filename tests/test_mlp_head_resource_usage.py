"""CPU (cross-compile only): registers and scratch of the MLP head's training kernels (include/finenvs_amd_mlp_head.h).

* every new kernel -- ``fe_rollout_mlp_sampled_kernel``, ``fe_mlp_forward_kernel``, ``fe_mlp_grad_kernel``,
  ``fe_mlp_wgrad_kernel``, ``fe_mlp_grad_reduce_kernel``, ``fe_mlp_pack_kernel`` -- uses no scratch memory and spills no
  VGPR, and the table of this build is committed as profiles/mlp_head_resource_usage.txt;
* the six ``fe_rollout_mlp_kernel`` instantiations kept the parent commit's VGPRs, scratch and occupancy: the first
  layer the new kernels share is restated (``mlp_head_first_layer``), not factored out of ``mlp_policy_block``.  The
  parent's rows were generated from the parent commit with the same tool and live in the same file.
"""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
PROFILE = os.path.join(ROOT, "profiles", "mlp_head_resource_usage.txt")
NEW = {"fe_rollout_mlp_sampled_kernel": 6, "fe_mlp_forward_kernel": 6, "fe_mlp_grad_kernel": 3, "fe_mlp_wgrad_kernel": 3,
       "fe_mlp_grad_reduce_kernel": 1, "fe_mlp_pack_kernel": 1}


@pytest.fixture(scope="module")
def table():
    import resource_usage

    from finenvs_amd.csrc import build as hip_build

    if not os.path.exists(hip_build.HIPCC):
        pytest.skip("hipcc not available")
    return resource_usage.kernel_table()


def _sections():
    """{section title: {kernel: (vgpr, agpr, sgpr, scratch, vgpr spill, sgpr spill, waves / SIMD, static LDS)}} of the file."""
    sections, rows = {}, None
    for line in open(PROFILE).read().splitlines():
        if line.startswith("# "):
            rows = sections.setdefault(line[2:], {})
        elif line.startswith("fe_"):
            rows[line[:58].strip()] = tuple(int(c) for c in line[58:].split())
    return sections


def _family(name):
    return re.sub(r"<.*", "", name)


def test_new_kernels_use_no_scratch_and_spill_no_vgpr(table):
    new = [r for r in table if _family(r["name"]) in NEW]
    counts = {f: len([r for r in new if _family(r["name"]) == f]) for f in NEW}
    assert counts == NEW
    bad = [(r["name"], r["scratch"], r["vgpr_spill"]) for r in new if r["scratch"] != 0 or r["vgpr_spill"] != 0]
    assert not bad, f"scratch / VGPR spills in the MLP head kernels: {bad}"
    # the three kernels with a weight image or accumulators per hidden tile fit two workgroups per CU
    for r in new:
        if _family(r["name"]) != "fe_mlp_grad_reduce_kernel" and _family(r["name"]) != "fe_mlp_pack_kernel":
            assert r["occupancy"] >= 2, (r["name"], r["occupancy"])


def test_committed_table_matches_this_build(table):
    sections = _sections()
    mine = next(rows for title, rows in sections.items() if title.startswith("the kernels of include/finenvs_amd_mlp_head.h"))
    new = [r for r in table if _family(r["name"]) in NEW]
    assert sorted(mine) == sorted(r["name"] for r in new), "regenerate profiles/mlp_head_resource_usage.txt"
    for r in new:
        vgpr, agpr, _, scratch, vgpr_spill, _, waves, _ = mine[r["name"]]
        assert (vgpr, agpr, scratch, vgpr_spill, waves) == (r["vgpr"], r["agpr"], r["scratch"], r["vgpr_spill"], r["occupancy"]), \
            (r["name"], mine[r["name"]])


def test_the_six_rollout_kernels_equal_the_parent_commits(table):
    sections = _sections()
    parent = next(rows for title, rows in sections.items() if title.startswith("fe_rollout_mlp_kernel, the parent commit"))
    assert len(parent) == 6
    six = [r for r in table if r["name"].startswith("fe_rollout_mlp_kernel")]
    assert sorted(r["name"] for r in six) == sorted(parent)  # and no new instantiation of it
    for r in six:
        vgpr, _, _, scratch, _, _, waves, _ = parent[r["name"]]
        assert (r["vgpr"], r["scratch"], r["occupancy"]) == (vgpr, scratch, waves), (r["name"], parent[r["name"]])
