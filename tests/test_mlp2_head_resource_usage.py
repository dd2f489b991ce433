"""CPU (cross-compile only): registers and scratch of the two-hidden-layer MLP head's kernels
(include/finenvs_amd_mlp2_head.h), and of everything that was there before them.

* every new kernel -- ``fe_rollout_mlp2_sampled_kernel``, ``fe_mlp2_forward_kernel``, ``fe_mlp2_grad_kernel``,
  ``fe_mlp2_dgrad_kernel``, ``fe_mlp2_wgrad2_kernel``, ``fe_mlp2_grad_reduce_kernel`` -- uses no scratch memory and spills
  no VGPR, and the table of this build is committed as profiles/mlp2_head_resource_usage.txt.  No waves-per-SIMD floor
  is asked of the H = 128 kernels that hold the W2 image next to W1^T: 66 KiB of LDS for W2 alone leave one workgroup
  per CU, and those instantiations take the registers of one wavefront per SIMD;
* every kernel that existed before kept every column of the parent commit's row -- VGPRs, AGPRs, SGPRs, scratch,
  spills, occupancy, static LDS -- and no existing kernel gained an instantiation: the new device code calls the
  one-layer head's device functions and launches its kernels as they stand.  The parent's rows were generated from the
  parent commit with the same tool and live in the same file.
"""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
PROFILE = os.path.join(ROOT, "profiles", "mlp2_head_resource_usage.txt")
NEW = {"fe_rollout_mlp2_sampled_kernel": 6, "fe_mlp2_forward_kernel": 6, "fe_mlp2_grad_kernel": 3, "fe_mlp2_dgrad_kernel": 3,
       "fe_mlp2_wgrad2_kernel": 3, "fe_mlp2_grad_reduce_kernel": 1}
COLUMNS = ("vgpr", "agpr", "sgpr", "scratch", "vgpr_spill", "sgpr_spill", "occupancy", "lds")


@pytest.fixture(scope="module")
def table():
    import resource_usage

    from finenvs_amd.csrc import build as hip_build

    if not os.path.exists(hip_build.HIPCC):
        pytest.skip("hipcc not available")
    return resource_usage.kernel_table()


def _sections():
    """{section title: [(kernel name as the tool prints it, vgpr, agpr, sgpr, scratch, vgpr spill, sgpr spill, waves / SIMD,
    static LDS)]} of the committed file."""
    sections, rows = {}, None
    for line in open(PROFILE).read().splitlines():
        if line.startswith("# "):
            rows = sections.setdefault(line[2:], [])
        elif line.startswith("fe_"):
            rows.append((line[:58].strip(),) + tuple(int(c) for c in line[58:].split()))
    return sections


def _section(prefix):
    return next(rows for title, rows in _sections().items() if title.startswith(prefix))


def _family(name):
    return re.sub(r"<.*", "", name)


def _row(r):
    return (r["name"][:58].strip(),) + tuple(r[c] for c in COLUMNS)  # the tool prints 58 characters of a name


def test_new_kernels_use_no_scratch_and_spill_no_vgpr(table):
    new = [r for r in table if _family(r["name"]) in NEW]
    counts = {f: len([r for r in new if _family(r["name"]) == f]) for f in NEW}
    assert counts == NEW
    assert not [r["name"] for r in table if "mlp2" in r["name"] and _family(r["name"]) not in NEW]
    bad = [(r["name"], r["scratch"], r["vgpr_spill"]) for r in new if r["scratch"] != 0 or r["vgpr_spill"] != 0]
    assert not bad, f"scratch / VGPR spills in the two-layer MLP head's kernels: {bad}"
    for r in new:  # H = 32 and 64 keep two workgroups per CU wherever a weight image or accumulators are held
        if not r["name"].endswith("4>") and _family(r["name"]) != "fe_mlp2_grad_reduce_kernel":
            assert r["occupancy"] >= 2, (r["name"], r["occupancy"])


def test_committed_table_matches_this_build(table):
    mine = _section("the kernels of include/finenvs_amd_mlp2_head.h")
    new = [r for r in table if _family(r["name"]) in NEW]
    assert sorted(mine) == sorted(_row(r) for r in new), "regenerate profiles/mlp2_head_resource_usage.txt"


def test_every_existing_kernel_equals_the_parent_commits_row_in_every_column(table):
    parent = _section("every kernel of the parent commit")
    assert len(parent) >= 200 and not [row for row in parent if "mlp2" in row[0]]
    assert {"fe_mlp_wgrad_kernel", "fe_mlp_grad_reduce_kernel", "fe_rollout_mlp_kernel", "fe_rollout_mlp_sampled_kernel",
            "fe_mlp_forward_kernel", "fe_mlp_grad_kernel", "fe_mlp_pack_kernel"} <= {_family(row[0]) for row in parent}
    existing = sorted(_row(r) for r in table if _family(r["name"]) not in NEW)
    parent = sorted(parent)
    changed = sorted(set(existing) ^ set(parent))
    assert not changed, f"rows that differ from the parent commit's: {changed[:10]}"
    assert existing == parent  # the same rows the same number of times: no kernel gained or lost an instantiation
