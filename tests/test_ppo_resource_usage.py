"""CPU (cross-compile only): every fe_ppo_* kernel exists exactly once and has no scratch memory and no VGPR spills
(tools/resource_usage.py)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("fe_ppo_minibatch_kernel", "fe_ppo_epochs_advance_kernel", "fe_ppo_actor_loss_kernel", "fe_ppo_value_loss_kernel")


@pytest.fixture(scope="module")
def table():
    import resource_usage

    from finenvs_amd.csrc import build as hip_build

    if not os.path.exists(hip_build.HIPCC):
        pytest.skip("hipcc not available")
    return resource_usage.kernel_table()


def test_ppo_kernels_exist_once_and_use_no_scratch(table):
    import finenvs_amd.ppo  # noqa: F401  (the Python side of these kernels)

    rows = [r for r in table if r["name"].startswith("fe_ppo_")]
    names = sorted(r["name"] for r in rows)
    for k in KERNELS:  # one kernel for every shape: no instantiations
        assert len([n for n in names if n.startswith(k)]) == 1, (k, names)
    assert len(rows) == len(KERNELS), names
    bad = [(r["name"], r["scratch"], r["vgpr_spill"]) for r in rows if r["scratch"] != 0 or r["vgpr_spill"] != 0]
    assert not bad, f"scratch / VGPR spills in the PPO kernels: {bad}"
    # none of them counts as a kernel of another family: the other resource-usage tests count those by prefix
    for prefix in ("fe_replay_", "fe_evo_", "fe_ring_draw_", "fe_lstm_", "fe_critic_", "fe_sac_", "fe_net_"):
        assert not [n for n in names if n.startswith(prefix)]
