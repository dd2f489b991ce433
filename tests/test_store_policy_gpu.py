"""GPU: at the size where the store policy of launch_env applies (one observation buffer of 160 MiB, the headline's), the
observation, rewards and dones do not depend on which launches stream past the Infinity Cache and which store plain.

Three envs with the same seed take the same actions: one rewrites ONE buffer (resident from its second launch: plain
stores), one goes round a ring of two (one member resident, one streamed), one gets a fresh tensor every step (always
streamed).  The host-side rule itself is tested in tests/test_store_policy_host.py."""
import pytest
import torch

import finenvs_amd
from finenvs_amd.data import synthetic

pytestmark = pytest.mark.gpu

N, W = 65536, 64  # 65 536 x 64 x 5 doubles = 160 MiB per observation


def test_results_do_not_depend_on_the_store_policy():
    dev = "cuda:0"
    prices, day_id, _ = synthetic.synthetic_series(12, 1, 200, 4321)
    envs = [finenvs_amd.TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=W, num_envs=N, redraw="device", seed=99,
                                      obs_buffers=k) for k in (1, 2, 0)]
    assert envs[0]._obs_ring[0].numel() * 8 == 160 << 20
    g = torch.Generator(device=dev).manual_seed(3)
    first = [e.reset().clone() for e in envs]
    assert torch.equal(torch.nan_to_num(first[0]), torch.nan_to_num(first[1])) and torch.equal(torch.nan_to_num(first[0]), torch.nan_to_num(first[2]))
    for t in range(24):  # past the 8 launches after which a resident buffer can change hands
        a = (torch.rand((N, 1), generator=g, device=dev) * 2 - 1).float()
        outs = [e.step(a) for e in envs]
        o0, r0, d0 = outs[0][0], outs[0][1], outs[0][2]
        for o, r, d, *_ in outs[1:]:
            assert torch.equal(torch.nan_to_num(o), torch.nan_to_num(o0)) and torch.equal(torch.isnan(o), torch.isnan(o0)), f"observation differs at step {t}"
            assert torch.equal(r, r0) and torch.equal(d, d0), f"rewards / dones differ at step {t}"
    assert torch.equal(envs[0].cash, envs[1].cash) and torch.equal(envs[0].cash, envs[2].cash)
