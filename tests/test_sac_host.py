"""CPU: SAC's LSTM actor (finenvs_amd/sac.py) against the reference's own outputs (tests/golden/sac_actor.npz, written by
tools/make_sac_golden.py from the reference's SAC ActorLSTM and SACAgent.step), the host-side weight packing of the fused
head, and the C ABI surface of include/finenvs_amd_sac.h."""
import os
import re

import numpy as np
import pytest
import torch

from tests.helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return load_golden("sac_actor.npz")


def _actor(gold):
    from finenvs_amd.sac import SACActorLSTM

    B, W, H = (int(x) for x in gold["meta"])
    actor = SACActorLSTM(H=H, W=W, A=1)
    actor.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in gold.items() if k.startswith("sd.")})
    return actor


def test_actor_reproduces_the_reference_distribution_and_samples(gold):
    actor = _actor(gold)
    states, eps = torch.from_numpy(gold["obs"]), torch.from_numpy(gold["eps"])
    with torch.no_grad():
        dist = actor.get_distribution(states)
        actions, log_probs = actor.get_actions_and_log_probs(states, eps)
        step = actor.step_actions(states, eps)
    for name, got in (("loc", dist.loc), ("scale", dist.scale), ("actions", actions), ("log_probs", log_probs),
                      ("step_actions", step)):
        np.testing.assert_allclose(got.numpy(), gold[name], rtol=0, atol=1e-6, err_msg=name)
    # the step row: the last env acts on the un-squashed mean, every other on tanh(u)
    assert step[-1, 0] == dist.loc[-1, 0] and not np.isclose(gold["step_actions"][-1, 0], gold["actions"][-1, 0])
    assert float(dist.scale.std()) > 0 and float(dist.loc.std()) > 0


def test_actor_shape_and_temperature():
    from finenvs_amd.sac import SACActorLSTM

    actor = SACActorLSTM(H=64, W=16, A=1, starting_alpha=0.2)
    assert [n for n, _ in actor.named_children()] == ["lstm", "last_layer", "mu_layer", "std_layer"]
    assert tuple(actor.last_layer[0].weight.shape) == (64, 64) and isinstance(actor.last_layer[1], torch.nn.Identity)
    assert actor.log_alpha.requires_grad and abs(float(actor.log_alpha.detach().exp()) - 0.2) < 1e-7
    assert all(p is not actor.log_alpha for p in actor.parameters()) and actor.target_entropy == -1.0
    with pytest.raises(ValueError):
        actor.get_distribution(torch.zeros((3, 4, 5)))


def test_pair_states_cuts_a_multi_asset_window_per_asset():
    from finenvs_amd.sac import pair_states

    obs = torch.arange(2 * 3 * 15, dtype=torch.float32).reshape(2, 3, 15)
    p = pair_states(obs, 3)
    assert tuple(p.shape) == (6, 3, 5)
    assert torch.equal(p[1 * 3 + 2], obs[1, :, 10:15])


@pytest.mark.parametrize("H", [32, 64, 128])
def test_weight_packing_round_trips(H):
    from finenvs_amd.rollout import lstm_row_order
    from finenvs_amd.sac import SACActorLSTM, pack_sac_weights, unpack_last_layer

    torch.manual_seed(H)
    actor = SACActorLSTM(H=H, W=4)
    w = pack_sac_weights(actor)
    assert torch.equal(unpack_last_layer(w["wl"]), actor.last_layer[0].weight.detach())
    # fragment-major: [row tile t][k group g][lane r + 32 h][m] = W_l[32 t + r][8 g + 4 h + m]
    frag = w["wl"].reshape(H // 32, H // 8, 64, 4)
    Wl = actor.last_layer[0].weight.detach()
    for t, g, r, h, m in ((0, 0, 0, 0, 0), (H // 32 - 1, H // 8 - 1, 31, 1, 3), (0, 1, 5, 1, 2)):
        assert frag[t, g, r + 32 * h, m] == Wl[32 * t + r, 8 * g + 4 * h + m]
    order = lstm_row_order(H)
    inv = torch.empty_like(order)
    inv[order] = torch.arange(4 * H)
    lstm = actor.lstm
    assert torch.equal(w["whh"][inv], lstm.weight_hh_l0.detach())
    assert torch.equal(w["wx"][inv, :5], lstm.weight_ih_l0.detach())
    assert torch.equal(w["wx"][inv, 5], lstm.bias_ih_l0.detach() + lstm.bias_hh_l0.detach())
    assert torch.equal(w["wmu"], actor.mu_layer.weight.detach().reshape(H))
    assert torch.equal(w["wstd"], actor.std_layer.weight.detach().reshape(H))
    assert torch.equal(w["bl"], actor.last_layer[0].bias.detach())


def test_fused_head_refuses_actors_it_cannot_run():
    from finenvs_amd.sac import SACActorLSTM, check_actor

    assert check_actor(SACActorLSTM(H=128, W=4)) == 128
    for bad in (SACActorLSTM(H=256, W=4), SACActorLSTM(H=48, W=4), SACActorLSTM(H=32, W=4, A=2)):
        with pytest.raises(ValueError):
            check_actor(bad)
    two = SACActorLSTM(H=32, W=4)
    two.lstm = torch.nn.LSTM(5, 32, num_layers=2, batch_first=True)
    with pytest.raises(ValueError, match="num_layers"):
        check_actor(two)


def test_header_declares_exactly_the_sac_signatures_and_the_library_exports_them():
    from finenvs_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "finenvs_amd_sac.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(fe_[a-z0-9_]+)\s*\(", text))) == sorted(_lib.SAC_SIGNATURES)
    others = set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.EVO_SIGNATURES) | set(_lib.REPLAY_SIGNATURES)
    assert not set(_lib.SAC_SIGNATURES) & others
    lib = _lib.load()
    for name in _lib.SAC_SIGNATURES:
        assert hasattr(lib, name)
    # argument checks that need no device
    args = [None] * 7 + [0.0, None, 0.0, 32, 4] + [None] * 11
    assert lib.fe_env_rollout_sac(*args) == _lib.FE_ERR_ARG
    assert b"fe_env_rollout_sac" in lib.fe_last_error()
    fargs = [None] * 7 + [0.0, None, 0.0, 32, None, None, 4] + [None] * 6
    assert lib.fe_sac_forward(*fargs) == _lib.FE_ERR_ARG
    assert b"bad argument" in lib.fe_last_error()
