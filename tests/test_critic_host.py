"""CPU: the twin LSTM critics of finenvs_amd/critic.py against the reference's own outputs (tests/golden/critic_targets.npz,
written by tools/make_critic_golden.py from the reference's CriticLSTM, SACAgent.compute_targets and
TD3Agent.compute_targets), the host-side weight packing, the refusals, and the C ABI surface of
include/finenvs_amd_critic.h with the argument checks that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests.helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return load_golden("critic_targets.npz")


def _sd(gold, tag):
    return {k[len(tag) + 1:]: torch.from_numpy(v) for k, v in gold.items() if k.startswith(tag + ".")}


def _nets(gold):
    from finenvs_amd.critic import CriticLSTM
    from finenvs_amd.sac import SACActorLSTM

    B, W, H = (int(x) for x in gold["meta"])
    c1, c2 = CriticLSTM(H, W), CriticLSTM(H, W)
    c1.load_state_dict(_sd(gold, "c1"))
    c2.load_state_dict(_sd(gold, "c2"))
    actor = SACActorLSTM(H=H, W=W)
    actor.load_state_dict(_sd(gold, "sac"))
    with torch.no_grad():  # the reference keeps log_alpha outside its state_dict
        actor.log_alpha.fill_(float(gold["params"][1]))

    class TanhActor(nn.Module):  # the reference's TD3 ActorLSTM((5, H, 1)): LSTM, Linear(H, 1), Tanh
        def __init__(self):
            super().__init__()
            self.lstm = nn.LSTM(5, H, batch_first=True)
            self.last_layer = nn.Sequential(nn.Linear(H, 1), nn.Tanh())

        def forward(self, x):
            return self.last_layer(self.lstm(x)[0][:, -1, :])

    td3 = TanhActor()
    td3.load_state_dict({k: v for k, v in _sd(gold, "td3").items() if k.startswith(("lstm.", "last_layer."))})
    return c1, c2, actor, td3


def test_critics_and_both_targets_reproduce_the_reference(gold):
    from finenvs_amd.critic import torch_sac_targets, torch_td3_targets

    c1, c2, actor, td3 = _nets(gold)
    s, a, r, d = (torch.from_numpy(gold[k]) for k in ("states", "actions", "rewards", "dones"))
    gamma, log_alpha, std, clip = (float(x) for x in gold["params"])
    assert abs(float(actor.log_alpha.detach()) - log_alpha) < 1e-7
    with torch.no_grad():
        q1, q2 = c1(s, a), c2(s, a)
    np.testing.assert_allclose(q1.numpy(), gold["q1"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(q2.numpy(), gold["q2"], rtol=0, atol=1e-6)
    y_sac = torch_sac_targets(actor, c1, c2, r, s, d, torch.from_numpy(gold["sac_eps"]), gamma)
    y_td3 = torch_td3_targets(td3, c1, c2, r, s, d, torch.from_numpy(gold["td3_eps"]), gamma, std, clip)
    np.testing.assert_allclose(y_sac.numpy(), gold["sac_targets"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(y_td3.numpy(), gold["td3_targets"], rtol=0, atol=1e-5)
    # done rows are the reward alone; the critics and targets are not degenerate
    done = gold["dones"][:, 0] == 1
    assert done.any() and (~done).any()
    assert np.array_equal(gold["sac_targets"][done], gold["rewards"][done])
    assert float(np.std(gold["q1"])) > 1e-3 and not np.allclose(gold["q1"], gold["q2"])


def test_reference_keyed_state_dict_loads(gold):
    from finenvs_amd.critic import CriticLSTM

    sd = _sd(gold, "c1")
    assert sorted(sd) == sorted(CriticLSTM(32, 4).state_dict())
    c = CriticLSTM(32, 4)
    c.load_state_dict(sd)  # strict
    assert [n for n, _ in c.named_children()] == ["lstm", "last_layer"]
    assert isinstance(c.last_layer[1], nn.Identity) and c.lstm.input_size == 6


@pytest.mark.parametrize("H", [32, 64, 128])
def test_weight_packing_round_trips(H):
    from finenvs_amd.critic import CriticLSTM, pack_critic_weights
    from finenvs_amd.rollout import lstm_row_order

    torch.manual_seed(H)
    c = CriticLSTM(H, 4)
    w = pack_critic_weights(c)
    assert tuple(w["whh"].shape) == (4 * H, H) and tuple(w["wx"].shape) == (4 * H, 8)
    assert w["wx"].dtype is torch.float32 and w["wx"].is_contiguous()
    order = lstm_row_order(H)
    inv = torch.empty_like(order)
    inv[order] = torch.arange(4 * H)
    lstm = c.lstm
    assert torch.equal(w["whh"][inv], lstm.weight_hh_l0.detach())
    assert torch.equal(w["wx"][inv, :5], lstm.weight_ih_l0.detach()[:, :5])
    assert torch.equal(w["wx"][inv, 5], lstm.bias_ih_l0.detach() + lstm.bias_hh_l0.detach())  # slot 5: the bias
    assert torch.equal(w["wx"][inv, 6], lstm.weight_ih_l0.detach()[:, 5])  # slot 6: the action's weight
    assert not w["wx"][:, 7].any()
    assert torch.equal(w["wout"], c.last_layer[0].weight.detach().reshape(H))
    assert torch.equal(w["bout"], c.last_layer[0].bias.detach())


def test_check_critic_refuses_what_the_kernel_cannot_run():
    from finenvs_amd.critic import CriticLSTM, check_critic

    assert check_critic(CriticLSTM(64, 4)) == 64
    for H in (48, 256):
        with pytest.raises(ValueError, match="H in"):
            check_critic(CriticLSTM(H, 4))
    wide = CriticLSTM(32, 4)
    wide.lstm = nn.LSTM(12, 32, batch_first=True)  # the reference's A = 2 critic: 5A + A inputs
    with pytest.raises(ValueError, match="nn.LSTM\\(6"):
        check_critic(wide)
    two = CriticLSTM(32, 4)
    two.lstm = nn.LSTM(6, 32, num_layers=2, batch_first=True)
    with pytest.raises(ValueError, match="num_layers"):
        check_critic(two)
    for last in (nn.Sequential(nn.Linear(32, 2), nn.Identity()), nn.Sequential(nn.Linear(32, 1), nn.Tanh()),
                 nn.Sequential(nn.Linear(32, 1))):
        bad = CriticLSTM(32, 4)
        bad.last_layer = last
        with pytest.raises(ValueError, match="last_layer"):
            check_critic(bad)


def test_header_declares_exactly_the_critic_signatures_and_the_library_exports_them():
    from finenvs_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "finenvs_amd_critic.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(fe_[a-z0-9_]+)\s*\(", text))) == sorted(_lib.CRITIC_SIGNATURES)
    others = (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.EVO_SIGNATURES) | set(_lib.REPLAY_SIGNATURES)
              | set(_lib.SAC_SIGNATURES))
    assert not set(_lib.CRITIC_SIGNATURES) & others
    lib = _lib.load()
    for name in _lib.CRITIC_SIGNATURES:
        assert hasattr(lib, name)


def _fake_args():
    """Non-null stand-ins: the checks below fail before anything is dereferenced on a device (or the env)."""
    from finenvs_amd import _lib

    w = _lib.FeCriticWeights(16, 16, 16, 16)
    ring = _lib.FeReplayRing(8, 1, 0, 16, 16, 16, 16, 16, 16, 16, 16)
    return w, ring


def _target(lib, w, ring, env=16, H=32, log_probs=None, alpha=None, smooth=None, count=4, indices=16):
    return lib.fe_twin_q_target(env, 16, C.byref(w), C.byref(w), H, C.byref(ring), 0, 4, indices, count, 16, smooth,
                                0.2, 0.5, log_probs, alpha, 0.99, 1.0, 16, 16, 16, None)


def test_argument_checks_need_no_device():
    from finenvs_amd import _lib

    lib = _lib.load()
    w, ring = _fake_args()
    assert lib.fe_twin_q_forward(None, 16, C.byref(w), C.byref(w), 32, 16, 16, 16, 4, 16, 16, None) == _lib.FE_ERR_ARG
    assert b"fe_twin_q_forward: bad argument" in lib.fe_last_error()
    assert lib.fe_twin_q_forward(16, 16, C.byref(w), C.byref(w), 32, 16, 16, 16, -1, 16, 16, None) == _lib.FE_ERR_ARG
    nob = _lib.FeCriticWeights(16, 16, 16, None)  # bout missing
    assert lib.fe_twin_q_forward(16, 16, C.byref(w), C.byref(nob), 32, 16, 16, 16, 4, 16, 16, None) == _lib.FE_ERR_ARG
    for H in (16, 48, 256):
        assert lib.fe_twin_q_forward(16, 16, C.byref(w), C.byref(w), H, 16, 16, 16, 4, 16, 16, None) == _lib.FE_ERR_ARG
        assert b"fe_twin_q_forward: H must be 32, 64 or 128" in lib.fe_last_error()
        assert _target(lib, w, ring, H=H) == _lib.FE_ERR_ARG
        assert b"fe_twin_q_target: H must be" in lib.fe_last_error()
    assert _target(lib, w, ring, env=None) == _lib.FE_ERR_ARG
    assert _target(lib, w, ring, indices=None) == _lib.FE_ERR_ARG
    assert b"fe_twin_q_target: bad argument" in lib.fe_last_error()
    assert _target(lib, w, ring, log_probs=16) == _lib.FE_ERR_ARG
    assert b"fe_twin_q_target: log_probs (SAC) need alpha" in lib.fe_last_error()
    assert _target(lib, w, ring, log_probs=16, alpha=16, smooth=16) == _lib.FE_ERR_ARG
    assert b"exclusive" in lib.fe_last_error()
    bad_ring = _lib.FeReplayRing(8, 1, 0, 16, 16, 16, 16, 16, 16, 16, None)  # no error counter
    assert _target(lib, w, bad_ring) == _lib.FE_ERR_ARG
