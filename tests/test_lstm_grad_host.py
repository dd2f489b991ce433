"""CPU: the gradient half of the one-output LSTM head -- the C ABI surface of include/finenvs_amd_lstm_grad.h with the
argument checks that need no device, the workspace size, and the repository's LSTMHead + the torch bodies of the PPO
actor, PPO critic and TD3 actor losses against the reference's own gradients (tests/golden/lstm_head_grads.npz, written
by tools/make_lstm_grad_golden.py from the reference's compute_actor_loss / compute_critic_loss / compute_loss and their
backward())."""
import ctypes as C
import os
import re

import numpy as np
import torch

from tests.helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "finenvs_amd_lstm_grad.h")


def test_header_declares_exactly_the_lstm_grad_signatures_and_the_library_exports_them():
    from finenvs_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(fe_[a-z0-9_]+)\s*\(", text))) == sorted(_lib.LSTM_GRAD_SIGNATURES)
    others = (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.EVO_SIGNATURES) | set(_lib.REPLAY_SIGNATURES)
              | set(_lib.SAC_SIGNATURES) | set(_lib.CRITIC_SIGNATURES) | set(_lib.CRITIC_GRAD_SIGNATURES)
              | set(_lib.SAC_GRAD_SIGNATURES))
    assert not set(_lib.LSTM_GRAD_SIGNATURES) & others
    lib = _lib.load()
    for name in _lib.LSTM_GRAD_SIGNATURES:
        assert hasattr(lib, name)
    assert lib.fe_version() == _lib.FE_ABI_VERSION == 5


def test_struct_fields_match_the_binding():
    from finenvs_amd import _lib
    from finenvs_amd.lstm_head import LSTM_GRAD_KEYS

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    fields = re.search(r"typedef struct fe_lstm_grads \{(.*?)\} fe_lstm_grads;", text, flags=re.S).group(1)
    assert re.findall(r"\*(\w+);", fields) == [f for f, _ in _lib.FeLstmGrads._fields_] == list(LSTM_GRAD_KEYS)


POINTERS = ("env", "lr32", "whh", "wx", "wout", "src", "pos", "outputs", "d_outputs", "workspace")


def _backward(lib, H=32, act=0, count=4, grads="ok", **null):
    """fe_lstm_backward on made-up non-null pointers (never dereferenced: every case here is refused first)."""
    from finenvs_amd import _lib

    p = {k: 16 for k in POINTERS}
    p.update(null)
    g = _lib.FeLstmGrads(*([16] * 6)) if grads == "ok" else grads
    return lib.fe_lstm_backward(p["env"], p["lr32"], p["whh"], p["wx"], p["wout"], H, act, p["src"], p["pos"], count,
                                p["outputs"], p["d_outputs"], p["workspace"], None if g is None else C.byref(g), None)


def test_argument_checks_need_no_device():
    from finenvs_amd import _lib

    lib = _lib.load()
    for name in POINTERS:
        if name == "outputs":
            continue  # may be null without an activation; refused with tanh below
        assert _backward(lib, **{name: None}) == _lib.FE_ERR_ARG, name
        assert b"fe_lstm_backward: bad argument" in lib.fe_last_error(), name
    for kw in (dict(grads=None), dict(count=-1)):
        assert _backward(lib, **kw) == _lib.FE_ERR_ARG, kw
        assert b"fe_lstm_backward: bad argument" in lib.fe_last_error()
    for k in range(6):  # every field of fe_lstm_grads is required
        ptrs = [16] * 6
        ptrs[k] = None
        assert _backward(lib, grads=_lib.FeLstmGrads(*ptrs)) == _lib.FE_ERR_ARG, k
        assert b"fe_lstm_backward: bad argument" in lib.fe_last_error()
    for H in (16, 48, 256):
        for act in (0, 2):
            assert _backward(lib, H=H, act=act) == _lib.FE_ERR_ARG
            assert b"fe_lstm_backward: H must be 32, 64 or 128" in lib.fe_last_error()
    for act in (1, -1, 3):  # clamp has no gradient to train on
        assert _backward(lib, act=act) == _lib.FE_ERR_ARG
        assert b"fe_lstm_backward: out_activation must be 0 (tanh) or 2 (none)" in lib.fe_last_error()
    assert _backward(lib, act=0, outputs=None) == _lib.FE_ERR_ARG
    msg = lib.fe_last_error()
    assert b"fe_lstm_backward" in msg and b"needs outputs" in msg, msg


def test_workspace_size_is_monotone_and_bounded():
    from finenvs_amd import _lib

    lib = _lib.load()
    per_pair = 0  # the O(count) term include/finenvs_amd_lstm_grad.h documents: no per-pair output leaves the kernel
    for H in (32, 64, 128):
        for W in (4, 16):
            sizes = [lib.fe_lstm_grad_workspace_floats(H, W, n) for n in
                     (0, 1, 31, 32, 33, 256, 4097, 65536, 1 << 20, 1 << 24)]
            assert all(b >= a for a, b in zip(sizes, sizes[1:])), (H, W, sizes)
            assert sizes[1] > sizes[0] > 0
            assert sizes[-1] - sizes[-2] == per_pair * ((1 << 24) - (1 << 20))
            # bounded by the resident workgroup count: 512 workgroups (256 at H = 128) of 32 pairs fill it
            full = 32 * (256 if H == 128 else 512)
            assert lib.fe_lstm_grad_workspace_floats(H, W, full) == sizes[-1]
            assert lib.fe_lstm_grad_workspace_floats(H, W, full - 32) < sizes[-1]
            # it does less than the SAC actor's backward, with less memory
            assert sizes[-1] < lib.fe_sac_grad_workspace_floats(H, W, 1 << 24)
        assert lib.fe_lstm_grad_workspace_floats(H, 16, 1000) > lib.fe_lstm_grad_workspace_floats(H, 4, 1000)
    for H, W, n in ((48, 4, 1), (16, 4, 1), (256, 4, 1), (32, 0, 1), (32, 4, -1)):
        assert lib.fe_lstm_grad_workspace_floats(H, W, n) == -1
    assert "per-pair term is 0 floats" in open(HEADER).read()


def _head(gold, tag, H, W, activation):
    from finenvs_amd.lstm_head import LSTMHead

    head = LSTMHead(H, W, activation)
    sd = {k[len(tag) + 1:]: torch.from_numpy(v) for k, v in gold.items() if k.startswith(tag + ".")}
    sd.pop("log_standard_deviation", None)  # the PPO learner's own parameter, not the network's
    assert sorted(sd) == sorted(head.state_dict())  # the reference's keys: lstm.* and last_layer.0.*
    head.load_state_dict(sd)
    return head


def _check(gold, tag, loss, named):
    assert abs(float(loss.detach()) - float(gold[f"loss.{tag}"])) <= 1e-6
    loss.backward()
    expected = {k[len(tag) + 3:] for k in gold if k.startswith(f"g.{tag}.")}
    assert expected == set(named)
    for name, p in named.items():
        ref = gold[f"g.{tag}.{name}"]
        assert np.abs(ref).max() > 0, (tag, name)
        np.testing.assert_allclose(p.grad.numpy(), ref, rtol=0, atol=1e-6, err_msg=f"{tag} {name}")


def test_head_and_losses_reproduce_the_reference_gradients():
    from finenvs_amd.critic import CriticLSTM
    from finenvs_amd.lstm_head import head_parameters, torch_ppo_actor_loss, torch_ppo_critic_loss

    gold = load_golden("lstm_head_grads.npz")
    B, W, H = (int(x) for x in gold["meta"])
    s = torch.from_numpy(gold["states"])
    assert tuple(s.shape) == (B, W, 5)
    column = lambda k: torch.from_numpy(gold[k])  # noqa: E731
    assert all(tuple(column(k).shape) == (B, 1) for k in ("actions", "old_log_probs", "advantages", "returns"))

    # PPO's actor (PPO/continuous_actor.py:59-78)
    actor = _head(gold, "ppo_actor", H, W, "tanh")
    log_std = torch.nn.Parameter(torch.from_numpy(gold["ppo_actor.log_standard_deviation"]).clone())
    loss = torch_ppo_actor_loss(actor(s), log_std, column("actions"), column("old_log_probs"), column("advantages"),
                                float(gold["clip_epsilon"]), float(gold["entropy_coefficient"]))
    named = dict(actor.named_parameters())
    assert len(named) == 6 and {id(p) for p in named.values()} == {id(p) for p in head_parameters(actor)}
    _check(gold, "ppo_actor", loss, {**named, "log_standard_deviation": log_std})

    # PPO's critic (PPO/critic.py:26-32)
    critic = _head(gold, "ppo_critic", H, W, "none")
    _check(gold, "ppo_critic", torch_ppo_critic_loss(critic(s), column("returns")), dict(critic.named_parameters()))

    # TD3's actor through its first critic (TD3/actor.py:50-56); the network is the PPO actor's
    td3 = _head(gold, "ppo_actor", H, W, "tanh")
    q = CriticLSTM(H, W)
    q.load_state_dict({k[11:]: torch.from_numpy(v) for k, v in gold.items() if k.startswith("td3_critic.")})
    _check(gold, "td3_actor", -q(s, td3(s)).mean(), dict(td3.named_parameters()))
