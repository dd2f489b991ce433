"""CPU: the twin MLP critics -- the C ABI surface of include/finenvs_amd_mlp_critic.h with the argument checks that need
no device, the workspace size against the formula the header states, the one error buffer of the library's two
translation units, and the repository's MLPCritic + the torch restatements against the reference's own values, losses,
targets and gradients (tests/golden/mlp_critic.npz, written by tools/make_mlp_critic_golden.py from the reference's
CriticMLP((5W + 1, H, H, 1)) x 2, its tanh ActorMLP, Critic.compute_loss / Actor.compute_loss with backward() and
TD3Agent.compute_targets).  The refusals that read the env (A != 1, the window) are tests/test_mlp_critic_gpu.py's."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests.helpers import load_golden
from tests.test_mlp2_head_host import _close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "finenvs_amd_mlp_critic.h")
P = 16  # a made-up non-null pointer, never dereferenced: every case here is refused first


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_exactly_the_mlp_critic_signatures_and_the_library_exports_them():
    from finenvs_amd import _lib

    assert sorted(set(re.findall(r"\b(fe_[a-z0-9_]+)\s*\(", _header()))) == sorted(_lib.MLP_CRITIC_SIGNATURES)
    others = set()
    for name in dir(_lib):
        if name.endswith("SIGNATURES") and name != "MLP_CRITIC_SIGNATURES":
            others |= set(getattr(_lib, name))
    assert len(others) > 50 and not set(_lib.MLP_CRITIC_SIGNATURES) & others
    lib = _lib.load()
    for name, (_, args) in _lib.MLP_CRITIC_SIGNATURES.items():
        assert hasattr(lib, name)
        decl = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", _header(), flags=re.S).group(1)
        assert len(decl.split(",")) == len(args), name  # one binding argument per declared parameter
    text = _header()
    from finenvs_amd.mlp_critic import MLPQ_GRAD_CHUNK_PAIRS, MLPQ_GRAD_KEYS

    fields = re.search(r"typedef struct fe_mlpq_grads \{(.*?)\} fe_mlpq_grads;", text, flags=re.S).group(1)
    assert re.findall(r"\*(\w+);", fields) == [f for f, _ in _lib.FeMlpqGrads._fields_] == list(MLPQ_GRAD_KEYS)
    fields = re.search(r"typedef struct fe_mlpq_weights \{(.*?)\} fe_mlpq_weights;", text, flags=re.S).group(1)
    assert re.findall(r"\*(\w+);", fields) == [f for f, _ in _lib.FeMlpqWeights._fields_]
    assert int(re.search(r"#define FE_MLPQ_GRAD_CHUNK_PAIRS (\d+)", text).group(1)) == MLPQ_GRAD_CHUNK_PAIRS == 512
    cites = open(HEADER).read()
    for ref in ("TD3/critic.py:49-64", "SAC/critic.py:48-58", "TD3_agent.py:231-251", "TD3/critic.py:31-46", "TD3/critic.py:55-64"):
        assert ref in cites, ref  # the reference lines each entry replaces


def _weights(**null):
    from finenvs_amd import _lib

    p = {k: P for k, _ in _lib.FeMlpqWeights._fields_}
    p.update(null)
    return _lib.FeMlpqWeights(*(p[k] for k, _ in _lib.FeMlpqWeights._fields_))


def _ref(x):
    return None if x is None else C.byref(x)


def _forward(lib, H=32, act=0, count=4, c1="ok", c2="ok", **null):
    p = {k: P for k in ("env", "lr32", "src", "pos", "actions", "q1", "q2")}
    p.update(null)
    c1, c2 = (_weights() if c == "ok" else c for c in (c1, c2))
    return lib.fe_twin_mlpq_forward(p["env"], p["lr32"], _ref(c1), _ref(c2), H, act, p["src"], p["pos"], p["actions"], count,
                                    p["q1"], p["q2"], None)


def _ring(**fields):
    from finenvs_amd import _lib

    f = dict(capacity=64, num_assets=1, reserved=0, state_src=P, state_pos=P, next_src=P, next_pos=P, actions=P, rewards=P,
             dones=P, errors=P)
    f.update(fields)
    return _lib.FeReplayRing(*(f[k] for k, _ in _lib.FeReplayRing._fields_))


def _target(lib, H=32, act=0, count=4, c1="ok", c2="ok", ring="ok", head=0, size=8, cursor=False, **null):
    p = {k: P for k in ("env", "lr32", "indices", "next_actions", "targets", "q1", "q2")}
    p.update(noise=None, log_probs=None, alpha=None)
    p.update(null)
    c1, c2 = (_weights() if c == "ok" else c for c in (c1, c2))
    ring = _ring() if ring == "ok" else ring
    tail = (p["indices"], count, p["next_actions"], p["noise"], 0.2, 0.5, p["log_probs"], p["alpha"], 0.99, 1.0, p["targets"],
            p["q1"], p["q2"], None)
    if cursor is not False:
        return lib.fe_twin_mlpq_target_c(p["env"], p["lr32"], _ref(c1), _ref(c2), H, act, _ref(ring), cursor, *tail)
    return lib.fe_twin_mlpq_target(p["env"], p["lr32"], _ref(c1), _ref(c2), H, act, _ref(ring), head, size, *tail)


def _backward(lib, H=32, act=0, count=4, c1="ok", c2="ok", g1="ok", g2="ok", **null):
    from finenvs_amd import _lib

    p = {k: P for k in ("env", "lr32", "src", "pos", "actions", "dq1", "dq2", "workspace", "d_actions")}
    p.update(null)
    c1, c2 = (_weights() if c == "ok" else c for c in (c1, c2))
    g1, g2 = (_lib.FeMlpqGrads(*([P] * 6)) if g == "ok" else g for g in (g1, g2))
    return lib.fe_twin_mlpq_backward(p["env"], p["lr32"], _ref(c1), _ref(c2), H, act, p["src"], p["pos"], p["actions"], count,
                                     p["dq1"], p["dq2"], p["workspace"], _ref(g1), _ref(g2), p["d_actions"], None)


def test_argument_checks_need_no_device():
    from finenvs_amd import _lib

    lib = _lib.load()
    ERR = _lib.FE_ERR_ARG
    calls = {"fe_twin_mlpq_forward": (_forward, ("env", "lr32", "src", "pos", "actions", "q1", "q2")),
             "fe_twin_mlpq_target": (_target, ("env", "lr32", "indices", "next_actions", "targets", "q1", "q2")),
             "fe_twin_mlpq_backward": (_backward, ("env", "lr32", "src", "pos", "actions", "workspace"))}
    for name, (call, required) in calls.items():
        who = name.encode()
        for ptr in required:
            assert call(lib, **{ptr: None}) == ERR, (name, ptr)
            assert who + b": bad argument" in lib.fe_last_error(), (name, ptr)
        assert call(lib, count=-1) == ERR and who + b": bad argument" in lib.fe_last_error()
        for H in (16, 48, 256):
            assert call(lib, H=H) == ERR
            assert who + b": H must be 32, 64 or 128" in lib.fe_last_error()
        for act in (-1, 3):
            assert call(lib, act=act) == ERR
            assert who + b": activation must be 0 (ELU), 1 (ReLU) or 2 (tanh)" in lib.fe_last_error()
    for call, who in ((_forward, b"fe_twin_mlpq_forward"), (_target, b"fe_twin_mlpq_target")):
        for c in ("c1", "c2"):  # both critics' weights, every field
            assert call(lib, **{c: None}) == ERR and who + b": bad argument" in lib.fe_last_error()
            for field, _ in _lib.FeMlpqWeights._fields_:
                assert call(lib, **{c: _weights(**{field: None})}) == ERR, (who, c, field)
                assert who + b": bad argument" in lib.fe_last_error()
    # the targets alone
    who = b"fe_twin_mlpq_target"
    assert _target(lib, ring=None) == ERR and who + b": bad argument" in lib.fe_last_error()
    for field in ("state_src", "state_pos", "next_src", "next_pos", "actions", "rewards", "dones", "errors"):
        assert _target(lib, ring=_ring(**{field: None})) == ERR and who + b": bad argument" in lib.fe_last_error(), field
    assert _target(lib, ring=_ring(capacity=0)) == ERR and who + b": bad argument" in lib.fe_last_error()
    assert _target(lib, log_probs=P) == ERR and who + b": log_probs (SAC) need alpha" in lib.fe_last_error()
    assert _target(lib, log_probs=P, alpha=P, noise=P) == ERR
    assert who + b": smooth_noise (TD3) and log_probs (SAC) are exclusive" in lib.fe_last_error()
    assert _target(lib, cursor=None) == ERR and b"fe_twin_mlpq_target_c: null cursor" in lib.fe_last_error()
    assert _target(lib, cursor=P, H=48) == ERR and who + b": H must be 32, 64 or 128" in lib.fe_last_error()
    # the backward alone: a dq without its weights, a gradient struct with a null field, nothing to compute
    who = b"fe_twin_mlpq_backward"
    assert _backward(lib, c1=None) == ERR and who + b": dq1 is given without critic 1's weights" in lib.fe_last_error()
    assert _backward(lib, c2=_weights(wact=None)) == ERR and who + b": dq2 is given without critic 2's weights" in lib.fe_last_error()
    for k in range(6):
        ptrs = [P] * 6
        ptrs[k] = None
        assert _backward(lib, g2=_lib.FeMlpqGrads(*ptrs)) == ERR and who + b": grads2 has a null field" in lib.fe_last_error(), k
    assert _backward(lib, g1=None, d_actions=None) == ERR
    assert who + b": critic 1 has neither its gradients nor d_actions" in lib.fe_last_error()
    assert _backward(lib, dq1=None, c1=None, g1=None, g2=None, d_actions=None) == ERR
    assert who + b": critic 2 has neither its gradients nor d_actions" in lib.fe_last_error()
    # a critic without dq needs neither weights nor gradients: the next check is reached
    assert _backward(lib, dq1=None, c1=None, g1=None, H=48) == ERR and who + b": H must be" in lib.fe_last_error()


def test_both_translation_units_write_one_error_buffer():
    from finenvs_amd import _lib

    lib = _lib.load()
    assert _forward(lib, H=48) == _lib.FE_ERR_ARG  # set by fe_mlp_critic.hip
    assert lib.fe_last_error() == b"fe_twin_mlpq_forward: H must be 32, 64 or 128 (got 48)"
    assert lib.fe_mlp2_forward(None, P, None, 32, 0, 0, P, P, 4, P, None) == _lib.FE_ERR_ARG  # then one set by fe_env.hip
    assert lib.fe_last_error() == b"fe_mlp2_forward: bad argument"
    assert _backward(lib, count=-1) == _lib.FE_ERR_ARG  # and back
    assert lib.fe_last_error() == b"fe_twin_mlpq_backward: bad argument"


def _formula(H, W, count):
    """The workspace size as include/finenvs_amd_mlp_critic.h states it."""
    if count == 0:
        return 0
    blocks, splits, F = -(-count // 32), -(-count // 512), 32 * -(-(4 * W + 3) // 32)
    waves = 4 * min(-(-blocks // 4), 512)
    return 3 * 32 * blocks * H + splits * H * (F + H + 32) + waves * (H + 4)


def test_workspace_size_is_monotone_and_equals_the_header_formula():
    from finenvs_amd import _lib

    lib = _lib.load()
    counts = (0, 1, 31, 32, 33, 256, 511, 512, 513, 1023, 1024, 1025, 4097, 65536, 65537, 70001, 1 << 20, 1 << 24)
    for H in (32, 64, 128):
        for W in (1, 4, 7, 8, 16, 40, 64):
            sizes = [lib.fe_twin_mlpq_grad_workspace_floats(H, W, n) for n in counts]
            assert sizes == [_formula(H, W, n) for n in counts], (H, W)
            assert all(b >= a for a, b in zip(sizes, sizes[1:])), (H, W, sizes)
            assert sizes[0] == 0 < sizes[1]
            # the action's column never opens a feature tile (4W + 2 is no multiple of 32): the two-layer head's size
            assert sizes == [lib.fe_mlp2_grad_workspace_floats(H, W, n) for n in counts]
    for H, W, n in ((48, 4, 1), (16, 4, 1), (256, 4, 1), (32, 0, 1), (32, 4, -1)):
        assert lib.fe_twin_mlpq_grad_workspace_floats(H, W, n) == -1
    assert "3 * 32 blocks H   +   splits H (F + H + 32)   +   waves (H + 4)" in open(HEADER).read()
    assert "F = 32 ceil((4W + 3) / 32)" in open(HEADER).read()


def _load(module, gold, tag):
    sd = {k[len(tag) + 1:]: torch.from_numpy(v) for k, v in gold.items() if k.startswith(tag + ".")}
    assert sorted(sd) == sorted(module.state_dict())  # the reference's keys: network.0.*, network.2.*, network.4.*
    assert sorted(sd) == sorted(f"network.{i}.{k}" for i in (0, 2, 4) for k in ("weight", "bias"))
    module.load_state_dict(sd)
    return module


def _check_grads(gold, tag, module):
    named = dict(module.named_parameters())
    assert {k[len(tag) + 3:] for k in gold if k.startswith(f"g.{tag}.")} == set(named)
    for name, p in named.items():
        _close(p.grad.numpy(), gold[f"g.{tag}.{name}"], f"{tag} {name}")


def test_module_and_restatements_reproduce_the_reference_values_losses_targets_and_gradients():
    from finenvs_amd.critic import torch_td3_targets
    from finenvs_amd.mlp2_head import MLP2Head
    from finenvs_amd.mlp_critic import (MLPCritic, check_mlp_critic, mlp_critic_parameters, torch_mlp_critic_loss,
                                        torch_td3_actor_loss)

    gold = load_golden("mlp_critic.npz")
    B, W, H = (int(x) for x in gold["meta"])
    assert (B, W, H) == (80, 4, 32)
    col = lambda k: torch.from_numpy(gold[k])  # noqa: E731
    s, s_next = col("states"), col("next_states")
    assert tuple(s.shape) == tuple(s_next.shape) == (B, 5 * W) and s.dtype is torch.float32
    assert all(tuple(col(k).shape) == (B, 1) for k in ("actions", "rewards", "dones", "targets", "td3_eps", "q1", "q2"))
    for k, v in gold.items():  # weights on the 1 / 128 grid
        if ".network." in k and not k.startswith("g."):
            assert np.array_equal(np.round(v * 128.0), v * 128.0), k
    c1, c2 = _load(MLPCritic(H, W), gold, "c1"), _load(MLPCritic(H, W), gold, "c2")
    actor = _load(MLP2Head(H, W, "elu", "tanh"), gold, "actor")
    assert check_mlp_critic(c1) == (H, W, "elu")
    assert tuple(c1.network[0].weight.shape) == (H, 5 * W + 1)
    assert [id(p) for p in dict(c1.named_parameters()).values()] == [id(p) for p in mlp_critic_parameters(c1)]
    a = col("actions")
    q1, q2 = c1(s, a), c2(s, a)
    assert torch.equal(q1, c1(s.reshape(B, W, 5), a))  # (B, W, 5) and (B, 5W) are the same input
    _close(q1.detach().numpy(), gold["q1"], "q1")
    _close(q2.detach().numpy(), gold["q2"], "q2")
    # Critic.compute_loss once per critic: the sum's gradients are each critic's own
    y = col("targets")
    loss = torch_mlp_critic_loss(c1, c2, s, a, y)
    _close(float(loss.detach()), float(gold["loss.c1"]) + float(gold["loss.c2"]), "critic loss")
    loss.backward()
    _check_grads(gold, "c1", c1)
    _check_grads(gold, "c2", c2)
    # Actor.compute_loss(states, critic_1)
    c1.zero_grad()
    loss = torch_td3_actor_loss(actor, c1, s)
    _close(float(loss.detach()), gold["loss.actor"], "actor loss")
    loss.backward()
    _check_grads(gold, "actor", actor)
    _check_grads(gold, "actor_c1", c1)
    # TD3Agent.compute_targets with the recorded normals
    gamma, std, clip = (float(x) for x in gold["params"])
    y_td3 = torch_td3_targets(actor, c1, c2, col("rewards"), s_next, col("dones"), col("td3_eps"), gamma, std, clip)
    _close(y_td3.numpy(), gold["td3_targets"], "td3 targets")


def test_check_mlp_critic_accepts_and_refuses():
    import torch.nn as nn

    from finenvs_amd.mlp2_head import MLP2Head
    from finenvs_amd.mlp_critic import MLPCritic, check_mlp_critic

    for H in (32, 64, 128):
        for act in ("elu", "relu", "tanh"):
            assert check_mlp_critic(MLPCritic(H, 7, act)) == (H, 7, act)
    with pytest.raises(ValueError, match="activation must be one of"):
        MLPCritic(32, 4, "gelu")
    with pytest.raises(ValueError, match=r"states must be"):
        MLPCritic(32, 4)(torch.zeros(3, 5, 4), torch.zeros(3, 1))
    with pytest.raises(ValueError, match=r"actions must be"):
        MLPCritic(32, 4)(torch.zeros(3, 20), torch.zeros(3))

    def module(*layers):
        m = nn.Module()
        m.network = nn.Sequential(*layers)
        return m

    lin = nn.Linear
    bad = {
        "network = Sequential": module(lin(21, 32), nn.ELU(), lin(32, 1), nn.Identity()),
        "same width": module(lin(21, 32), nn.ELU(), lin(32, 64), nn.ELU(), lin(64, 1), nn.Identity()),
        "H in": module(lin(21, 48), nn.ELU(), lin(48, 48), nn.ELU(), lin(48, 1), nn.Identity()),
        r"in_features = 5 W \+ 1": MLP2Head(32, 4, "elu", "none"),
        "must be Linear": module(lin(21, 32), nn.ELU(), lin(32, 32), nn.ELU(), lin(32, 2), nn.Identity()),
        "need a bias": module(lin(21, 32), nn.ELU(), lin(32, 32, bias=False), nn.ELU(), lin(32, 1), nn.Identity()),
        "same activation": module(lin(21, 32), nn.ELU(), lin(32, 32), nn.ReLU(), lin(32, 1), nn.Identity()),
        "hidden activations": module(lin(21, 32), nn.ELU(), lin(32, 32), nn.GELU(), lin(32, 1), nn.Identity()),
        "must be Identity": module(lin(21, 32), nn.ELU(), lin(32, 32), nn.ELU(), lin(32, 1), nn.Tanh()),
    }
    for match, m in bad.items():
        with pytest.raises(ValueError, match=match):
            check_mlp_critic(m)
    with pytest.raises(ValueError, match="network = Sequential"):
        check_mlp_critic(nn.Linear(21, 1))


def test_td3_actor_loss_refuses_mixed_families_before_it_touches_anything():
    from types import SimpleNamespace

    from finenvs_amd.lstm_head import td3_actor_loss
    from finenvs_amd.mlp2_head import FusedMLP2Head
    from finenvs_amd.mlp_critic import FusedTwinMLPCritic

    plain = SimpleNamespace(cursor=None)
    head, twin = object.__new__(FusedMLP2Head), object.__new__(FusedTwinMLPCritic)
    head.env, twin.env = object(), object()
    with pytest.raises(ValueError, match="do not mix"):
        td3_actor_loss(head, plain, torch.zeros(1), SimpleNamespace(env=head.env))
    with pytest.raises(ValueError, match="do not mix"):
        td3_actor_loss(SimpleNamespace(env=twin.env), plain, torch.zeros(1), twin)
    with pytest.raises(ValueError, match="do not mix"):  # the same family on different envs
        td3_actor_loss(head, plain, torch.zeros(1), twin)
    with pytest.raises(ValueError, match="twin must be a FusedTwinCritic of this head's env"):
        td3_actor_loss(SimpleNamespace(env=None), plain, torch.zeros(1), object())
