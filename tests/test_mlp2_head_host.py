"""CPU: the two-hidden-layer MLP head -- the C ABI surface of include/finenvs_amd_mlp2_head.h with the argument checks
that need no device, the workspace size against the formula the header states, and the repository's MLP2Head + the torch
bodies of the PPO actor and critic losses against the reference's own outputs, losses and gradients
(tests/golden/mlp2_head.npz, written by tools/make_mlp2_golden.py from the reference's ContinuousActorMLP / CriticMLP
of shape (5W, H, H, 1), compute_actor_loss / compute_critic_loss and their backward())."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests.helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "finenvs_amd_mlp2_head.h")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_exactly_the_mlp2_head_signatures_and_the_library_exports_them():
    from finenvs_amd import _lib

    assert sorted(set(re.findall(r"\b(fe_[a-z0-9_]+)\s*\(", _header()))) == sorted(_lib.MLP2_HEAD_SIGNATURES)
    others = set()
    for name in dir(_lib):
        if name.endswith("SIGNATURES") and name != "MLP2_HEAD_SIGNATURES":
            others |= set(getattr(_lib, name))
    assert len(others) > 50 and not set(_lib.MLP2_HEAD_SIGNATURES) & others
    lib = _lib.load()
    for name, (_, args) in _lib.MLP2_HEAD_SIGNATURES.items():
        assert hasattr(lib, name)
        decl = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", _header(), flags=re.S).group(1)
        assert len(decl.split(",")) == len(args), name  # one binding argument per declared parameter


def test_struct_fields_chunk_size_and_window_limits_match_the_binding():
    from finenvs_amd import _lib
    from finenvs_amd.mlp2_head import MLP2_GRAD_CHUNK_PAIRS, MLP2_GRAD_KEYS, MLP2_MAX_WINDOW

    text = _header()
    fields = re.search(r"typedef struct fe_mlp2_grads \{(.*?)\} fe_mlp2_grads;", text, flags=re.S).group(1)
    assert re.findall(r"\*(\w+);", fields) == [f for f, _ in _lib.FeMlp2Grads._fields_] == list(MLP2_GRAD_KEYS)
    fields = re.search(r"typedef struct fe_mlp2_weights \{(.*?)\} fe_mlp2_weights;", text, flags=re.S).group(1)
    assert re.findall(r"\*(\w+);", fields) == [f for f, _ in _lib.FeMlp2Weights._fields_]
    assert int(re.search(r"#define FE_MLP2_GRAD_CHUNK_PAIRS (\d+)", text).group(1)) == MLP2_GRAD_CHUNK_PAIRS == 512
    limits = {int(h): int(w) for h, w in re.findall(r"#define FE_MLP2_MAX_WINDOW_H(\d+) (\d+)", text)}
    assert limits == MLP2_MAX_WINDOW == {32: 296, 64: 128, 128: 40}
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for H, W in limits.items():  # the header's comment and DESIGN.md state the same limits
        assert f"H = {H}: W <= {W}" in open(HEADER).read() and f"H = {H}: W <= {W}" in design, (H, W)


def _weights(**null):
    from finenvs_amd import _lib

    p = {k: 16 for k, _ in _lib.FeMlp2Weights._fields_}
    p.update(null)
    return _lib.FeMlp2Weights(*(p[k] for k, _ in _lib.FeMlp2Weights._fields_))


# made-up non-null pointers, never dereferenced: every case here is refused first
def _backward(lib, H=32, act=0, out_act=0, count=4, weights="ok", grads="ok", **null):
    from finenvs_amd import _lib

    p = {k: 16 for k in ("env", "lr32", "src", "pos", "outputs", "d_outputs", "workspace")}
    p.update(null)
    w = _weights() if weights == "ok" else weights
    g = _lib.FeMlp2Grads(*([16] * 6)) if grads == "ok" else grads
    return lib.fe_mlp2_backward(p["env"], p["lr32"], None if w is None else C.byref(w), H, act, out_act, p["src"], p["pos"], count,
                                p["outputs"], p["d_outputs"], p["workspace"], None if g is None else C.byref(g), None)


def _forward(lib, H=32, act=0, out_act=0, count=4, weights="ok", **null):
    p = {k: 16 for k in ("env", "lr32", "src", "pos", "out")}
    p.update(null)
    w = _weights() if weights == "ok" else weights
    return lib.fe_mlp2_forward(p["env"], p["lr32"], None if w is None else C.byref(w), H, act, out_act, p["src"], p["pos"], count,
                               p["out"], None)


def _sampled(lib, H=32, act=0, out_act=0, K=2, weights="ok", std=0.5, **null):
    p = {k: 16 for k in ("env", "lr32", "src", "pos", "noise", "actions", "means", "rewards", "dones", "ssrc", "spos")}
    p.update(null)
    w = _weights() if weights == "ok" else weights
    return lib.fe_env_rollout_mlp2_sampled(p["env"], p["lr32"], None if w is None else C.byref(w), H, act, out_act, K, p["src"],
                                           p["pos"], p["noise"], std, p["actions"], p["means"], p["rewards"], p["dones"],
                                           p["ssrc"], p["spos"], None)


def test_argument_checks_need_no_device():
    from finenvs_amd import _lib

    lib = _lib.load()
    ERR = _lib.FE_ERR_ARG
    calls = {"fe_mlp2_backward": (_backward, ("env", "lr32", "src", "pos", "d_outputs", "workspace")),
             "fe_mlp2_forward": (_forward, ("env", "lr32", "src", "pos", "out")),
             "fe_env_rollout_mlp2_sampled": (_sampled, ("env", "lr32", "src", "pos", "rewards", "dones"))}
    for name, (call, required) in calls.items():
        who = name.encode()
        for ptr in required:
            assert call(lib, **{ptr: None}) == ERR, (name, ptr)
            assert who + b": bad argument" in lib.fe_last_error(), (name, ptr)
        assert call(lib, weights=None) == ERR and who + b": bad argument" in lib.fe_last_error()
        for field, _ in _lib.FeMlp2Weights._fields_:  # every field of fe_mlp2_weights is required, b3 included
            assert call(lib, weights=_weights(**{field: None})) == ERR, (name, field)
            assert who + b": bad argument" in lib.fe_last_error()
        for H in (16, 48, 256):
            assert call(lib, H=H) == ERR
            assert who + b": H must be 32, 64 or 128" in lib.fe_last_error()
        for act in (-1, 3):
            assert call(lib, act=act) == ERR
            assert who + b": activation must be 0 (ELU), 1 (ReLU) or 2 (tanh)" in lib.fe_last_error()
        for out_act in (-1, 3):
            assert call(lib, out_act=out_act) == ERR
            assert who + b": out_activation must be" in lib.fe_last_error()
    for call, who in ((_backward, b"fe_mlp2_backward"), (_forward, b"fe_mlp2_forward")):
        assert call(lib, count=-1) == ERR and who + b": bad argument" in lib.fe_last_error()
    # the backward alone: the gradient struct and its fields, the clamp, the tanh output without its values
    assert _backward(lib, grads=None) == ERR and b"fe_mlp2_backward: bad argument" in lib.fe_last_error()
    for k in range(6):
        ptrs = [16] * 6
        ptrs[k] = None
        assert _backward(lib, grads=_lib.FeMlp2Grads(*ptrs)) == ERR, k
        assert b"fe_mlp2_backward: bad argument" in lib.fe_last_error()
    assert _backward(lib, out_act=1) == ERR  # clamp has no gradient to train on
    assert b"fe_mlp2_backward: out_activation must be 0 (tanh) or 2 (none)" in lib.fe_last_error()
    assert _backward(lib, out_act=0, outputs=None) == ERR
    msg = lib.fe_last_error()
    assert b"fe_mlp2_backward" in msg and b"needs outputs" in msg, msg
    # the sampled rollout alone: the two descriptor outputs go together, K, std
    for kw in (dict(ssrc=None), dict(spos=None)):
        assert _sampled(lib, **kw) == ERR
        assert b"fe_env_rollout_mlp2_sampled: states_src_out and states_pos_out go together" in lib.fe_last_error()
    assert _sampled(lib, K=0) == ERR and b"fe_env_rollout_mlp2_sampled: bad argument" in lib.fe_last_error()
    for std in (-0.5, float("nan")):
        assert _sampled(lib, std=std) == ERR and b"fe_env_rollout_mlp2_sampled: std must be >= 0" in lib.fe_last_error()


# one refusal each, and pairs of refusals that apply at once: which one wins is the order of the checks
_REFUSED = {
    "backward": [dict(src=None), dict(lr32=None), dict(env=None), dict(weights=None), dict(grads=None), dict(count=-1),
                 dict(H=48), dict(act=3), dict(out_act=-1), dict(out_act=1), dict(out_act=0, outputs=None),
                 dict(workspace=None, H=48), dict(H=48, act=3), dict(act=3, out_act=3), dict(H=16, out_act=1),
                 dict(out_act=1, outputs=None)],
    "forward": [dict(out=None), dict(env=None), dict(weights=None), dict(count=-1), dict(H=256), dict(act=-1), dict(out_act=3),
                dict(count=-1, H=48), dict(H=48, act=3), dict(act=3, out_act=3)],
    "sampled": [dict(ssrc=None), dict(spos=None), dict(std=-0.5), dict(K=0), dict(rewards=None), dict(env=None),
                dict(weights=None), dict(H=48), dict(act=3), dict(out_act=3), dict(ssrc=None, std=-0.5), dict(std=-0.5, K=0),
                dict(K=0, H=48), dict(dones=None, weights=None), dict(H=48, act=3)],
}


@pytest.mark.parametrize("entry", sorted(_REFUSED))
def test_both_depths_refuse_alike(entry):
    """The one- and two-hidden-layer entries share their host path: the same arguments get the same return code and the
    same message, apart from the entry's name (and the forward entry a message names)."""
    from finenvs_amd import _lib
    from tests import test_mlp_head_host as one

    lib = _lib.load()
    for kw in _REFUSED[entry]:
        rc1 = getattr(one, "_" + entry)(lib, **kw)
        msg1 = lib.fe_last_error()
        rc2 = globals()["_" + entry](lib, **kw)
        msg2 = lib.fe_last_error()
        assert rc1 == rc2 == _lib.FE_ERR_ARG, kw
        assert msg1 and msg2.replace(b"mlp2", b"mlp") == msg1, (kw, msg1, msg2)


def _formula(H, W, count):
    """The workspace size as include/finenvs_amd_mlp2_head.h states it."""
    if count == 0:
        return 0
    blocks, splits, F = -(-count // 32), -(-count // 512), 32 * -(-(4 * W + 2) // 32)
    waves = 4 * min(-(-blocks // 4), 512)
    return 3 * 32 * blocks * H + splits * H * (F + H + 32) + waves * (H + 4)


def test_workspace_size_is_monotone_and_equals_the_header_formula():
    from finenvs_amd import _lib

    lib = _lib.load()
    # both sides of a block (32), of a chunk (512, 1024) and of the first kernel's workgroup cap (4 * 512 blocks)
    counts = (0, 1, 31, 32, 33, 256, 511, 512, 513, 1023, 1024, 1025, 4097, 65536, 65537, 70001, 1 << 20, 1 << 24)
    for H in (32, 64, 128):
        for W in (1, 4, 7, 8, 16, 40, 64):
            sizes = [lib.fe_mlp2_grad_workspace_floats(H, W, n) for n in counts]
            assert sizes == [_formula(H, W, n) for n in counts], (H, W)
            assert all(b >= a for a, b in zip(sizes, sizes[1:])), (H, W, sizes)
            assert sizes[0] == 0 < sizes[1]
        assert lib.fe_mlp2_grad_workspace_floats(H, 16, 1000) > lib.fe_mlp2_grad_workspace_floats(H, 4, 1000)
        assert lib.fe_mlp2_grad_workspace_floats(H, 4, 1000) > lib.fe_mlp_grad_workspace_floats(H, 4, 1000)
    for H, W, n in ((48, 4, 1), (16, 4, 1), (256, 4, 1), (32, 0, 1), (32, 4, -1)):
        assert lib.fe_mlp2_grad_workspace_floats(H, W, n) == -1
    assert "3 * 32 blocks H   +   splits H (F + H + 32)   +   waves (H + 4)" in open(HEADER).read()


def _head(gold, tag, H, W, activation):
    from finenvs_amd.mlp2_head import MLP2Head

    head = MLP2Head(H, W, "elu", activation)
    sd = {k[len(tag) + 1:]: torch.from_numpy(v) for k, v in gold.items() if k.startswith(tag + ".")}
    sd.pop("log_standard_deviation", None)  # the PPO learner's own parameter, not the network's
    assert sorted(sd) == sorted(head.state_dict())  # the reference's keys: network.0.*, network.2.*, network.4.*
    assert sorted(sd) == sorted(f"network.{i}.{k}" for i in (0, 2, 4) for k in ("weight", "bias"))
    head.load_state_dict(sd)
    return head


def _close(a, ref, what):
    """1e-6 relative to the largest reference element: the same torch arithmetic on the same machine class."""
    ref = np.asarray(ref, dtype=np.float64)
    scale = float(np.abs(ref).max())
    assert scale > 0, what
    assert float(np.abs(np.asarray(a, dtype=np.float64) - ref).max()) <= 1e-6 * scale, what


def _check(gold, tag, out, loss, named):
    _close(out.detach().numpy(), gold[f"out.{tag}"], f"{tag} output")
    _close(float(loss.detach()), gold[f"loss.{tag}"], f"{tag} loss")
    loss.backward()
    assert {k[len(tag) + 3:] for k in gold if k.startswith(f"g.{tag}.")} == set(named)
    for name, p in named.items():
        _close(p.grad.numpy(), gold[f"g.{tag}.{name}"], f"{tag} {name}")


def test_head_and_losses_reproduce_the_reference_outputs_losses_and_gradients():
    from finenvs_amd.lstm_head import torch_ppo_actor_loss, torch_ppo_critic_loss
    from finenvs_amd.mlp2_head import check_mlp2_head, mlp2_head_parameters

    gold = load_golden("mlp2_head.npz")
    B, W, H = (int(x) for x in gold["meta"])
    assert (B, W, H) == (80, 4, 32)
    s = torch.from_numpy(gold["states"])
    assert tuple(s.shape) == (B, 5 * W) and s.dtype is torch.float32
    window = s.reshape(B, W, 5)
    assert bool((window[:, :, 4] == window[:, :1, 4]).all())  # the position feature is constant over the window
    column = lambda k: torch.from_numpy(gold[k])  # noqa: E731
    assert all(tuple(column(k).shape) == (B, 1) for k in ("actions", "old_log_probs", "advantages", "returns"))
    for tag in ("ppo_actor", "ppo_critic"):  # weights on the 1 / 128 grid
        for k, v in gold.items():
            if k.startswith(tag + ".network."):
                assert np.array_equal(np.round(v * 128.0), v * 128.0), k

    actor = _head(gold, "ppo_actor", H, W, "tanh")  # PPO/continuous_actor.py:59-78
    assert check_mlp2_head(actor) == (H, W, "elu", "tanh")
    log_std = torch.nn.Parameter(torch.from_numpy(gold["ppo_actor.log_standard_deviation"]).clone())
    out = actor(s)
    assert torch.equal(out, actor(window))  # (B, W, 5) and (B, 5W) are the same input
    loss = torch_ppo_actor_loss(out, log_std, column("actions"), column("old_log_probs"), column("advantages"),
                                float(gold["clip_epsilon"]), float(gold["entropy_coefficient"]))
    named = dict(actor.named_parameters())
    assert len(named) == 6 and [id(p) for p in named.values()] == [id(p) for p in mlp2_head_parameters(actor)]
    _check(gold, "ppo_actor", out, loss, {**named, "log_standard_deviation": log_std})

    critic = _head(gold, "ppo_critic", H, W, "none")  # PPO/critic.py:26-32
    assert check_mlp2_head(critic) == (H, W, "elu", "none")
    out = critic(s)
    _check(gold, "ppo_critic", out, torch_ppo_critic_loss(out, column("returns")), dict(critic.named_parameters()))


def test_check_mlp2_head_accepts_and_refuses():
    import torch.nn as nn

    from finenvs_amd.mlp2_head import MLP2Head, check_mlp2_head
    from finenvs_amd.mlp_head import MLPHead, check_mlp_head

    for H in (32, 64, 128):
        for act in ("elu", "relu", "tanh"):
            for out in ("tanh", "none"):
                assert check_mlp2_head(MLP2Head(H, 7, act, out)) == (H, 7, act, out)
    with pytest.raises(ValueError, match="output_activation"):
        MLP2Head(32, 4, "elu", "clamp")
    with pytest.raises(ValueError, match="activation must be one of"):
        MLP2Head(32, 4, "gelu")
    with pytest.raises(ValueError, match=r"states must be"):
        MLP2Head(32, 4)(torch.zeros(3, 5, 4))

    def module(*layers):
        m = nn.Module()
        m.network = nn.Sequential(*layers)
        return m

    lin = nn.Linear
    bad = {
        "two hidden layers": MLPHead(32, 4),
        "same width": module(lin(20, 32), nn.ELU(), lin(32, 64), nn.ELU(), lin(64, 1), nn.Tanh()),
        "H in": module(lin(20, 48), nn.ELU(), lin(48, 48), nn.ELU(), lin(48, 1), nn.Tanh()),
        "in_features = 5 W": module(lin(18, 32), nn.ELU(), lin(32, 32), nn.ELU(), lin(32, 1), nn.Tanh()),
        "one output": module(lin(20, 32), nn.ELU(), lin(32, 32), nn.ELU(), lin(32, 2), nn.Tanh()),
        "need a bias": module(lin(20, 32), nn.ELU(), lin(32, 32, bias=False), nn.ELU(), lin(32, 1), nn.Tanh()),
        "same activation": module(lin(20, 32), nn.ELU(), lin(32, 32), nn.ReLU(), lin(32, 1), nn.Tanh()),
        "hidden activations": module(lin(20, 32), nn.ELU(), lin(32, 32), nn.GELU(), lin(32, 1), nn.Tanh()),
        "alpha = 1": module(lin(20, 32), nn.ELU(), lin(32, 32), nn.ELU(alpha=0.5), lin(32, 1), nn.Tanh()),
        "output activation must be Tanh or Identity": module(lin(20, 32), nn.ELU(), lin(32, 32), nn.ELU(), lin(32, 1), nn.Hardtanh()),
    }
    for match, m in bad.items():
        with pytest.raises(ValueError, match=match):
            check_mlp2_head(m)
    with pytest.raises(ValueError, match="network = Sequential"):
        check_mlp2_head(nn.Linear(20, 1))
    with pytest.raises(ValueError, match="one hidden layer"):  # the one-layer head keeps refusing the deeper module
        check_mlp_head(MLP2Head(32, 4))
