"""CPU: the gradient half of the SAC LSTM actor -- the C ABI surface of include/finenvs_amd_sac_grad.h with the argument
checks that need no device, the workspace size, and the repository's SACActorLSTM + CriticLSTM + the actor loss against
the reference's own gradients (tests/golden/sac_actor_grads.npz, written by tools/make_sac_grad_golden.py from the
reference's ActorLSTM.compute_losses(...) and its backward())."""
import ctypes as C
import os
import re

import numpy as np
import torch

from tests.helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_exactly_the_sac_grad_signatures_and_the_library_exports_them():
    from finenvs_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "finenvs_amd_sac_grad.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(fe_[a-z0-9_]+)\s*\(", text))) == sorted(_lib.SAC_GRAD_SIGNATURES)
    others = (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.EVO_SIGNATURES) | set(_lib.REPLAY_SIGNATURES)
              | set(_lib.SAC_SIGNATURES) | set(_lib.CRITIC_SIGNATURES) | set(_lib.CRITIC_GRAD_SIGNATURES))
    assert not set(_lib.SAC_GRAD_SIGNATURES) & others
    lib = _lib.load()
    for name in _lib.SAC_GRAD_SIGNATURES:
        assert hasattr(lib, name)
    assert lib.fe_version() == _lib.FE_ABI_VERSION == 5


def test_struct_fields_match_the_binding():
    from finenvs_amd import _lib
    from finenvs_amd.sac import SAC_GRAD_KEYS

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "finenvs_amd_sac_grad.h")).read(), flags=re.S)
    fields = re.search(r"typedef struct fe_sac_grads \{(.*?)\} fe_sac_grads;", text, flags=re.S).group(1)
    assert re.findall(r"\*(\w+);", fields) == [f for f, _ in _lib.FeSacGrads._fields_] == list(SAC_GRAD_KEYS)


def _backward(lib, env=16, H=32, count=4, src=16, d_actions=16, d_log_probs=16, workspace=16, grads="ok"):
    from finenvs_amd import _lib

    g = _lib.FeSacGrads(*([16] * 10)) if grads == "ok" else grads
    return lib.fe_sac_backward(env, 16, 16, 16, 16, 16, 16, 0.0, 16, 0.0, H, src, 16, count, 16, 16, 16, d_actions,
                               d_log_probs, workspace, None if g is None else C.byref(g), None)


def test_argument_checks_need_no_device():
    from finenvs_amd import _lib

    lib = _lib.load()
    for kw in (dict(env=None), dict(src=None), dict(workspace=None), dict(grads=None), dict(count=-1),
               dict(d_actions=None, d_log_probs=None)):
        assert _backward(lib, **kw) == _lib.FE_ERR_ARG, kw
        assert b"fe_sac_backward: bad argument" in lib.fe_last_error()
    for k in range(10):  # every field of fe_sac_grads is required
        ptrs = [16] * 10
        ptrs[k] = None
        assert _backward(lib, grads=_lib.FeSacGrads(*ptrs)) == _lib.FE_ERR_ARG, k
        assert b"fe_sac_backward: bad argument" in lib.fe_last_error()
    for H in (16, 48, 256):
        assert _backward(lib, H=H) == _lib.FE_ERR_ARG
        assert b"fe_sac_backward: H must be 32, 64 or 128" in lib.fe_last_error()


def test_workspace_size_is_monotone_and_bounded():
    from finenvs_amd import _lib

    lib = _lib.load()
    per_pair = 0  # the O(count) term include/finenvs_amd_sac_grad.h documents: no per-pair output leaves the kernel
    for H in (32, 64, 128):
        for W in (4, 16):
            sizes = [lib.fe_sac_grad_workspace_floats(H, W, n) for n in
                     (0, 1, 31, 32, 33, 256, 4097, 65536, 1 << 20, 1 << 24)]
            assert all(b >= a for a, b in zip(sizes, sizes[1:])), (H, W, sizes)
            assert sizes[1] > sizes[0] > 0
            assert sizes[-1] - sizes[-2] == per_pair * ((1 << 24) - (1 << 20))
        assert lib.fe_sac_grad_workspace_floats(H, 16, 1000) > lib.fe_sac_grad_workspace_floats(H, 4, 1000)
    for H, W, n in ((48, 4, 1), (16, 4, 1), (256, 4, 1), (32, 0, 1), (32, 4, -1)):
        assert lib.fe_sac_grad_workspace_floats(H, W, n) == -1
    text = open(os.path.join(ROOT, "include", "finenvs_amd_sac_grad.h")).read()
    assert "per-pair term is 0 floats" in text


def test_actor_and_loss_reproduce_the_reference_gradients():
    from finenvs_amd.critic import CriticLSTM
    from finenvs_amd.sac import SACActorLSTM, actor_parameters

    gold = load_golden("sac_actor_grads.npz")
    B, W, H = (int(x) for x in gold["meta"])
    s, eps = torch.from_numpy(gold["states"]), torch.from_numpy(gold["eps"])
    assert tuple(s.shape) == (B, W, 5) and tuple(eps.shape) == (B, 1)
    actor = SACActorLSTM(H, W)
    actor.load_state_dict({k[6:]: torch.from_numpy(v) for k, v in gold.items() if k.startswith("actor.")})
    with torch.no_grad():
        actor.log_alpha.copy_(torch.tensor(float(gold["log_alpha"])))
    assert actor.target_entropy == float(gold["target_entropy"])
    critics = []
    for tag in ("c1", "c2"):
        c = CriticLSTM(H, W)
        c.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in gold.items() if k.startswith(tag + ".")})
        critics.append(c)
    actions, log_probs = actor.get_actions_and_log_probs(s, eps)
    mean_lp = log_probs.mean(dim=1, keepdim=True)
    q = torch.min(critics[0](s, actions), critics[1](s, actions))
    loss = -(q + -actor.log_alpha.exp() * mean_lp).mean()  # SAC/actor.py:63-81
    alpha_loss = (-actor.log_alpha.exp() * (mean_lp + actor.target_entropy).detach()).mean()
    loss.backward()
    assert abs(float(loss.detach()) - float(gold["loss"])) <= 1e-6
    assert abs(float(alpha_loss.detach()) - float(gold["alpha_loss"])) <= 1e-6
    named = dict(actor.named_parameters())
    assert len(named) == 10 and {id(p) for p in named.values()} == {id(p) for p in actor_parameters(actor)}
    for name, p in named.items():
        ref = gold[f"g.{name}"]
        assert np.abs(ref).max() > 0, name
        np.testing.assert_allclose(p.grad.numpy(), ref, rtol=0, atol=1e-6, err_msg=name)
