"""CPU: the gradient half of the twin LSTM critics -- the C ABI surface of include/finenvs_amd_critic_grad.h with the
argument checks that need no device, the workspace size, the un-permutation of the kernel's packed gradient rows, and
the repository's CriticLSTM + MSE against the reference's own gradients (tests/golden/critic_grads.npz, written by
tools/make_critic_grad_golden.py from the reference's CriticLSTM.compute_loss(...).backward())."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_exactly_the_critic_grad_signatures_and_the_library_exports_them():
    from finenvs_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "finenvs_amd_critic_grad.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(fe_[a-z0-9_]+)\s*\(", text))) == sorted(_lib.CRITIC_GRAD_SIGNATURES)
    others = (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.EVO_SIGNATURES) | set(_lib.REPLAY_SIGNATURES)
              | set(_lib.SAC_SIGNATURES) | set(_lib.CRITIC_SIGNATURES))
    assert not set(_lib.CRITIC_GRAD_SIGNATURES) & others
    lib = _lib.load()
    for name in _lib.CRITIC_GRAD_SIGNATURES:
        assert hasattr(lib, name)
    fields = re.search(r"typedef struct fe_critic_grads \{(.*?)\} fe_critic_grads;", text, flags=re.S).group(1)
    assert re.findall(r"\*(\w+);", fields) == [f for f, _ in _lib.FeCriticGrads._fields_]


def _backward(lib, env=16, H=32, count=4, dq1=16, dq2=16, g1=True, g2=True, w2=None, d_actions=16, workspace=16,
              src=16):
    from finenvs_amd import _lib

    w = _lib.FeCriticWeights(16, 16, 16, 16)
    g = _lib.FeCriticGrads(16, 16, 16, 16, 16, 16)
    return lib.fe_twin_q_backward(env, 16, C.byref(w), C.byref(w2 or w), H, src, 16, 16, count, dq1, dq2, workspace,
                                  C.byref(g) if g1 else None, C.byref(g) if g2 else None, d_actions, None)


def test_argument_checks_need_no_device():
    from finenvs_amd import _lib

    lib = _lib.load()
    for kw in (dict(env=None), dict(src=None), dict(workspace=None), dict(count=-1),
               dict(w2=_lib.FeCriticWeights(16, 16, 16, None)), dict(g1=False, d_actions=None)):
        assert _backward(lib, **kw) == _lib.FE_ERR_ARG, kw
        assert b"fe_twin_q_backward: bad argument" in lib.fe_last_error()
    bad = _lib.FeCriticGrads(16, 16, 16, None, 16, 16)  # b_hh missing
    w = _lib.FeCriticWeights(16, 16, 16, 16)
    assert lib.fe_twin_q_backward(16, 16, C.byref(w), C.byref(w), 32, 16, 16, 16, 4, 16, None, 16, C.byref(bad), None,
                                  None, None) == _lib.FE_ERR_ARG
    for H in (16, 48, 256):
        assert _backward(lib, H=H) == _lib.FE_ERR_ARG
        assert b"fe_twin_q_backward: H must be 32, 64 or 128" in lib.fe_last_error()
    # a critic without dq needs neither weights nor gradients: only the argument checks above can refuse
    assert _backward(lib, dq2=None, g2=False, w2=_lib.FeCriticWeights(16, 16, 16, None), H=48) == _lib.FE_ERR_ARG
    assert b"H must be" in lib.fe_last_error()


def test_workspace_size_is_monotone_and_bounded():
    from finenvs_amd import _lib

    lib = _lib.load()
    for H in (32, 64, 128):
        for W in (4, 16):
            sizes = [lib.fe_twin_q_grad_workspace_floats(H, W, n) for n in
                     (0, 1, 31, 32, 33, 256, 4097, 65536, 1 << 20, 1 << 24)]
            assert all(b >= a for a, b in zip(sizes, sizes[1:])), (H, W, sizes)
            assert sizes[1] > sizes[0] > 0
            # beyond the resident workgroup count only the per-pair action gradients grow
            assert sizes[-1] - sizes[-2] == 2 * ((1 << 24) - (1 << 20))
        assert lib.fe_twin_q_grad_workspace_floats(H, 16, 1000) > lib.fe_twin_q_grad_workspace_floats(H, 4, 1000)
    for H, W, n in ((48, 4, 1), (32, 0, 1), (32, 4, -1)):
        assert lib.fe_twin_q_grad_workspace_floats(H, W, n) == -1


@pytest.mark.parametrize("H", [32, 64, 128])
def test_gradient_unpermutation_round_trips(H):
    from finenvs_amd.critic import CriticLSTM, critic_parameters, packed_grads_to_torch, torch_grads_to_packed
    from finenvs_amd.rollout import lstm_row_order

    torch.manual_seed(H)
    shapes = [tuple(p.shape) for p in critic_parameters(CriticLSTM(H, 4))]
    keys = ("w_ih", "w_hh", "b_ih", "b_hh", "w_out", "b_out")
    g = {k: torch.randn(s) for k, s in zip(keys, shapes)}
    packed = torch_grads_to_packed(g, H)
    order = lstm_row_order(H)
    assert torch.equal(packed["w_hh"], g["w_hh"][order]) and torch.equal(packed["b_ih"], g["b_ih"][order])
    assert tuple(packed["w_out"].shape) == (H,) and tuple(packed["b_out"].shape) == (1,)
    back = packed_grads_to_torch(packed, H)
    for k, s in zip(keys, shapes):
        assert tuple(back[k].shape) == s and torch.equal(back[k], g[k]), k


def test_critic_and_mse_reproduce_the_reference_gradients():
    from finenvs_amd.critic import CriticLSTM

    gold = load_golden("critic_grads.npz")
    B, W, H = (int(x) for x in gold["meta"])
    s, a, y = (torch.from_numpy(gold[k]) for k in ("states", "actions", "targets"))
    a = a.clone().requires_grad_()
    for c, tag in ((1, "c1"), (2, "c2")):
        net = CriticLSTM(H, W)
        net.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in gold.items() if k.startswith(tag + ".")})
        loss = F.mse_loss(net(s, a), y)
        loss.backward()
        assert abs(float(loss.detach()) - float(gold[f"loss{c}"])) <= 1e-6
        for name, p in net.named_parameters():
            ref = gold[f"g{c}.{name}"]
            assert np.abs(ref).max() > 0, name
            np.testing.assert_allclose(p.grad.numpy(), ref, rtol=0, atol=1e-6, err_msg=name)
    np.testing.assert_allclose(a.grad.numpy(), gold["d_actions"], rtol=0, atol=1e-6)
