"""CPU: the host side of finenvs_amd/optim.py (FusedAdam, fe_net_update of include/finenvs_amd_optim.h).

* the packed-destination maps the kernel restates: scattering a module's parameters through them, from NaN-filled
  buffers, equals ``lstm_pack`` / ``pack_critic_weights`` / ``pack_sac_weights`` / ``lstm_fragment_major`` bit for bit
  (H = 32, 64, 128 for the head, the critic and the SAC actor; H = 256 for the head's fragment-major ``whh``);
* ``reference_update`` -- the element-wise contract in separate f32 torch operations -- against
  ``torch.optim.Adam(foreach=False)`` and an f64 Adam over five steps with gradients scaled from 1e-3 to 10:
  ``max|p_ref - p64| <= 4 max|p_torch32 - p64|``, the project's margin in the gradient tests.  Measured here: the two
  distances are equal at every step (5.9e-8 to 1.2e-7 at |p| <= 1), 99.6-99.9 % of the elements bit-equal to torch;
* the running products ``b^t`` against ``b ** t``; the soft update against the examples' ``soft_update``;
* the new header's symbols are exported and bound; null and bad arguments are FE_ERR_ARG without a GPU.
"""
import ctypes as C
import os
import re

import pytest
import torch

from finenvs_amd import _lib, optim
from finenvs_amd.critic import CriticLSTM, pack_critic_weights
from finenvs_amd.lstm_head import LSTMHead
from finenvs_amd.rollout import lstm_fragment_major, lstm_pack
from finenvs_amd.sac import SACActorLSTM, pack_sac_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "finenvs_amd_optim.h")


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype is b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _pack_head(m):
    H = m.lstm.hidden_size
    whh, wx = lstm_pack(m.lstm.weight_ih_l0, m.lstm.weight_hh_l0, m.lstm.bias_ih_l0, m.lstm.bias_hh_l0, H)
    if H > 128:
        whh = lstm_fragment_major(whh, H)
    last = m.last_layer[0]
    return {"whh": whh, "wx": wx, "wout": last.weight.detach().reshape(H).clone(), "bout": last.bias.detach().reshape(1).clone()}


CASES = [("head", H) for H in (32, 64, 128, 256)] + [(k, H) for k in ("critic", "actor") for H in (32, 64, 128)]


@pytest.mark.parametrize("kind,H", CASES)
def test_destination_maps_equal_the_python_packers(kind, H):
    torch.manual_seed(H)
    module, packer = {"head": (LSTMHead(H, 4), _pack_head), "critic": (CriticLSTM(H, 4), pack_critic_weights),
                      "actor": (SACActorLSTM(H, 4), pack_sac_weights)}[kind]
    assert optim.network_kind(module) == (kind, H)
    want, got = packer(module), optim.scatter_packed(module)
    assert set(want) == set(got)
    for k in want:
        assert not bool(torch.isnan(got[k]).any()), f"{k}: a destination nobody writes"
        assert _same_bits(got[k], want[k].detach()), k
    # every destination of a buffer is written exactly once
    _, _, segs, shapes = optim.network_segments(module)
    for name, shape in shapes.items():
        dests = [optim.packed_destinations(s.kind, s.H, s.cols, s.numel) for s in segs if s.dest == name]
        dests += [optim.bias_pair_zero_destinations(H, s.cols) for s in segs if s.dest == name and s.kind == optim.SEG_BIAS_PAIR]
        d = torch.cat(dests)
        n = int(torch.tensor(shape).prod())
        assert d.numel() == n and torch.equal(d.sort().values, torch.arange(n)), name


def _adam64(p, g, m, v, t, lr, b1, b2, eps):
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    denom = v.sqrt() / (1 - b2 ** t) ** 0.5 + eps
    p.addcdiv_(m, denom, value=-lr / (1 - b1 ** t))


def test_reference_update_is_as_close_to_f64_adam_as_torch_is():
    torch.manual_seed(0)
    lr, (b1, b2), eps = 3e-4, (0.9, 0.999), 1e-8
    shapes = [(512, 128), (128, 5), (512,), (1, 128), (1,), ()]
    scales = [1e-3, 1e-2, 0.1, 1.0, 10.0, 1.0]
    p0 = [torch.rand(s) * 2 - 1 for s in shapes]
    ref = [p.clone() for p in p0]
    m = [torch.zeros_like(p) for p in p0]
    v = [torch.zeros_like(p) for p in p0]
    t32 = [p.clone().requires_grad_(True) for p in p0]
    adam = torch.optim.Adam(t32, lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    p64 = [p.double() for p in p0]
    m64 = [torch.zeros_like(p) for p in p64]
    v64 = [torch.zeros_like(p) for p in p64]
    state = optim.initial_state()
    for t in range(1, 6):
        grads = [torch.randn(s) * sc for s, sc in zip(shapes, scales)]
        state = optim.reference_update(ref, [g.clone() for g in grads], m, v, state, lr, (b1, b2), eps)
        for p, g in zip(t32, grads):
            p.grad = g.clone()
        adam.step()
        for p, g, mm, vv in zip(p64, grads, m64, v64):
            _adam64(p, g.double(), mm, vv, t, lr, b1, b2, eps)
        e_ref = max(float((a.double() - b).abs().max()) for a, b in zip(ref, p64))
        e_t32 = max(float((a.detach().double() - b).abs().max()) for a, b in zip(t32, p64))
        same = sum(int((a.view(torch.int32) == b.detach().view(torch.int32)).sum()) for a, b in zip(ref, t32))
        total = sum(a.numel() for a in ref)
        print(f"step {t}: |ref - f64| {e_ref:.3e}  |torch32 - f64| {e_t32:.3e}  bit-equal {100.0 * same / total:.1f} %")
        assert e_t32 > 0
        assert e_ref <= 4 * e_t32, (t, e_ref, e_t32)
    assert state["step"] == 5


def test_running_products_stay_with_pow():
    state = optim.initial_state()
    p = [torch.zeros(1)]
    for _ in range(2000):
        state = optim.reference_update(p, [torch.ones(1)], [torch.zeros(1)], [torch.zeros(1)], state, 1e-3)
    assert abs(state["beta2_pow"] / 0.999 ** 2000 - 1) < 1e-12 and abs(state["beta1_pow"] / 0.9 ** 2000 - 1) < 1e-12


def test_reference_soft_update_is_the_examples_expression():
    torch.manual_seed(1)
    p, t = torch.randn(300), torch.randn(300)
    tt = t.clone()
    optim.reference_update([p], [torch.randn(300)], [torch.zeros(300)], [torch.zeros(300)], optim.initial_state(), 1e-3,
                           targets=[t], rho=0.005)
    want = tt * torch.tensor(1.0 - 0.005, dtype=torch.float32) + p * torch.tensor(0.005, dtype=torch.float32)
    assert _same_bits(t, want)
    # the examples' soft_update (mul_ then add_ with alpha, which may fuse the second multiply) within one rounding
    tt.mul_(1.0 - 0.005).add_(p, alpha=0.005)
    assert float((tt - t).abs().max()) <= 2.0 ** -23 * float(t.abs().max())
    # soft_update=False leaves the target alone
    t2 = t.clone()
    optim.reference_update([p], [torch.randn(300)], [torch.zeros(300)], [torch.zeros(300)], optim.initial_state(), 1e-3,
                           targets=[t2], rho=0.005, soft_update=False)
    assert _same_bits(t, t2)


def test_registration_refuses_what_the_kernel_cannot_take():
    opt = optim.FusedAdam(lr=1e-3)
    with pytest.raises(ValueError, match="device"):
        opt.add(LSTMHead(32, 4))  # a CPU module: no host path
    with pytest.raises(ValueError, match="float32"):
        opt.add_tensor(torch.zeros(1, dtype=torch.float64))
    with pytest.raises(ValueError, match="nn.LSTM"):
        opt.add(torch.nn.Linear(3, 3))
    with pytest.raises(ValueError, match="nothing is registered"):
        opt.step()
    with pytest.raises(ValueError):
        optim.FusedAdam(lr=-1.0)
    with pytest.raises(ValueError):
        optim.FusedAdam(betas=(1.0, 0.999))


# ---------------------------------------------------------------- the C ABI of include/finenvs_amd_optim.h
@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_header_symbols_are_exported_and_bound(lib):
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(fe_[a-z0-9_]+)\s*\(", text))
    assert "fe_net_update" in names and len(names) == 7, names
    assert names == set(_lib.OPTIM_SIGNATURES)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in finenvs_amd_optim.h but not exported"
    others = [_lib.SIGNATURES, _lib.EXT_SIGNATURES, _lib.SAC_SIGNATURES, _lib.SAC_GRAD_SIGNATURES]
    assert not any(set(_lib.OPTIM_SIGNATURES) & set(t) for t in others)


def test_struct_layouts_match_the_header():
    assert C.sizeof(_lib.FeOptimSegment) == 12 * 8 + 2 * 8 + 4 * 4 + 2 * 4
    assert _lib.FeOptimSegment.numel.offset == 96 and _lib.FeOptimSegment.kind.offset == 112
    assert _lib.FeOptimSegment.one_minus_rho.offset == 128
    assert C.sizeof(_lib.FeOptimDesc) == 80 and _lib.FeOptimDesc.beta1.offset == 40
    assert _lib.FeOptimDesc.one_minus_beta1.offset == 64


def _desc(**kw):
    d = _lib.FeOptimDesc(segments=0x1000, state=0x2000, num_segments=1, mode=optim.MODE_STEP, num_blocks=1, soft_update=1,
                         zero_grad=1, beta1=0.9, beta2=0.999, lr=1e-3, one_minus_beta1=0.1, beta2_f32=0.999,
                         one_minus_beta2=0.001, eps=1e-8)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("bad", [dict(segments=None), dict(state=None), dict(num_segments=0), dict(num_blocks=0),
                                 dict(num_blocks=1 << 31), dict(mode=3), dict(mode=-1), dict(beta1=1.0), dict(beta2=-0.1),
                                 dict(lr=-1.0), dict(lr=float("nan")), dict(eps=-1.0)])
def test_net_update_refuses_bad_arguments_before_touching_a_device(lib, bad):
    assert lib.fe_net_update(C.byref(_desc(**bad)), None) == _lib.FE_ERR_ARG
    assert b"fe_net_update" in lib.fe_last_error()


def test_null_arguments_are_refused(lib):
    assert lib.fe_net_update(None, None) == _lib.FE_ERR_ARG
    # the pointer siblings: a null bias first, then the by-value entry's own checks (a null env)
    for name in ("fe_lstm_forward_p", "fe_env_rollout_lstm_p", "fe_env_rollout_lstm_split_p", "fe_env_rollout_sac_p",
                 "fe_sac_forward_p", "fe_sac_backward_p"):
        fn = getattr(lib, name)
        args = [None if a is C.c_void_p or a is C.POINTER(_lib.FeSacGrads) else 0 for a in fn.argtypes]
        assert fn(*args) == _lib.FE_ERR_ARG, name
        assert name.encode() in lib.fe_last_error(), name
        if name.startswith("fe_sac") or name == "fe_env_rollout_sac_p":
            args[7] = args[9] = 0x1000  # the two biases given, the env still null
        else:
            args[5] = 0x1000
        assert fn(*args) == _lib.FE_ERR_ARG, name
