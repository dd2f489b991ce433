"""GPU: the memory contract of tests/test_memory_contract_gpu.py for the MLP families -- the one- and the
two-hidden-layer head (``fe_mlp_*``, ``fe_mlp2_*``) and the twin critics Q(s, a) (``fe_twin_mlpq_*``).

The C entries are called directly through ``env._lib`` with the arguments the front ends build (the packed weights of
``rollout._weights()`` / ``twin._weights()``, ``_lr32``); EVERYTHING the caller owns per batch is a window inside a larger
allocation, ``GUARD`` elements on either side (the machinery of tests/test_memory_contract_gpu.py, imported):
``obs_src``, ``obs_pos``, ``actions``, the upstream gradients, the outputs, ``d_actions``, the workspace (exactly the size
function's result) and every gradient buffer; for the target entries also ``indices``, ``next_actions``,
``smooth_noise``, ``log_probs`` and ``alpha``.  The bands of index inputs repeat entry 0 (nothing can index outside a
table), those of float inputs hold NaN, those of written buffers the sentinel: no band can cause a fault.  These kernels
clamp ``qc = min(q, count - 1)`` in some places and guard ``q < count ? x[q] : 0`` in others, and every workspace row of a
padding pair feeds an MFMA chain: one missing guard is ``0 * NaN`` in a gradient here.

Backward passes (``fe_mlp_backward``, ``fe_mlp2_backward``, ``fe_twin_mlpq_backward`` with both critics and ``d_actions``,
with critic 1 alone and ``grads1 = NULL``, and with critic 2 alone and ``dq1 = NULL``, where ``d_actions`` must be
overwritten, not added to) run twice, from NaN-filled and from sentinel-filled workspace and buffers (ELU modules:
``fmaxf`` swallows a NaN, and a ReLU would hide a stale read): the same finite bits, bands intact, inputs bit-unchanged,
bit equality with the front end's ``backward()``, and the family's yardstick ``2e-5 max|g64| + 4 max|g_torch32 - g64|``
against f64 torch (the siblings' ``_torch_grads``) for count in {1, 33, 1 057}.  ``UNEVEN`` = 32 (2 048 + 1) + 1 pairs are
2 050 blocks of 32: the first backward kernel is capped at 512 workgroups of 4 wavefronts, so two wavefronts take a second
block under bands, the last block holds one pair, and there are 129 splits; bit equality with the front end there (the
siblings compare that path with f64 at B = 70 001).

Outputs only (bands intact, window overwritten from NaN, bit-equal to the front end, inputs bit-unchanged; count in
{1, 33, 4 097}): ``fe_mlp_forward``, ``fe_mlp2_forward``, ``fe_twin_mlpq_forward``, ``fe_twin_mlpq_target`` on a wrapped
ring in its TD3 and its SAC form, ``fe_twin_mlpq_target_c``; the ring's arrays, ``errors`` included, keep their bits.

The three autograd front ends give the same bits when the upstream gradient arrives expanded (stride 0), as a strided
slice or as float64, when the descriptors or the actions are strided views, and for actions shaped (B,) or (B, 1).
"""
import copy
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import test_memory_contract_gpu as mc
from tests import test_mlp2_head_gpu as t2
from tests import test_mlp_critic_gpu as tq
from tests import test_mlp_head_gpu as th

pytestmark = pytest.mark.gpu

_Window, _written, _index, _floats, _two_poisons, _same_bits = (mc._Window, mc._written, mc._index, mc._floats,
                                                                mc._two_poisons, mc._same_bits)
GUARD, SENTINEL, NAN = mc.GUARD, mc.SENTINEL, mc.NAN
F32, F64, I64 = torch.float32, torch.float64, torch.int64
UNEVEN = 32 * (2048 + 1) + 1  # 65 569 pairs: 2 050 blocks, 129 splits
BACKWARD_CASES = [(32, 4, 1), (64, 7, 33), (128, 16, 1057), (32, 4, UNEVEN)]
FORWARD_COUNTS = (1, 33, 4097)
GAMMA, SCALE = 0.97, 0.5


def _no_mask(count):
    return torch.zeros((count, 1), dtype=torch.bool, device="cuda")  # ELU has no kink: no sample is masked


def _off_centre(values, count, gen):
    """Targets around ``values - 0.5``: the upstream gradient of a squared error is then not zero-mean, so the output
    bias' gradient is no cancelling sum (``_upstream`` of tests/test_memory_contract_gpu.py)."""
    return values.detach() - 0.5 + 0.3 * torch.randn((count, 1), generator=gen, device="cuda")


# ---------------------------------------------------------------- the heads: fe_mlp_backward, fe_mlp2_backward
def _head_backward_banded(t, Head, H, W, count):
    from finenvs_amd import _lib

    env, src, pos, _ = tq._batch(H, W, count)
    head = Head(env, t._module(H, W, 13, "elu", "tanh"))
    params = t._params(head.module)
    kink = _no_mask(count)
    with torch.no_grad():
        returns = _off_centre(head(src, pos), count, mc._gen())
    t._zero(head.module)
    y = head(src, pos)
    y.retain_grad()
    th._loss("ppo_critic", y, kink, returns, F32).backward()
    c = y.grad.clone()  # the upstream gradient backward() ran with
    front = [p.grad.clone() for p in params]

    lib, roll = env._lib, head.rollout
    weights = roll._weights()  # the buffers head(src, pos) just packed
    ws = _written(int(getattr(lib, head.WORKSPACE)(H, W, count)))
    ins = {"obs_src": _index(src), "obs_pos": _floats(pos, F64), "outputs": _floats(y), "d_outputs": _floats(c)}
    outs = {k: _written(p.numel()) for k, p in zip(head.GRAD_KEYS, params)}
    mg = head.GRADS(*(outs[k].ptr for k in head.GRAD_KEYS))

    def launch():
        _lib.check(getattr(lib, head.BACKWARD)(
            env._handle, roll._lr32.data_ptr(), C.byref(weights), H, roll.act, roll.out_act, ins["obs_src"].ptr,
            ins["obs_pos"].ptr, count, ins["outputs"].ptr, ins["d_outputs"].ptr, ws.ptr, C.byref(mg), env._stream()), lib)

    got = _two_poisons(launch, outs, ws, ins)
    for k, f in zip(head.GRAD_KEYS, front):
        assert float(f.abs().max()) > 0, k
        assert _same_bits(got[k], f), f"{k}: differs from the front end's gradient"
    if count == UNEVEN:
        return
    states = env.render(src, pos.reshape(count, 1))
    _, g32 = t._torch_grads("ppo_critic", head.module, states.float(), kink, returns, F32)
    _, g64 = t._torch_grads("ppo_critic", head.module, states.double(), kink, returns, F64)
    mc._yardstick(head.GRAD_KEYS, front, g32, g64)


@pytest.mark.parametrize("H,W,count", BACKWARD_CASES)
def test_mlp_backward_memory_contract(H, W, count):
    from finenvs_amd.mlp_head import FusedMLPHead

    _head_backward_banded(th, FusedMLPHead, H, W, count)


@pytest.mark.parametrize("H,W,count", BACKWARD_CASES)
def test_mlp2_backward_memory_contract(H, W, count):
    from finenvs_amd.mlp2_head import FusedMLP2Head

    _head_backward_banded(t2, FusedMLP2Head, H, W, count)


# ---------------------------------------------------------------- the twin critics: fe_twin_mlpq_backward
FORMS = ("both_critics", "critic_1_d_actions_only", "critic_2_alone")
CRITIC_NAMES = [f"c{c}.{k}" for c in (1, 2) for k in tq.NAMES]


def _form_loss(form, q1, q2, y):
    if form == "both_critics":  # MSE(q1, y) + MSE(q2, y)
        return tq._loss("critic", q1, q2, ~_no_mask(y.shape[0]), y)
    if form == "critic_1_d_actions_only":  # -q1.mean()
        return tq._loss("actor", q1, q2, ~_no_mask(y.shape[0]), y)
    return F.mse_loss(q2, y.to(q2.dtype))


def _form_torch_grads(form, critics, states, actions, y, dtype):
    """The thirteen gradients as tests/test_mlp_critic_gpu.py::_torch_grads lists them (None: not part of the loss)."""
    if form != "critic_2_alone":
        kind = "critic" if form == "both_critics" else "actor"
        return tq._torch_grads(kind, critics, states, actions, ~_no_mask(y.shape[0]), y, dtype)[1]
    cs = [copy.deepcopy(c).to(dtype) for c in critics]  # the sibling has no arm in which critic 2 runs alone
    a = actions.detach().to(dtype).requires_grad_(True)
    _form_loss(form, None, cs[1](states.to(dtype), a), y).backward()
    return [None] * 6 + [p.grad for p in tq._params(cs[1])] + [a.grad]


@pytest.mark.parametrize("H,W,count", BACKWARD_CASES)
@pytest.mark.parametrize("form", FORMS)
def test_twin_mlpq_backward_memory_contract(form, H, W, count):
    from finenvs_amd import _lib
    from finenvs_amd.mlp_critic import FusedTwinMLPCritic, mlpq_grad_shapes

    env, src, pos, actions = tq._batch(H, W, count)
    critics = [tq._critic(H, W, 13), tq._critic(H, W, 14)]
    twin = FusedTwinMLPCritic(env, *critics)
    with torch.no_grad():
        q = twin.forward(src, pos, actions)
        y = _off_centre(0.5 * (q[0] + q[1]), count, mc._gen())
    runs = {"both_critics": (0, 1), "critic_1_d_actions_only": (0,), "critic_2_alone": (1,)}[form]
    with_grads = () if form == "critic_1_d_actions_only" else runs
    if form == "critic_1_d_actions_only":
        critics[0].requires_grad_(False)  # frozen: it passes dQ/da on, and gets nothing
    tq._zero(*critics)
    a = actions.clone().requires_grad_(True)
    q1, q2 = twin.q(src, pos, a)
    q1.retain_grad()
    q2.retain_grad()
    _form_loss(form, q1, q2, y).backward()
    ups = [q1.grad, q2.grad]
    for c in (0, 1):
        assert (ups[c] is not None) == (c in runs)
        assert all((p.grad is not None) == (c in with_grads) for p in tq._params(critics[c]))
    front = {f"c{c + 1}.{k}": p.grad.clone() for c in with_grads for k, p in zip(tq.NAMES, tq._params(critics[c]))}
    front["d_actions"] = a.grad.clone()

    lib = env._lib
    w = twin._weights()
    packed = twin._packed  # the buffers w points to, kept while the raw calls below use them
    ws = _written(int(lib.fe_twin_mlpq_grad_workspace_floats(H, W, count)))
    ins = {"obs_src": _index(src), "obs_pos": _floats(pos, F64), "actions": _floats(actions)}
    for c in runs:
        ins[f"dq{c + 1}"] = _floats(ups[c])
    outs = {"d_actions": _written(count)}
    for c in with_grads:
        for k, shape in zip(tq.NAMES, mlpq_grad_shapes(H, W)):
            outs[f"c{c + 1}.{k}"] = _written(int(torch.Size(shape).numel()))
    mg = [_lib.FeMlpqGrads(*(outs[f"c{c + 1}.{k}"].ptr for k in tq.NAMES)) if c in with_grads else None for c in (0, 1)]
    ref = lambda x: None if x is None else C.byref(x)  # noqa: E731
    ptr = lambda k: ins[k].ptr if k in ins else None  # noqa: E731

    def launch():
        _lib.check(lib.fe_twin_mlpq_backward(
            env._handle, twin._lr32.data_ptr(), C.byref(w[0]), C.byref(w[1]), H, twin.act, ins["obs_src"].ptr,
            ins["obs_pos"].ptr, ins["actions"].ptr, count, ptr("dq1"), ptr("dq2"), ws.ptr, ref(mg[0]), ref(mg[1]),
            outs["d_actions"].ptr, env._stream()), lib)

    got = _two_poisons(launch, outs, ws, ins)
    assert len(packed) == 2
    for k, f in front.items():
        assert float(f.abs().max()) > 0, k
        assert _same_bits(got[k], f), f"{k}: differs from FusedTwinMLPCritic.q's gradient"
    if count == UNEVEN:
        return
    states = env.render(src, pos.reshape(count, 1))
    names = list(front)
    pick = lambda g: [g[CRITIC_NAMES.index(k)] if k != "d_actions" else g[12] for k in names]  # noqa: E731
    g32 = pick(_form_torch_grads(form, critics, states, actions, y, F32))
    g64 = pick(_form_torch_grads(form, critics, states, actions, y, F64))
    mc._yardstick(names, [front[k] for k in names], g32, g64)


# ---------------------------------------------------------------- outputs only: the forwards and the targets
def _overwritten_from_nan(launch, outs, ins, expected):
    mc._overwritten_from_nan(launch, outs, ins, expected)
    for k in expected:
        assert float(expected[k].abs().max()) > 0, k


@pytest.mark.parametrize("count", FORWARD_COUNTS)
@pytest.mark.parametrize("family", ["mlp", "mlp2"])
def test_mlp_forward_outputs(family, count):
    from finenvs_amd import _lib
    from finenvs_amd.mlp2_head import FusedMLP2Head
    from finenvs_amd.mlp_head import FusedMLPHead

    t, Head, H, W, entry = (th, FusedMLPHead, 32, 4, "fe_mlp_forward") if family == "mlp" else \
        (t2, FusedMLP2Head, 64, 7, "fe_mlp2_forward")
    env, src, pos, _ = tq._batch(H, W, count)
    roll = Head(env, t._module(H, W, 13, "elu", "tanh")).rollout
    expected = roll.forward(src, pos.reshape(count, 1))
    weights = roll._weights()
    ins = {"obs_src": _index(src), "obs_pos": _floats(pos, F64)}
    outs = {"out": _written(count)}
    lib = env._lib
    _overwritten_from_nan(lambda: _lib.check(getattr(lib, entry)(
        env._handle, roll._lr32.data_ptr(), C.byref(weights), H, roll.act, roll.out_act, ins["obs_src"].ptr,
        ins["obs_pos"].ptr, count, outs["out"].ptr, env._stream()), lib), outs, ins, {"out": expected})


@pytest.mark.parametrize("count", FORWARD_COUNTS)
def test_twin_mlpq_forward_outputs(count):
    from finenvs_amd import _lib
    from finenvs_amd.mlp_critic import FusedTwinMLPCritic

    H, W = 32, 4
    env, src, pos, actions = tq._batch(H, W, count)
    twin = FusedTwinMLPCritic(env, tq._critic(H, W, 13), tq._critic(H, W, 14))
    q1, q2 = twin.forward(src, pos, actions)
    w = twin._weights()
    packed = twin._packed
    ins = {"obs_src": _index(src), "obs_pos": _floats(pos, F64), "actions": _floats(actions)}
    outs = {"q1": _written(count), "q2": _written(count)}
    lib = env._lib
    _overwritten_from_nan(lambda: _lib.check(lib.fe_twin_mlpq_forward(
        env._handle, twin._lr32.data_ptr(), C.byref(w[0]), C.byref(w[1]), H, twin.act, ins["obs_src"].ptr, ins["obs_pos"].ptr,
        ins["actions"].ptr, count, outs["q1"].ptr, outs["q2"].ptr, env._stream()), lib), outs, ins, {"q1": q1, "q2": q2})
    assert len(packed) == 2


def _ring_arrays(buffer):
    arrays = {k: getattr(buffer, k) for k in ("state_src", "state_pos", "next_src", "next_pos", "actions", "rewards",
                                              "dones", "errors")}
    if buffer.cursor is not None:
        arrays["cursor"] = buffer.cursor
    return arrays


@pytest.mark.parametrize("count", FORWARD_COUNTS)
@pytest.mark.parametrize("form", ["td3", "sac", "td3_cursor"])
def test_twin_mlpq_target_outputs_on_a_wrapped_ring(form, count):
    from finenvs_amd import _lib
    from finenvs_amd.mlp_critic import FusedTwinMLPCritic

    H, W = 32, 4
    env = th._env(190, W)
    cursor = form == "td3_cursor"
    buffer, store = tq._filled(env, H, 2, cursor=cursor, max_size=3 * 190 - 50)
    store(1)  # wrapped: head != 0
    assert buffer.head != 0 and buffer.size() == buffer.max_size
    with torch.no_grad():
        buffer.dones[1::5] = 1.0
    twin = FusedTwinMLPCritic(env, tq._critic(H, W, 50), tq._critic(H, W, 51))
    target = t2._rollout(env, tq._actor(H, W, 52))
    gen = mc._gen(6)
    noise = torch.randn((count, 1), generator=gen, device="cuda")
    if cursor:
        draw = buffer.draw(count)
        idx = draw.indices
        y = twin.td3_targets(buffer, draw, target, noise, GAMMA, 0.2, 0.5, SCALE)
    else:
        idx = torch.randint(0, buffer.size(), (count,), generator=gen, device="cuda")
        idx[0] = buffer.size() - 1  # the newest transition: the slot just below the head
        y = twin.td3_targets(buffer, idx, target, noise, GAMMA, 0.2, 0.5, SCALE)
    nxt = twin.last["next_actions"].clone()
    logp = alpha = None
    if form == "sac":  # no smoothing, log-probabilities and alpha
        logp = torch.randn((count, 1), generator=gen, device="cuda")
        alpha = torch.full((1,), 0.2, device="cuda")
        y = twin._targets(buffer, idx, nxt, None, 0.0, 0.0, logp, alpha, GAMMA, SCALE)
    expected = {"y": y, "q1": twin.last["q1"], "q2": twin.last["q2"]}
    w = twin._weights()
    packed = twin._packed
    ins = {"indices": _index(idx), "next_actions": _floats(nxt)}
    if form == "sac":
        ins["log_probs"], ins["alpha"] = _floats(logp), _floats(alpha)
    else:
        ins["smooth_noise"] = _floats(noise)
    outs = {k: _written(count) for k in ("y", "q1", "q2")}
    ptr = lambda k: ins[k].ptr if k in ins else None  # noqa: E731
    ring = {k: v.clone() for k, v in _ring_arrays(buffer).items()}
    lib = env._lib
    net = (env._handle, twin._lr32.data_ptr(), C.byref(w[0]), C.byref(w[1]), H, twin.act, C.byref(buffer._desc))
    where = (buffer.cursor.data_ptr(),) if cursor else (buffer.head, buffer.size())
    entry = lib.fe_twin_mlpq_target_c if cursor else lib.fe_twin_mlpq_target
    std, clip = (0.0, 0.0) if form == "sac" else (0.2, 0.5)
    _overwritten_from_nan(lambda: _lib.check(entry(
        *net, *where, ins["indices"].ptr, count, ins["next_actions"].ptr, ptr("smooth_noise"), std, clip, ptr("log_probs"),
        ptr("alpha"), GAMMA, SCALE, outs["y"].ptr, outs["q1"].ptr, outs["q2"].ptr, env._stream()), lib), outs, ins, expected)
    assert len(packed) == 2
    for k, v in _ring_arrays(buffer).items():
        assert _same_bits(v, ring[k]), f"the ring's {k} changed"
    assert int(buffer.errors.item()) == 0  # every index was in range: nothing was counted


# ---------------------------------------------------------------- the autograd front ends: argument layouts
LAYOUT_B, LAYOUT_H, LAYOUT_W = 33, 32, 4


def _descriptor_layouts(env):
    B = LAYOUT_B
    """B descriptors as every second element of 2 B (strided views), and a contiguous copy."""
    src, pos, _ = th._descriptors(env, 2 * B)
    strided = (src[::2], pos[::2])
    assert strided[0].numel() == B and not strided[0].is_contiguous() and not strided[1].is_contiguous()
    assert float(strided[1].abs().max()) > 0  # stepped rows: positions that are not zero
    return strided, (strided[0].contiguous(), strided[1].contiguous())


def _head_argument_layouts(t, Head):
    B, H, W = LAYOUT_B, LAYOUT_H, LAYOUT_W
    env = th._env(16, W)
    strided, plain = _descriptor_layouts(env)
    head = Head(env, t._module(H, W, 20, "elu", "tanh"))
    params = t._params(head.module)
    for name, g, g32 in mc._layouts(B):
        want = mc._backward_bits([head(*plain)], [g32], params)
        assert all(float(x.abs().max()) > 0 for x in want)
        for which, d in (("contiguous", plain), ("strided", strided)):
            for up in (g32, g):  # contiguous float32, then the layout under test
                got = mc._backward_bits([head(*d)], [up], params)
                for x, z in zip(got, want):
                    assert _same_bits(x, z), (name, which)


def test_mlp_head_argument_layouts():
    from finenvs_amd.mlp_head import FusedMLPHead

    _head_argument_layouts(th, FusedMLPHead)


def test_mlp2_head_argument_layouts():
    from finenvs_amd.mlp2_head import FusedMLP2Head

    _head_argument_layouts(t2, FusedMLP2Head)


def test_twin_mlpq_argument_layouts():
    from finenvs_amd.mlp_critic import FusedTwinMLPCritic

    B, H, W = LAYOUT_B, LAYOUT_H, LAYOUT_W
    env = th._env(16, W)
    strided, plain = _descriptor_layouts(env)
    critics = [tq._critic(H, W, 10), tq._critic(H, W, 11)]
    twin = FusedTwinMLPCritic(env, *critics)
    params = tq._params(critics[0]) + tq._params(critics[1])
    wide = torch.rand((B, 2), generator=mc._gen(), device="cuda") * 2 - 1
    values = wide[:, 0].contiguous()

    def run(d, shape, up, strided_actions=False):
        """The twelve parameter gradients and the actions' own, flattened; its shape is that of the actions."""
        if strided_actions:  # the actions are column 0 of a (B, 2) leaf
            leaf = wide.clone().requires_grad_(True)
            a = leaf[:, :1] if shape == (B, 1) else leaf[:, 0]
            assert not a.is_contiguous()
        else:
            leaf = a = values.clone().reshape(shape).requires_grad_(True)
        got = mc._backward_bits(list(twin.q(d[0], d[1].reshape(B), a)), [up, up], params)
        assert leaf.grad.shape == leaf.shape
        da = leaf.grad[:, 0] if strided_actions else leaf.grad
        if strided_actions:
            assert float(leaf.grad[:, 1].abs().max()) == 0.0
        return got + [da.reshape(B).clone()]

    for name, g, g32 in mc._layouts(B):
        want = run(plain, (B, 1), g32)
        assert all(float(x.abs().max()) > 0 for x in want)
        for which, d in (("contiguous", plain), ("strided", strided)):
            for shape in ((B, 1), (B,)):
                for strided_actions in (False, True):
                    for up in (g32, g):
                        got = run(d, shape, up, strided_actions)
                        for x, z in zip(got, want):
                            assert _same_bits(x, z), (name, which, shape, strided_actions)
