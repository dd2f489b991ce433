"""GPU: where the streamed twin-critic entries write and what they read from a workspace they did not fill -- the
contract of tests/test_memory_contract_gpu.py (its windows, guard bands and two poisons) through the C entries of
include/finenvs_amd_critic_streamed.h.

Every pointer under test is a window between 65 536-element guard bands; the workspace window is exactly
``fe_twin_q_streamed_grad_workspace_floats`` elements.  ``fe_twin_q_forward_streamed``, ``fe_twin_q_target_streamed`` (on
a wrapped ring) and ``fe_twin_q_backward_streamed`` each run once from NaN-filled and once from sentinel-filled
workspace and output buffers: the bands stay intact, both runs agree bit for bit, nothing in the outputs is
non-finite, the inputs keep their bits, and the results equal the front end's.  Cases (H, W, count): (256, 4, 33),
(1024, 4, 1100) -- an empty trailing K split that must write zeros for the final kernel to add -- and (256, 4,
chunk + 33): the second chunk adds into gradients the first overwrote, from poisoned buffers.  The upstream gradients
are drawn around 0.5 (``_upstream`` there)."""
import ctypes as C

import pytest
import torch

from tests import test_critic_streamed_gpu as tcs
from tests.test_memory_contract_gpu import (F32, F64, _floats, _gen, _index, _same_bits, _two_poisons, _upstream, _written)

pytestmark = pytest.mark.gpu
GAMMA = 0.97
CASES = [(256, 4, 33), (1024, 4, 1100), (256, 4, "chunk + 33")]


def _weights(fused):
    from finenvs_amd import _lib

    return [_lib.FeCriticWeights(x["whh"].data_ptr(), x["wx"].data_ptr(), x["wout"].data_ptr(), x["bout"].data_ptr())
            for x in fused._packed]  # what the front end just ran with


@pytest.mark.parametrize("H,W,count", CASES)
def test_forward_and_backward_memory_contract(H, W, count):
    from finenvs_amd import _lib
    from finenvs_amd.critic import GRAD_KEYS

    if count == "chunk + 33":
        count = tcs._chunk(H, W) + 33
    env, fused, src, pos, actions, _ = tcs._batch(H, W, count)
    gen = _gen()
    c1, c2 = _upstream(count, gen), _upstream(count, gen)
    tcs._zero(fused.critic_1, fused.critic_2)
    a = actions.clone().requires_grad_()
    q1, q2 = fused.q(src, pos, a)
    ((q1 * c1).sum() + (q2 * c2).sum()).backward()
    params = tcs._params(fused.critic_1) + tcs._params(fused.critic_2)
    names = [f"c{c}.{k}" for c in (1, 2) for k in GRAD_KEYS]
    front = {n: p.grad.clone() for n, p in zip(names, params)}
    front["d_actions"] = a.grad.clone()

    lib, cw = env._lib, _weights(fused)
    ins = {"obs_src": _index(src), "obs_pos": _floats(pos, F64), "actions": _floats(actions), "dq1": _floats(c1),
           "dq2": _floats(c2)}
    # forward
    outs = {"q1": _written(count), "q2": _written(count)}

    def forward():
        _lib.check(lib.fe_twin_q_forward_streamed(
            env._handle, fused._lr32.data_ptr(), C.byref(cw[0]), C.byref(cw[1]), H, ins["obs_src"].ptr, ins["obs_pos"].ptr,
            ins["actions"].ptr, count, outs["q1"].ptr, outs["q2"].ptr, env._stream()), lib)

    got = _two_poisons(forward, outs, None, ins)
    assert _same_bits(got["q1"], q1.detach().reshape(-1)) and _same_bits(got["q2"], q2.detach().reshape(-1))
    # backward
    ws = _written(int(lib.fe_twin_q_streamed_grad_workspace_floats(H, W, count)))
    outs = {n: _written(p.numel()) for n, p in zip(names, params)}
    outs["d_actions"] = _written(count)
    cg = [_lib.FeCriticGrads(*(outs[f"c{c}.{k}"].ptr for k in GRAD_KEYS)) for c in (1, 2)]

    def backward():
        _lib.check(lib.fe_twin_q_backward_streamed(
            env._handle, fused._lr32.data_ptr(), C.byref(cw[0]), C.byref(cw[1]), H, ins["obs_src"].ptr, ins["obs_pos"].ptr,
            ins["actions"].ptr, count, ins["dq1"].ptr, ins["dq2"].ptr, ws.ptr, C.byref(cg[0]), C.byref(cg[1]),
            outs["d_actions"].ptr, env._stream()), lib)

    got = _two_poisons(backward, outs, ws, ins)
    for k, f in front.items():
        assert float(f.abs().max()) > 0, k
        assert _same_bits(got[k], f.reshape(-1)), f"{k}: differs from FusedTwinCritic's gradient"


@pytest.mark.parametrize("H,W,count", CASES)
def test_target_memory_contract(H, W, count):
    from finenvs_amd import _lib
    from finenvs_amd.lstm_head import LSTMHead
    from finenvs_amd.rollout import FusedLSTMRollout

    if count == "chunk + 33":
        count = tcs._chunk(H, W) + 33
    env, buffer = tcs._ring(W)
    idx = torch.randint(0, buffer.size(), (count,), generator=_gen(), device="cuda")
    twin, _ = tcs._twin_on(env, buffer, idx[:4096], H, W, (50, 51))
    torch.manual_seed(52)
    actor = LSTMHead(32, W, "tanh").cuda()
    target = FusedLSTMRollout.from_modules(env, actor.lstm, actor.last_layer[0], output_activation="tanh")
    eps = torch.randn((count, 1), generator=_gen(6), device="cuda")
    y = twin.td3_targets(buffer, idx, target, eps, GAMMA, 0.2, 0.5).clone()
    front = {"y": y, "q1": twin.last["q1"].clone(), "q2": twin.last["q2"].clone()}
    lib, cw = env._lib, _weights(twin)
    ins = {"indices": _index(idx), "next_actions": _floats(twin.last["next_actions"]), "noise": _floats(eps)}
    outs = {k: _written(count) for k in ("y", "q1", "q2")}
    errors = int(buffer.errors.item())

    def launch():
        _lib.check(lib.fe_twin_q_target_streamed(
            env._handle, twin._lr32.data_ptr(), C.byref(cw[0]), C.byref(cw[1]), H, C.byref(buffer._desc), buffer.head,
            buffer.size(), ins["indices"].ptr, count, ins["next_actions"].ptr, ins["noise"].ptr, 0.2, 0.5, None, None, GAMMA,
            1.0, outs["y"].ptr, outs["q1"].ptr, outs["q2"].ptr, env._stream()), lib)

    got = _two_poisons(launch, outs, None, ins)
    for k, f in front.items():
        assert f.dtype is F32 and _same_bits(got[k], f.reshape(-1)), f"{k}: differs from FusedTwinCritic.td3_targets"
    assert int(buffer.errors.item()) == errors
