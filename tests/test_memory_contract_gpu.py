"""GPU: where the descriptor-consuming kernels write, and what they read from a workspace they did not fill.

The C entries are called directly through ``env._lib`` with the arguments the Python front ends build (packed weights
and ``_lr32`` from ``FusedLSTMHead.rollout``, ``FusedTwinCritic`` and ``FusedSACRollout``); only the pointers under test
are replaced by windows INSIDE larger allocations, ``GUARD`` elements on either side, as
tests/test_store_bounds_gpu.py does for the observation.  No band can cause a fault:

* buffers the call writes (outputs, gradients, workspace): the bands hold ``SENTINEL`` and are compared exactly
  afterwards -- an overrun lands in memory the test owns;
* float inputs the call reads: the bands hold NaN, so a read past ``count`` that reaches a result shows up;
* ``obs_src`` and index inputs: the bands repeat a valid entry of the batch, so nothing indexes outside a table;
* the workspace window is exactly the number of elements the size function returns (the front ends' ``torch.empty``
  is rounded up by the caching allocator and handed back on the next call with the previous call's contents).

Every backward pass (``fe_twin_q_backward`` with both critics and with critic 1 alone plus ``d_actions``,
``fe_sac_backward``, ``fe_lstm_backward``, ``fe_lstm_backward_streamed``; H = 32 / 32 / 64 / 256, W = 4, count in
{1, 33, 16 449}) runs twice: with the workspace and every gradient buffer full of NaN, then full of the finite sentinel.
Two poisons because ``lstm_act2`` swallows a NaN pre-activation: a stale read behind an activation is finite but
different.  The two runs must agree bit for bit, be finite everywhere (``b_ih``, ``b_hh`` and ``d_actions`` included),
equal what the front end returns for the batch, and lie within the project's yardstick ``2e-5 max|g64| + 4
max|g_torch32 - g64|`` of an f64 torch copy (the modules and descriptors of the existing gradient tests); all bands
stay intact and every input window keeps its bits.  16 449 = 32 (512 + 1) + 33 pairs are 515 tiles, a multiple of no
workgroup count a launch can choose: some workgroups add a second tile to partials they own, others do not.  The
streamed pass also runs three chunks at H = 256, W = 390 (768 + 768 + 1 pairs): the later chunks add into gradients
the first one overwrote, from NaN-filled buffers.  The same two-poison and band checks for the workspace and outputs of
``fe_env_rollout_lstm_split`` (against ``FusedLSTMRollout.run`` on twin envs) and ``fe_evo_gradient`` (against the f64
sum built from ``fe_evo_noise``).

Outputs only (bands intact, window overwritten from NaN, values bit-equal to the front end; count in {1, 33, 4 097}):
``fe_lstm_forward`` at H = 32 and 256, ``fe_sac_forward``, ``fe_twin_q_forward``, ``fe_twin_q_target`` and
``fe_replay_sample`` on a wrapped ring.

The three autograd front ends (``FusedLSTMHead``, ``FusedTwinCritic.q``, ``FusedSACRollout.sample``) give the same bits
when the upstream gradient arrives expanded (stride 0), as a strided slice or as float64, and when the descriptors are a
strided view of a trajectory.
"""
import copy
import ctypes as C

import pytest
import torch

from tests import test_critic_grad_gpu as tc
from tests import test_lstm_grad_gpu as tl
from tests import test_lstm_grad_streamed_gpu as ts
from tests import test_sac_grad_gpu as tsac

pytestmark = pytest.mark.gpu

GUARD = 1 << 16  # elements on either side
SENTINEL = -12345.5
NAN = float("nan")
W = 4
UNEVEN = 32 * (512 + 1) + 33  # 515 tiles
COUNTS = (1, 33, UNEVEN)
FORWARD_COUNTS = (1, 33, 4097)
F32, F64, I64, I32 = torch.float32, torch.float64, torch.int64, torch.int32


def _bits(t):
    t = t.detach().reshape(-1)
    return t if not t.is_floating_point() else t.view(I32 if t.element_size() == 4 else I64)


def _same_bits(a, b):
    return a.numel() == b.numel() and a.dtype is b.dtype and torch.equal(_bits(a), _bits(b))


class _Window:
    """``n`` elements inside an allocation of ``GUARD + n + GUARD``, the window's start 16-byte aligned; the bands hold
    ``band``, the window ``data`` (an input) or ``band`` (a buffer the call writes)."""

    def __init__(self, n, dtype, band, data=None):
        self.n = int(n)
        self.big = torch.full((GUARD + self.n + GUARD,), band, dtype=dtype, device="cuda")
        self.win = self.big[GUARD:GUARD + self.n]
        assert self.win.data_ptr() - self.big.data_ptr() == GUARD * self.big.element_size()
        assert self.win.data_ptr() % 16 == 0
        if data is not None:
            assert data.dtype is dtype and data.numel() == self.n, (data.dtype, data.numel(), self.n)
            self.win.copy_(data.detach().reshape(-1))
        self.before = self.big.clone()

    @property
    def ptr(self):
        return self.win.data_ptr()

    def bands_intact(self):
        lo = torch.equal(_bits(self.big[:GUARD]), _bits(self.before[:GUARD]))
        return lo and torch.equal(_bits(self.big[GUARD + self.n:]), _bits(self.before[GUARD + self.n:]))

    def unchanged(self):
        return torch.equal(_bits(self.big), _bits(self.before))

    def poison(self, value):
        self.win.fill_(value if self.win.is_floating_point() else -7)


def _written(n, dtype=F32):
    return _Window(n, dtype, SENTINEL if dtype.is_floating_point else -9)


def _index(data):
    """An index input (descriptors, logical ring indices): the bands repeat its first, valid, entry."""
    return _Window(data.numel(), I64, int(data.reshape(-1)[0]), data)


def _floats(data, dtype=F32):
    return _Window(data.numel(), dtype, NAN, data)


def _two_poisons(launch, outs, ws, ins):
    """`launch` from NaN-filled, then from sentinel-filled output and workspace windows: the same finite bits, all
    bands intact, the inputs untouched.  Returns the outputs."""
    runs = []
    for value in (NAN, SENTINEL):
        for w in list(outs.values()) + ([ws] if ws is not None else []):
            w.poison(value)
        launch()
        torch.cuda.synchronize()
        runs.append({k: w.win.clone() for k, w in outs.items()})
    for k in outs:
        assert bool(torch.isfinite(runs[0][k]).all()) and bool(torch.isfinite(runs[1][k]).all()), f"{k}: not finite"
        assert _same_bits(runs[0][k], runs[1][k]), f"{k}: depends on what the workspace / the buffer held before"
    for k, w in list(outs.items()) + list(ins.items()) + ([("workspace", ws)] if ws is not None else []):
        assert w.bands_intact(), f"{k}: store outside the buffer"
    for k, w in ins.items():
        assert w.unchanged(), f"{k}: an input was written"
    return runs[0]


def _yardstick(names, g, g32, g64):
    """The gradient tests' bound, per tensor: err <= 2e-5 max|g64| + 4 max|g_torch32 - g64|."""
    assert len(names) == len(g) == len(g32) == len(g64)
    worst = 0.0
    for name, gf, gt, gd in zip(names, g, g32, g64):
        assert gf.numel() == gd.numel() and gf.dtype is F32, name
        assert float(gd.abs().max()) > 0, name  # not degenerate
        err = float((gf.double().reshape(-1) - gd.reshape(-1)).abs().max())
        tol = 2e-5 * float(gd.abs().max()) + 4 * float((gt.double() - gd).abs().max())
        print(f"{name:10s} err {err:.3e} tol {tol:.3e} ratio {err / tol:.3f}")
        assert err <= tol, (name, err, tol)
        worst = max(worst, err / tol)
    return worst


def _gen(seed=5):
    return torch.Generator(device="cuda").manual_seed(seed)


def _upstream(count, gen):
    """An upstream gradient (count, 1): normal draws around 0.5.  Not zero-mean: the output bias' gradient is the plain
    sum of the upstream gradient whatever the network, and a zero-mean one makes it a cancelling sum -- at 16 449 pairs
    |sum| < 1 against sum|.| = 13 000, where the yardstick's relative term vanishes and two ulps of a partial sum of
    magnitude 100 (1.5e-5) already exceed what is left of it.  Measured with zero-mean draws: ratio 1.09 for c2.b_out
    (err 1.7e-5, the error c1.b_out has at ratio 0.003 because its sum happens to be 160), every other tensor below
    0.07."""
    return 0.5 + torch.randn((count, 1), generator=gen, device="cuda")


# ---------------------------------------------------------------- the one-output head: fe_lstm_backward[_streamed]
def _head_torch_grads(module, states, c, dtype):
    m = copy.deepcopy(module).to(dtype)
    tl._zero(m)
    s = states.to(dtype)
    (m(s) * c.to(dtype)).sum().backward()
    with torch.no_grad():
        pmax = float(m.last_layer[0](m.lstm(s)[0][:, -1, :]).abs().max())
    return [p.grad for p in tl._params(m)], pmax


def _lstm_backward_banded(H, window, count, streamed):
    from finenvs_amd import _lib
    from finenvs_amd.lstm_head import LSTM_GRAD_KEYS, FusedLSTMHead

    env = tl._env(min(count, 4096), window)
    src, pos, _ = tl._descriptors(env, count)
    states = env.render(src, pos)
    module = ts._module(H, window, 20, "tanh", states[:4096]) if streamed else tl._module(H, window, 20, "tanh")
    head = FusedLSTMHead(env, module, streamed=streamed)
    c = _upstream(count, _gen())
    tl._zero(module)
    y = head(src, pos)
    (y * c).sum().backward()
    front = [p.grad.clone() for p in tl._params(module)]

    lib, roll = env._lib, head.rollout  # the packed weights head(src, pos) just ran with
    size = lib.fe_lstm_streamed_grad_workspace_floats if streamed else lib.fe_lstm_grad_workspace_floats
    backward = lib.fe_lstm_backward_streamed if streamed else lib.fe_lstm_backward
    ws = _written(int(size(H, window, count)))
    ins = {"obs_src": _index(src), "obs_pos": _floats(pos, F64), "outputs": _floats(y), "d_outputs": _floats(c)}
    outs = {k: _written(p.numel()) for k, p in zip(LSTM_GRAD_KEYS, tl._params(module))}
    lg = _lib.FeLstmGrads(*(outs[k].ptr for k in LSTM_GRAD_KEYS))

    def launch():
        _lib.check(backward(env._handle, roll._lr32.data_ptr(), roll.whh.data_ptr(), roll.wx.data_ptr(),
                            roll.wout.data_ptr(), H, roll.out_act, ins["obs_src"].ptr, ins["obs_pos"].ptr, count,
                            ins["outputs"].ptr, ins["d_outputs"].ptr, ws.ptr, C.byref(lg), env._stream()), lib)

    got = _two_poisons(launch, outs, ws, ins)
    for k, f in zip(LSTM_GRAD_KEYS, front):
        assert _same_bits(got[k], f), f"{k}: differs from FusedLSTMHead's gradient"
    g32, _ = _head_torch_grads(module, states.float(), c, F32)
    g64, pmax = _head_torch_grads(module, states.double(), c, F64)
    assert pmax < 4.0, pmax  # not saturated
    return _yardstick(LSTM_GRAD_KEYS, front, g32, g64)


@pytest.mark.parametrize("count", COUNTS)
def test_lstm_backward_memory_contract(count):
    _lstm_backward_banded(64, W, count, streamed=False)


@pytest.mark.parametrize("count", COUNTS)
def test_lstm_backward_streamed_memory_contract(count):
    _lstm_backward_banded(256, W, count, streamed=True)


def test_lstm_backward_streamed_three_chunks_add_into_overwritten_gradients():
    from finenvs_amd import _lib

    H, window = 256, 390
    # the header's rule: the stash is W (6H + 32) floats per pair; the chunk is the largest multiple of 256 pairs whose
    # stash stays within 2^31 bytes, and at least 256 pairs
    chunk = max((2 ** 31) // (4 * window * (6 * H + 32)) // 256, 1) * 256
    assert chunk == 768
    assert int(_lib.load().fe_lstm_streamed_grad_chunk_pairs(H, window)) == chunk
    _lstm_backward_banded(H, window, 2 * chunk + 1, streamed=True)  # the last chunk is a single pair


# ---------------------------------------------------------------- the twin critics: fe_twin_q_backward
CRITIC_NAMES = [f"c{c}.{k}" for c in (1, 2) for k in ("w_ih", "w_hh", "b_ih", "b_hh", "w_out", "b_out")]


def _critic_torch_grads(fused, states, actions, c1, c2, dtype):
    """Gradients of (q1 * c1).sum() [+ (q2 * c2).sum()] of copies of the critics in `dtype`."""
    d1, d2 = copy.deepcopy(fused.critic_1).to(dtype), copy.deepcopy(fused.critic_2).to(dtype)
    tl._zero(d1, d2)
    a = actions.detach().to(dtype).clone().requires_grad_()
    s = states.to(dtype)
    loss = (d1(s, a) * c1.to(dtype)).sum()
    if c2 is not None:
        loss = loss + (d2(s, a) * c2.to(dtype)).sum()
    loss.backward()
    return [p.grad for p in tc._params(d1) + (tc._params(d2) if c2 is not None else [])] + [a.grad]


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("both", [True, False], ids=["both_critics", "critic_1_and_d_actions"])
def test_twin_q_backward_memory_contract(both, count):
    from finenvs_amd import _lib
    from finenvs_amd.critic import GRAD_KEYS, FusedTwinCritic, empty_packed_grads, packed_grads_to_torch

    H = 32
    env = tc._env(min(count, 4096), W)
    src, pos, _ = tc._descriptors(env, count)
    fused = FusedTwinCritic(env, tc._critic(H, W, 10), tc._critic(H, W, 11))
    gen = _gen()
    actions = torch.rand((count, 1), generator=gen, device="cuda") * 2 - 1
    c1 = _upstream(count, gen)
    c2 = _upstream(count, gen) if both else None
    tl._zero(fused.critic_1, fused.critic_2)
    a = actions.clone().requires_grad_()
    q1, q2 = fused.q(src, pos, a)
    loss = (q1 * c1).sum() + ((q2 * c2).sum() if both else 0.0)
    loss.backward()
    nets = (fused.critic_1, fused.critic_2) if both else (fused.critic_1,)
    front = [p.grad.clone() for n in nets for p in tc._params(n)] + [a.grad.clone()]
    assert both or all(p.grad is None for p in fused.critic_2.parameters())

    lib = env._lib
    cw = [_lib.FeCriticWeights(x["whh"].data_ptr(), x["wx"].data_ptr(), x["wout"].data_ptr(), x["bout"].data_ptr())
          for x in fused._packed]  # what q() just ran with
    ws = _written(int(lib.fe_twin_q_grad_workspace_floats(H, W, count)))
    ins = {"obs_src": _index(src), "obs_pos": _floats(pos, F64), "actions": _floats(actions), "dq1": _floats(c1)}
    if both:
        ins["dq2"] = _floats(c2)
    shapes = {k: tuple(v.shape) for k, v in empty_packed_grads(H, "cuda").items()}
    outs = {"d_actions": _written(count)}
    for n in range(len(nets)):
        for k in GRAD_KEYS:
            outs[f"c{n + 1}.{k}"] = _written(int(torch.Size(shapes[k]).numel()))
    cg = [_lib.FeCriticGrads(*(outs[f"c{n + 1}.{k}"].ptr for k in GRAD_KEYS)) for n in range(len(nets))]

    def launch():
        _lib.check(lib.fe_twin_q_backward(
            env._handle, fused._lr32.data_ptr(), C.byref(cw[0]), C.byref(cw[1]), H, ins["obs_src"].ptr, ins["obs_pos"].ptr,
            ins["actions"].ptr, count, ins["dq1"].ptr, ins["dq2"].ptr if both else None, ws.ptr, C.byref(cg[0]),
            C.byref(cg[1]) if both else None, outs["d_actions"].ptr, env._stream()), lib)

    got = _two_poisons(launch, outs, ws, ins)
    mine = []
    for n in range(len(nets)):
        t = packed_grads_to_torch({k: got[f"c{n + 1}.{k}"].reshape(shapes[k]) for k in GRAD_KEYS}, H)
        mine += [t[k] for k in GRAD_KEYS]
    mine.append(got["d_actions"])
    names = CRITIC_NAMES[:6 * len(nets)] + ["d_actions"]
    for name, m, f in zip(names, mine, front):
        assert _same_bits(m, f), f"{name}: differs from FusedTwinCritic.q's gradient"
    states = env.render(src, pos)
    g32 = _critic_torch_grads(fused, states.float(), actions, c1, c2, F32)
    g64 = _critic_torch_grads(fused, states.double(), actions, c1, c2, F64)
    _yardstick(names, front, g32, g64)


# ---------------------------------------------------------------- the SAC actor: fe_sac_backward
def _sac_torch_grads(actor, states, eps, ca, cl, dtype):
    a = copy.deepcopy(actor).to(dtype)
    tl._zero(a)
    s = states.to(dtype)
    actions, log_probs = a.get_actions_and_log_probs(s, eps.to(dtype))
    ((actions * ca.to(dtype)).sum() + (log_probs * cl.to(dtype)).sum()).backward()
    with torch.no_grad():
        dist = a.get_distribution(s)
        umax = float((dist.loc + eps.to(dtype) * dist.scale).abs().max())
    return [p.grad for p in tsac._params(a)], umax


@pytest.mark.parametrize("count", COUNTS)
def test_sac_backward_memory_contract(count):
    from finenvs_amd import _lib
    from finenvs_amd.sac import SAC_GRAD_KEYS, FusedSACRollout

    H = 32
    env = tsac._env(min(count, 4096), W)
    src, pos, _ = tsac._descriptors(env, count)
    roll = FusedSACRollout(env, tsac._actor(H, W, 20))
    gen = _gen()
    eps = torch.randn((count, 1), generator=gen, device="cuda")
    ca = _upstream(count, gen)
    cl = _upstream(count, gen)
    tl._zero(roll.actor)
    actions, log_probs = roll.sample(src, pos, eps)
    stds = roll.last["stds"]
    ((actions * ca).sum() + (log_probs * cl).sum()).backward()
    front = [p.grad.clone() for p in tsac._params(roll.actor)]

    lib, w, (bmu, bstd) = env._lib, roll._packed, roll._biases  # what sample() just ran with
    ws = _written(int(lib.fe_sac_grad_workspace_floats(H, W, count)))
    ins = {"obs_src": _index(src), "obs_pos": _floats(pos, F64), "noise": _floats(eps), "actions": _floats(actions),
           "stds": _floats(stds), "d_actions": _floats(ca), "d_log_probs": _floats(cl)}
    outs = {k: _written(p.numel()) for k, p in zip(SAC_GRAD_KEYS, tsac._params(roll.actor))}
    sg = _lib.FeSacGrads(*(outs[k].ptr for k in SAC_GRAD_KEYS))

    def launch():
        _lib.check(lib.fe_sac_backward(
            env._handle, roll._lr32.data_ptr(), w["whh"].data_ptr(), w["wx"].data_ptr(), w["wl"].data_ptr(),
            w["bl"].data_ptr(), w["wmu"].data_ptr(), bmu, w["wstd"].data_ptr(), bstd, H, ins["obs_src"].ptr,
            ins["obs_pos"].ptr, count, ins["noise"].ptr, ins["actions"].ptr, ins["stds"].ptr, ins["d_actions"].ptr,
            ins["d_log_probs"].ptr, ws.ptr, C.byref(sg), env._stream()), lib)

    got = _two_poisons(launch, outs, ws, ins)
    for k, f in zip(SAC_GRAD_KEYS, front):
        assert _same_bits(got[k], f), f"{k}: differs from FusedSACRollout.sample's gradient"
    states = env.render(src, pos)
    g32, _ = _sac_torch_grads(roll.actor, states.float(), eps, ca, cl, F32)
    g64, umax = _sac_torch_grads(roll.actor, states.double(), eps, ca, cl, F64)
    assert umax < 4.0, umax  # not saturated
    _yardstick(SAC_GRAD_KEYS, front, g32, g64)


# ---------------------------------------------------------------- workspace and outputs: the split rollout, the ES sum
def test_rollout_lstm_split_memory_contract():
    from finenvs_amd import _lib
    from finenvs_amd.rollout import FusedLSTMRollout

    H, N, K, std = 256, 40, 3, 0.5
    module = tl._module(H, W, 20)
    noise = torch.randn((K, N, 1), generator=_gen(), device="cuda")
    runs = []
    for value in (None, NAN, SENTINEL):  # three twin envs: the front end, then the C entry from either poison
        env = tl._env(N, W)
        roll = FusedLSTMRollout.from_modules(env, module.lstm, module.last_layer[0])
        if value is None:
            actions, rewards, dones = roll.run(K, noise=noise, std=std, record_means=True)
            assert roll._workspace is not None  # the split path ran
            runs.append({"actions": actions, "means": roll.means, "rewards": rewards, "dones": dones,
                         "obs_src": roll.obs_src, "obs_pos": roll.obs_pos})
            continue
        lib = env._lib
        ws = _written(int(lib.fe_lstm_split_workspace_floats(H, N)))
        ins = {"noise": _floats(noise)}
        outs = {"actions": _written(K * N), "means": _written(K * N), "rewards": _written(K * N, F64),
                "dones": _written(K * N, I32)}
        for w in list(outs.values()) + [ws]:
            w.poison(value)
        roll._begin_run()
        _lib.check(lib.fe_env_rollout_lstm_split(
            env._handle, roll._lr32.data_ptr(), roll.whh.data_ptr(), roll.wx.data_ptr(), roll.wout.data_ptr(), roll.bout,
            H, roll.out_act, K, roll.obs_src.data_ptr(), roll.obs_pos.data_ptr(), ins["noise"].ptr, std,
            outs["actions"].ptr, outs["means"].ptr, outs["rewards"].ptr, outs["dones"].ptr, None, None, ws.ptr,
            env._stream()), lib)
        roll._end_run()
        torch.cuda.synchronize()
        for k, w in list(outs.items()) + [("noise", ins["noise"]), ("workspace", ws)]:
            assert w.bands_intact(), f"{k}: store outside the buffer"
        assert ins["noise"].unchanged()
        got = {k: w.win.clone() for k, w in outs.items()}
        got.update(obs_src=roll.obs_src, obs_pos=roll.obs_pos)
        runs.append(got)
    assert bool(torch.isfinite(runs[0]["actions"]).all()) and float(runs[0]["rewards"].abs().max()) > 0
    for k, expected in runs[0].items():
        for got in runs[1:]:
            assert _same_bits(got[k], expected), f"{k}: differs from FusedLSTMRollout.run"


def test_evo_gradient_memory_contract():
    from finenvs_amd import _lib

    lib = _lib.load()
    pairs, params, seed, generation = 130, 1377, 99, 3  # not multiples of the 64-pair block / the 4-parameter quad
    st = torch.cuda.current_stream().cuda_stream
    diffed = torch.rand((pairs,), generator=_gen(), device="cuda") - 0.5
    index = torch.arange(pairs, device="cuda")
    z = torch.empty((pairs, params), dtype=F32, device="cuda")
    _lib.check(lib.fe_evo_noise(seed, generation, index.data_ptr(), pairs, params, z.data_ptr(), st), lib)
    ws = _written(int(lib.fe_evo_gradient_workspace_doubles(pairs, params)), F64)
    ins = {"diffed": _floats(diffed)}
    outs = {"out": _written(params, F64)}
    got = _two_poisons(lambda: _lib.check(lib.fe_evo_gradient(seed, generation, pairs, params, ins["diffed"].ptr, ws.ptr,
                                                              outs["out"].ptr, st), lib), outs, ws, ins)["out"]
    terms = diffed.double().unsqueeze(1) * z.double()  # exact: f32 x f32 in f64
    want = terms.sum(dim=0)
    # both sides add `pairs` exact products in f64, in their own order: each within pairs * 2^-53 * sum|terms| of the sum
    bound = 2 * pairs * 2.0 ** -53 * terms.abs().sum(dim=0)
    assert float(want.abs().max()) > 0 and bool(((got - want).abs() <= bound).all())


# ---------------------------------------------------------------- outputs only: the forwards and the sampler
def _overwritten_from_nan(launch, outs, ins, expected):
    for w in outs.values():
        w.poison(NAN)
    launch()
    torch.cuda.synchronize()
    for k, w in list(outs.items()) + list(ins.items()):
        assert w.bands_intact(), f"{k}: store outside the buffer"
    for k, w in ins.items():
        assert w.unchanged(), f"{k}: an input was written"
    for k, e in expected.items():
        assert bool(torch.isfinite(e).all()), k
        assert _same_bits(outs[k].win, e), f"{k}: differs from the front end"


@pytest.mark.parametrize("count", FORWARD_COUNTS)
@pytest.mark.parametrize("H", [32, 256])
def test_lstm_forward_outputs(H, count):
    from finenvs_amd import _lib
    from finenvs_amd.rollout import FusedLSTMRollout

    env = tl._env(min(count, 4096), W)
    src, pos, _ = tl._descriptors(env, count)
    module = tl._module(H, W, 20)
    roll = FusedLSTMRollout.from_modules(env, module.lstm, module.last_layer[0])
    expected = roll.forward(src, pos)
    ins = {"obs_src": _index(src), "obs_pos": _floats(pos, F64)}
    outs = {"out": _written(count)}
    lib = env._lib
    _overwritten_from_nan(lambda: _lib.check(lib.fe_lstm_forward(
        env._handle, roll._lr32.data_ptr(), roll.whh.data_ptr(), roll.wx.data_ptr(), roll.wout.data_ptr(), roll.bout, H,
        roll.out_act, ins["obs_src"].ptr, ins["obs_pos"].ptr, count, outs["out"].ptr, env._stream()), lib),
        outs, ins, {"out": expected})


@pytest.mark.parametrize("count", FORWARD_COUNTS)
def test_sac_forward_outputs(count):
    from finenvs_amd import _lib
    from finenvs_amd.sac import FusedSACRollout

    H = 32
    env = tsac._env(min(count, 4096), W)
    src, pos, _ = tsac._descriptors(env, count)
    roll = FusedSACRollout(env, tsac._actor(H, W, 20))
    eps = torch.randn((count, 1), generator=_gen(), device="cuda")
    actions, log_probs, means, stds = roll.forward(src, pos, eps)
    weights = roll._weights()
    ins = {"obs_src": _index(src), "obs_pos": _floats(pos, F64), "noise": _floats(eps)}
    outs = {k: _written(count) for k in ("actions", "log_probs", "means", "stds")}
    lib = env._lib
    _overwritten_from_nan(lambda: _lib.check(lib.fe_sac_forward(
        env._handle, *weights, ins["obs_src"].ptr, ins["obs_pos"].ptr, count, ins["noise"].ptr, outs["actions"].ptr,
        outs["log_probs"].ptr, outs["means"].ptr, outs["stds"].ptr, env._stream()), lib),
        outs, ins, {"actions": actions, "log_probs": log_probs, "means": means, "stds": stds})


def _ring(env, count):
    """A wrapped replay ring of the env's own transitions and `count` logical indices into it."""
    from finenvs_amd.replay import ReplayBuffer

    N, K = env.num_envs, 6
    _, _, traj = tc._descriptors(env, N * (K + 1))
    buffer = ReplayBuffer(env, max_size=N * K // 2 + 37)
    buffer.extend(traj)
    assert buffer.size() == buffer.max_size and buffer.head != 0  # wrapped
    idx = torch.randint(0, buffer.size(), (count,), generator=_gen(), device="cuda")
    idx[0] = buffer.size() - 1  # the newest transition: the slot just below the head
    return buffer, idx


@pytest.mark.parametrize("count", FORWARD_COUNTS)
def test_twin_q_forward_and_target_outputs(count):
    from finenvs_amd import _lib
    from finenvs_amd.critic import FusedTwinCritic
    from finenvs_amd.rollout import FusedLSTMRollout

    H = 32
    env = tc._env(200, W)
    buffer, idx = _ring(env, count)
    fused = FusedTwinCritic(env, tc._critic(H, W, 10), tc._critic(H, W, 11))
    gen = _gen(6)
    lib = env._lib
    # fe_twin_q_forward on the sampled states' descriptors and a batch of actions
    slots = buffer.physical(idx)
    src, pos = buffer.state_src[slots].contiguous(), buffer.state_pos[slots].reshape(count).contiguous()
    actions = torch.rand((count, 1), generator=gen, device="cuda") * 2 - 1
    q1, q2 = fused.forward(src, pos, actions)
    c1, c2 = fused._weights()
    ins = {"obs_src": _index(src), "obs_pos": _floats(pos, F64), "actions": _floats(actions)}
    outs = {"q1": _written(count), "q2": _written(count)}
    _overwritten_from_nan(lambda: _lib.check(lib.fe_twin_q_forward(
        env._handle, fused._lr32.data_ptr(), C.byref(c1), C.byref(c2), H, ins["obs_src"].ptr, ins["obs_pos"].ptr,
        ins["actions"].ptr, count, outs["q1"].ptr, outs["q2"].ptr, env._stream()), lib), outs, ins, {"q1": q1, "q2": q2})
    # fe_twin_q_target: TD3's smoothed targets straight from the ring
    actor = tl._module(H, W, 20)
    target_actor = FusedLSTMRollout.from_modules(env, actor.lstm, actor.last_layer[0])
    noise = torch.randn((count, 1), generator=gen, device="cuda")
    y = fused.td3_targets(buffer, idx, target_actor=target_actor, noise=noise, gamma=0.97, policy_std=0.2,
                          policy_clip=0.5, reward_scale=2.0)
    last = fused.last
    c1, c2 = fused._weights()
    ins = {"indices": _index(idx), "next_actions": _floats(last["next_actions"]), "noise": _floats(noise)}
    outs = {"y": _written(count), "q1": _written(count), "q2": _written(count)}
    _overwritten_from_nan(lambda: _lib.check(lib.fe_twin_q_target(
        env._handle, fused._lr32.data_ptr(), C.byref(c1), C.byref(c2), H, C.byref(buffer._desc), buffer.head,
        buffer.size(), ins["indices"].ptr, count, ins["next_actions"].ptr, ins["noise"].ptr, 0.2, 0.5, None, None, 0.97,
        2.0, outs["y"].ptr, outs["q1"].ptr, outs["q2"].ptr, env._stream()), lib),
        outs, ins, {"y": y, "q1": last["q1"], "q2": last["q2"]})


@pytest.mark.parametrize("count", FORWARD_COUNTS)
def test_replay_sample_outputs_on_a_wrapped_ring(count):
    from finenvs_amd import _lib

    env = tc._env(200, W)
    buffer, idx = _ring(env, count)
    expected = buffer.get_mini_batch(count, indices=idx)
    ins = {"indices": _index(idx)}
    outs = {k: _written(v.numel()) for k, v in expected.items()}
    _overwritten_from_nan(lambda: _lib.check(buffer._lib.fe_replay_sample(
        env._handle, C.byref(buffer._desc), buffer.head, buffer.size(), ins["indices"].ptr, count, outs["states"].ptr,
        outs["next_states"].ptr, outs["actions"].ptr, outs["rewards"].ptr, outs["dones"].ptr, buffer._stream()),
        buffer._lib), outs, ins, expected)


# ---------------------------------------------------------------- the autograd front ends: argument layouts
def _layouts(B):
    """(name, upstream gradient as it arrives, the same values contiguous in float32)."""
    gen = _gen(8)
    wide = torch.randn((B, 3), generator=gen, device="cuda")
    yield "expanded", torch.full((1, 1), 0.75, device="cuda").expand(B, 1), torch.full((B, 1), 0.75, device="cuda")
    yield "strided", wide[:, 1:2], wide[:, 1:2].contiguous()
    yield "float64", wide[:, :1].double().contiguous(), wide[:, :1].contiguous()


def _strided_descriptors(env, make_descriptors, B):
    """B descriptors as a strided view of a trajectory (every second env of its first rows), and a contiguous copy."""
    _, _, traj = make_descriptors(env, 2 * env.num_envs)
    src, pos = traj.obs_src[:2, ::2], traj.obs_pos[:2, ::2]
    assert src.numel() == B and not src.is_contiguous() and not pos.is_contiguous()
    return (src, pos), (src.contiguous(), pos.contiguous())


def _backward_bits(outputs, grads, params):
    for p in params:
        p.grad = None
    torch.autograd.backward(outputs, grads)
    return [p.grad.clone() for p in params]


def test_lstm_head_argument_layouts():
    from finenvs_amd.lstm_head import FusedLSTMHead

    B = 300
    env = tl._env(B, W)
    strided, plain = _strided_descriptors(env, tl._descriptors, B)
    module = tl._module(64, W, 20)
    head = FusedLSTMHead(env, module)
    params = tl._params(module)
    for name, g, g32 in _layouts(B):
        want = _backward_bits([head(*plain)], [g32], params)
        assert all(float(x.abs().max()) > 0 for x in want)
        for which, d in (("contiguous", plain), ("strided", strided)):
            got = _backward_bits([head(*d)], [g], params)
            for x, z in zip(got, want):
                assert _same_bits(x, z), (name, which)


def test_twin_q_argument_layouts():
    from finenvs_amd.critic import FusedTwinCritic

    B, H = 300, 32
    env = tc._env(B, W)
    strided, plain = _strided_descriptors(env, tc._descriptors, B)
    fused = FusedTwinCritic(env, tc._critic(H, W, 10), tc._critic(H, W, 11))
    actions = torch.rand((B, 1), generator=_gen(), device="cuda") * 2 - 1
    for name, g, g32 in _layouts(B):
        a = actions.clone().requires_grad_()
        params = tc._params(fused.critic_1) + tc._params(fused.critic_2) + [a]
        want = _backward_bits(list(fused.q(*plain, a)), [g32, g32], params)
        assert all(float(x.abs().max()) > 0 for x in want)
        for which, d in (("contiguous", plain), ("strided", strided)):
            got = _backward_bits(list(fused.q(*d, a)), [g, g], params)
            for x, z in zip(got, want):
                assert _same_bits(x, z), (name, which)


def test_sac_sample_argument_layouts():
    from finenvs_amd.sac import FusedSACRollout

    B, H = 300, 32
    env = tsac._env(B, W)
    strided, plain = _strided_descriptors(env, tsac._descriptors, B)
    roll = FusedSACRollout(env, tsac._actor(H, W, 20))
    params = tsac._params(roll.actor)
    eps = torch.randn((B, 1), generator=_gen(), device="cuda")
    for name, g, g32 in _layouts(B):
        want = _backward_bits(list(roll.sample(*plain, eps)), [g32, g32], params)
        assert all(float(x.abs().max()) > 0 for x in want)
        for which, d in (("contiguous", plain), ("strided", strided)):
            got = _backward_bits(list(roll.sample(*d, eps)), [g, g], params)
            for x, z in zip(got, want):
                assert _same_bits(x, z), (name, which)
