"""SAC's MLP actor: the torch module a learner trains, its folded head, and the fused path on descriptors.

``SACActorMLP`` restates the reference's ``finenvs/agents/SAC/actor.py:ActorMLP`` (lines 106-120) for one output per
(env, asset) pair: ``network = MLPNetwork((5W, H, H), ELU, nn.Identity)`` -- ``Sequential(Linear(5W, H), act,
Linear(H, H), Identity())``, so the second ``Linear`` has no activation -- then ``mu_layer`` and ``std_layer =
Linear(H, 1)`` with ``softplus`` on the std (SAC/actor.py:44-49) and the tanh-squashed sample with its log-probability
(SAC/actor.py:51-61).  ``SACAgentMLP`` (SAC_agent.py:244-279) builds it with ``hidden_dims=(128, 128)``.  Its submodule
names are the reference's, so a reference ``state_dict`` loads unchanged.

Because nothing non-linear stands between the first hidden layer's activations ``a1`` and ``mu`` / the pre-softplus std
``q``, the H x H layer folds into two H-vectors and two constants (``fold_head``; on the device ``fe_mlp_sac_pack``,
include/finenvs_amd_mlp_sac.h)::

    v_mu = W2^T w_mu   c_mu = w_mu . b2 + b_mu      v_s = W2^T w_s   c_s = w_s . b2 + b_s
    mu = c_mu + v_mu . a1                           q = c_s + v_s . a1

``FusedMLPSACRollout`` is ``FusedSACRollout``'s front end (finenvs_amd/sac.py) on that form: ``run`` steps the env K
times per launch with the actor in the kernel (``fe_env_rollout_mlp_sac``), ``forward`` is the no-grad actor half of
``compute_targets`` on descriptors (``fe_mlp_sac_forward``), ``sample`` the same values as a differentiable function of
the actor's eight parameters (``fe_mlp_sac_backward``: the rank-two algebra ``reference_backward`` restates in torch) and
``actor_losses`` the losses of ``Actor.compute_losses`` with a ``FusedTwinMLPCritic``.  Nothing is rendered.  Scope:
H in {32, 64, 128}, both layers of width H, a window the one-layer head admits (``MLP_SAC_MAX_WINDOW``); gradients run
one asset.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.distributions import Normal

from . import _lib
from .mlp_head import MLP_HEAD_HIDDEN_SIZES, MLP_HEAD_LAYER_ACTIVATIONS, _layer_activation
from .rollout import FusedMLPRollout, _FusedEvaluation, log_return_f32, rollout_outputs

MLP_SAC_GRAD_KEYS = ("w1", "b1", "w2", "b2", "w_mu", "b_mu", "w_std", "b_std")  # fe_mlp_sac_grads' fields
MLP_SAC_MAX_WINDOW = _lib.MLP_SAC_MAX_WINDOW
MLP_SAC_STATE_DICT_KEYS = ("network.0.weight", "network.0.bias", "network.2.weight", "network.2.bias", "mu_layer.weight",
                           "mu_layer.bias", "std_layer.weight", "std_layer.bias")


class SACActorMLP(nn.Module):
    """The reference's SAC ``ActorMLP((5W, H, H), ...)`` with one output per pair as a plain module (no optimizer
    inside): ``network = Sequential(Linear(5W, H), act, Linear(H, H), Identity())``, ``mu_layer``, ``std_layer``;
    ``log_alpha`` the entropy temperature (a leaf tensor outside ``parameters()``, as ``SACActorLSTM`` keeps it) and
    ``target_entropy = -1``."""

    def __init__(self, H: int = 128, W: int = 4, activation: str = "elu", starting_alpha: float = 1.0, device=None):
        super().__init__()
        if activation not in MLP_HEAD_LAYER_ACTIVATIONS:
            raise ValueError(f"activation must be one of {sorted(MLP_HEAD_LAYER_ACTIVATIONS)} (got {activation!r})")
        self.hidden_size, self.sequence_length, self.activation, self.num_actions = int(H), int(W), activation, 1
        H, W = self.hidden_size, self.sequence_length
        self.network = nn.Sequential(nn.Linear(5 * W, H, device=device), MLP_HEAD_LAYER_ACTIVATIONS[activation](),
                                     nn.Linear(H, H, device=device), nn.Identity())
        self.mu_layer = nn.Linear(H, 1, device=device)
        self.std_layer = nn.Linear(H, 1, device=device)
        self.log_alpha = torch.tensor(math.log(starting_alpha), device=device, requires_grad=True)
        self.target_entropy = -1.0

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        self.log_alpha = fn(self.log_alpha.detach()).requires_grad_(True)  # .to(device) moves the temperature too
        return self

    def forward(self, states: torch.Tensor) -> torch.Tensor:
        """(B, W, 5) or (B, 5W) -> the network's output z (B, H)."""
        W = self.sequence_length
        if states.dim() == 3 and tuple(states.shape[1:]) == (W, 5):
            states = states.reshape(states.shape[0], 5 * W)
        elif states.dim() != 2 or states.shape[1] != 5 * W:
            raise ValueError(f"states must be (B, {W}, 5) or (B, {5 * W}), got {tuple(states.shape)}")
        return self.network(states.to(self.network[0].weight.dtype))

    def get_distribution(self, states: torch.Tensor) -> Normal:
        hiddens = self.forward(states)
        return Normal(self.mu_layer(hiddens), F.softplus(self.std_layer(hiddens)))

    def get_actions_and_log_probs(self, states: torch.Tensor, eps: Optional[torch.Tensor] = None):
        """(tanh(u), log_prob) with u = dist.rsample(), or u = loc + eps * scale for given standard normals ``eps``
        (the same reparameterisation, with the caller's draws: what the fused path takes as ``noise``)."""
        dist = self.get_distribution(states)
        u = dist.rsample() if eps is None else dist.loc + eps * dist.scale
        actions = torch.tanh(u)
        log_probs = dist.log_prob(u) - torch.log(1 - torch.tanh(u).pow(2) + 1e-7)
        return actions, log_probs

    def step_actions(self, states: torch.Tensor, eps: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``SACAgent.step`` (SAC_agent.py:110-121): tanh of the sample, the LAST row acting on the un-squashed mean."""
        with torch.no_grad():
            dist = self.get_distribution(states)
            u = dist.rsample() if eps is None else dist.loc + eps * dist.scale
            actions = torch.tanh(u)
            actions[-1, :] = dist.loc[-1, :]
        return actions


def check_mlp_sac_actor(actor: nn.Module) -> Tuple[int, int, str]:
    """(hidden size, window, activation) of an actor the fused SAC MLP path can run; ValueError otherwise."""
    net = getattr(actor, "network", None)
    if not isinstance(net, nn.Sequential) or len(net) != 4 or not all(isinstance(net[i], nn.Linear) for i in (0, 2)):
        raise ValueError("the fused SAC MLP actor needs a module with `network = Sequential(Linear(5W, H), act, Linear(H, H), "
                         "Identity())`")
    first, second = net[0], net[2]
    H = int(first.out_features)
    if H not in MLP_HEAD_HIDDEN_SIZES:
        raise ValueError(f"the fused SAC MLP actor runs H in {MLP_HEAD_HIDDEN_SIZES} (got {H})")
    if second.in_features != H or second.out_features != H:
        raise ValueError(f"both layers must have the same width: Linear(5W, {H}) needs Linear({H}, {H}) (got "
                         f"Linear({second.in_features}, {second.out_features}))")
    if first.in_features % 5 != 0 or first.in_features < 5:
        raise ValueError(f"the first layer must take a flattened (W, 5) window: in_features = 5 W (got {first.in_features})")
    if not isinstance(net[3], nn.Identity):
        raise ValueError("the second layer must have no activation (Identity): the fold of the H x H layer into the head "
                         f"depends on it (got {type(net[3]).__name__})")
    for name in ("mu_layer", "std_layer"):
        layer = getattr(actor, name, None)
        if not isinstance(layer, nn.Linear) or layer.in_features != H or layer.out_features != 1 or layer.bias is None:
            raise ValueError(f"{name} must be Linear({H}, 1): the fused head has one output per (env, asset) pair")
    if first.bias is None or second.bias is None:
        raise ValueError("both layers need a bias")
    return H, first.in_features // 5, _layer_activation(net[1])


def mlp_sac_parameters(actor: nn.Module) -> Tuple[torch.Tensor, ...]:
    """The eight parameter tensors of an actor in ``MLP_SAC_GRAD_KEYS`` order, which is ``named_parameters()``' order:
    ``network[0].weight (H, 5W)`` / ``.bias (H)``, ``network[2].weight (H, H)`` / ``.bias (H)``, ``mu_layer.weight
    (1, H)`` / ``.bias (1)``, ``std_layer.weight (1, H)`` / ``.bias (1)``."""
    net = actor.network
    return (net[0].weight, net[0].bias, net[2].weight, net[2].bias, actor.mu_layer.weight, actor.mu_layer.bias,
            actor.std_layer.weight, actor.std_layer.bias)


def mlp_sac_grad_shapes(H: int, W: int):
    return (H, 5 * W), (H,), (H, H), (H,), (1, H), (1,), (1, H), (1,)


def fold_head(actor: nn.Module, dtype: Optional[torch.dtype] = None) -> Dict[str, torch.Tensor]:
    """The host mirror of ``fe_mlp_sac_pack``'s fold: ``v_mu``, ``v_s`` (H) and ``c_mu``, ``c_s`` (scalars) with every sum
    formed in float64 from the parameters and rounded once to ``dtype`` (default: the parameters' dtype)."""
    w2, b2, wmu, bmu, wstd, bstd = (p.detach().double() for p in mlp_sac_parameters(actor)[2:])
    dtype = mlp_sac_parameters(actor)[0].dtype if dtype is None else dtype
    wmu, wstd = wmu.reshape(-1), wstd.reshape(-1)
    return {"v_mu": (w2.t() @ wmu).to(dtype), "v_s": (w2.t() @ wstd).to(dtype),
            "c_mu": (wmu @ b2 + bmu.reshape(())).to(dtype), "c_s": (wstd @ b2 + bstd.reshape(())).to(dtype)}


def reference_backward(actor: nn.Module, states: torch.Tensor, eps: torch.Tensor, d_actions: Optional[torch.Tensor],
                       d_log_probs: Optional[torch.Tensor]) -> Tuple[torch.Tensor, ...]:
    """The host mirror of ``fe_mlp_sac_backward``: the eight parameter gradients (``MLP_SAC_GRAD_KEYS`` order, torch's
    shapes) of ``get_actions_and_log_probs(states, eps)`` for the upstream gradients ``d_actions`` / ``d_log_probs``
    ((B, 1), either may be None), by the rank-two algebra of the fold and without autograd, in the actor's dtype."""
    H, W, activation = check_mlp_sac_actor(actor)
    w1, b1, w2, b2, wmu, bmu, wstd, bstd = (p.detach() for p in mlp_sac_parameters(actor))
    B = states.shape[0]
    x = states.reshape(B, 5 * W).to(w1.dtype)
    z1 = x @ w1.t() + b1
    if activation == "relu":
        a1, d1 = torch.relu(z1), (z1 > 0).to(z1.dtype)
    elif activation == "tanh":
        a1 = torch.tanh(z1)
        d1 = 1 - a1 * a1
    else:
        ez = torch.exp(z1)
        a1, d1 = torch.where(z1 > 0, z1, ez - 1), torch.where(z1 > 0, torch.ones_like(z1), ez)
    f = fold_head(actor, w1.dtype)
    mu = f["c_mu"] + a1 @ f["v_mu"]
    q = f["c_s"] + a1 @ f["v_s"]
    s = F.softplus(q)
    e = eps.reshape(B).to(w1.dtype)
    a = torch.tanh(mu + e * s)
    zero = torch.zeros((B,), dtype=w1.dtype, device=w1.device)
    ga = zero if d_actions is None else d_actions.reshape(B).to(w1.dtype)
    gl = zero if d_log_probs is None else d_log_probs.reshape(B).to(w1.dtype)
    om = 1 - a * a
    dmu = ga * om + gl * (2 * a * om / (om + 1e-7))
    dq = (dmu * e - gl / s) * torch.where(q > 20, torch.ones_like(q), torch.sigmoid(q))
    S_mu, S_q, A_mu, A_q = dmu.sum(), dq.sum(), dmu @ a1, dq @ a1
    wmu_v, wstd_v = wmu.reshape(H), wstd.reshape(H)
    dz1 = (dmu[:, None] * f["v_mu"][None, :] + dq[:, None] * f["v_s"][None, :]) * d1
    return (dz1.t() @ x, dz1.sum(0), torch.outer(wmu_v, A_mu) + torch.outer(wstd_v, A_q), wmu_v * S_mu + wstd_v * S_q,
            (w2 @ A_mu + b2 * S_mu).reshape(1, H), S_mu.reshape(1), (w2 @ A_q + b2 * S_q).reshape(1, H), S_q.reshape(1))


def pack_mlp_sac_weights(env, actor: nn.Module, snapshot: bool = True) -> Dict[str, torch.Tensor]:
    """The actor's current parameters as ``fe_mlp_sac_weights`` reads them (f32, on the parameters' device, no host sync):
    one ``fe_mlp_sac_pack`` launch writes ``w1t`` / ``wpos`` and the fold ``vmu`` / ``vstd`` / ``cfold`` into one fresh buffer.
    ``snapshot``: every other tensor is a fresh copy, so that a forward whose ``backward()`` is still pending keeps the
    weights it ran with; without it they are the parameters themselves (acting and the no-grad forward: one allocation and
    one launch per call)."""
    H, W, _ = check_mlp_sac_actor(actor)
    w1, b1, w2, b2, wmu, bmu, wstd, bstd = (p.detach() for p in mlp_sac_parameters(actor))
    keep = (lambda t: t.clone()) if snapshot else (lambda t: t)
    n1 = H * 4 * W
    flat = torch.empty((n1 + 3 * H + 2,), dtype=torch.float32, device=w1.device)
    x = {"w1t": flat[:n1].view(H, 4 * W), "wpos": flat[n1:n1 + H], "b1": keep(b1), "w2": keep(w2.contiguous()), "b2": keep(b2),
         "wmu": keep(wmu.reshape(H)), "bmu": keep(bmu.reshape(1)), "wstd": keep(wstd.reshape(H)), "bstd": keep(bstd.reshape(1)),
         "vmu": flat[n1 + H:n1 + 2 * H], "vstd": flat[n1 + 2 * H:n1 + 3 * H], "cfold": flat[n1 + 3 * H:], "_w1": w1.contiguous()}
    _lib.check(env._lib.fe_mlp_sac_pack(
        x["_w1"].data_ptr(), x["w2"].data_ptr(), x["b2"].data_ptr(), x["wmu"].data_ptr(), x["bmu"].data_ptr(),
        x["wstd"].data_ptr(), x["bstd"].data_ptr(), H, W, x["w1t"].data_ptr(), x["wpos"].data_ptr(), x["vmu"].data_ptr(),
        x["vstd"].data_ptr(), x["cfold"].data_ptr(), env._stream()), env._lib)
    return x


def _weights_struct(x: Dict[str, torch.Tensor]) -> "_lib.FeMlpSacWeights":
    return _lib.FeMlpSacWeights(*(x[k].data_ptr() for k, _ in _lib.FeMlpSacWeights._fields_))


class _MlpSacSample(torch.autograd.Function):
    """(actions, log_probs) of ``FusedMLPSACRollout.forward`` as a differentiable function of the actor's eight
    parameters: the forward is ``fe_mlp_sac_forward``, the backward ``fe_mlp_sac_backward`` (``a1`` recomputed)."""

    @staticmethod
    def forward(ctx, roll, src, pos, noise, *params):
        actions, log_probs, means, stds = roll.forward(src, pos, noise, _snapshot=True)  # the backward reads this pack
        roll.last = {"means": means, "stds": stds}
        ctx.set_materialize_grads(False)  # an output nobody used gets None, not zeros: its pointer is null
        ctx.roll, ctx.packed = roll, getattr(roll, "_packed", None)  # (none yet: B = 0)
        ctx.save_for_backward(src, pos, noise, actions, stds)
        return actions, log_probs

    @staticmethod
    def backward(ctx, g_a, g_lp):
        roll = ctx.roll
        out = [None] * 12
        if (g_a is None and g_lp is None) or not any(ctx.needs_input_grad[4:]):
            return tuple(out)
        src, pos, noise, actions, stds = ctx.saved_tensors
        env, H, B = roll.env, roll.H, int(src.numel())
        W, dev = int(env.num_intervals), env._dev
        grads = [torch.empty(shape, dtype=torch.float32, device=dev) for shape in mlp_sac_grad_shapes(H, W)]
        if B:
            g_a, g_lp = (None if g is None else g.reshape(B).float().contiguous() for g in (g_a, g_lp))
            ws = torch.empty((int(env._lib.fe_mlp_sac_grad_workspace_floats(H, W, B)),), dtype=torch.float32, device=dev)
            cw = _weights_struct(ctx.packed)
            sg = _lib.FeMlpSacGrads(*(g.data_ptr() for g in grads))
            ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
            _lib.check(env._lib.fe_mlp_sac_backward(
                env._handle, roll._lr32.data_ptr(), C.byref(cw), H, roll.act, src.data_ptr(), pos.data_ptr(), B,
                noise.data_ptr(), actions.data_ptr(), stds.data_ptr(), ptr(g_a), ptr(g_lp), ws.data_ptr(), C.byref(sg),
                env._stream()), env._lib)
        else:  # nothing to launch: the sums over an empty batch are zeros
            for g in grads:
                g.zero_()
        for k in range(8):
            if ctx.needs_input_grad[4 + k]:
                out[4 + k] = grads[k]
        return tuple(out)


class FusedMLPSACRollout(_FusedEvaluation):
    """K env steps per launch with the SAC MLP actor in the kernel (C ABI ``fe_env_rollout_mlp_sac``,
    include/finenvs_amd_mlp_sac.h), and its head on descriptors: ``FusedSACRollout``'s front end for a ``SACActorMLP``
    (or the reference's ``ActorMLP`` of that shape with one output).

    The actor's parameters are re-packed and re-folded on the device at every ``run`` / ``forward`` / ``sample`` (one
    allocation and one launch; ``sample`` also copies the eight tensors, which its ``backward()`` reads; nothing goes to
    the host: the biases are read on the device), so an optimizer step on ``actor`` is seen by the next call.  The actor must live on the env's device."""

    def __init__(self, env, actor: nn.Module):
        self.H, W, self.activation = check_mlp_sac_actor(actor)
        self.act = FusedMLPRollout.ACTIVATIONS[self.activation]
        if W != int(env.num_intervals):
            raise ValueError(f"the actor's first layer takes {5 * W} inputs, a window of {W} rows; the env renders "
                             f"{env.num_intervals} rows: in_features must be {5 * int(env.num_intervals)}")
        if env.redraw != "device" and not env.evaluate:
            raise ValueError('the fused rollout needs redraw="device" (or evaluate mode): no host in the loop')
        if int(env.num_assets) == 1 and W > MLP_SAC_MAX_WINDOW[self.H]:
            raise ValueError(f"a window of {W} rows does not fit the LDS at H = {self.H} (at most {MLP_SAC_MAX_WINDOW[self.H]})")
        self.env, self.actor = env, actor
        self._check_device()
        dev = env._dev
        self.obs_src = torch.empty((env.num_envs,), dtype=torch.int64, device=dev)
        self.obs_pos = torch.empty((env.num_envs, env.num_assets), dtype=torch.float64, device=dev)
        self._lr32 = log_return_f32(env)
        self.means = self.stds = None
        self.last: Dict[str, torch.Tensor] = {}  # means / stds of the latest sample()
        self.sync_from_env()

    def _check_device(self) -> None:
        params = mlp_sac_parameters(self.actor)
        if any(p.device != torch.device(self.env._dev) for p in params):
            raise ValueError(f"the actor's parameters must live on the env's device {self.env._dev}")
        if any(p.dtype is not torch.float32 for p in params):
            raise ValueError("the fused SAC MLP actor needs float32 parameters")

    def _weights(self, snapshot: bool = False) -> "_lib.FeMlpSacWeights":
        self._check_device()
        self._packed = pack_mlp_sac_weights(self.env, self.actor, snapshot)  # kept alive until the launch has been queued
        return _weights_struct(self._packed)

    def folded(self) -> Dict[str, torch.Tensor]:
        """The device tensors the pack kernel wrote at the latest call: ``w1t`` (H, 4W), ``wpos`` (H), ``b1`` (H) and the
        fold ``v_mu``, ``v_s`` (H), ``c_mu``, ``c_s`` (1 each, views of one buffer).  Packs now if nothing ran yet."""
        if getattr(self, "_packed", None) is None:
            self._weights()
        x = self._packed
        return {"w1t": x["w1t"], "wpos": x["wpos"], "b1": x["b1"], "v_mu": x["vmu"], "v_s": x["vstd"],
                "c_mu": x["cfold"][0:1], "c_s": x["cfold"][1:2]}

    def _check_noise(self, noise, shape):
        if noise is None:
            return None
        if not isinstance(noise, torch.Tensor) or noise.dtype is not torch.float32 or tuple(noise.shape) != shape \
                or noise.device != torch.device(self.env._dev):
            raise ValueError(f"noise must be a {shape} float32 tensor of standard normals on {self.env._dev}, got "
                             f"{getattr(noise, 'dtype', type(noise))} {tuple(getattr(noise, 'shape', ()))} on "
                             f"{getattr(noise, 'device', None)}")
        return noise.contiguous()

    def run(self, num_steps: int, noise: Optional[torch.Tensor] = None, record_means: bool = False,
            record_stds: bool = False, trajectory=None, record_actions: bool = True):
        """Returns (actions (K, N, A) f32, rewards (K, N) f64, dones (K, N) int32), as ``FusedSACRollout.run``.

        With ``noise`` -- (K, N, A) f32 standard normals from the caller's generator -- every env acts with
        ``tanh(mu + eps * std)`` except the training-mode env's evaluation env, which acts on ``mu`` (SACAgent.step,
        SAC_agent.py:110-121); without noise every env acts on ``mu``.  An evaluate-mode env has no evaluation env:
        there every env samples.  ``record_means`` / ``record_stds`` keep mu / std in ``self.means`` / ``self.stds``
        ((K, N, A)).  ``trajectory``: an empty ``TrajectoryBuffer(K, N, A, states=True)`` without capacity padding,
        filled as ``FusedLSTMRollout.run`` fills it.  ``record_actions=False`` (``evaluate_returns``) keeps no actions."""
        env, K = self.env, int(num_steps)
        N, A, dev = env.num_envs, env.num_assets, env._dev
        if K < 1:
            raise ValueError("num_steps must be >= 1")
        noise = self._check_noise(noise, (K, N, A))
        actions, rewards, dones, src_out, pos_out = rollout_outputs(env, K, trajectory, record_actions)
        self._begin_run()
        w = self._weights()
        self.means = torch.empty((K, N, A), dtype=torch.float32, device=dev) if record_means else None
        self.stds = torch.empty((K, N, A), dtype=torch.float32, device=dev) if record_stds else None
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        _lib.check(env._lib.fe_env_rollout_mlp_sac(
            env._handle, self._lr32.data_ptr(), C.byref(w), self.H, self.act, K, self.obs_src.data_ptr(),
            self.obs_pos.data_ptr(), ptr(noise), ptr(actions), ptr(self.means), ptr(self.stds), rewards.data_ptr(),
            dones.data_ptr(), ptr(src_out), ptr(pos_out), env._stream()), env._lib)
        self._end_run()
        if trajectory is not None:
            trajectory.mark_filled(K)
        return actions, rewards, dones

    def forward(self, obs_src: torch.Tensor, obs_pos: torch.Tensor, noise: Optional[torch.Tensor] = None,
                _snapshot: bool = False):
        """The head on B observation descriptors (``obs_src (B,)`` int64, ``obs_pos (B, A)`` f64 -- rows of a
        ``TrajectoryBuffer(states=True)`` or of the replay ring) without stepping the env: (actions, log_probs, means,
        stds), each (B, A) f32.  ``actions = tanh(mu + eps * std)`` and ``log_probs`` (SAC/actor.py:51-61) need
        ``noise`` (B, A) and are None without it; every descriptor samples (no evaluation env here)."""
        env, A = self.env, self.env.num_assets
        B = int(obs_src.numel())
        src = obs_src.reshape(B).to(device=env._dev, dtype=torch.int64).contiguous()
        pos = obs_pos.reshape(B, A).to(device=env._dev, dtype=torch.float64).contiguous()
        noise = self._check_noise(noise, (B, A))
        dev = env._dev
        means = torch.empty((B, A), dtype=torch.float32, device=dev)
        stds = torch.empty((B, A), dtype=torch.float32, device=dev)
        actions = torch.empty((B, A), dtype=torch.float32, device=dev) if noise is not None else None
        log_probs = torch.empty((B, A), dtype=torch.float32, device=dev) if noise is not None else None
        if B:
            self._check_epoch()
            w = self._weights(_snapshot)
            ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
            _lib.check(env._lib.fe_mlp_sac_forward(
                env._handle, self._lr32.data_ptr(), C.byref(w), self.H, self.act, src.data_ptr(), pos.data_ptr(), B,
                ptr(noise), ptr(actions), ptr(log_probs), means.data_ptr(), stds.data_ptr(), env._stream()), env._lib)
        return actions, log_probs, means, stds

    # ---------------------------------------------------------------- the gradient half
    def sample(self, obs_src: torch.Tensor, obs_pos: torch.Tensor, noise: torch.Tensor):
        """``forward``'s ``(actions, log_probs)``, each (B, 1) float32 and the same values bit for bit, as a
        differentiable function of the actor's eight parameters (C ABI ``fe_mlp_sac_backward``):
        ``get_actions_and_log_probs`` (SAC/actor.py:51-61) with ``noise`` (B, 1) the standard normals of ``rsample``.
        ``backward()`` accumulates into the parameters' ``.grad`` as the torch module would; an output that received no
        gradient costs nothing, and with every parameter frozen nothing launches.  The means and stds of the call stay
        in ``self.last`` (not differentiable)."""
        env = self.env
        if int(env.num_assets) != 1:
            raise ValueError(f"the fused actor gradient runs one asset (the env has {env.num_assets}): its consumer, the "
                             "fused twin critic, does")
        if not isinstance(obs_src, torch.Tensor) or not isinstance(obs_pos, torch.Tensor):
            raise ValueError("obs_src / obs_pos must be tensors of observation descriptors")
        B = int(obs_src.numel())
        if noise is None:
            raise ValueError(f"sample needs noise: a ({B}, 1) float32 tensor of standard normals on {env._dev}")
        noise = self._check_noise(noise, (B, 1))
        self._check_device()
        src = obs_src.reshape(B).to(device=env._dev, dtype=torch.int64).contiguous()
        pos = obs_pos.reshape(B, 1).to(device=env._dev, dtype=torch.float64).contiguous()
        return _MlpSacSample.apply(self, src, pos, noise, *mlp_sac_parameters(self.actor))

    def actor_losses(self, buffer, indices: torch.Tensor, twin, noise: Optional[torch.Tensor] = None):
        """``(actor_loss, alpha_loss)`` of ``Actor.compute_losses`` (SAC/actor.py:63-81) on the transitions ``indices``
        (logical, (B,), or a ``ReplayDraw`` of a ``cursor=True`` buffer) of ``buffer``, as
        ``FusedSACRollout.actor_losses``: ``sample`` with ``noise`` (B, 1) -- by default ``torch.randn`` -- then ``q =
        min(twin.q(src, pos, actions))`` of ``twin``, a ``FusedTwinMLPCritic`` of this env, and

            actor_loss = -(q + -log_alpha.exp() * mean_log_probs).mean()
            alpha_loss = (-log_alpha.exp() * (mean_log_probs + target_entropy).detach()).mean()

        ``backward()`` of the actor loss also accumulates into the critics' ``.grad`` unless they are frozen (as in
        torch); an index outside ``[0, size)`` makes the actor loss NaN."""
        from .mlp_critic import FusedTwinMLPCritic
        from .replay import as_draw

        draw = as_draw(buffer, indices, "actor_losses")
        if not isinstance(twin, FusedTwinMLPCritic) or twin.env is not self.env:
            raise ValueError("twin must be a FusedTwinMLPCritic of this rollout's env")
        if indices is None:
            raise ValueError("actor_losses needs the indices of the sampled transitions")
        idx = twin._indices(buffer, indices if draw is None else draw.indices, None)
        B = int(idx.numel())
        if noise is None:
            noise = torch.randn((B, 1), device=self.env._dev)
        if draw is not None:  # the draw's gathered descriptors; its indices are in range by construction
            src, pos = draw.state_src, draw.state_pos.reshape(B)
            actions, log_probs = self.sample(src, pos, noise)
            q = torch.min(*twin.q(src, pos, actions))
        else:
            slots = buffer.physical(idx)
            src, pos = buffer.state_src[slots], buffer.state_pos[slots].reshape(B)
            actions, log_probs = self.sample(src, pos, noise)
            q = torch.min(*twin.q(src, pos, actions))
            valid = ((idx >= 0) & (idx < buffer.size())).reshape(B, 1)
            q = torch.where(valid, q, torch.full((), float("nan"), device=q.device))
        mean_log_probs = log_probs.mean(dim=1, keepdim=True)
        log_alpha = self.actor.log_alpha
        actor_loss = -(q + -log_alpha.exp() * mean_log_probs).mean()
        alpha_loss = (-log_alpha.exp() * (mean_log_probs + self.actor.target_entropy).detach()).mean()
        return actor_loss, alpha_loss


# ---------------------------------------------------------------- the torch restatement (host or device)
def torch_sac_mlp_actor_losses(actor, critic_1, critic_2, states, eps):
    """``Actor.compute_losses`` (SAC/actor.py:63-81) in torch with the standard normals ``eps`` given: states (B, W, 5)."""
    actions, log_probs = actor.get_actions_and_log_probs(states, eps)
    mean_log_probs = log_probs.mean(dim=1, keepdim=True)
    q = torch.min(critic_1(states, actions), critic_2(states, actions))
    actor_loss = -(q + -actor.log_alpha.exp() * mean_log_probs).mean()
    alpha_loss = (-actor.log_alpha.exp() * (mean_log_probs + actor.target_entropy).detach()).mean()
    return actor_loss, alpha_loss
