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

from . import _lib
from .mlp_critic import FusedTwinMLPCritic
from .mlp_head import MLP_HEAD_HIDDEN_SIZES, MLP_HEAD_LAYER_ACTIVATIONS, _layer_activation
from .rollout import FusedMLPRollout
from .sac import _FusedSAC, _SACActor

MLP_SAC_GRAD_KEYS = ("w1", "b1", "w2", "b2", "w_mu", "b_mu", "w_std", "b_std")  # fe_mlp_sac_grads' fields
MLP_SAC_MAX_WINDOW = _lib.MLP_SAC_MAX_WINDOW
MLP_SAC_STATE_DICT_KEYS = ("network.0.weight", "network.0.bias", "network.2.weight", "network.2.bias", "mu_layer.weight",
                           "mu_layer.bias", "std_layer.weight", "std_layer.bias")


class SACActorMLP(_SACActor):
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

    def forward(self, states: torch.Tensor) -> torch.Tensor:
        """(B, W, 5) or (B, 5W) -> the network's output z (B, H)."""
        W = self.sequence_length
        if states.dim() == 3 and tuple(states.shape[1:]) == (W, 5):
            states = states.reshape(states.shape[0], 5 * W)
        elif states.dim() != 2 or states.shape[1] != 5 * W:
            raise ValueError(f"states must be (B, {W}, 5) or (B, {5 * W}), got {tuple(states.shape)}")
        return self.network(states.to(self.network[0].weight.dtype))


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


class FusedMLPSACRollout(_FusedSAC):
    """K env steps per launch with the SAC MLP actor in the kernel (C ABI ``fe_env_rollout_mlp_sac``,
    include/finenvs_amd_mlp_sac.h), and its head on descriptors: ``FusedSACRollout``'s front end for a ``SACActorMLP``
    (or the reference's ``ActorMLP`` of that shape with one output).

    The actor's parameters are re-packed and re-folded on the device at every ``run`` / ``forward`` / ``sample`` (one
    allocation and one launch; ``sample`` also copies the eight tensors, which its ``backward()`` reads; nothing goes to
    the host: the biases are read on the device), so an optimizer step on ``actor`` is seen by the next call.  The actor must live on the env's device."""

    ENTRIES = {"rollout": "fe_env_rollout_mlp_sac", "forward": "fe_mlp_sac_forward", "backward": "fe_mlp_sac_backward",
               "workspace": "fe_mlp_sac_grad_workspace_floats"}
    GRADS, TWIN = _lib.FeMlpSacGrads, FusedTwinMLPCritic
    _grad_shapes = staticmethod(mlp_sac_grad_shapes)

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
        self._parameters()
        self._bind()

    def _parameters(self) -> Tuple[torch.Tensor, ...]:
        params = mlp_sac_parameters(self.actor)
        if any(p.device != torch.device(self.env._dev) for p in params):
            raise ValueError(f"the actor's parameters must live on the env's device {self.env._dev}")
        if any(p.dtype is not torch.float32 for p in params):
            raise ValueError("the fused SAC MLP actor needs float32 parameters")
        return params

    def _weights(self, snapshot: bool = False) -> "_lib.FeMlpSacWeights":
        self._parameters()
        self._packed = pack_mlp_sac_weights(self.env, self.actor, snapshot)  # kept alive until the launch has been queued
        return _weights_struct(self._packed)

    def _net_args(self, w):
        return self._lr32.data_ptr(), C.byref(w), self.H, self.act

    def _saved_args(self, x, biases=None):
        return self._net_args(_weights_struct(x))

    def folded(self) -> Dict[str, torch.Tensor]:
        """The device tensors the pack kernel wrote at the latest call: ``w1t`` (H, 4W), ``wpos`` (H), ``b1`` (H) and the
        fold ``v_mu``, ``v_s`` (H), ``c_mu``, ``c_s`` (1 each, views of one buffer).  Packs now if nothing ran yet."""
        if getattr(self, "_packed", None) is None:
            self._weights()
        x = self._packed
        return {"w1t": x["w1t"], "wpos": x["wpos"], "b1": x["b1"], "v_mu": x["vmu"], "v_s": x["vstd"],
                "c_mu": x["cfold"][0:1], "c_s": x["cfold"][1:2]}


# ---------------------------------------------------------------- the torch restatement (host or device)
def torch_sac_mlp_actor_losses(actor, critic_1, critic_2, states, eps):
    """``Actor.compute_losses`` (SAC/actor.py:63-81) in torch with the standard normals ``eps`` given: states (B, W, 5)."""
    actions, log_probs = actor.get_actions_and_log_probs(states, eps)
    mean_log_probs = log_probs.mean(dim=1, keepdim=True)
    q = torch.min(critic_1(states, actions), critic_2(states, actions))
    actor_loss = -(q + -actor.log_alpha.exp() * mean_log_probs).mean()
    alpha_loss = (-actor.log_alpha.exp() * (mean_log_probs + actor.target_entropy).detach()).mean()
    return actor_loss, alpha_loss
