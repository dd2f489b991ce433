"""The one-hidden-layer MLP head of the reference's PPO learner: the torch module, and its fused training path.

``MLPHead`` restates ``MLPNetwork((5W, H, 1), layer_activation, output_activation)`` of
finenvs/agents/networks/multilayer_perceptron.py:6-26 -- ``network = Sequential(Linear(5W, H), act, Linear(H, 1), out)``
on the flattened observation window.  Two of the reference's networks are this module: PPO's ``ContinuousActorMLP``
(PPO/continuous_actor.py:81-101, ELU and Tanh) and PPO's ``CriticMLP`` (PPO/critic.py:35-50, ELU and Identity), the pair
``PPOAgentMLP`` (PPO/PPO_agent.py:209-243) trains.  Its submodule names are the reference's, so a reference ``state_dict``
(without the learner's own ``log_standard_deviation``) loads unchanged.

``FusedMLPHead`` evaluates such a module on observation descriptors (C ABI ``fe_mlp_forward``) as a differentiable
function of its four parameters (C ABI ``fe_mlp_backward``, include/finenvs_amd_mlp_head.h): no observation is rendered
in either direction.  It owns the ``FusedMLPRollout`` that acts with the same packed weights in the kernel.  The losses
are those of finenvs_amd/lstm_head.py: ``ppo_actor_loss`` / ``ppo_critic_loss`` take either head.  Scope: one asset, one
hidden layer of H in {32, 64, 128}, a window whose ``W1^T`` fits the LDS.
"""
from __future__ import annotations

import ctypes as C
from typing import Tuple

import torch
import torch.nn as nn

from . import _lib
from .lstm_head import _FusedHead
from .rollout import FusedMLPRollout

MLP_HEAD_HIDDEN_SIZES = FusedMLPRollout.HIDDEN_SIZES
MLP_HEAD_LAYER_ACTIVATIONS = {"elu": nn.ELU, "relu": nn.ReLU, "tanh": nn.Tanh}
MLP_HEAD_ACTIVATIONS = {"tanh": nn.Tanh, "none": nn.Identity}
MLP_GRAD_KEYS = ("w1", "b1", "w2", "b2")  # fe_mlp_grads' fields, in mlp_head_parameters' order
MLP_GRAD_CHUNK_PAIRS = _lib.MLP_GRAD_CHUNK_PAIRS  # pairs per split of the weight-gradient contraction


class _MLPModule(nn.Module):
    """The reference's ``MLPNetwork((5W, H, ..., 1), layer_activation, output_activation)`` with ``HIDDEN_LAYERS`` hidden
    layers of width H as a plain module (no optimizer inside); ``MLPHead`` and ``MLP2Head`` are its two depths."""

    HIDDEN_LAYERS = 1

    def __init__(self, H: int = 128, W: int = 4, activation: str = "elu", output_activation: str = "tanh", device=None):
        super().__init__()
        if activation not in MLP_HEAD_LAYER_ACTIVATIONS:
            raise ValueError(f"activation must be one of {sorted(MLP_HEAD_LAYER_ACTIVATIONS)} (got {activation!r})")
        if output_activation not in MLP_HEAD_ACTIVATIONS:
            raise ValueError(f"output_activation must be one of {sorted(MLP_HEAD_ACTIVATIONS)} (got {output_activation!r}): "
                             '"clamp" bounds an action, it is not an output a learner trains through')
        self.hidden_size, self.sequence_length = int(H), int(W)
        self.activation, self.output_activation = activation, output_activation
        layers, width = [], 5 * self.sequence_length
        for _ in range(self.HIDDEN_LAYERS):
            layers += [nn.Linear(width, self.hidden_size, device=device), MLP_HEAD_LAYER_ACTIVATIONS[activation]()]
            width = self.hidden_size
        self.network = nn.Sequential(*layers, nn.Linear(width, 1, device=device), MLP_HEAD_ACTIVATIONS[output_activation]())

    def forward(self, states: torch.Tensor) -> torch.Tensor:
        """(B, W, 5) or (B, 5W) -> (B, 1)."""
        W = self.sequence_length
        if states.dim() == 3 and tuple(states.shape[1:]) == (W, 5):
            states = states.reshape(states.shape[0], 5 * W)
        elif states.dim() != 2 or states.shape[1] != 5 * W:
            raise ValueError(f"states must be (B, {W}, 5) or (B, {5 * W}), got {tuple(states.shape)}")
        return self.network(states)


class MLPHead(_MLPModule):
    """The reference's ``MLPNetwork((5W, H, 1), layer_activation, output_activation)`` as a plain module (no optimizer
    inside): ``network = Sequential(Linear(5W, H), ELU() | ReLU() | Tanh(), Linear(H, 1), Tanh() | Identity())``.
    ``output_activation``: ``"tanh"`` (the actor) or ``"none"`` (the critic)."""


def _layer_activation(layer: nn.Module) -> str:
    name = next((k for k, cls in MLP_HEAD_LAYER_ACTIVATIONS.items() if type(layer) is cls), None)
    if name is None or (name == "elu" and layer.alpha != 1.0):
        raise ValueError(f"the hidden activations must be ELU (alpha = 1), ReLU or Tanh (got {type(layer).__name__}"
                         + (f" with alpha = {layer.alpha}" if name == "elu" else "") + ")")
    return name


def check_head(module: nn.Module, hidden_layers: int, shape_error: str) -> Tuple[int, int, str, str]:
    """(hidden size, window, activation, output activation) of a module with ``hidden_layers`` hidden layers that a fused
    head can run; ValueError otherwise -- ``shape_error`` when ``module.network`` is not that ``Sequential``."""
    net = getattr(module, "network", None)
    linear = range(0, 2 * hidden_layers + 1, 2)
    if not isinstance(net, nn.Sequential) or len(net) != 2 * hidden_layers + 2 \
            or not all(isinstance(net[i], nn.Linear) for i in linear):
        raise ValueError(shape_error)
    layers = [net[i] for i in linear]
    first, last = layers[0], layers[-1]
    H = int(first.out_features)
    for layer in layers[1:-1]:
        if layer.in_features != H or layer.out_features != H:
            raise ValueError(f"both hidden layers must have the same width: Linear(5W, {H}) needs Linear({H}, {H}) "
                             f"(got Linear({layer.in_features}, {layer.out_features}))")
    if H not in MLP_HEAD_HIDDEN_SIZES:
        raise ValueError(f"the fused MLP head runs H in {MLP_HEAD_HIDDEN_SIZES} (got {H})")
    if first.in_features % 5 != 0 or first.in_features < 5:
        raise ValueError(f"the first layer must take a flattened (W, 5) window: in_features = 5 W (got {first.in_features})")
    if last.in_features != H or last.out_features != 1:
        raise ValueError(f"the last layer must be Linear({H}, 1): one output per (env, asset) pair")
    if any(layer.bias is None for layer in layers):
        raise ValueError(f"all {len(layers)} layers need a bias")
    activations = [_layer_activation(net[i]) for i in range(1, 2 * hidden_layers, 2)]
    if len(set(activations)) != 1:
        raise ValueError(f"both hidden layers must use the same activation (got {' and '.join(activations)})")
    output = "tanh" if isinstance(net[-1], nn.Tanh) else ("none" if isinstance(net[-1], nn.Identity) else None)
    if output is None:
        raise ValueError(f"the output activation must be Tanh or Identity (got {type(net[-1]).__name__}): a clamp has no "
                         "gradient to train on")
    return H, first.in_features // 5, activations[0], output


def check_mlp_head(module: nn.Module) -> Tuple[int, int, str, str]:
    """(hidden size, window, activation, output activation) of a module the fused head can run; ValueError otherwise."""
    return check_head(module, 1, "the fused MLP head needs a module with `network = Sequential(Linear(5W, H), act, Linear(H, 1), "
                                 "out)`: one hidden layer (the reference's default of two needs another kernel)")


def mlp_head_parameters(module: nn.Module) -> Tuple[torch.Tensor, ...]:
    """The four parameter tensors of a head in ``MLP_GRAD_KEYS`` order: ``network[0].weight (H, 5W)``, ``network[0].bias
    (H)``, ``network[2].weight (1, H)`` and ``network[2].bias (1)``."""
    first, last = module.network[0], module.network[2]
    return first.weight, first.bias, last.weight, last.bias


class _FusedMLPDepth(_FusedHead):
    """What ``FusedMLPHead`` and ``FusedMLP2Head`` share on top of ``_FusedHead`` (finenvs_amd/lstm_head.py): the
    constructor, ``refresh`` and the backward launch.  A depth names: ``GRAD_KEYS`` and ``grad_shapes(H, W)`` (the
    gradients, in its parameters' order), ``WEIGHTS`` / ``GRADS`` (the ctypes structs), ``WORKSPACE`` / ``BACKWARD`` (the C
    entries), ``PACKED`` (the rollout's attributes that fill ``WEIGHTS``: ``w1t``, ``wpos``, then one per parameter after
    the first), ``_check`` / ``_parameters`` (of the module) and ``_make_rollout``."""

    _DTYPE_ERROR = "the fused MLP head's gradient needs float32 parameters"

    def __init__(self, env, module: nn.Module):
        self.H, W, self.activation, self.output_activation = self._check(module)
        if W != int(env.num_intervals):
            raise ValueError(f"the module's first layer takes a window of {W} rows, the env renders {env.num_intervals}")
        if int(env.num_assets) != 1:
            raise ValueError(f"the fused MLP head trains one asset (the env has {env.num_assets}), as the fused LSTM head does")
        self.env, self.module = env, module
        self.rollout = self._make_rollout(self._check_parameters())
        self.refresh()

    def refresh(self) -> None:
        """The module's current parameters into ``self.rollout``, on the device into fresh buffers (``fe_mlp_pack`` for
        the first layer, a copy of each other tensor): no copy to the host, and a forward whose ``backward()`` is still
        pending keeps the weights it ran with."""
        params = self._check_parameters()
        env, roll, H, dev = self.env, self.rollout, self.H, self.env._dev
        W = int(env.num_intervals)
        w1t = torch.empty((H, 4 * W), dtype=torch.float32, device=dev)
        wpos = torch.empty((H,), dtype=torch.float32, device=dev)
        _lib.check(env._lib.fe_mlp_pack(params[0].detach().contiguous().data_ptr(), H, W, w1t.data_ptr(), wpos.data_ptr(),
                                        env._stream()), env._lib)
        roll.w1t, roll.wpos = w1t, wpos
        for name, p in zip(self.PACKED[2:], params[1:]):  # a (1, H) output weight is kept as (H)
            setattr(roll, name, p.detach().reshape(p.shape[-1:] if p.shape[0] == 1 else p.shape).clone())

    def _backward(self, packed, src, pos, B, values, g_out, ws, grads) -> None:
        env, roll = self.env, self.rollout
        weights = self.WEIGHTS(*(t.data_ptr() for t in packed))
        _lib.check(getattr(env._lib, self.BACKWARD)(
            env._handle, roll._lr32.data_ptr(), C.byref(weights), self.H, roll.act, roll.out_act, src.data_ptr(),
            pos.data_ptr(), B, values.data_ptr(), g_out.data_ptr(), ws.data_ptr(), C.byref(grads), env._stream()), env._lib)


class FusedMLPHead(_FusedMLPDepth):
    """An ``MLPHead`` (or the reference's network of that shape) trained on observation descriptors.

    ``head(obs_src, obs_pos)`` is ``module(env.render(obs_src, obs_pos).float())`` computed by ``fe_mlp_forward`` --
    (B, 1) float32, differentiable with respect to the module's four parameters through ``fe_mlp_backward``;
    ``backward()`` accumulates into their ``.grad`` as the torch module would.  ``.rollout`` is a ``FusedMLPRollout``
    acting with the same packed buffers: ``run`` steps the env with them (sampled, into a trajectory chunk),
    ``forward`` is the head without autograd.  The module's parameters are re-packed on the device at every call
    (``refresh``: ``fe_mlp_pack`` and three small copies, nothing goes to the host), so an optimizer step is seen by
    the next call and by the next ``rollout.run`` after a ``refresh()``.  The module must live on the env's device."""

    GRAD_KEYS = MLP_GRAD_KEYS
    WEIGHTS, GRADS = _lib.FeMlpWeights, _lib.FeMlpGrads
    WORKSPACE, BACKWARD = "fe_mlp_grad_workspace_floats", "fe_mlp_backward"
    PACKED = ("w1t", "wpos", "b1", "w2", "b2_dev")
    _check, _parameters = staticmethod(check_mlp_head), staticmethod(mlp_head_parameters)

    @staticmethod
    def grad_shapes(H: int, W: int):
        return (H, 5 * W), (H,), (1, H), (1,)

    def _make_rollout(self, params) -> FusedMLPRollout:
        w1, b1, w2, _ = params
        rollout = FusedMLPRollout(self.env, w1.detach().t(), b1, w2, 0.0, self.activation, self.output_activation)
        rollout.b2 = None  # the output bias lives on the device (rollout.b2_dev): nothing of this head's weights on the host
        return rollout
