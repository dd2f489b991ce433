"""The two-hidden-layer MLP head of the reference's MLP learners at their defaults: the torch module, and its fused
training path.

``MLP2Head`` restates ``MLPNetwork((5W, H, H, 1), layer_activation, output_activation)`` of
finenvs/agents/networks/multilayer_perceptron.py:6-26 -- ``network = Sequential(Linear(5W, H), act, Linear(H, H), act,
Linear(H, 1), out)`` on the flattened observation window: what ``PPOAgentMLP`` and ``TD3AgentMLP`` build with their
default ``hidden_dims=(128, 128)``.  Its submodule names are the reference's, so a reference ``state_dict`` (keys
``network.0.*``, ``network.2.*``, ``network.4.*``) loads unchanged.

``FusedMLP2Head`` evaluates such a module on observation descriptors (C ABI ``fe_mlp2_forward``) as a differentiable
function of its six parameters (C ABI ``fe_mlp2_backward``, include/finenvs_amd_mlp2_head.h): no observation is
rendered in either direction.  It owns the ``FusedMLP2Rollout`` that acts with the same weights in the kernel.  The
losses are those of finenvs_amd/lstm_head.py: ``ppo_actor_loss`` / ``ppo_critic_loss`` take this head as they take
``FusedMLPHead``.  Scope: one asset, two hidden layers of the same width H in {32, 64, 128}, the same activation in
both, a window whose weight image fits the LDS (``MLP2_MAX_WINDOW``).
"""
from __future__ import annotations

from typing import Tuple

import torch
import torch.nn as nn

from . import _lib
from .mlp_head import _FusedMLPDepth, _MLPModule, check_head
from .rollout import FusedMLP2Rollout

MLP2_GRAD_KEYS = ("w1", "b1", "w2", "b2", "w3", "b3")  # fe_mlp2_grads' fields, in mlp2_head_parameters' order
MLP2_GRAD_CHUNK_PAIRS = _lib.MLP2_GRAD_CHUNK_PAIRS  # pairs per split of the two weight-gradient contractions
MLP2_MAX_WINDOW = _lib.MLP2_MAX_WINDOW  # {H: the largest window admitted with one asset}


class MLP2Head(_MLPModule):
    """The reference's ``MLPNetwork((5W, H, H, 1), layer_activation, output_activation)`` as a plain module (no
    optimizer inside).  ``output_activation``: ``"tanh"`` (the actor) or ``"none"`` (the critic)."""

    HIDDEN_LAYERS = 2


def check_mlp2_head(module: nn.Module) -> Tuple[int, int, str, str]:
    """(hidden size, window, activation, output activation) of a module the fused two-layer head can run; ValueError
    otherwise."""
    return check_head(module, 2, "the fused two-layer MLP head needs a module with `network = Sequential(Linear(5W, H), act, "
                                 "Linear(H, H), act, Linear(H, 1), out)`: two hidden layers (one hidden layer is FusedMLPHead's)")


def mlp2_head_parameters(module: nn.Module) -> Tuple[torch.Tensor, ...]:
    """The six parameter tensors of a head in ``MLP2_GRAD_KEYS`` order, which is ``named_parameters()``' order:
    ``network[0].weight (H, 5W)``, ``network[0].bias (H)``, ``network[2].weight (H, H)``, ``network[2].bias (H)``,
    ``network[4].weight (1, H)`` and ``network[4].bias (1)``."""
    net = module.network
    return net[0].weight, net[0].bias, net[2].weight, net[2].bias, net[4].weight, net[4].bias


class FusedMLP2Head(_FusedMLPDepth):
    """An ``MLP2Head`` (or the reference's network of that shape) trained on observation descriptors.

    ``head(obs_src, obs_pos)`` is ``module(env.render(obs_src, obs_pos).float())`` computed by ``fe_mlp2_forward`` --
    (B, 1) float32, differentiable with respect to the module's six parameters through ``fe_mlp2_backward``;
    ``backward()`` accumulates into their ``.grad`` as the torch module would.  ``.rollout`` is a ``FusedMLP2Rollout``
    acting with the same buffers.  The module's parameters are taken over on the device at every call (``refresh``:
    ``fe_mlp_pack`` for the first layer and five copies into fresh buffers, nothing goes to the host), so an optimizer
    step is seen by the next call and by the next ``rollout.run`` after a ``refresh()``.  The module must live on the
    env's device."""

    GRAD_KEYS = MLP2_GRAD_KEYS
    WEIGHTS, GRADS = _lib.FeMlp2Weights, _lib.FeMlp2Grads
    WORKSPACE, BACKWARD = "fe_mlp2_grad_workspace_floats", "fe_mlp2_backward"
    PACKED = ("w1t", "wpos", "b1", "w2", "b2", "w3", "b3_dev")
    _check, _parameters = staticmethod(check_mlp2_head), staticmethod(mlp2_head_parameters)

    @staticmethod
    def grad_shapes(H: int, W: int):
        return (H, 5 * W), (H,), (H, H), (H,), (1, H), (1,)

    def _make_rollout(self, params) -> FusedMLP2Rollout:
        w1, b1, w2, b2, w3, _ = params
        return FusedMLP2Rollout(self.env, w1.detach().t(), b1, w2, b2, w3, 0.0, self.activation, self.output_activation)
