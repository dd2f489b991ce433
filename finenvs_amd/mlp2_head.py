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

import ctypes as C
from typing import Tuple

import torch
import torch.nn as nn

from . import _lib
from .mlp_head import MLP_HEAD_ACTIVATIONS, MLP_HEAD_HIDDEN_SIZES, MLP_HEAD_LAYER_ACTIVATIONS
from .rollout import FusedMLP2Rollout

MLP2_GRAD_KEYS = ("w1", "b1", "w2", "b2", "w3", "b3")  # fe_mlp2_grads' fields, in mlp2_head_parameters' order
MLP2_GRAD_CHUNK_PAIRS = _lib.MLP2_GRAD_CHUNK_PAIRS  # pairs per split of the two weight-gradient contractions
MLP2_MAX_WINDOW = _lib.MLP2_MAX_WINDOW  # {H: the largest window admitted with one asset}


class MLP2Head(nn.Module):
    """The reference's ``MLPNetwork((5W, H, H, 1), layer_activation, output_activation)`` as a plain module (no
    optimizer inside).  ``output_activation``: ``"tanh"`` (the actor) or ``"none"`` (the critic)."""

    def __init__(self, H: int = 128, W: int = 4, activation: str = "elu", output_activation: str = "tanh", device=None):
        super().__init__()
        if activation not in MLP_HEAD_LAYER_ACTIVATIONS:
            raise ValueError(f"activation must be one of {sorted(MLP_HEAD_LAYER_ACTIVATIONS)} (got {activation!r})")
        if output_activation not in MLP_HEAD_ACTIVATIONS:
            raise ValueError(f"output_activation must be one of {sorted(MLP_HEAD_ACTIVATIONS)} (got {output_activation!r}): "
                             '"clamp" bounds an action, it is not an output a learner trains through')
        self.hidden_size, self.sequence_length = int(H), int(W)
        self.activation, self.output_activation = activation, output_activation
        act = MLP_HEAD_LAYER_ACTIVATIONS[activation]
        self.network = nn.Sequential(nn.Linear(5 * self.sequence_length, self.hidden_size, device=device), act(),
                                     nn.Linear(self.hidden_size, self.hidden_size, device=device), act(),
                                     nn.Linear(self.hidden_size, 1, device=device),
                                     MLP_HEAD_ACTIVATIONS[output_activation]())

    def forward(self, states: torch.Tensor) -> torch.Tensor:
        """(B, W, 5) or (B, 5W) -> (B, 1)."""
        W = self.sequence_length
        if states.dim() == 3 and tuple(states.shape[1:]) == (W, 5):
            states = states.reshape(states.shape[0], 5 * W)
        elif states.dim() != 2 or states.shape[1] != 5 * W:
            raise ValueError(f"states must be (B, {W}, 5) or (B, {5 * W}), got {tuple(states.shape)}")
        return self.network(states)


def _layer_activation(layer: nn.Module):
    name = next((k for k, cls in MLP_HEAD_LAYER_ACTIVATIONS.items() if type(layer) is cls), None)
    if name is None or (name == "elu" and layer.alpha != 1.0):
        raise ValueError(f"the hidden activations must be ELU (alpha = 1), ReLU or Tanh (got {type(layer).__name__}"
                         + (f" with alpha = {layer.alpha}" if name == "elu" else "") + ")")
    return name


def check_mlp2_head(module: nn.Module) -> Tuple[int, int, str, str]:
    """(hidden size, window, activation, output activation) of a module the fused two-layer head can run; ValueError
    otherwise."""
    net = getattr(module, "network", None)
    if not isinstance(net, nn.Sequential) or len(net) != 6 or not all(isinstance(net[i], nn.Linear) for i in (0, 2, 4)):
        raise ValueError("the fused two-layer MLP head needs a module with `network = Sequential(Linear(5W, H), act, "
                         "Linear(H, H), act, Linear(H, 1), out)`: two hidden layers (one hidden layer is FusedMLPHead's)")
    first, second, last = net[0], net[2], net[4]
    H = int(first.out_features)
    if second.in_features != H or second.out_features != H:
        raise ValueError(f"both hidden layers must have the same width: Linear(5W, {H}) needs Linear({H}, {H}) "
                         f"(got Linear({second.in_features}, {second.out_features}))")
    if H not in MLP_HEAD_HIDDEN_SIZES:
        raise ValueError(f"the fused MLP head runs H in {MLP_HEAD_HIDDEN_SIZES} (got {H})")
    if first.in_features % 5 != 0 or first.in_features < 5:
        raise ValueError(f"the first layer must take a flattened (W, 5) window: in_features = 5 W (got {first.in_features})")
    if last.in_features != H or last.out_features != 1:
        raise ValueError(f"the last layer must be Linear({H}, 1): one output per (env, asset) pair")
    if first.bias is None or second.bias is None or last.bias is None:
        raise ValueError("all three layers need a bias")
    activation, activation2 = _layer_activation(net[1]), _layer_activation(net[3])
    if activation != activation2:
        raise ValueError(f"both hidden layers must use the same activation (got {activation} and {activation2})")
    if isinstance(net[5], nn.Tanh):
        return H, first.in_features // 5, activation, "tanh"
    if isinstance(net[5], nn.Identity):
        return H, first.in_features // 5, activation, "none"
    raise ValueError(f"the output activation must be Tanh or Identity (got {type(net[5]).__name__}): a clamp has no gradient "
                     "to train on")


def mlp2_head_parameters(module: nn.Module) -> Tuple[torch.Tensor, ...]:
    """The six parameter tensors of a head in ``MLP2_GRAD_KEYS`` order, which is ``named_parameters()``' order:
    ``network[0].weight (H, 5W)``, ``network[0].bias (H)``, ``network[2].weight (H, H)``, ``network[2].bias (H)``,
    ``network[4].weight (1, H)`` and ``network[4].bias (1)``."""
    net = module.network
    return net[0].weight, net[0].bias, net[2].weight, net[2].bias, net[4].weight, net[4].bias


class _MLP2HeadValue(torch.autograd.Function):
    """``FusedMLP2Rollout.forward`` as a differentiable function of the head's six parameters: the forward is
    ``fe_mlp2_forward``, the backward ``fe_mlp2_backward`` (both hidden layers recomputed)."""

    @staticmethod
    def forward(ctx, head, src, pos, *params):
        roll = head.rollout
        out = roll.forward(src, pos)
        ctx.set_materialize_grads(False)
        # the weight buffers forward() ran with: backward packs nothing again and makes no copy to the host
        ctx.head, ctx.packed = head, (roll.w1t, roll.wpos, roll.b1, roll.w2, roll.b2, roll.w3, roll.b3_dev)
        ctx.save_for_backward(src, pos, out)
        return out

    @staticmethod
    def backward(ctx, g_out):
        out = [None] * 9
        if g_out is None or not any(ctx.needs_input_grad[3:]):
            return tuple(out)
        head = ctx.head
        src, pos, values = ctx.saved_tensors
        env, H, B = head.env, head.H, int(src.numel())
        W, dev = int(env.num_intervals), env._dev
        shapes = {"w1": (H, 5 * W), "b1": (H,), "w2": (H, H), "b2": (H,), "w3": (1, H), "b3": (1,)}
        grads = [torch.empty(shapes[k], dtype=torch.float32, device=dev) for k in MLP2_GRAD_KEYS]
        if B:
            g_out = g_out.reshape(B).float().contiguous()
            ws = torch.empty((int(env._lib.fe_mlp2_grad_workspace_floats(H, W, B)),), dtype=torch.float32, device=dev)
            weights = _lib.FeMlp2Weights(*(t.data_ptr() for t in ctx.packed))
            mg = _lib.FeMlp2Grads(*(g.data_ptr() for g in grads))
            roll = head.rollout
            _lib.check(env._lib.fe_mlp2_backward(
                env._handle, roll._lr32.data_ptr(), C.byref(weights), H, roll.act, roll.out_act, src.data_ptr(),
                pos.data_ptr(), B, values.data_ptr(), g_out.data_ptr(), ws.data_ptr(), C.byref(mg), env._stream()), env._lib)
        else:
            for g in grads:
                g.zero_()
        for k in range(6):
            if ctx.needs_input_grad[3 + k]:
                out[3 + k] = grads[k]
        return tuple(out)


class FusedMLP2Head:
    """An ``MLP2Head`` (or the reference's network of that shape) trained on observation descriptors.

    ``head(obs_src, obs_pos)`` is ``module(env.render(obs_src, obs_pos).float())`` computed by ``fe_mlp2_forward`` --
    (B, 1) float32, differentiable with respect to the module's six parameters through ``fe_mlp2_backward``;
    ``backward()`` accumulates into their ``.grad`` as the torch module would.  ``.rollout`` is a ``FusedMLP2Rollout``
    acting with the same buffers.  The module's parameters are taken over on the device at every call (``refresh``:
    ``fe_mlp_pack`` for the first layer and five copies into fresh buffers, nothing goes to the host), so an optimizer
    step is seen by the next call and by the next ``rollout.run`` after a ``refresh()``.  The module must live on the
    env's device."""

    def __init__(self, env, module: nn.Module):
        self.H, W, self.activation, self.output_activation = check_mlp2_head(module)
        if W != int(env.num_intervals):
            raise ValueError(f"the module's first layer takes a window of {W} rows, the env renders {env.num_intervals}")
        if int(env.num_assets) != 1:
            raise ValueError(f"the fused MLP head trains one asset (the env has {env.num_assets}), as the fused LSTM head does")
        self.env, self.module = env, module
        w1, b1, w2, b2, w3, b3 = self._check_parameters()
        self.rollout = FusedMLP2Rollout(env, w1.detach().t(), b1, w2, b2, w3, 0.0, self.activation, self.output_activation)
        self.refresh()

    def _check_parameters(self) -> Tuple[torch.Tensor, ...]:
        params = mlp2_head_parameters(self.module)
        if any(p.dtype is not torch.float32 for p in params):
            raise ValueError("the fused MLP head's gradient needs float32 parameters")
        if any(p.device != torch.device(self.env._dev) for p in params):
            raise ValueError(f"the head's parameters must live on the env's device {self.env._dev}")
        return params

    def refresh(self) -> None:
        """The module's current parameters into ``self.rollout``, on the device into fresh buffers (``fe_mlp_pack`` for
        the first layer): no copy to the host, and a forward whose ``backward()`` is still pending keeps the weights it
        ran with."""
        w1, b1, w2, b2, w3, b3 = self._check_parameters()
        env, roll, H, dev = self.env, self.rollout, self.H, self.env._dev
        W = int(env.num_intervals)
        w1t = torch.empty((H, 4 * W), dtype=torch.float32, device=dev)
        wpos = torch.empty((H,), dtype=torch.float32, device=dev)
        _lib.check(env._lib.fe_mlp_pack(w1.detach().contiguous().data_ptr(), H, W, w1t.data_ptr(), wpos.data_ptr(),
                                        env._stream()), env._lib)
        roll.w1t, roll.wpos = w1t, wpos
        roll.b1, roll.w2 = b1.detach().reshape(H).clone(), w2.detach().reshape(H, H).clone()
        roll.b2, roll.w3 = b2.detach().reshape(H).clone(), w3.detach().reshape(H).clone()
        roll.b3_dev = b3.detach().reshape(1).clone()

    def __call__(self, obs_src: torch.Tensor, obs_pos: torch.Tensor) -> torch.Tensor:
        """The head on B observation descriptors (``obs_src (B,)`` int64, ``obs_pos (B,)`` or ``(B, 1)`` float64):
        (B, 1) float32, ``self.rollout.forward``'s values bit for bit."""
        env = self.env
        if not isinstance(obs_src, torch.Tensor) or not isinstance(obs_pos, torch.Tensor):
            raise ValueError("obs_src / obs_pos must be tensors of observation descriptors")
        B = int(obs_src.numel())
        if obs_pos.numel() != B:
            raise ValueError(f"obs_pos must hold one position per descriptor ({B}), got {tuple(obs_pos.shape)}")
        params = self._check_parameters()
        src = obs_src.reshape(B).to(device=env._dev, dtype=torch.int64).contiguous()
        pos = obs_pos.reshape(B, 1).to(device=env._dev, dtype=torch.float64).contiguous()
        if B:  # an empty batch packs nothing and launches nothing, in either direction
            self.refresh()
        return _MLP2HeadValue.apply(self, src, pos, *params)
