"""TD3's and SAC's twin MLP critics Q(s, a): the torch module a learner trains, and the fused path on descriptors.

``MLPCritic`` restates the reference's ``CriticMLP((5W + 1, H, H, 1))`` (finenvs/agents/TD3/critic.py:49-64, the same
class in agents/SAC/critic.py:48-58; networks/multilayer_perceptron.py:6-26) for one asset: ``network = Sequential(
Linear(5W + 1, H), act, Linear(H, H), act, Linear(H, 1), Identity())`` on ``cat([states.flatten(1), actions], dim=1)``
(agent_utils.py:5-14 with 2-D states), so the action is input column 5W.  ``TD3AgentMLP`` builds two of them and two
targets with ``hidden_dims=(128, 128)``.  Its submodule names are the reference's, so a reference ``state_dict`` (keys
``network.0.*``, ``network.2.*``, ``network.4.*``) loads unchanged.

``FusedTwinMLPCritic`` is ``FusedTwinCritic``'s front end (finenvs_amd/critic.py) for two such critics: values on
observation descriptors (C ABI ``fe_twin_mlpq_forward``, include/finenvs_amd_mlp_critic.h), ``q`` as a differentiable
function of the actions and both critics' parameters (``fe_twin_mlpq_backward``), ``critic_loss`` on replayed
transitions, ``td3_targets`` straight from the replay ring (``fe_twin_mlpq_target``), the target actor a
``FusedMLP2Rollout``, and ``sac_targets`` with a ``FusedMLPSACRollout`` (finenvs_amd/mlp_sac.py) as the actor.  Nothing is
rendered.  Scope: one asset, two hidden layers of the same width H in {32, 64, 128} and the same activation, a window the
two-layer head admits (``MLP2_MAX_WINDOW``).
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch
import torch.nn as nn

from . import _lib
from .critic import _FusedTwin
from .mlp_head import MLP_HEAD_HIDDEN_SIZES, MLP_HEAD_LAYER_ACTIVATIONS, _layer_activation
from .rollout import FusedMLP2Rollout, log_return_f32

MLPQ_GRAD_KEYS = ("w1", "b1", "w2", "b2", "w3", "b3")  # fe_mlpq_grads' fields, in mlp_critic_parameters' order
MLPQ_GRAD_CHUNK_PAIRS = _lib.MLPQ_GRAD_CHUNK_PAIRS


class MLPCritic(nn.Module):
    """The reference's ``CriticMLP((5W + 1, H, H, 1))`` as a plain module (no optimizer inside)."""

    def __init__(self, H: int = 128, W: int = 4, activation: str = "elu", device=None):
        super().__init__()
        if activation not in MLP_HEAD_LAYER_ACTIVATIONS:
            raise ValueError(f"activation must be one of {sorted(MLP_HEAD_LAYER_ACTIVATIONS)} (got {activation!r})")
        self.hidden_size, self.sequence_length, self.activation = int(H), int(W), activation
        act = MLP_HEAD_LAYER_ACTIVATIONS[activation]
        H, W = self.hidden_size, self.sequence_length
        self.network = nn.Sequential(nn.Linear(5 * W + 1, H, device=device), act(), nn.Linear(H, H, device=device), act(),
                                     nn.Linear(H, 1, device=device), nn.Identity())

    def forward(self, states: torch.Tensor, actions: torch.Tensor) -> torch.Tensor:
        """states (B, W, 5) or (B, 5W), actions (B, 1) -> Q (B, 1)."""
        W = self.sequence_length
        if states.dim() == 3 and tuple(states.shape[1:]) == (W, 5):
            states = states.reshape(states.shape[0], 5 * W)
        elif states.dim() != 2 or states.shape[1] != 5 * W:
            raise ValueError(f"states must be (B, {W}, 5) or (B, {5 * W}), got {tuple(states.shape)}")
        if actions.dim() != 2 or tuple(actions.shape) != (states.shape[0], 1):
            raise ValueError(f"actions must be ({states.shape[0]}, 1), got {tuple(actions.shape)}")
        return self.network(torch.cat([states, actions], dim=1))


def check_mlp_critic(critic: nn.Module) -> Tuple[int, int, str]:
    """(hidden size, window, activation) of a critic the fused twin MLP critic can run; ValueError otherwise."""
    net = getattr(critic, "network", None)
    if not isinstance(net, nn.Sequential) or len(net) != 6 or not all(isinstance(net[i], nn.Linear) for i in (0, 2, 4)):
        raise ValueError("the fused MLP critic needs a module with `network = Sequential(Linear(5W + 1, H), act, Linear(H, H), "
                         "act, Linear(H, 1), Identity())`")
    first, second, last = net[0], net[2], net[4]
    H = int(first.out_features)
    if second.in_features != H or second.out_features != H:
        raise ValueError(f"both hidden layers must have the same width: Linear(5W + 1, {H}) needs Linear({H}, {H}) "
                         f"(got Linear({second.in_features}, {second.out_features}))")
    if H not in MLP_HEAD_HIDDEN_SIZES:
        raise ValueError(f"the fused MLP critic runs H in {MLP_HEAD_HIDDEN_SIZES} (got {H})")
    if first.in_features % 5 != 1 or first.in_features < 6:
        raise ValueError("the first layer must take a flattened (W, 5) window and one action: in_features = 5 W + 1 "
                         f"(got {first.in_features})")
    if last.in_features != H or last.out_features != 1:
        raise ValueError(f"the last layer must be Linear({H}, 1)")
    if any(layer.bias is None for layer in (first, second, last)):
        raise ValueError("all 3 layers need a bias")
    activations = [_layer_activation(net[1]), _layer_activation(net[3])]
    if activations[0] != activations[1]:
        raise ValueError(f"both hidden layers must use the same activation (got {' and '.join(activations)})")
    if not isinstance(net[5], nn.Identity):
        raise ValueError(f"the output activation must be Identity (got {type(net[5]).__name__})")
    return H, (first.in_features - 1) // 5, activations[0]


def mlp_critic_parameters(critic: nn.Module) -> Tuple[torch.Tensor, ...]:
    """The six parameter tensors of a critic in ``MLPQ_GRAD_KEYS`` order, which is ``named_parameters()``' order:
    ``network[0].weight (H, 5W + 1)``, ``network[0].bias (H)``, ``network[2].weight (H, H)``, ``network[2].bias (H)``,
    ``network[4].weight (1, H)`` and ``network[4].bias (1)``."""
    net = critic.network
    return net[0].weight, net[0].bias, net[2].weight, net[2].bias, net[4].weight, net[4].bias


def pack_mlp_critic_weights(env, critic: nn.Module) -> Dict[str, torch.Tensor]:
    """The critic's current parameters as ``fe_mlpq_weights`` reads them (f32, on the parameters' device, no host sync):
    ``w1t`` / ``wpos`` by ``fe_mlp_pack`` from a contiguous copy of the first 5W columns of ``network[0].weight``,
    ``wact`` its last column, and a copy of each other tensor (fresh buffers: a forward whose ``backward()`` is still
    pending keeps the weights it ran with)."""
    H, W, _ = check_mlp_critic(critic)
    w1, b1, w2, b2, w3, b3 = (p.detach() for p in mlp_critic_parameters(critic))
    dev = w1.device
    w1t = torch.empty((H, 4 * W), dtype=torch.float32, device=dev)
    wpos = torch.empty((H,), dtype=torch.float32, device=dev)
    obs = w1[:, :5 * W].contiguous()
    _lib.check(env._lib.fe_mlp_pack(obs.data_ptr(), H, W, w1t.data_ptr(), wpos.data_ptr(), env._stream()), env._lib)
    return {"w1t": w1t, "wpos": wpos, "wact": w1[:, 5 * W].contiguous(), "b1": b1.clone(), "w2": w2.contiguous().clone(),
            "b2": b2.clone(), "w3": w3.reshape(H).clone(), "b3": b3.reshape(1).clone(), "_obs": obs}


def _weights_struct(x: Dict[str, torch.Tensor]) -> "_lib.FeMlpqWeights":
    return _lib.FeMlpqWeights(*(x[k].data_ptr() for k, _ in _lib.FeMlpqWeights._fields_))


def mlpq_grad_shapes(H: int, W: int):
    return (H, 5 * W + 1), (H,), (H, H), (H,), (1, H), (1,)


class FusedTwinMLPCritic(_FusedTwin):
    """Two MLP critics of the same H and activation evaluated together on the device (C ABI of
    include/finenvs_amd_mlp_critic.h): ``FusedTwinCritic``'s front end -- ``forward`` / ``__call__``, ``q``,
    ``critic_loss(buffer, indices, targets)``, ``td3_targets(...)`` and ``.last`` -- for ``MLPCritic`` modules (or the
    reference's ``CriticMLP`` of that shape).

    The critics' parameters are re-packed on the device at every call (``fe_mlp_pack`` for the observation columns and a
    copy of each other tensor, no host round trip), so an optimizer step or a soft update is seen by the next call.
    Both critics must live on the env's device."""

    def __init__(self, env, critic_1: nn.Module, critic_2: nn.Module):
        if int(env.num_assets) != 1:
            raise ValueError(f"the fused twin MLP critic runs one asset (the env has {env.num_assets}): the reference's "
                             "critic for A > 1 takes the whole env's window and all its actions, not a per-(env, asset) pair")
        (H1, W1, a1), (H2, W2, a2) = check_mlp_critic(critic_1), check_mlp_critic(critic_2)
        if H1 != H2:
            raise ValueError(f"the two critics must have the same hidden size (got {H1} and {H2})")
        if a1 != a2:
            raise ValueError(f"the two critics must use the same activation (got {a1} and {a2})")
        for name, W in (("critic_1", W1), ("critic_2", W2)):
            if W != int(env.num_intervals):
                raise ValueError(f"{name}'s first layer takes {5 * W + 1} inputs, a window of {W} rows and one action; the env "
                                 f"renders {env.num_intervals} rows: in_features must be {5 * int(env.num_intervals) + 1}")
        if int(env.num_intervals) > _lib.MLP2_MAX_WINDOW[H1]:
            raise ValueError(f"a window of {env.num_intervals} rows does not fit the LDS at H = {H1} (at most "
                             f"{_lib.MLP2_MAX_WINDOW[H1]})")
        self.env, self.critic_1, self.critic_2, self.H = env, critic_1, critic_2, H1
        self.activation, self.act = a1, FusedMLP2Rollout.ACTIVATIONS[a1]
        self._check_devices()
        self._lr32 = log_return_f32(env)
        self.last: Dict[str, torch.Tensor] = {}

    ENTRIES = {"forward": "fe_twin_mlpq_forward", "backward": "fe_twin_mlpq_backward",
               "workspace": "fe_twin_mlpq_grad_workspace_floats"}
    GRADS = _lib.FeMlpqGrads
    _parameters, _struct = staticmethod(mlp_critic_parameters), staticmethod(_weights_struct)
    _DTYPE_ERROR = "the fused MLP critic's gradient needs float32 parameters"

    def _weights(self):
        self._check_devices()
        self._packed = [pack_mlp_critic_weights(self.env, c) for c in (self.critic_1, self.critic_2)]  # alive until queued
        return [_weights_struct(x) for x in self._packed]

    def _empty_grads(self):
        shapes = mlpq_grad_shapes(self.H, int(self.env.num_intervals))
        return [torch.empty(shape, dtype=torch.float32, device=self.env._dev) for shape in shapes]

    def _shape_args(self):
        return (self.H, self.act)

    def _target_entry(self, cursor: bool):
        return self.env._lib.fe_twin_mlpq_target_c if cursor else self.env._lib.fe_twin_mlpq_target

    def _check_target_actor(self, target_actor) -> None:
        if not isinstance(target_actor, FusedMLP2Rollout) or target_actor.out_act != 0 or target_actor.env is not self.env:
            raise ValueError('target_actor must be a FusedMLP2Rollout of this env with output_activation="tanh" (e.g. '
                             "FusedMLP2Head(...).rollout)")

    def _check_sac_actor(self, actor_roll) -> None:
        from .mlp_sac import FusedMLPSACRollout

        if not isinstance(actor_roll, FusedMLPSACRollout) or actor_roll.env is not self.env:
            raise ValueError("actor_roll must be a FusedMLPSACRollout of this env (the SAC MLP actor)")


# ---------------------------------------------------------------- the torch restatements (host or device)
def torch_mlp_critic_loss(critic_1, critic_2, states, actions, targets) -> torch.Tensor:
    """``Critic.compute_loss`` (TD3/critic.py:31-46) of both critics: ``MSE(q1, y) + MSE(q2, y)``."""
    mse = nn.functional.mse_loss
    return mse(critic_1(states, actions), targets) + mse(critic_2(states, actions), targets)


def torch_td3_actor_loss(actor, critic_1, states) -> torch.Tensor:
    """``Actor.compute_loss(states, critic_1)`` (TD3/actor.py:50-56): ``-critic_1(states, actor(states)).mean()``."""
    return -critic_1(states, actor(states)).mean()
