"""The one-output LSTM head of the reference's PPO and TD3 learners: the torch module, and its fused training path.

``LSTMHead`` restates ``LSTMNetwork((5, H, 1), sequence_length=W, output_activation)`` of
finenvs/agents/networks/lstm.py:28-57 -- ``nn.LSTM(5, H)`` over the observation window, ``last_layer = Linear(H, 1)``
on the last hidden state, then ``Tanh`` or ``Identity``.  Three of the reference's networks are this module:
PPO's ``ContinuousActorLSTM`` (PPO/continuous_actor.py:104-124, tanh), PPO's ``CriticLSTM`` (PPO/critic.py:53-68,
identity) and TD3's ``ActorLSTM`` (TD3/actor.py:83-94, tanh).  Its submodule names are the reference's, so a reference
``state_dict`` (without the learner's own ``log_standard_deviation``) loads unchanged.

``FusedLSTMHead`` evaluates such a module on observation descriptors (C ABI ``fe_lstm_forward``) as a differentiable
function of its six parameters (C ABI ``fe_lstm_backward``, include/finenvs_amd_lstm_grad.h): no observation is
rendered in either direction.  It owns the ``FusedLSTMRollout`` that acts with the same parameters in the kernel.
``ppo_actor_loss`` / ``ppo_critic_loss`` / ``td3_actor_loss`` are the reference's three losses on that output; with
``fused=True`` the two PPO losses and their gradients are one launch each (include/finenvs_amd_ppo.h).  Scope:
one asset, H in {32, 64, 128}; with ``streamed=True`` also H in {256, 512, 1024} (C ABI ``fe_lstm_backward_streamed``,
include/finenvs_amd_lstm_grad_streamed.h).
"""
from __future__ import annotations

import ctypes as C
from typing import TYPE_CHECKING, Tuple, Union

import torch
import torch.nn as nn
from torch.distributions import Normal

from . import _lib
from .rollout import FusedLSTMRollout, lstm_fragment_major, lstm_pack

if TYPE_CHECKING:
    from .mlp_head import FusedMLPHead

LSTM_HEAD_HIDDEN_SIZES = (32, 64, 128)
LSTM_HEAD_STREAMED_HIDDEN_SIZES = (256, 512, 1024)  # with streamed=True
LSTM_HEAD_ACTIVATIONS = {"tanh": nn.Tanh, "none": nn.Identity}
LSTM_GRAD_KEYS = ("w_ih", "w_hh", "b_ih", "b_hh", "w_out", "b_out")  # fe_lstm_grads' fields, in head_parameters' order


class LSTMHead(nn.Module):
    """The reference's ``LSTMNetwork((5, H, 1), sequence_length=W, output_activation)`` as a plain module (no optimizer
    inside): ``lstm = nn.LSTM(5, H, batch_first=True)`` and ``last_layer = Sequential(Linear(H, 1), Tanh() |
    Identity())``.  ``output_activation``: ``"tanh"`` (the two actors) or ``"none"`` (PPO's critic)."""

    def __init__(self, H: int = 128, W: int = 4, output_activation: str = "tanh", device=None):
        super().__init__()
        if output_activation not in LSTM_HEAD_ACTIVATIONS:
            raise ValueError(f"output_activation must be one of {sorted(LSTM_HEAD_ACTIVATIONS)} (got {output_activation!r}): "
                             '"clamp" bounds an action, it is not an output a learner trains through')
        self.input_size, self.hidden_size, self.output_size, self.sequence_length = 5, int(H), 1, int(W)
        self.output_activation = output_activation
        self.lstm = nn.LSTM(5, self.hidden_size, num_layers=1, batch_first=True, device=device)
        self.last_layer = nn.Sequential(nn.Linear(self.hidden_size, 1, device=device),
                                        LSTM_HEAD_ACTIVATIONS[output_activation]())

    def forward(self, states: torch.Tensor) -> torch.Tensor:
        """(B, W, 5) -> (B, 1)."""
        if states.dim() != 3 or states.shape[1] != self.sequence_length or states.shape[2] != self.input_size:
            raise ValueError(f"states must be (B, {self.sequence_length}, {self.input_size}), got {tuple(states.shape)}")
        out, _ = self.lstm(states)
        return self.last_layer(out[:, -1, :])


def check_head(module: nn.Module, streamed: bool = False) -> Tuple[int, str]:
    """(hidden size, output activation) of a module the fused head can run; ValueError otherwise.  ``streamed``: H may
    also be 256, 512 or 1024 (the chunked backward of ``fe_lstm_backward_streamed``)."""
    lstm = getattr(module, "lstm", None)
    if not isinstance(lstm, nn.LSTM):
        raise ValueError("the fused LSTM head needs a module with an nn.LSTM `lstm`")
    if lstm.num_layers != 1 or lstm.bidirectional or lstm.input_size != 5 or not lstm.batch_first or lstm.proj_size:
        raise ValueError("the fused LSTM head needs nn.LSTM(5, H, num_layers=1, batch_first=True)")
    H = int(lstm.hidden_size)
    if streamed and H not in LSTM_HEAD_HIDDEN_SIZES + LSTM_HEAD_STREAMED_HIDDEN_SIZES:
        raise ValueError(f"the fused LSTM head trains H in {LSTM_HEAD_HIDDEN_SIZES + LSTM_HEAD_STREAMED_HIDDEN_SIZES} "
                         f"(got {H})")
    if not streamed and H not in LSTM_HEAD_HIDDEN_SIZES:
        raise ValueError(f"the fused LSTM head trains H in {LSTM_HEAD_HIDDEN_SIZES} (got {H}): the streamed-weight forward "
                         "of H >= 256 has no register-resident recurrence for a backward to mirror"
                         + ("; pass streamed=True for the chunked backward of H in "
                            f"{LSTM_HEAD_STREAMED_HIDDEN_SIZES}" if H in LSTM_HEAD_STREAMED_HIDDEN_SIZES else ""))
    last = getattr(module, "last_layer", None)
    if not isinstance(last, nn.Sequential) or len(last) != 2 or not isinstance(last[0], nn.Linear) \
            or last[0].in_features != H or last[0].out_features != 1 or last[0].bias is None:
        raise ValueError(f"last_layer must be Sequential(Linear({H}, 1), Tanh() or Identity()): one output per (env, asset) "
                         "pair")
    if isinstance(last[1], nn.Tanh):
        return H, "tanh"
    if isinstance(last[1], nn.Identity):
        return H, "none"
    raise ValueError(f"the output activation must be Tanh or Identity (got {type(last[1]).__name__}): a clamp has no "
                     "gradient to train on")


def head_parameters(module: nn.Module) -> Tuple[torch.Tensor, ...]:
    """The six parameter tensors of a head in ``LSTM_GRAD_KEYS`` order: ``lstm.weight_ih_l0 (4H, 5)``, ``weight_hh_l0
    (4H, H)``, ``bias_ih_l0``, ``bias_hh_l0`` (4H), ``last_layer[0].weight (1, H)`` and ``.bias (1)``."""
    lstm, last = module.lstm, module.last_layer[0]
    return lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0, last.weight, last.bias


class _HeadValue(torch.autograd.Function):
    """``head.rollout.forward`` as a differentiable function of the head's parameters: the forward is the rollout's
    forward entry, the backward the head's ``_backward`` launch (the same activations, recomputed)."""

    @staticmethod
    def forward(ctx, head, src, pos, *params):
        roll = head.rollout
        out = roll.forward(src, pos)
        ctx.set_materialize_grads(False)
        # the weight buffers forward() ran with: backward packs nothing again and makes no copy to the host
        ctx.head, ctx.packed = head, tuple(getattr(roll, name) for name in head.PACKED)
        ctx.version = None if head.weights is None else head.weights.version
        ctx.save_for_backward(src, pos, out)
        return out

    @staticmethod
    def backward(ctx, g_out):
        head, need = ctx.head, ctx.needs_input_grad
        out = [None] * len(need)
        if g_out is None or not any(need[3:]):
            return tuple(out)
        src, pos, values = ctx.saved_tensors
        env, H, B = head.env, head.H, int(src.numel())
        W, dev = int(env.num_intervals), env._dev
        grads = [torch.empty(shape, dtype=torch.float32, device=dev) for shape in head.grad_shapes(H, W)]
        if B:
            g_out = g_out.reshape(B).float().contiguous()
            ws = torch.empty((int(getattr(env._lib, head.WORKSPACE)(H, W, B)),), dtype=torch.float32, device=dev)
            if head.weights is not None:
                head.weights.check_version(ctx.version)
            sg = head.GRADS(*(g.data_ptr() for g in grads))
            head._backward(ctx.packed, src, pos, B, values, g_out, ws, sg)
        else:
            for g in grads:
                g.zero_()
        for k, g in enumerate(grads):
            if need[3 + k]:
                out[3 + k] = g
        return tuple(out)


class _FusedHead:
    """What ``FusedLSTMHead``, ``FusedMLPHead`` and ``FusedMLP2Head`` (finenvs_amd/mlp_head.py, mlp2_head.py) share: the
    checks of the descriptors and of the module's parameters, and the call with its autograd function.  A family
    provides ``env``, ``module``, ``H`` and ``rollout``; ``_parameters`` (of the module) with ``_DTYPE_ERROR``;
    ``refresh``; ``PACKED`` (the rollout's attributes a forward ran with, which its backward reads); ``grad_shapes(H, W)``
    and ``GRADS`` (the gradients in the parameters' order, and their ctypes struct); ``WORKSPACE`` (the sizing entry) and
    ``_backward(packed, src, pos, B, values, g_out, ws, grads)`` (the backward launch: its argument list is the
    family's).  ``weights`` (a ``FusedAdam``) is the LSTM's alone."""

    weights = None

    def _check_parameters(self) -> Tuple[torch.Tensor, ...]:
        params = self._parameters(self.module)
        if any(p.dtype is not torch.float32 for p in params):
            raise ValueError(self._DTYPE_ERROR)
        if any(p.device != torch.device(self.env._dev) for p in params):
            raise ValueError(f"the head's parameters must live on the env's device {self.env._dev}")
        return params

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
        return _HeadValue.apply(self, src, pos, *params)


class FusedLSTMHead(_FusedHead):
    """An ``LSTMHead`` (or the reference's network of that shape) trained on observation descriptors.

    ``head(obs_src, obs_pos)`` is ``module(env.render(obs_src, obs_pos).float())`` computed by ``fe_lstm_forward`` --
    (B, 1) float32, differentiable with respect to the module's six parameters through ``fe_lstm_backward``;
    ``backward()`` accumulates into their ``.grad`` as the torch module would.  ``.rollout`` is a ``FusedLSTMRollout``
    of the same parameters: ``run`` steps the env with them, ``evaluate_returns`` evaluates them, and it serves as
    ``FusedTwinCritic.td3_targets(target_actor=head.rollout)``.  The module's parameters are re-packed on the device at
    every call (``refresh``), so an optimizer step is seen by the next call and by the next ``rollout.run`` after a
    ``refresh()``.  The module must live on the env's device.

    ``streamed=True`` also admits H in {256, 512, 1024}, the sizes whose recurrent weights stream from L2.  It is an
    opt-in because that backward is several launches per LSTM time step and its workspace grows with the batch up to
    ``fe_lstm_streamed_grad_chunk_pairs`` pairs (2 GiB of activations), unlike the bounded one of H <= 128; H <= 128
    runs the register-resident way either way.

    ``weights``: a ``FusedAdam`` (finenvs_amd/optim.py) that ``module`` is registered with, as a network or as a target.
    The head and its rollout then read that optimizer's packed buffers and its output bias on the device: nothing is
    packed per call, nothing is copied to the host, and ``refresh()`` does nothing -- ``weights.step()`` has already
    written what the next call and the next ``rollout.run`` read.  Those buffers are rewritten in place, so a
    ``weights.step()`` or ``weights.repack()`` between a forward and its ``backward()`` is a RuntimeError (torch's
    version check for the same mistake); and ``self.rollout.set_weights(...)`` takes the rollout off the optimizer's
    buffers, output bias included, until a new head is built."""

    GRADS, PACKED = _lib.FeLstmGrads, ("whh", "wx", "wout")
    _parameters = staticmethod(head_parameters)
    _DTYPE_ERROR = "the fused LSTM head's gradient needs float32 parameters"

    def __init__(self, env, module: nn.Module, streamed: bool = False, weights=None):
        self.H, self.output_activation = check_head(module, streamed)
        if int(env.num_assets) != 1:
            raise ValueError(f"the fused LSTM head trains one asset (the env has {env.num_assets}), as the fused twin "
                             "critic does")
        self.env, self.module = env, module
        # which entries run: a function of H alone
        self.WORKSPACE = "fe_lstm_streamed_grad_workspace_floats" if self.H > 128 else "fe_lstm_grad_workspace_floats"
        self._check_parameters()
        self.weights = weights
        packed = weights.packed(module) if weights is not None else None  # ValueError if the module is not registered
        self.rollout = FusedLSTMRollout.from_modules(env, module.lstm, module.last_layer[0], self.output_activation)
        if packed is not None:
            roll = self.rollout
            roll.whh, roll.wx, roll.wout, roll.bout_dev = packed["whh"], packed["wx"], packed["wout"], packed["bout"]

    @staticmethod
    def grad_shapes(H: int, W: int):
        return (4 * H, 5), (4 * H, H), (4 * H,), (4 * H,), (1, H), (1,)

    def refresh(self) -> None:
        """The module's current parameters into ``self.rollout``, packed on the device (``lstm_pack``).  One 4-byte copy
        of the output bias goes to the host, ordered after any pending update: ``fe_lstm_forward`` takes it by value.
        With ``weights=`` nothing happens: the rollout reads the optimizer's buffers."""
        if self.weights is not None:
            return
        w_ih, w_hh, b_ih, b_hh, w_out, b_out = self._check_parameters()
        roll = self.rollout
        roll.whh, roll.wx = lstm_pack(w_ih, w_hh, b_ih, b_hh, self.H)
        if self.H > 128:  # the streaming kernels read whh fragment-major, as FusedLSTMRollout.set_weights packs it
            roll.whh = lstm_fragment_major(roll.whh, self.H)
        roll.wout = w_out.detach().reshape(self.H).clone()
        roll.bout = float(b_out.detach())

    def _backward(self, packed, src, pos, B, values, g_out, ws, grads) -> None:
        env, roll = self.env, self.rollout
        whh, wx, wout = packed
        backward = env._lib.fe_lstm_backward_streamed if self.H > 128 else env._lib.fe_lstm_backward
        _lib.check(backward(
            env._handle, roll._lr32.data_ptr(), whh.data_ptr(), wx.data_ptr(), wout.data_ptr(), self.H, roll.out_act,
            src.data_ptr(), pos.data_ptr(), B, values.data_ptr(), g_out.data_ptr(), ws.data_ptr(), C.byref(grads),
            env._stream()), env._lib)


# ---------------------------------------------------------------- the reference's losses, plain torch on the output
def torch_ppo_actor_loss(means: torch.Tensor, log_std: torch.Tensor, actions: torch.Tensor, old_log_probs: torch.Tensor,
                         advantages: torch.Tensor, clip_epsilon: float = 0.2, entropy_coefficient: float = 0.01) -> torch.Tensor:
    """``ContinuousActor.compute_actor_loss`` (PPO/continuous_actor.py:59-78), its operations in its order, on the
    actor's output ``means`` (B, 1); ``log_std`` is the learner's ``log_standard_deviation`` (1, 1)."""
    distribution = Normal(means, torch.exp(log_std))
    new_log_probs = distribution.log_prob(actions)
    prob_ratios = torch.exp(new_log_probs - old_log_probs)
    first_term = prob_ratios * advantages
    second_term = torch.clamp(prob_ratios, 1 - clip_epsilon, 1 + clip_epsilon) * advantages
    mean_clipped_objective = torch.minimum(first_term, second_term).mean().mean()
    entropy = distribution.entropy().mean()
    return -(mean_clipped_objective + entropy_coefficient * entropy)


def torch_ppo_critic_loss(values: torch.Tensor, returns: torch.Tensor) -> torch.Tensor:
    """``Critic.compute_critic_loss`` (PPO/critic.py:26-32) on the critic's output ``values`` (B, 1)."""
    return ((returns - values) ** 2).mean()


def _column(t: torch.Tensor, B: int, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.numel() != B:
        raise ValueError(f"{name} must be a tensor of {B} elements ((B,) or (B, 1)), got {tuple(getattr(t, 'shape', ()))}")
    return t.reshape(B, 1)


def ppo_loss_workspace(B: int, device) -> torch.Tensor:
    """A zeroed workspace for one fused loss launch on ``B`` samples (``fe_ppo_loss_workspace_doubles``).  A launch
    leaves it as it found it, so a caller that keeps it (``PPOUpdate``) allocates once."""
    n = int(_lib.load().fe_ppo_loss_workspace_doubles(int(B)))
    if n < 1:
        raise ValueError(f"a loss launch needs at least one sample (got {B})")
    return torch.zeros((n,), dtype=torch.float64, device=device)


def _loss_workspace(workspace, B: int, device) -> torch.Tensor:
    """The caller's workspace if it can hold a launch on ``B`` samples (ValueError otherwise), or a fresh one."""
    if workspace is None:
        return ppo_loss_workspace(B, device)
    need = int(_lib.load().fe_ppo_loss_workspace_doubles(int(B)))
    if not isinstance(workspace, torch.Tensor) or workspace.dtype is not torch.float64 or workspace.device != device \
            or not workspace.is_contiguous() or workspace.numel() < need:
        raise ValueError(f"workspace must be a contiguous float64 tensor of at least {need} elements on {device} "
                         "(ppo_loss_workspace(B, device))")
    return workspace


def _loss_input(t: torch.Tensor, B: int) -> torch.Tensor:
    return t.detach().reshape(B).to(dtype=torch.float32).contiguous()


class _FusedActorLoss(torch.autograd.Function):
    """``torch_ppo_actor_loss`` as one launch (C ABI ``fe_ppo_actor_loss``, include/finenvs_amd_ppo.h): the forward also
    writes d loss / d means and d loss / d log_std, the backward scales them by ``grad_output``."""

    @staticmethod
    def forward(ctx, means, log_std, actions, old_log_probs, advantages, clip_epsilon, entropy_coefficient, workspace):
        B, dev = int(means.numel()), means.device
        if B < 1:
            raise ValueError("the fused PPO loss needs at least one sample")
        if log_std.numel() != 1 or log_std.dtype is not torch.float32 or log_std.device != dev:
            raise ValueError("the fused PPO actor loss takes one float32 log_std on the means' device (A = 1)")
        lib = _lib.load()
        m, a, o, adv = (_loss_input(t, B) for t in (means, actions, old_log_probs, advantages))
        if any(t.device != dev for t in (a, o, adv)):
            raise ValueError("actions, old_log_probs and advantages must live on the means' device")
        ws = _loss_workspace(workspace, B, dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        g_means = torch.empty((B,), dtype=torch.float32, device=dev)
        g_log_std = torch.empty((1,), dtype=torch.float32, device=dev)
        _lib.check(lib.fe_ppo_actor_loss(
            m.data_ptr(), log_std.detach().contiguous().data_ptr(), a.data_ptr(), o.data_ptr(), adv.data_ptr(), B,
            float(clip_epsilon), float(entropy_coefficient), loss.data_ptr(), g_means.data_ptr(), g_log_std.data_ptr(),
            ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), lib)
        ctx.save_for_backward(g_means, g_log_std)
        ctx.shapes = (tuple(means.shape), tuple(log_std.shape))
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        g_means, g_log_std = ctx.saved_tensors
        out = [None] * 8
        if ctx.needs_input_grad[0]:
            out[0] = (g_means * g_loss).reshape(ctx.shapes[0])
        if ctx.needs_input_grad[1]:
            out[1] = (g_log_std * g_loss).reshape(ctx.shapes[1])
        return tuple(out)


class _FusedValueLoss(torch.autograd.Function):
    """``torch_ppo_critic_loss`` as one launch (C ABI ``fe_ppo_value_loss``): the forward also writes d loss / d values."""

    @staticmethod
    def forward(ctx, values, returns, workspace):
        B, dev = int(values.numel()), values.device
        if B < 1:
            raise ValueError("the fused PPO loss needs at least one sample")
        lib = _lib.load()
        v, r = _loss_input(values, B), _loss_input(returns, B)
        if r.device != dev:
            raise ValueError("returns must live on the values' device")
        ws = _loss_workspace(workspace, B, dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        g_values = torch.empty((B,), dtype=torch.float32, device=dev)
        _lib.check(lib.fe_ppo_value_loss(v.data_ptr(), r.data_ptr(), B, loss.data_ptr(), g_values.data_ptr(), ws.data_ptr(),
                                         torch.cuda.current_stream(dev).cuda_stream), lib)
        ctx.save_for_backward(g_values)
        ctx.shape = tuple(values.shape)
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        (g_values,) = ctx.saved_tensors
        return ((g_values * g_loss).reshape(ctx.shape) if ctx.needs_input_grad[0] else None), None, None


def fused_ppo_actor_loss(means: torch.Tensor, log_std: torch.Tensor, actions: torch.Tensor, old_log_probs: torch.Tensor,
                         advantages: torch.Tensor, clip_epsilon: float = 0.2, entropy_coefficient: float = 0.01,
                         workspace: torch.Tensor = None) -> torch.Tensor:
    """``torch_ppo_actor_loss`` on device tensors as ONE launch, differentiable in ``means`` and ``log_std`` (one
    action per sample): evaluated in f64 from the f32 inputs and rounded once, so it agrees with the torch expression
    to f32 rounding, not bit for bit.  ``workspace``: a kept ``ppo_loss_workspace(B, device)``; allocated if None."""
    return _FusedActorLoss.apply(means, log_std, actions, old_log_probs, advantages, clip_epsilon, entropy_coefficient,
                                 workspace)


def fused_ppo_critic_loss(values: torch.Tensor, returns: torch.Tensor, workspace: torch.Tensor = None) -> torch.Tensor:
    """``torch_ppo_critic_loss`` on device tensors as ONE launch, differentiable in ``values``."""
    return _FusedValueLoss.apply(values, returns, workspace)


def ppo_actor_loss(head: "Union[FusedLSTMHead, FusedMLPHead]", log_std: torch.Tensor, src: torch.Tensor, pos: torch.Tensor, actions: torch.Tensor,
                   old_log_probs: torch.Tensor, advantages: torch.Tensor, clip_epsilon: float = 0.2,
                   entropy_coefficient: float = 0.01, fused: bool = False, workspace: torch.Tensor = None) -> torch.Tensor:
    """``compute_actor_loss`` (PPO/continuous_actor.py:59-78) on B state descriptors, nothing rendered: the clipped
    surrogate of ``Normal(head(src, pos), exp(log_std))`` plus the entropy bonus, negated.  ``actions``,
    ``old_log_probs``, ``advantages``: B elements each.  ``log_std`` gets its gradient from autograd.  ``head``: a
    ``FusedLSTMHead`` or a ``FusedMLPHead`` (finenvs_amd/mlp_head.py) -- anything that maps ``(src, pos)`` to a
    differentiable (B, 1) float32 output.

    ``fused=True``: the loss and its gradients from one launch (``fused_ppo_actor_loss``) instead of some thirty
    element-wise ones; ``backward()`` accumulates into ``log_std.grad`` and the head's ``.grad`` as before.
    ``workspace``: see ``fused_ppo_actor_loss``."""
    B = int(src.numel())
    cols = (_column(actions, B, "actions"), _column(old_log_probs, B, "old_log_probs"), _column(advantages, B, "advantages"))
    if fused:
        return fused_ppo_actor_loss(head(src, pos), log_std, *cols, clip_epsilon, entropy_coefficient, workspace)
    return torch_ppo_actor_loss(head(src, pos), log_std, *cols, clip_epsilon, entropy_coefficient)


def ppo_critic_loss(head: "Union[FusedLSTMHead, FusedMLPHead]", src: torch.Tensor, pos: torch.Tensor, returns: torch.Tensor, fused: bool = False,
                    workspace: torch.Tensor = None) -> torch.Tensor:
    """``compute_critic_loss`` (PPO/critic.py:26-32) on B state descriptors: the mean squared error of
    ``head(src, pos)`` against ``returns`` (B elements); ``head``: a ``FusedLSTMHead`` or a ``FusedMLPHead``
    (finenvs_amd/mlp_head.py).  ``fused=True``: loss and gradient from one launch (``fused_ppo_critic_loss``)."""
    ret = _column(returns, int(src.numel()), "returns")
    if fused:
        return fused_ppo_critic_loss(head(src, pos), ret, workspace)
    return torch_ppo_critic_loss(head(src, pos), ret)


def td3_actor_loss(head: FusedLSTMHead, buffer, indices: torch.Tensor, twin) -> torch.Tensor:
    """``Actor.compute_loss`` (TD3/actor.py:50-56) on the transitions ``indices`` (logical, (B,)) of ``buffer``:
    ``-twin.q(src, pos, head(src, pos))[0].mean()`` on the ring's state descriptors, nothing rendered (the reference
    passes its first critic).  ``head`` / ``twin``: a ``FusedLSTMHead`` with a ``FusedTwinCritic``, or a ``FusedMLP2Head``
    (tanh output) with a ``FusedTwinMLPCritic`` (finenvs_amd/mlp_critic.py).  ``backward()`` also accumulates into that critic's ``.grad`` unless it is frozen (as in
    torch); an index outside ``[0, size)`` makes the loss NaN.  ``indices`` may be a ``ReplayDraw`` of a ``cursor=True``
    buffer (no host integer enters then: capturable)."""
    from .critic import FusedTwinCritic
    from .mlp2_head import FusedMLP2Head
    from .mlp_critic import FusedTwinMLPCritic
    from .replay import as_draw

    draw = as_draw(buffer, indices, "td3_actor_loss")
    if isinstance(head, FusedMLP2Head) or isinstance(twin, FusedTwinMLPCritic):  # the MLP family: both or neither
        if not isinstance(head, FusedMLP2Head) or not isinstance(twin, FusedTwinMLPCritic) or twin.env is not head.env:
            raise ValueError("a FusedMLP2Head goes with a FusedTwinMLPCritic of its env, an LSTM head with a FusedTwinCritic: "
                             "the two families do not mix")
    elif not isinstance(twin, FusedTwinCritic) or twin.env is not head.env:
        raise ValueError("twin must be a FusedTwinCritic of this head's env")
    if indices is None:
        raise ValueError("td3_actor_loss needs the indices of the sampled transitions")
    idx = twin._indices(buffer, indices if draw is None else draw.indices, None)
    B = int(idx.numel())
    if draw is not None:  # the draw's gathered descriptors; its indices are in range by construction
        src, pos = draw.state_src, draw.state_pos.reshape(B)
        return -twin.q(src, pos, head(src, pos))[0].mean()
    slots = buffer.physical(idx)
    src, pos = buffer.state_src[slots], buffer.state_pos[slots].reshape(B)
    q = twin.q(src, pos, head(src, pos))[0]
    valid = ((idx >= 0) & (idx < buffer.size())).reshape(B, 1)
    q = torch.where(valid, q, torch.full((), float("nan"), device=q.device))
    return -q.mean()
