"""SAC's and TD3's twin LSTM critics: the torch module a learner trains, and the fused no-grad target half.

``CriticLSTM`` restates the reference's ``CriticLSTM((6, H, 1), W)`` (finenvs/agents/SAC/critic.py, the same class in
agents/TD3/critic.py; networks/lstm.py:28-57) for one asset: ``nn.LSTM(6, H)`` over ``[state row | action]`` -- the
action repeated over the window (agent_utils.py:5-14) -- and ``last_layer = Linear(H, 1)`` + Identity on the last hidden
state.  Its submodule names are the reference's, so a reference ``state_dict`` loads unchanged.

``FusedTwinCritic`` evaluates two such critics on observation descriptors in one launch (C ABI ``fe_twin_q_forward``,
include/finenvs_amd_critic.h) and forms the Bellman targets of ``SACAgent.compute_targets`` (SAC_agent.py:200-227) and
``TD3Agent.compute_targets`` (TD3_agent.py:231-251) straight from the replay ring (``fe_twin_q_target``): the sampled
next states are never rendered.  The actor half runs on the same descriptors in ``FusedSACRollout.forward`` /
``FusedLSTMRollout.forward``.  The gradient half runs on descriptors too: ``FusedTwinCritic.q`` is the values as a
differentiable function of the actions and both critics' parameters (C ABI ``fe_twin_q_backward``,
include/finenvs_amd_critic_grad.h), and ``critic_loss`` the critics' MSE on replayed transitions.  Scope: one asset (the reference's multi-asset critic is ``nn.LSTM(5A + A, H)`` over the
whole env, not a per-pair network) and H in {32, 64, 128}; with ``streamed=True`` also H in {256, 512, 1024} (C ABI
``fe_twin_q_forward_streamed`` / ``fe_twin_q_target_streamed`` / ``fe_twin_q_backward_streamed``,
include/finenvs_amd_critic_streamed.h).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .replay import as_draw
from .rollout import log_return_f32, lstm_fragment_major, lstm_pack, lstm_row_order_on

CRITIC_HIDDEN_SIZES = (32, 64, 128)
CRITIC_STREAMED_HIDDEN_SIZES = (256, 512, 1024)  # with streamed=True


def match_actions_dim_with_states(states: torch.Tensor, actions: torch.Tensor) -> Tuple[torch.Tensor, int]:
    """agent_utils.py:5-14: actions (B, A) repeated over the window of (B, W, F) states, and the dim to concatenate on."""
    if actions.dim() < states.dim():
        return actions.unsqueeze(1).repeat(1, states.shape[1], 1), 2
    return actions, 1


class CriticLSTM(nn.Module):
    """The reference's ``CriticLSTM((6, H, 1), sequence_length=W)`` as a plain module (no optimizer inside): submodules
    ``lstm = nn.LSTM(6, H, batch_first=True)`` and ``last_layer = Sequential(Linear(H, 1), Identity())``."""

    def __init__(self, H: int = 128, W: int = 4, device=None):
        super().__init__()
        self.input_size, self.hidden_size, self.output_size, self.sequence_length = 6, int(H), 1, int(W)
        self.lstm = nn.LSTM(6, self.hidden_size, num_layers=1, batch_first=True, device=device)
        self.last_layer = nn.Sequential(nn.Linear(self.hidden_size, 1, device=device), nn.Identity())

    def forward(self, states: torch.Tensor, actions: torch.Tensor) -> torch.Tensor:
        """states (B, W, 5), actions (B, 1) -> Q (B, 1)."""
        if states.dim() != 3 or states.shape[1] != self.sequence_length or states.shape[2] != 5:
            raise ValueError(f"states must be (B, {self.sequence_length}, 5), got {tuple(states.shape)}")
        actions, dim = match_actions_dim_with_states(states, actions)
        out, _ = self.lstm(torch.cat([states, actions], dim=dim))
        return self.last_layer(out[:, -1, :])


def check_critic(critic: nn.Module, streamed: bool = False) -> int:
    """The hidden size of a critic the fused twin critic can run; ValueError otherwise.  ``streamed``: H may also be 256,
    512 or 1024 (the streamed kernels of include/finenvs_amd_critic_streamed.h)."""
    lstm = getattr(critic, "lstm", None)
    if not isinstance(lstm, nn.LSTM):
        raise ValueError("the fused critic needs a module with an nn.LSTM `lstm`")
    if lstm.num_layers != 1 or lstm.bidirectional or lstm.input_size != 6 or not lstm.batch_first or lstm.proj_size:
        raise ValueError("the fused critic needs nn.LSTM(6, H, num_layers=1, batch_first=True) (5 observation features "
                         "and one action: A = 1)")
    H = int(lstm.hidden_size)
    if streamed and H not in CRITIC_HIDDEN_SIZES + CRITIC_STREAMED_HIDDEN_SIZES:
        raise ValueError(f"the fused critic supports H in {CRITIC_HIDDEN_SIZES + CRITIC_STREAMED_HIDDEN_SIZES} (got {H})")
    if not streamed and H not in CRITIC_HIDDEN_SIZES:
        raise ValueError(f"the fused critic supports H in {CRITIC_HIDDEN_SIZES} (got {H})"
                         + ("; pass streamed=True for the streamed kernels of H in "
                            f"{CRITIC_STREAMED_HIDDEN_SIZES}" if H in CRITIC_STREAMED_HIDDEN_SIZES else ""))
    last = getattr(critic, "last_layer", None)
    if not isinstance(last, nn.Sequential) or len(last) != 2 or not isinstance(last[0], nn.Linear) \
            or not isinstance(last[1], nn.Identity) or last[0].in_features != H or last[0].out_features != 1 \
            or last[0].bias is None:
        raise ValueError(f"last_layer must be Sequential(Linear({H}, 1), Identity())")
    return H


def pack_critic_weights(critic: nn.Module) -> Dict[str, torch.Tensor]:
    """The critic's current parameters as fe_twin_q_forward reads them (f32, on the parameters' device, no host sync):
    whh / wx as ``lstm_pack`` of the five observation inputs (slot 5 = b_ih + b_hh) plus slot 6 = the action's input
    weight ``w_ih[:, 5]``; ``wout`` (H) and ``bout`` (1).  At H > 128 ``whh`` is fragment-major
    (``lstm_fragment_major``), as the streamed kernels read it."""
    H = check_critic(critic, streamed=True)
    lstm = critic.lstm
    w_ih = lstm.weight_ih_l0.detach().float()
    whh, wx = lstm_pack(w_ih[:, :5], lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0, H)
    if H > 128:
        whh = lstm_fragment_major(whh, H)
    wx[:, 6] = w_ih[lstm_row_order_on(H, w_ih.device), 5]
    last = critic.last_layer[0]
    return {
        "whh": whh, "wx": wx,
        "wout": last.weight.detach().float().reshape(H).contiguous(),
        "bout": last.bias.detach().float().reshape(1).contiguous(),
    }


GRAD_KEYS = ("w_ih", "w_hh", "b_ih", "b_hh", "w_out", "b_out")  # fe_critic_grads' fields, in critic_parameters' order


def critic_parameters(critic: nn.Module) -> Tuple[torch.Tensor, ...]:
    """The six parameter tensors of a critic in ``GRAD_KEYS`` order: ``lstm.weight_ih_l0 (4H, 6)``, ``weight_hh_l0
    (4H, H)``, ``bias_ih_l0``, ``bias_hh_l0`` (4H), ``last_layer[0].weight (1, H)`` and ``.bias (1)``."""
    lstm, last = critic.lstm, critic.last_layer[0]
    return lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0, last.weight, last.bias


def empty_packed_grads(H: int, device) -> Dict[str, torch.Tensor]:
    """Buffers for one critic's gradients as fe_twin_q_backward writes them (include/finenvs_amd_critic_grad.h).  At
    H > 128 the same buffers, ``w_out`` (1, H): fe_twin_q_backward_streamed writes torch's row order and layout."""
    shapes = {"w_ih": (4 * H, 6), "w_hh": (4 * H, H), "b_ih": (4 * H,), "b_hh": (4 * H,),
              "w_out": (1, H) if H > 128 else (H,), "b_out": (1,)}
    return {k: torch.empty(shapes[k], dtype=torch.float32, device=device) for k in GRAD_KEYS}


def packed_grads_to_torch(g: Dict[str, torch.Tensor], H: int) -> Dict[str, torch.Tensor]:
    """fe_twin_q_backward's gradients (rows of the 4H-row tensors in ``lstm_row_order``) in the layout and row order of
    the critic's parameters (``critic_parameters``)."""
    order = lstm_row_order_on(H, g["w_hh"].device)
    inv = torch.empty_like(order)
    inv[order] = torch.arange(4 * H, device=order.device)
    return {"w_ih": g["w_ih"][inv], "w_hh": g["w_hh"][inv], "b_ih": g["b_ih"][inv], "b_hh": g["b_hh"][inv],
            "w_out": g["w_out"].reshape(1, H), "b_out": g["b_out"].reshape(1)}


def torch_grads_to_packed(g: Dict[str, torch.Tensor], H: int) -> Dict[str, torch.Tensor]:
    """The inverse of ``packed_grads_to_torch``."""
    order = lstm_row_order_on(H, g["w_hh"].device)
    return {"w_ih": g["w_ih"][order], "w_hh": g["w_hh"][order], "b_ih": g["b_ih"][order], "b_hh": g["b_hh"][order],
            "w_out": g["w_out"].reshape(H), "b_out": g["b_out"].reshape(1)}


class _TwinQ(torch.autograd.Function):
    """(q1, q2) of a ``_FusedTwin`` as a differentiable function of the actions and the twelve parameters: the forward
    is the family's forward entry, the backward its backward entry on the weights the forward packed (the activations
    recomputed)."""

    @staticmethod
    def forward(ctx, fused, src, pos, actions, *params):
        q1, q2 = fused.forward(src, pos, actions.detach())
        ctx.set_materialize_grads(False)  # an output nobody used gets None, not zeros: its critic does not run
        ctx.fused, ctx.packed, ctx.action_shape = fused, getattr(fused, "_packed", None), actions.shape  # (none yet: B = 0)
        ctx.version = None if fused.weights is None else fused.weights.version
        ctx.save_for_backward(src, pos, actions.detach().reshape(-1).contiguous())
        return q1, q2

    @staticmethod
    def backward(ctx, g1, g2):
        fused = ctx.fused
        if fused.weights is not None:
            fused.weights.check_version(ctx.version)
        src, pos, act = ctx.saved_tensors
        env, H, B = fused.env, fused.H, int(src.numel())
        W, dev = int(env.num_intervals), env._dev
        need = ctx.needs_input_grad
        n = (len(need) - 4) // 2  # parameters per critic
        need_a = need[3]
        need_w = (any(need[4:4 + n]), any(need[4 + n:]))
        dq = [g if g is not None and (need_w[c] or need_a) else None for c, g in enumerate((g1, g2))]
        out = [None] * len(need)
        if dq[0] is None and dq[1] is None:
            return tuple(out)
        dq = [None if g is None else g.reshape(B).float().contiguous() for g in dq]
        grads = [fused._empty_grads() if dq[c] is not None and need_w[c] else None for c in range(2)]
        da = torch.empty((B,), dtype=torch.float32, device=dev) if need_a else None
        if B == 0:  # nothing to launch (an empty tensor has no address to pass): the sums over an empty batch are zeros
            for g in grads:
                if g is not None:
                    for t in g:
                        t.zero_()
        else:
            ws = torch.empty((int(fused._entry("workspace")(H, W, B)),), dtype=torch.float32, device=dev)
            cw = [fused._struct(x) for x in ctx.packed]
            cg = [None if g is None else fused.GRADS(*(t.data_ptr() for t in g)) for g in grads]
            ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
            ref = lambda x: None if x is None else C.byref(x)  # noqa: E731
            _lib.check(fused._entry("backward")(
                env._handle, fused._lr32.data_ptr(), C.byref(cw[0]), C.byref(cw[1]), *fused._shape_args(), src.data_ptr(),
                pos.data_ptr(), act.data_ptr(), B, ptr(dq[0]), ptr(dq[1]), ws.data_ptr(), ref(cg[0]), ref(cg[1]), ptr(da),
                env._stream()), env._lib)
        if need_a:
            out[3] = da.reshape(ctx.action_shape)
        for c in range(2):
            if grads[c] is None:
                continue
            for k, g in enumerate(fused._grads_to_torch(grads[c])):
                if need[4 + n * c + k]:
                    out[4 + n * c + k] = g
        return tuple(out)


class _FusedTwin:
    """What ``FusedTwinCritic`` and ``FusedTwinMLPCritic`` (finenvs_amd/mlp_critic.py) share: everything that does not
    depend on the network -- the checks of devices, vectors and indices, ``forward`` and ``q`` with its autograd function,
    the ring's descriptors, the NaN rule for an index outside ``[0, size)``, ``ReplayDraw`` handling, the critic loss and
    the target launches' argument lists.  A family provides ``_weights()`` (packs both critics into ``self._packed`` and
    returns their two ctypes weight structs), ``_struct(x)`` (that struct of one packed critic), ``_shape_args()`` (what
    its C entries take between the weights and the descriptors: ``H``, or ``H`` and the activation), ``ENTRIES`` or
    ``_entry(kind)`` (the ``"forward"``, ``"backward"`` and ``"workspace"`` entries), ``_target_entry(cursor)``,
    ``_parameters(critic)`` (one critic's parameter tuple) and ``_DTYPE_ERROR``, ``_empty_grads()`` and ``GRADS`` (one
    critic's gradient buffers as its backward writes them, in the parameters' order, and their ctypes struct),
    ``_grads_to_torch(grads)`` (those in torch's layout), ``_check_target_actor`` and ``_check_sac_actor``.  ``weights``
    (a ``FusedAdam``) is the LSTM's alone."""

    weights = None

    def _entry(self, kind: str):
        return getattr(self.env._lib, self.ENTRIES[kind])

    def _grads_to_torch(self, grads):
        return grads

    def _check_devices(self) -> None:
        dev = torch.device(self.env._dev)
        for name, c in (("critic_1", self.critic_1), ("critic_2", self.critic_2)):
            if any(p.device != dev for p in c.parameters()):
                raise ValueError(f"{name}'s parameters must live on the env's device {dev}")

    def _vector(self, t, B: int, name: str, dtype=torch.float32) -> torch.Tensor:
        if not isinstance(t, torch.Tensor) or t.dtype is not dtype or t.numel() != B or t.device != torch.device(self.env._dev):
            raise ValueError(f"{name} must be a {dtype} tensor of {B} elements ((B,) or (B, 1)) on {self.env._dev}, got "
                             f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))} on {getattr(t, 'device', None)}")
        return t.reshape(B).contiguous()

    def forward(self, obs_src: torch.Tensor, obs_pos: torch.Tensor, actions: torch.Tensor):
        """Both critics on B (state, action) pairs: ``obs_src (B,)`` int64 / ``obs_pos (B, 1)`` float64 observation
        descriptors and ``actions (B, 1)`` float32 -> ``(q1, q2)``, each (B, 1) float32."""
        env = self.env
        B = int(obs_src.numel()) if isinstance(obs_src, torch.Tensor) else -1
        src = self._vector(obs_src, B, "obs_src", torch.int64)
        pos = self._vector(obs_pos, B, "obs_pos", torch.float64)
        act = self._vector(actions, B, "actions")
        q1 = torch.empty((B, 1), dtype=torch.float32, device=env._dev)
        q2 = torch.empty((B, 1), dtype=torch.float32, device=env._dev)
        if B:
            c1, c2 = self._weights()
            _lib.check(self._entry("forward")(
                env._handle, self._lr32.data_ptr(), C.byref(c1), C.byref(c2), *self._shape_args(), src.data_ptr(),
                pos.data_ptr(), act.data_ptr(), B, q1.data_ptr(), q2.data_ptr(), env._stream()), env._lib)
        return q1, q2

    __call__ = forward

    # ---------------------------------------------------------------- the gradient half
    def q(self, obs_src: torch.Tensor, obs_pos: torch.Tensor, actions: torch.Tensor):
        """``forward`` as a differentiable function (C ABI ``fe_twin_q_backward``, include/finenvs_amd_critic_grad.h;
        the MLP critics': ``fe_twin_mlpq_backward``): ``(q1, q2)`` (B, 1) float32, the same values bit for bit.
        ``backward()`` accumulates into the ``.grad`` of both critics' parameters and of ``actions`` (float32, (B, 1) or
        (B,)) as the torch modules would: the critic loss of SAC/critic.py:30-45 / TD3/critic.py:31-46, ``dQ/da`` for
        TD3/actor.py ``compute_loss`` and the SAC actor loss.  A critic whose output gets no gradient does not run; one
        whose parameters are frozen has no weight reduction."""
        B = int(obs_src.numel()) if isinstance(obs_src, torch.Tensor) else -1
        src = self._vector(obs_src, B, "obs_src", torch.int64)
        pos = self._vector(obs_pos, B, "obs_pos", torch.float64)
        self._vector(actions, B, "actions")
        params = self._parameters(self.critic_1) + self._parameters(self.critic_2)
        if any(p.dtype is not torch.float32 for p in params):
            raise ValueError(self._DTYPE_ERROR)
        return _TwinQ.apply(self, src, pos, actions, *params)

    def critic_loss(self, buffer, indices: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
        """``MSE(q1, y) + MSE(q2, y)`` of both critics (SAC/critic.py:30-45 compute_loss, once per critic) on the
        transitions ``indices`` (logical, (B,)) of ``buffer``: the ring's state descriptors and stored actions of those
        transitions, nothing rendered.  ``targets`` (B, 1) float32, e.g. from ``sac_targets`` / ``td3_targets``.  An
        index outside ``[0, size)`` makes its values NaN (as ``fe_twin_q_target``).  ``indices`` may be a ``ReplayDraw``
        of a ``cursor=True`` buffer (no host integer enters then: capturable)."""
        draw = as_draw(buffer, indices, "critic_loss")
        if indices is None:
            raise ValueError("critic_loss needs the indices of the sampled transitions")
        if draw is not None:  # the draw's gathered descriptors and actions; its indices are in range by construction
            self._indices(buffer, draw.indices, None)
            B = int(draw.indices.numel())
            y = self._vector(targets, B, "targets").reshape(B, 1)
            q1, q2 = self.q(draw.state_src, draw.state_pos.reshape(B), draw.actions.reshape(B, 1))
            return F.mse_loss(q1, y) + F.mse_loss(q2, y)
        idx = self._indices(buffer, indices, None)
        B = int(idx.numel())
        y = self._vector(targets, B, "targets").reshape(B, 1)
        slots = buffer.physical(idx)
        q1, q2 = self.q(buffer.state_src[slots], buffer.state_pos[slots].reshape(B), buffer.actions[slots].reshape(B, 1))
        valid = ((idx >= 0) & (idx < buffer.size())).reshape(B, 1)
        nan = torch.full((), float("nan"), device=q1.device)
        q1, q2 = torch.where(valid, q1, nan), torch.where(valid, q2, nan)
        return F.mse_loss(q1, y) + F.mse_loss(q2, y)

    # ---------------------------------------------------------------- targets from the replay ring
    def _indices(self, buffer, indices, batch_size) -> torch.Tensor:
        if buffer.A != 1 or buffer.W != int(self.env.num_intervals) or buffer.device != torch.device(self.env._dev):
            raise ValueError("the replay buffer must hold one-asset descriptors of this env's tables, on its device")
        buffer._ring.check_sample()
        if indices is None:
            if batch_size is None:
                raise ValueError("give indices or batch_size")
            # the draw ReplayBuffer.get_mini_batch makes (OPB:69): pass the same tensor to get_mini_batch for the grad half
            return torch.randint(0, buffer.size(), (int(batch_size),), device=buffer.device)
        if not isinstance(indices, torch.Tensor) or indices.dtype.is_floating_point or indices.dtype.is_complex \
                or indices.dtype is torch.bool or indices.device != buffer.device:
            raise ValueError(f"indices must be an integer tensor of logical indices on {buffer.device}")
        return indices.reshape(-1).to(torch.int64).contiguous()

    def _next_descriptors(self, buffer, idx, draw=None):
        if draw is not None:
            return draw.next_src, draw.next_pos
        # the actor half reads the sampled next states' descriptors (an out-of-range index wraps to some slot here; its
        # target is NaN all the same and fe_twin_q_target counts it)
        slots = buffer.physical(idx)
        return buffer.next_src[slots], buffer.next_pos[slots]

    def _targets(self, buffer, idx, next_actions, smooth_noise, smooth_std, smooth_clip, log_probs, alpha, gamma,
                 reward_scale, draw=None) -> torch.Tensor:
        env, B = self.env, int(idx.numel())
        dev = env._dev
        y = torch.empty((B, 1), dtype=torch.float32, device=dev)
        q1 = torch.empty((B, 1), dtype=torch.float32, device=dev)
        q2 = torch.empty((B, 1), dtype=torch.float32, device=dev)
        if B:
            c1, c2 = self._weights()
            ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
            tail = (idx.data_ptr(), B, next_actions.data_ptr(), ptr(smooth_noise), float(smooth_std), float(smooth_clip),
                    ptr(log_probs), ptr(alpha), float(gamma), float(reward_scale), y.data_ptr(), q1.data_ptr(),
                    q2.data_ptr(), env._stream())
            net = (env._handle, self._lr32.data_ptr(), C.byref(c1), C.byref(c2), *self._shape_args(), C.byref(buffer._desc))
            entry = self._target_entry(cursor=draw is not None)
            if draw is None:
                _lib.check(entry(*net, buffer.head, buffer.size(), *tail), env._lib)
            else:  # head and size from the cursor, when the launches run
                _lib.check(entry(*net, buffer.cursor.data_ptr(), *tail), env._lib)
        self.last = {"indices": idx, "next_actions": next_actions.reshape(B, 1), "q1": q1, "q2": q2}
        return y

    def td3_targets(self, buffer, indices: Optional[torch.Tensor], target_actor, noise: Optional[torch.Tensor] = None,
                    gamma: float = 0.99, policy_std: float = 0.2, policy_clip: float = 0.5, reward_scale: float = 1.0,
                    batch_size: Optional[int] = None) -> torch.Tensor:
        """``TD3Agent.compute_targets`` (TD3_agent.py:231-251): the target actor (``FusedTwinCritic``: a
        ``FusedLSTMRollout``, ``FusedTwinMLPCritic``: a ``FusedMLP2Rollout``; ``output_activation="tanh"``) on the sampled
        next descriptors, the smoothed action ``clamp(a + clamp(noise * policy_std, -policy_clip, policy_clip), -1, 1)`` with ``noise`` (B, 1) standard normals (default ``torch.randn``),
        both target critics and ``y = r + gamma * (1 - d) * min(q1, q2)``.  (B, 1) float32."""
        draw = as_draw(buffer, indices, "td3_targets")
        self._check_target_actor(target_actor)
        idx = self._indices(buffer, indices if draw is None else draw.indices, batch_size)
        B = int(idx.numel())
        src, pos = self._next_descriptors(buffer, idx, draw)
        actions = target_actor.forward(src, pos)
        if noise is None:
            noise = torch.randn((B, 1), device=self.env._dev)
        noise = self._vector(noise, B, "noise")
        return self._targets(buffer, idx, actions, noise, policy_std, policy_clip, None, None, gamma, reward_scale, draw)

    def sac_targets(self, buffer, indices: Optional[torch.Tensor], actor_roll, noise: Optional[torch.Tensor] = None,
                    gamma: float = 0.99, log_alpha: Optional[torch.Tensor] = None, reward_scale: float = 1.0,
                    batch_size: Optional[int] = None) -> torch.Tensor:
        """``SACAgent.compute_targets`` (SAC_agent.py:200-227) for the transitions ``indices`` (logical, (B,)) of
        ``buffer``: the actor half in ``actor_roll.forward`` (``FusedTwinCritic``: a ``FusedSACRollout``,
        ``FusedTwinMLPCritic``: a ``FusedMLPSACRollout`` of its env) on the sampled next descriptors with
        ``noise`` (B, 1) standard normals -- by default ``torch.randn``, the draw ``rsample`` makes -- then both target
        critics and ``y = r + gamma * (1 - d) * (min(q1, q2) - alpha * log_prob)`` with ``alpha = log_alpha.exp()``,
        ``r`` the stored reward times ``reward_scale``.  (B, 1) float32.  ``indices=None`` draws ``batch_size`` of them as
        ``get_mini_batch`` does; ``self.last`` keeps the indices, next actions, log-probabilities and values.
        ``indices`` may be a ``ReplayDraw`` of a ``cursor=True`` buffer: its gathered next descriptors are used and the
        ring's head and size are read from the cursor (``fe_twin_q_target_c``), so the call is capturable."""
        draw = as_draw(buffer, indices, "sac_targets")
        self._check_sac_actor(actor_roll)
        if not isinstance(log_alpha, torch.Tensor) or log_alpha.numel() != 1 or log_alpha.device != torch.device(self.env._dev):
            raise ValueError(f"log_alpha must be a one-element tensor on {self.env._dev}")
        idx = self._indices(buffer, indices if draw is None else draw.indices, batch_size)
        B = int(idx.numel())
        if noise is None:
            noise = torch.randn((B, 1), device=self.env._dev)
        src, pos = self._next_descriptors(buffer, idx, draw)
        actions, log_probs, _, _ = actor_roll.forward(src, pos, noise=noise.reshape(B, 1))
        alpha = log_alpha.detach().exp().float().reshape(1).contiguous()
        y = self._targets(buffer, idx, actions, None, 0.0, 0.0, log_probs, alpha, gamma, reward_scale, draw)
        self.last.update(log_probs=log_probs, alpha=alpha)
        return y


class FusedTwinCritic(_FusedTwin):
    """Two LSTM critics of the same H evaluated together on the device (C ABI of include/finenvs_amd_critic.h).

    The critics' parameters are re-packed on the device at every call (a few small launches, no host round trip), so an
    optimizer step or a soft update is seen by the next call.  Both critics must live on the env's device.

    ``weights``: a ``FusedAdam`` (finenvs_amd/optim.py) that both critics are registered with, as networks or as
    targets.  Nothing is packed per call then: every launch reads that optimizer's packed buffers, which its ``step()``
    keeps current.  Those buffers are rewritten in place: a ``weights.step()`` or ``weights.repack()`` between a
    forward and its ``backward()`` is a RuntimeError.

    ``streamed=True`` also admits H in {256, 512, 1024}, the sizes whose recurrent weights stream from L2
    (include/finenvs_amd_critic_streamed.h).  It is an opt-in because that backward is several launches per LSTM time
    step and per critic, and its workspace grows with the batch, up to ``fe_lstm_streamed_grad_chunk_pairs`` pairs
    (2 GiB of activations; the two critics share it), unlike the bounded one of H <= 128; H <= 128 runs the
    register-resident way whether or not ``streamed`` is passed."""

    def __init__(self, env, critic_1: nn.Module, critic_2: nn.Module, weights=None, streamed: bool = False):
        if int(env.num_assets) != 1:
            raise ValueError(f"the fused twin critic runs one asset (the env has {env.num_assets}): the reference's critic "
                             "for A > 1 is one nn.LSTM(5A + A, H) over the whole env's window, not a per-(env, asset) pair "
                             "network")
        H1, H2 = check_critic(critic_1, streamed), check_critic(critic_2, streamed)
        if H1 != H2:
            raise ValueError(f"the two critics must have the same hidden size (got {H1} and {H2})")
        self.env, self.critic_1, self.critic_2, self.H = env, critic_1, critic_2, H1
        self.streamed = H1 > 128  # which entries run: a function of H alone
        self._check_devices()
        self.weights = weights
        if weights is not None:
            weights.packed(critic_1), weights.packed(critic_2)  # ValueError if a critic is not registered with it
        self._lr32 = log_return_f32(env)
        self.last: Dict[str, torch.Tensor] = {}

    GRADS = _lib.FeCriticGrads
    _parameters = staticmethod(critic_parameters)
    _DTYPE_ERROR = "the fused critic's gradient needs float32 parameters"

    def _weights(self):
        self._check_devices()
        if self.weights is not None:
            w = [self.weights.packed(c) for c in (self.critic_1, self.critic_2)]
        else:
            w = [pack_critic_weights(c) for c in (self.critic_1, self.critic_2)]
        self._packed = w  # kept alive until the launch has been queued
        return [self._struct(x) for x in w]

    @staticmethod
    def _struct(x) -> "_lib.FeCriticWeights":
        return _lib.FeCriticWeights(x["whh"].data_ptr(), x["wx"].data_ptr(), x["wout"].data_ptr(), x["bout"].data_ptr())

    def _entry(self, kind: str):
        lib = self.env._lib
        if kind == "workspace":
            return lib.fe_twin_q_streamed_grad_workspace_floats if self.streamed else lib.fe_twin_q_grad_workspace_floats
        return getattr(lib, f"fe_twin_q_{kind}" + ("_streamed" if self.streamed else ""))

    def _empty_grads(self):
        return list(empty_packed_grads(self.H, self.env._dev).values())

    def _grads_to_torch(self, grads):
        """fe_twin_q_backward_streamed writes torch's row order and layout; the resident kernel the packed one."""
        if self.streamed:
            return grads
        return list(packed_grads_to_torch(dict(zip(GRAD_KEYS, grads)), self.H).values())

    def _shape_args(self):
        return (self.H,)

    def _target_entry(self, cursor: bool):
        lib = self.env._lib
        if cursor:
            return lib.fe_twin_q_target_streamed_c if self.streamed else lib.fe_twin_q_target_c
        return lib.fe_twin_q_target_streamed if self.streamed else lib.fe_twin_q_target

    def _check_target_actor(self, target_actor) -> None:
        from .rollout import FusedLSTMRollout

        if not isinstance(target_actor, FusedLSTMRollout) or target_actor.out_act != 0:
            raise ValueError('target_actor must be a FusedLSTMRollout with output_activation="tanh"')

    def _check_sac_actor(self, actor_roll) -> None:
        from .sac import FusedSACRollout

        if not isinstance(actor_roll, FusedSACRollout):
            raise ValueError("actor_roll must be a FusedSACRollout (the SAC actor's head)")


# ---------------------------------------------------------------- the torch restatements (host or device)
def torch_sac_targets(actor, critic_1, critic_2, rewards, next_states, dones, eps, gamma: float, reward_scale: float = 1.0):
    """``SACAgent.compute_targets`` (SAC_agent.py:200-227) in torch, its operations in its order, with the actor's
    standard normals ``eps`` given: ``actor`` a ``SACActorLSTM``, next_states (B, W, 5), rewards / dones (B, 1)."""
    with torch.no_grad():
        next_actions, next_log_probs = actor.get_actions_and_log_probs(next_states, eps)
        mean_log_probs = next_log_probs.mean(dim=1, keepdim=True)
        q = torch.min(critic_1(next_states, next_actions), critic_2(next_states, next_actions))
        next_entropy = -actor.log_alpha.exp() * mean_log_probs
        return rewards * reward_scale + gamma * (1 - dones) * (q + next_entropy)


def torch_td3_targets(target_actor, critic_1, critic_2, rewards, next_states, dones, eps, gamma: float, std: float,
                      clip: float, reward_scale: float = 1.0):
    """``TD3Agent.compute_targets`` (TD3_agent.py:231-251) in torch with the smoothing normals ``eps`` given:
    ``target_actor`` maps (B, W, 5) to tanh actions (B, 1)."""
    with torch.no_grad():
        target_actions = target_actor(next_states.float())
        clipped_noise = torch.clamp(eps * std, -clip, +clip)
        target_actions = torch.clamp(target_actions + clipped_noise, -1, +1)
        q = torch.minimum(critic_1(next_states, target_actions), critic_2(next_states, target_actions))
        return rewards * reward_scale + gamma * (1 - dones) * q
