"""SAC's LSTM actor: the torch module a learner trains, and the fused rollout that acts with it in the kernel.

``SACActorLSTM`` restates the reference's ``finenvs/agents/SAC/actor.py:ActorLSTM`` with shape ``(5, H, A)``:
``nn.LSTM(5, H)`` over the observation window, ``last_layer = Linear(H, H)`` + Identity on the last hidden state
(``LSTMNetwork`` duplicates the last size of ``(5, H)``, networks/lstm.py:21-23, 36-39), then ``mu_layer`` and
``std_layer = Linear(H, A)`` with ``softplus`` on the std (SAC/actor.py:44-49) and the tanh-squashed sample with its
log-probability (SAC/actor.py:51-61).  It runs per (env, asset) pair on ``(B, W, 5)`` windows; ``pair_states`` cuts a
multi-asset observation ``(B, W, 5A)`` into those.

``FusedSACRollout`` runs ``SACAgent.step`` -> ``env.step`` (SAC_agent.py:110-121) for K steps in one launch of
``fe_env_rollout_sac`` (include/finenvs_amd_sac.h): the LSTM recurrence of ``FusedLSTMRollout`` plus the SAC head,
with ``mu_layer`` / ``std_layer`` of one output per pair (``A = 1``).  Its ``forward`` is the no-grad actor half of
``compute_targets`` (SAC_agent.py:200-225) on observation descriptors, e.g. replayed next states.  The gradient half
runs on descriptors too: ``sample`` is ``forward``'s (actions, log_probs) as a differentiable function of the actor's
ten parameters (C ABI ``fe_sac_backward``, include/finenvs_amd_sac_grad.h), and ``actor_losses`` the actor's and the
temperature's losses of ``Actor.compute_losses`` (SAC/actor.py:63-81) on replayed transitions.

H in {32, 64, 128}; with ``streamed=True`` also H in {256, 512, 1024}, the reference's own ``hidden_dim``: the same
methods on the entries of include/finenvs_amd_sac_streamed.h, whose recurrent and last-layer weights stream from L2.
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
from .critic import FusedTwinCritic
from .replay import as_draw
from .rollout import _FusedEvaluation, log_return_f32, lstm_fragment_major, lstm_pack, rollout_outputs

SAC_HIDDEN_SIZES = (32, 64, 128)
SAC_STREAMED_HIDDEN_SIZES = (256, 512, 1024)  # with streamed=True


class _SACActor(nn.Module):
    """What ``SACActorLSTM`` and ``SACActorMLP`` (finenvs_amd/mlp_sac.py) share: the tanh-Gaussian distribution on the
    network's output ``forward(states)`` and the temperature that moves with the module.  It holds no parameters; a
    module provides ``forward``, ``mu_layer``, ``std_layer`` and ``log_alpha``."""

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        self.log_alpha = fn(self.log_alpha.detach()).requires_grad_(True)  # .to(device) moves the temperature too
        return self

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


class SACActorLSTM(_SACActor):
    """The reference's SAC ``ActorLSTM((5, H, A), sequence_length=W)`` as a plain module (no optimizer inside):
    submodules ``lstm``, ``last_layer``, ``mu_layer``, ``std_layer``; ``log_alpha`` the entropy temperature (a leaf
    tensor outside ``parameters()``, as the reference keeps it with its own optimizer) and ``target_entropy = -A``."""

    def __init__(self, H: int = 128, W: int = 4, A: int = 1, starting_alpha: float = 1.0, device=None):
        super().__init__()
        self.input_size, self.hidden_size, self.sequence_length, self.num_actions = 5, int(H), int(W), int(A)
        self.lstm = nn.LSTM(5, self.hidden_size, num_layers=1, batch_first=True, device=device)
        self.last_layer = nn.Sequential(nn.Linear(self.hidden_size, self.hidden_size, device=device), nn.Identity())
        self.mu_layer = nn.Linear(self.hidden_size, self.num_actions, device=device)
        self.std_layer = nn.Linear(self.hidden_size, self.num_actions, device=device)
        self.log_alpha = torch.tensor(math.log(starting_alpha), device=device, requires_grad=True)
        self.target_entropy = -float(self.num_actions)

    def forward(self, states: torch.Tensor) -> torch.Tensor:
        """(B, W, 5) -> the last layer's output z (B, H)."""
        if states.dim() != 3 or states.shape[1] != self.sequence_length or states.shape[2] != self.input_size:
            raise ValueError(f"states must be (B, {self.sequence_length}, {self.input_size}), got {tuple(states.shape)}")
        out, _ = self.lstm(states)
        return self.last_layer(out[:, -1, :])


def pair_states(states: torch.Tensor, A: int) -> torch.Tensor:
    """(B, W, 5A) observations -> (B * A, W, 5) per-pair windows, row b * A + a (the fused heads' pair order)."""
    B, W, F5 = states.shape
    if F5 != 5 * A:
        raise ValueError(f"states have {F5} features per row, expected 5 * {A}")
    return states.reshape(B, W, A, 5).permute(0, 2, 1, 3).reshape(B * A, W, 5)


def check_actor(actor: nn.Module, streamed: bool = False) -> int:
    """The hidden size of an actor the fused SAC head can run; ValueError otherwise.  ``streamed``: H may also be 256,
    512 or 1024 (the streamed kernels of include/finenvs_amd_sac_streamed.h)."""
    lstm = actor.lstm
    if lstm.num_layers != 1 or lstm.bidirectional or lstm.input_size != 5 or not lstm.batch_first or lstm.proj_size:
        raise ValueError("the fused SAC head needs nn.LSTM(5, H, num_layers=1, batch_first=True)")
    H = int(lstm.hidden_size)
    if streamed and H not in SAC_HIDDEN_SIZES + SAC_STREAMED_HIDDEN_SIZES:
        raise ValueError(f"the fused SAC head supports H in {SAC_HIDDEN_SIZES + SAC_STREAMED_HIDDEN_SIZES} (got {H})")
    if not streamed and H not in SAC_HIDDEN_SIZES:
        raise ValueError(f"the fused SAC head supports H in {SAC_HIDDEN_SIZES} (got {H})"
                         + ("; pass streamed=True for the streamed kernels of H in "
                            f"{SAC_STREAMED_HIDDEN_SIZES}" if H in SAC_STREAMED_HIDDEN_SIZES else ""))
    last = actor.last_layer[0]
    if last.in_features != H or last.out_features != H:
        raise ValueError(f"last_layer must be Linear({H}, {H})")
    for name in ("mu_layer", "std_layer"):
        layer = getattr(actor, name)
        if layer.in_features != H or layer.out_features != 1:
            raise ValueError(f"{name} must be Linear({H}, 1): the fused head has one output per (env, asset) pair")
    return H


def pack_sac_weights(actor: nn.Module) -> Dict[str, torch.Tensor]:
    """The actor's current parameters as fe_env_rollout_sac reads them (f32, on the parameters' device, no host sync):
    whh / wx as ``lstm_pack``, ``wl`` the last layer fragment-major ([row tile][k group][lane = r + 32 h][4] =
    W_l[32 t + r][8 g + 4 h + m]), ``bl``, ``wmu``, ``wstd`` (H), ``bmu`` / ``bstd`` (1).  At H > 128 ``whh`` is
    fragment-major (``lstm_fragment_major``), as the streamed kernels read it."""
    H = check_actor(actor, streamed=True)
    lstm = actor.lstm
    whh, wx = lstm_pack(lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0, H)
    if H > 128:
        whh = lstm_fragment_major(whh, H)
    last = actor.last_layer[0]
    wl = last.weight.detach().float().reshape(H // 32, 32, H // 8, 2, 4).permute(0, 2, 3, 1, 4).contiguous().reshape(H, H)
    return {
        "whh": whh, "wx": wx, "wl": wl,
        "bl": last.bias.detach().float().reshape(H).contiguous(),
        "wmu": actor.mu_layer.weight.detach().float().reshape(H).contiguous(),
        "bmu": actor.mu_layer.bias.detach().float().reshape(1).clone(),
        "wstd": actor.std_layer.weight.detach().float().reshape(H).contiguous(),
        "bstd": actor.std_layer.bias.detach().float().reshape(1).clone(),
    }


def unpack_last_layer(wl: torch.Tensor) -> torch.Tensor:
    """Inverse of the fragment-major packing of ``pack_sac_weights``: (H, H) in torch's [out, in] order."""
    H = int(wl.shape[0])
    return wl.reshape(H // 32, H // 8, 2, 32, 4).permute(0, 3, 1, 2, 4).reshape(H, H)


SAC_GRAD_KEYS = ("w_ih", "w_hh", "b_ih", "b_hh", "w_l", "b_l", "w_mu", "b_mu", "w_std", "b_std")  # fe_sac_grads' fields


def actor_parameters(actor: nn.Module) -> Tuple[torch.Tensor, ...]:
    """The ten parameter tensors of a SAC actor in ``SAC_GRAD_KEYS`` order: ``lstm.weight_ih_l0 (4H, 5)``,
    ``weight_hh_l0 (4H, H)``, ``bias_ih_l0``, ``bias_hh_l0`` (4H), ``last_layer[0].weight (H, H)`` / ``.bias (H)``,
    ``mu_layer.weight (1, H)`` / ``.bias (1)``, ``std_layer.weight (1, H)`` / ``.bias (1)``."""
    lstm, last = actor.lstm, actor.last_layer[0]
    return (lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0, last.weight, last.bias,
            actor.mu_layer.weight, actor.mu_layer.bias, actor.std_layer.weight, actor.std_layer.bias)


class _SacSample(torch.autograd.Function):
    """(actions, log_probs) of a ``_FusedSAC.forward`` as a differentiable function of the actor's parameters: the
    forward is the family's forward entry, the backward its backward entry on the weights the forward packed (the
    activations recomputed)."""

    @staticmethod
    def forward(ctx, roll, src, pos, noise, *params):
        actions, log_probs, means, stds = roll.forward(src, pos, noise, _snapshot=True)  # the backward reads this pack
        roll.last = {"means": means, "stds": stds}
        ctx.set_materialize_grads(False)  # an output nobody used gets None, not zeros: its pointer is null
        # the packed weights (and the LSTM's two bias floats) forward() fetched: backward makes no second copy to the
        # host (an empty batch packs nothing and launches nothing, in either direction)
        ctx.roll, ctx.packed, ctx.biases = roll, getattr(roll, "_packed", None), getattr(roll, "_biases", None)
        ctx.version = None if roll.weights is None else roll.weights.version
        ctx.save_for_backward(src, pos, noise, actions, stds)
        return actions, log_probs

    @staticmethod
    def backward(ctx, g_a, g_lp):
        roll, need = ctx.roll, ctx.needs_input_grad
        out = [None] * len(need)
        if (g_a is None and g_lp is None) or not any(need[4:]):
            return tuple(out)
        src, pos, noise, actions, stds = ctx.saved_tensors
        env, H, B = roll.env, roll.H, int(src.numel())
        W, dev = int(env.num_intervals), env._dev
        grads = [torch.empty(shape, dtype=torch.float32, device=dev) for shape in roll._grad_shapes(H, W)]
        if B:
            g_a, g_lp = (None if g is None else g.reshape(B).float().contiguous() for g in (g_a, g_lp))
            ws = torch.empty((int(roll._entry("workspace")(H, W, B)),), dtype=torch.float32, device=dev)
            if roll.weights is not None:
                roll.weights.check_version(ctx.version)
            sg = roll.GRADS(*(g.data_ptr() for g in grads))
            ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
            _lib.check(roll._entry("backward")(
                env._handle, *roll._saved_args(ctx.packed, ctx.biases), src.data_ptr(), pos.data_ptr(), B, noise.data_ptr(),
                actions.data_ptr(), stds.data_ptr(), ptr(g_a), ptr(g_lp), ws.data_ptr(), C.byref(sg), env._stream()),
                env._lib)
        else:  # nothing to launch: the sums over an empty batch are zeros
            for g in grads:
                g.zero_()
        for k, g in enumerate(grads):
            if need[4 + k]:
                out[4 + k] = g
        return tuple(out)


class _FusedSAC(_FusedEvaluation):
    """What ``FusedSACRollout`` and ``FusedMLPSACRollout`` (finenvs_amd/mlp_sac.py) share: everything that does not
    depend on the network -- the noise check, ``run``, ``forward``, ``sample`` with its autograd function, and
    ``actor_losses``.  A family provides ``_weights(snapshot=False)`` (packs the actor's current parameters into
    ``self._packed`` and returns them as its callers pass them on; ``snapshot``, meaningful for the MLP only, makes them
    copies a pending ``backward()`` can keep), ``_net_args(w)`` (of that return value, what its C entries take between
    the env and the descriptors or the step count) and ``_saved_args(packed, biases)`` (the same of a kept pack),
    ``ENTRIES`` or ``_entry(kind)`` (the ``"rollout"``, ``"forward"``, ``"backward"`` and ``"workspace"`` entries),
    ``_parameters()`` (the actor's parameter tuple, checked: its dtype and device messages), ``_grad_shapes(H, W)`` and
    ``GRADS`` (the gradients in the parameters' order, and their ctypes struct) and ``TWIN`` (the twin critic
    ``actor_losses`` accepts).  ``weights`` (a ``FusedAdam``) and ``self._biases`` are the LSTM's alone."""

    weights = None

    def _bind(self) -> None:
        """The descriptors and buffers of a rollout object of ``self.env``."""
        env, dev = self.env, self.env._dev
        self.obs_src = torch.empty((env.num_envs,), dtype=torch.int64, device=dev)
        self.obs_pos = torch.empty((env.num_envs, env.num_assets), dtype=torch.float64, device=dev)
        self._lr32 = log_return_f32(env)
        self.means = self.stds = None
        self.last: Dict[str, torch.Tensor] = {}  # means / stds of the latest sample()
        self.sync_from_env()

    def _entry(self, kind: str):
        return getattr(self.env._lib, self.ENTRIES[kind])

    def _net_args(self, w):
        return w

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
        """Returns (actions (K, N, A) f32, rewards (K, N) f64, dones (K, N) int32).

        With ``noise`` -- (K, N, A) f32 standard normals from the caller's generator -- every env acts with
        ``tanh(mu + eps * std)`` except the training-mode env's evaluation env, which acts on ``mu`` (SACAgent.step,
        SAC_agent.py:110-121); the env scales, rounds and clamps the action as ``env.step`` does, so a mean beyond
        [-1, 1] trades the clamped amount.  Without noise every env acts on ``mu``: the deterministic evaluation form.
        (An evaluate-mode env has no evaluation env, so there every env samples, while the reference's ``agent.step``
        overwrites the LAST row with the mean whatever the env's mode; a caller who wants deterministic evaluation
        passes no noise.)  ``record_means`` / ``record_stds`` keep mu / std in ``self.means`` / ``self.stds``
        ((K, N, A)).  ``trajectory``: an empty ``TrajectoryBuffer(K, N, A, states=True)`` without capacity padding,
        filled as ``FusedLSTMRollout.run`` fills it (``ReplayBuffer.extend(trajectory)`` then stores the chunk).
        ``record_actions=False`` (``evaluate_returns``) keeps no actions: the first element is None."""
        env, K = self.env, int(num_steps)
        N, A, dev = env.num_envs, env.num_assets, env._dev
        if K < 1:
            raise ValueError("num_steps must be >= 1")
        noise = self._check_noise(noise, (K, N, A))
        actions, rewards, dones, src_out, pos_out = rollout_outputs(env, K, trajectory, record_actions)
        self._begin_run()
        w = self._net_args(self._weights())
        self.means = torch.empty((K, N, A), dtype=torch.float32, device=dev) if record_means else None
        self.stds = torch.empty((K, N, A), dtype=torch.float32, device=dev) if record_stds else None
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        _lib.check(self._entry("rollout")(
            env._handle, *w, K, self.obs_src.data_ptr(), self.obs_pos.data_ptr(), ptr(noise), ptr(actions), ptr(self.means),
            ptr(self.stds), rewards.data_ptr(), dones.data_ptr(), ptr(src_out), ptr(pos_out), env._stream()), env._lib)
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
            w = self._net_args(self._weights(_snapshot))
            ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
            _lib.check(self._entry("forward")(
                env._handle, *w, src.data_ptr(), pos.data_ptr(), B, ptr(noise), ptr(actions), ptr(log_probs),
                means.data_ptr(), stds.data_ptr(), env._stream()), env._lib)
        return actions, log_probs, means, stds

    # ---------------------------------------------------------------- the gradient half
    def sample(self, obs_src: torch.Tensor, obs_pos: torch.Tensor, noise: torch.Tensor):
        """``forward``'s ``(actions, log_probs)``, each (B, 1) float32 and the same values bit for bit, as a
        differentiable function of the actor's parameters (the LSTM's ten: C ABI ``fe_sac_backward``,
        include/finenvs_amd_sac_grad.h; the MLP's eight: ``fe_mlp_sac_backward``): ``get_actions_and_log_probs``
        (SAC/actor.py:51-61) with ``noise`` (B, 1) the standard normals of ``rsample``.  ``backward()`` accumulates into
        the parameters' ``.grad`` as the torch module would; an output that received no gradient costs nothing, and with
        every parameter frozen nothing launches.  The means and stds of the call stay in ``self.last`` (not
        differentiable)."""
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
        params = self._parameters()
        src = obs_src.reshape(B).to(device=env._dev, dtype=torch.int64).contiguous()
        pos = obs_pos.reshape(B, 1).to(device=env._dev, dtype=torch.float64).contiguous()
        return _SacSample.apply(self, src, pos, noise, *params)

    def actor_losses(self, buffer, indices: torch.Tensor, twin, noise: Optional[torch.Tensor] = None):
        """``(actor_loss, alpha_loss)`` of ``Actor.compute_losses`` (SAC/actor.py:63-81) on the transitions ``indices``
        (logical, (B,)) of ``buffer``: the ring's state descriptors, nothing rendered.  ``sample`` with ``noise`` (B, 1)
        -- by default ``torch.randn``, the draw ``rsample`` makes -- then ``q = min(twin.q(src, pos, actions))`` of
        ``twin``, this family's twin critic of this env (``FusedSACRollout``: a ``FusedTwinCritic``,
        ``FusedMLPSACRollout``: a ``FusedTwinMLPCritic``), and

            entropy_term = -log_alpha.exp() * mean_log_probs
            actor_loss = -(q + entropy_term).mean()
            alpha_loss = (-log_alpha.exp() * (mean_log_probs + target_entropy).detach()).mean()

        with ``log_alpha`` / ``target_entropy`` the actor's.  ``alpha`` enters the actor loss as the reference combines
        it, with its graph: ``actor_loss.backward()`` also leaves ``mean(log_probs) * alpha`` in ``log_alpha.grad``, which
        the reference discards (its temperature optimizer zeroes the gradient before ``alpha_loss.backward()``).
        examples/sac_time_series.py writes the detached form ``-(q - alpha.detach() * mean_log_probs).mean()``: the same
        value and the same actor gradients, without that stray temperature gradient.  ``backward()`` of the actor loss
        also accumulates into the critics' ``.grad`` unless they are frozen (as in torch); an index outside
        ``[0, size)`` makes the actor loss NaN.  ``indices`` may be a ``ReplayDraw`` of a ``cursor=True`` buffer (no
        host integer enters then: capturable)."""
        draw = as_draw(buffer, indices, "actor_losses")
        if not isinstance(twin, self.TWIN) or twin.env is not self.env:
            raise ValueError(f"twin must be a {self.TWIN.__name__} of this rollout's env")
        if indices is None:
            raise ValueError("actor_losses needs the indices of the sampled transitions")
        idx = twin._indices(buffer, indices if draw is None else draw.indices, None)
        B = int(idx.numel())
        if noise is None:
            noise = torch.randn((B, 1), device=self.env._dev)
        if draw is not None:  # the draw's gathered descriptors; its indices are in range by construction
            src, pos = draw.state_src, draw.state_pos.reshape(B)
        else:
            slots = buffer.physical(idx)
            src, pos = buffer.state_src[slots], buffer.state_pos[slots].reshape(B)
        actions, log_probs = self.sample(src, pos, noise)
        q = torch.min(*twin.q(src, pos, actions))
        if draw is None:
            valid = ((idx >= 0) & (idx < buffer.size())).reshape(B, 1)
            q = torch.where(valid, q, torch.full((), float("nan"), device=q.device))
        mean_log_probs = log_probs.mean(dim=1, keepdim=True)
        log_alpha = self.actor.log_alpha
        actor_loss = -(q + -log_alpha.exp() * mean_log_probs).mean()
        alpha_loss = (-log_alpha.exp() * (mean_log_probs + self.actor.target_entropy).detach()).mean()
        return actor_loss, alpha_loss


class FusedSACRollout(_FusedSAC):
    """K env steps per launch with the SAC actor's head in the kernel (C ABI ``fe_env_rollout_sac``).

    The actor's parameters are re-packed on the device at every ``run`` / ``forward`` (a few small launches and one
    8-byte copy of the two output biases to the host, which the C ABI takes by value), so an optimizer step on ``actor``
    is seen by the next call.  The actor must live on the env's device.

    ``weights``: a ``FusedAdam`` (finenvs_amd/optim.py) that ``actor`` is registered with.  ``run``, ``forward`` and
    ``sample`` then read that optimizer's packed buffers and the two output biases on the device: nothing is packed
    per call and nothing is copied to the host.  Those buffers are rewritten in place: a ``weights.step()`` or
    ``weights.repack()`` between ``sample`` and its ``backward()`` is a RuntimeError.

    ``streamed=True`` also admits H in {256, 512, 1024}, the sizes whose recurrent and last-layer weights stream from L2
    (C ABI ``fe_env_rollout_sac_streamed`` / ``fe_sac_forward_streamed`` / ``fe_sac_backward_streamed``,
    include/finenvs_amd_sac_streamed.h), with the same methods and semantics.  There the two output biases are always
    read on the device (nothing is copied to the host, with or without ``weights=``), the backward is several launches
    per LSTM time step and its workspace grows with the batch up to ``fe_lstm_streamed_grad_chunk_pairs`` pairs, and
    ``run`` is the fused kernel at every env count: the split-by-time-step form of ``fe_env_rollout_lstm_split`` is not
    extended to SAC, so below a few thousand pairs one CU walks the whole matrix.  The small sizes go the
    register-resident way whether or not ``streamed`` is passed."""

    GRADS, TWIN = _lib.FeSacGrads, FusedTwinCritic

    def __init__(self, env, actor: nn.Module, weights=None, streamed: bool = False):
        self.H = check_actor(actor, streamed)
        self.streamed = self.H > 128  # which entries run: a function of H alone
        self.weights = weights
        if weights is not None:
            weights.packed(actor)  # ValueError if the actor is not registered with it
        if env.redraw != "device" and not env.evaluate:
            raise ValueError('the fused rollout needs redraw="device" (or evaluate mode): no host in the loop')
        if actor.lstm.weight_hh_l0.device != torch.device(env._dev):
            raise ValueError(f"the actor's parameters must live on the env's device {env._dev}")
        self.env, self.actor = env, actor
        self._bind()

    def _entry(self, kind: str):
        """The entry of include/finenvs_amd_sac*.h for the hidden size and for where the weights live: ``_streamed`` at
        H > 128, ``_p`` with ``weights=`` (the two biases device addresses), else the by-value form."""
        lib = self.env._lib
        if kind == "workspace":
            return lib.fe_sac_streamed_grad_workspace_floats if self.streamed else lib.fe_sac_grad_workspace_floats
        name = {"rollout": "fe_env_rollout_sac", "forward": "fe_sac_forward", "backward": "fe_sac_backward"}[kind]
        return getattr(lib, name + ("_streamed" if self.streamed else "_p" if self.weights is not None else ""))

    def _weights(self, snapshot: bool = False):
        """The weight arguments of fe_env_rollout_sac / fe_sac_forward -- of their ``_p`` siblings with ``weights=``
        and of their ``_streamed`` ones at H > 128, where the two biases are device addresses."""
        w = self.weights.packed(self.actor) if self.weights is not None else pack_sac_weights(self.actor)
        if w["whh"].device != torch.device(self.env._dev):
            raise ValueError(f"the actor's parameters must live on the env's device {self.env._dev}")
        if self.weights is not None or self.streamed:  # the biases are read on the device
            bmu, bstd = w["bmu"].data_ptr(), w["bstd"].data_ptr()
        else:
            # the two output biases are kernel arguments: one small copy to the host, ordered after any pending update
            bmu, bstd = torch.cat([w["bmu"], w["bstd"]]).cpu().tolist()
        self._packed, self._biases = w, (bmu, bstd)  # kept alive until the launch has been queued
        return self._saved_args(w, self._biases)

    def _saved_args(self, w, biases):
        return (self._lr32.data_ptr(), w["whh"].data_ptr(), w["wx"].data_ptr(), w["wl"].data_ptr(), w["bl"].data_ptr(),
                w["wmu"].data_ptr(), biases[0], w["wstd"].data_ptr(), biases[1], self.H)

    def _parameters(self) -> Tuple[torch.Tensor, ...]:
        params = actor_parameters(self.actor)
        if any(p.dtype is not torch.float32 for p in params):
            raise ValueError("the fused actor's gradient needs float32 parameters")
        if any(p.device != torch.device(self.env._dev) for p in params):
            raise ValueError(f"the actor's parameters must live on the env's device {self.env._dev}")
        return params

    @staticmethod
    def _grad_shapes(H: int, W: int):
        return (4 * H, 5), (4 * H, H), (4 * H,), (4 * H,), (H, H), (H,), (1, H), (1,), (1, H), (1,)
