"""``PPOAgent.train`` (finenvs/agents/PPO/PPO_agent.py:164-196) for the fused LSTM heads as ONE capturable call.

The reference's update evaluates the critic on the stored states, computes returns and advantages (buffer.py:80-100),
then runs ``epochs`` shuffles of the ``T * N`` samples in ``minibatches`` mini-batches each (buffer.py:127-146), an
actor and a critic step per mini-batch.  ``PPOUpdate.train`` is that update on a ``TrajectoryBuffer(states=True)``
with nothing in it that depends on a host integer that changes between two updates:

* the shuffle is a keyed permutation evaluated on the device (``fe_ppo_minibatch``, include/finenvs_amd_ppo.h; host
  mirror ``rng.ppo_permute``): mini-batch ``m`` of epoch ``e`` is drawn and gathered -- descriptors, actions, old
  log-probs, advantages, returns -- by one launch into static tensors, with the base epoch read from device memory;
* both heads are ``FusedLSTMHead(..., weights=FusedAdam)``: packed weights, gradients, moments and step counters live
  at fixed addresses on the device, ``log_std`` is a plain tensor of the actor's optimizer;
* the values, returns, advantages and old log-probs of the chunk are written into buffers this object owns;
* with ``fused_loss`` the two losses and their gradients are one launch each (``fe_ppo_actor_loss`` /
  ``fe_ppo_value_loss``) instead of some thirty-five element-wise ones.

So ``GraphedUpdate(update.train)`` (finenvs_amd/graphed.py) replays a whole update as one hipGraph launch.  Between two
replays the caller runs the rollout into the same trajectory chunk and hands the rollout's means over with
``load_means`` (``FusedLSTMRollout.run`` allocates them afresh at every call).  Scope: one asset (A = 1), fewer than
2^32 samples; the warm-up calls of ``GraphedUpdate`` are real updates; the epoch counter lives on the device, the
host's copy (``epochs_drawn``) counts eager ``run()`` calls only.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import List, Optional, Tuple

import torch
from torch.distributions import Distribution, Normal

from . import _lib
from .lstm_head import FusedLSTMHead, ppo_actor_loss, ppo_critic_loss, ppo_loss_workspace
from .optim import FusedAdam
from .rng import ppo_permute


def minibatch_size(num_samples: int, minibatches: int) -> int:
    """Samples per mini-batch: ``num_samples // minibatches``, the remainder dropped as in buffer.py:127-146."""
    n, M = int(num_samples), int(minibatches)
    if n < 1 or not 1 <= M <= n:
        raise ValueError(f"need 1 <= minibatches <= num_samples (got {M}, {n})")
    return n // M


def minibatch_indices(seed: int, epoch: int, num_samples: int, minibatches: int, m: int) -> List[int]:
    """Host mirror of ``fe_ppo_minibatch``'s ``indices_out``: the samples (``env * T + step``) of mini-batch ``m`` of
    ``minibatches`` in epoch ``epoch``'s shuffle of ``num_samples`` samples."""
    B = minibatch_size(num_samples, minibatches)
    if not 0 <= int(m) < int(minibatches):
        raise ValueError(f"mini-batch {m} of {minibatches}")
    return [ppo_permute(seed, epoch, num_samples, int(m) * B + b) for b in range(B)]


@contextlib.contextmanager
def no_distribution_checks():
    """torch's distributions validate their arguments with a reduction the host waits for, which a stream capture
    refuses; the values they compute do not depend on it."""
    before = Distribution._validate_args
    Distribution.set_default_validate_args(False)
    try:
        yield
    finally:
        Distribution.set_default_validate_args(before)


class PPOUpdate:
    """One ``PPOAgent.train`` on a trajectory chunk of descriptors; see the module docstring.

        opt_a, opt_c = FusedAdam(lr=3e-4), FusedAdam(lr=3e-4)
        opt_a.add(actor); opt_a.add_tensor(log_std); opt_c.add(critic)
        actor_head, critic_head = FusedLSTMHead(env, actor, weights=opt_a), FusedLSTMHead(env, critic, weights=opt_c)
        update = PPOUpdate(env, traj, actor_head, critic_head, log_std, opt_a, opt_c)
        graph = None
        for it in range(iterations):
            actor_head.rollout.run(T, noise=noise, std=std, record_means=True, trajectory=traj)
            update.load_means(actor_head.rollout.means)
            if graph is None:
                graph = GraphedUpdate(update.train, warmup=1)     # a real update, then the capture
            else:
                graph.replay()
            traj.clear()

    ``seed``: the permutation's key (default: the env's seed).  ``fused_loss=False`` keeps the torch expressions of
    ``lstm_head.torch_ppo_actor_loss`` / ``torch_ppo_critic_loss``."""

    def __init__(self, env, traj, actor_head, critic_head, log_std, actor_opt, critic_opt, epochs: int = 4,
                 minibatches: int = 4, clip_epsilon: float = 0.2, entropy_coefficient: float = 0.01, gamma: float = 0.99,
                 seed: Optional[int] = None, fused_loss: bool = True):
        for head, opt, what in ((actor_head, actor_opt, "actor"), (critic_head, critic_opt, "critic")):
            if not isinstance(head, FusedLSTMHead):
                raise ValueError(f"the {what} head must be a FusedLSTMHead")
            if not isinstance(opt, FusedAdam) or head.weights is not opt:
                raise ValueError(f"the {what} head must be built with weights= its FusedAdam ({what}_opt): a head that "
                                 "packs its module per call is not capturable")
        if not isinstance(log_std, torch.Tensor) or not any(s.param is log_std for s in actor_opt.plain):
            raise ValueError("log_std must be registered with actor_opt.add_tensor")
        if log_std.numel() != 1:
            raise ValueError("PPOUpdate trains one action per env (A = 1): log_std must have one element")
        if actor_head.env is not env or critic_head.env is not env:
            raise ValueError("both heads must belong to `env`")
        if not getattr(traj, "has_states", False) or traj.A != 1 or traj.N != int(env.num_envs) or traj.device != env._dev:
            raise ValueError("traj must be a TrajectoryBuffer(T, num_envs, 1, states=True) on the env's device")
        self.epochs, self.minibatches = int(epochs), int(minibatches)
        self.T, self.N = traj.T, traj.N
        self.n = self.T * self.N
        if self.epochs < 1:
            raise ValueError("epochs must be >= 1")
        if self.n >= 1 << 32:
            raise ValueError(f"{self.n} samples do not fit the 32-bit permutation")
        self.B = minibatch_size(self.n, self.minibatches)
        self.env, self.traj, self.actor_head, self.critic_head, self.log_std = env, traj, actor_head, critic_head, log_std
        self.actor_opt, self.critic_opt = actor_opt, critic_opt
        self.clip_epsilon, self.entropy_coefficient, self.gamma = float(clip_epsilon), float(entropy_coefficient), float(gamma)
        self.seed = (int(env.seed) if seed is None else int(seed)) & 0xFFFFFFFFFFFFFFFF
        self.fused_loss = bool(fused_loss)
        self._lib = _lib.load()
        dev, T, N, B = env._dev, self.T, self.N, self.B
        f32 = dict(dtype=torch.float32, device=dev)
        # the chunk's per-sample columns, time-major as the trajectory's own fields
        self.means = torch.zeros((T, N, 1), **f32)
        self.old_log_probs = torch.zeros((T, N), **f32)
        self.all_values = torch.zeros((T + 1, N), **f32)  # row T: the bootstrap state's
        self.values = self.all_values[:T]
        self.returns = torch.zeros((T, N), **f32)
        self.advantages = torch.zeros((T, N), **f32)
        self.cursor = torch.zeros((_lib.PPO_CURSOR_WORDS,), dtype=torch.int64, device=dev)  # epoch, errors
        self.epochs_drawn = 0  # the host's copy of cursor[0]: advanced by eager run() calls, not by a graph's replays
        # one mini-batch, overwritten by every draw
        self.indices = torch.zeros((B,), dtype=torch.int64, device=dev)
        self.mb_src = torch.zeros((B,), dtype=torch.int64, device=dev)
        self.mb_pos = torch.zeros((B, 1), dtype=torch.float64, device=dev)
        self.mb_actions = torch.zeros((B, 1), **f32)
        self.mb_old_log_probs, self.mb_advantages, self.mb_returns = (torch.zeros((B,), **f32) for _ in range(3))
        cols = (self.old_log_probs, self.advantages, self.returns)
        outs = (self.mb_old_log_probs, self.mb_advantages, self.mb_returns)
        self._columns = (C.c_void_p * len(cols))(*(t.data_ptr() for t in cols))
        self._columns_out = (C.c_void_p * len(outs))(*(t.data_ptr() for t in outs))
        self._workspaces = (ppo_loss_workspace(B, dev), ppo_loss_workspace(B, dev)) if self.fused_loss else (None, None)
        self._bound = self._chunk_addresses()

    def _chunk_addresses(self) -> Tuple[int, ...]:
        tr = self.traj
        return tuple(t.data_ptr() for t in (tr.obs_src, tr.obs_pos, tr.actions, tr.rewards, tr.dones))

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.env._dev).cuda_stream

    def _check_chunk(self) -> None:
        if not self.traj.full():
            raise RuntimeError(f"the trajectory holds {len(self.traj)} of {self.T} steps: train() takes a full chunk")
        if self._chunk_addresses() != self._bound:
            raise RuntimeError("the trajectory switched chunks since this PPOUpdate was built: its launches (and a graph "
                               "captured around them) read the chunk bound at construction")

    # ---- between the rollout and the update
    def load_means(self, means: torch.Tensor) -> None:
        """The rollout's ``means`` ((T, N, 1), ``FusedLSTMRollout.run(record_means=True)``) into the static buffer the
        old log-probs are computed from: a device copy, outside the graph."""
        if means.numel() != self.n:
            raise ValueError(f"means must hold {self.T} x {self.N} elements, got {tuple(means.shape)}")
        self.means.copy_(means.reshape(self.T, self.N, 1), non_blocking=True)

    # ---- the update
    def prepare(self) -> None:
        """Values of the T + 1 stored states (PPO_agent.py:166-171), returns and advantages (buffer.py:80-100) and the
        old log-probs (PPO_agent.py:100-103) of the chunk, into the static buffers."""
        self._check_chunk()
        tr, T, N = self.traj, self.T, self.N
        with torch.no_grad(), no_distribution_checks():
            self.critic_head.rollout.forward(tr.obs_src, tr.obs_pos, out=self.all_values)
            rew, don = tr.rewards, tr.dones
            if tr.C != tr.N:  # the scan kernel wants dense (T, N) inputs
                rew, don = rew.contiguous(), don.contiguous()
            _lib.check(self._lib.fe_traj_returns(
                rew.data_ptr(), don.data_ptr(), self.values.data_ptr(), self.all_values[T].data_ptr(), T, N, self.gamma,
                self.returns.data_ptr(), self.advantages.data_ptr(), self._stream()), self._lib)
            log_probs = Normal(self.means, self.log_std.detach().exp()).log_prob(tr.actions)  # log_std read on the device
            self.old_log_probs.copy_(log_probs.reshape(T, N))

    def draw(self, epoch_offset: int, m: int) -> None:
        """Mini-batch ``m`` of epoch ``cursor[0] + epoch_offset`` into the static mini-batch tensors (one launch)."""
        tr = self.traj
        src, pos, act = self._bound[:3]
        _lib.check(self._lib.fe_ppo_minibatch(
            src, pos, act, self.T, self.N, tr.C, 1, self._columns, self._columns_out, len(self._columns),
            self.cursor.data_ptr(), self.seed, int(epoch_offset), self.minibatches, int(m), self.indices.data_ptr(),
            self.mb_src.data_ptr(), self.mb_pos.data_ptr(), self.mb_actions.data_ptr(), self._stream()), self._lib)

    def run(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """``epochs`` x ``minibatches`` actor and critic steps (PPO_agent.py:175-196), then the epoch counter moves on.
        Returns the last (actor loss, critic loss) as device tensors."""
        self._check_chunk()
        ws_a, ws_c = self._workspaces
        loss_a = loss_c = None
        with no_distribution_checks():
            for e in range(self.epochs):
                for m in range(self.minibatches):
                    self.draw(e, m)
                    loss_a = ppo_actor_loss(self.actor_head, self.log_std, self.mb_src, self.mb_pos, self.mb_actions,
                                            self.mb_old_log_probs, self.mb_advantages, self.clip_epsilon,
                                            self.entropy_coefficient, fused=self.fused_loss, workspace=ws_a)
                    loss_a.backward()
                    self.actor_opt.step()
                    loss_c = ppo_critic_loss(self.critic_head, self.mb_src, self.mb_pos, self.mb_returns,
                                             fused=self.fused_loss, workspace=ws_c)
                    loss_c.backward()
                    self.critic_opt.step()
        _lib.check(self._lib.fe_ppo_epochs_advance(self.cursor.data_ptr(), self.epochs, self._stream()), self._lib)
        if not torch.cuda.is_current_stream_capturing():  # a capture executes nothing
            self.epochs_drawn += self.epochs
        return loss_a.detach(), loss_c.detach()

    def train(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """``prepare(); run()``: the whole update, capturable."""
        self.prepare()
        return self.run()

    # ---- for tests and debugging
    def minibatch_indices(self, epoch_offset: int, m: int, base: Optional[int] = None) -> torch.Tensor:
        """The samples ``draw(epoch_offset, m)`` gathers, from the host mirror, as a (B,) int64 tensor on the device.
        ``base``: the epoch counter's value (default: ``epochs_drawn``, what the host last knew -- replays of a
        captured graph advance the device's counter only)."""
        e = (self.epochs_drawn if base is None else int(base)) + int(epoch_offset)
        return torch.tensor(minibatch_indices(self.seed, e, self.n, self.minibatches, m), dtype=torch.int64,
                            device=self.env._dev)
