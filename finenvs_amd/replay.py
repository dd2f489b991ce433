"""Off-policy replay on the device: the reference's TD3 / SAC buffer (finenvs/agents/off_policy_buffer.py, "OPB") with
states kept as observation descriptors.

OPB stores every transition's ``states`` and ``next_states`` as rendered ``.float()`` observations (2 x 20WA bytes) and
each ``store`` moves the whole container (``torch.cat`` + ``index_select``, OPB:24-31, 56-66).  ``ReplayBuffer`` keeps a
ring of ``max_size`` transitions in HBM as descriptors (``obs_src`` i64, ``obs_pos`` A x f64 per state: what
``env.step(..., descriptors_out=)`` emits) plus the f32 action, reward and done -- 2 (8 + 8A) + 4A + 8 bytes -- and a
store is one O(N) kernel (C ABI ``fe_replay_append``, include/finenvs_amd_replay.h).  ``get_mini_batch`` gathers the
sampled transitions and renders their states and next states in ONE launch (``fe_replay_sample``), returning OPB's five
fields with OPB's dtypes and shapes, bit for bit.

The ring's bookkeeping (``head``, ``size``) is host-side Python ints: no device sync.  Logical index i in [0, size) is
OPB's row i (the i-th oldest retained transition; within one store, env order) and lives in slot
``(head - size + i) mod max_size`` -- ``physical_index`` below, which the CPU tests check against the reference.

One divergence from OPB: a single store of more than ``max_size`` transitions (num_envs > max_size) is refused (OPB
would keep its last ``max_size`` rows).

``ReplayBuffer(env, max_size, cursor=True)`` also keeps ``head``, ``size`` and a draw counter in 32 bytes of device
memory (the CURSOR, include/finenvs_amd_replay_cursor.h): every store mirrors the host's integers into it, and
``draw(B)`` draws a mini-batch's logical indices on the device from it and gathers their descriptors in one launch
(``fe_ring_draw``).  Nothing on that path depends on a host integer, so an update iteration captured as a hipGraph
(finenvs_amd/graphed.py) follows the ring while transitions are stored between its replays."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from .rng import philox_u32

_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)

KEYS = ("states", "actions", "rewards", "next_states", "dones")  # OPB's container order


# ---------------------------------------------------------------- host bookkeeping (no device needed)
def physical_index(indices, head: int, size: int, capacity: int):
    """Ring slot of logical index i (the i-th oldest of the ``size`` retained transitions): (head - size + i) mod C.
    Works on ints, numpy arrays and torch tensors alike."""
    return (indices + (head - size) % capacity) % capacity


def draw_indices(seed: int, first_draw: int, size: int, count: int) -> List[int]:
    """Host mirror of ``fe_ring_draw``'s index rule: draw ``first_draw + b`` of the stream ``seed`` is logical index
    ``(philox_u32(seed, first_draw + b) * size) >> 32`` (``rng.redraw_day``'s multiply-shift), in ``[0, size)``."""
    size, first = int(size), int(first_draw)
    if size < 1:
        raise ValueError(f"cannot draw from {size} transitions")
    return [(philox_u32(seed, first + b) * size) >> 32 for b in range(int(count))]


@dataclass
class ReplayDraw:
    """One mini-batch drawn on the device (``ReplayBuffer.draw``): the B logical ``indices`` (B,) int64 and the
    transitions gathered at them -- ``state_src`` (B,) int64 / ``state_pos`` (B, A) float64, ``next_src`` / ``next_pos``,
    ``actions`` (B, A), ``rewards`` (B,), ``dones`` (B,) float32.  The fused consumers take it where they take
    ``indices``."""

    indices: torch.Tensor
    state_src: torch.Tensor
    state_pos: torch.Tensor
    next_src: torch.Tensor
    next_pos: torch.Tensor
    actions: torch.Tensor
    rewards: torch.Tensor
    dones: torch.Tensor


def as_draw(buffer, indices, who: str) -> Optional[ReplayDraw]:
    """``indices`` if it is a ``ReplayDraw`` (of a ``cursor=True`` buffer: ValueError otherwise, before any device
    work), else None."""
    if not isinstance(indices, ReplayDraw):
        return None
    if getattr(buffer, "cursor", None) is None:
        raise ValueError(f"{who}: a ReplayDraw needs a ReplayBuffer(cursor=True) -- this buffer keeps head and size on "
                         "the host only; pass draw.indices to use the by-value path")
    return indices


class RingIndex:
    """head / size of a ring of ``capacity`` transitions, as OPB's store + discard_old_data (OPB:33-66) move them."""

    def __init__(self, capacity: int):
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError(f"max_size must be >= 1, got {capacity}")
        self.capacity = capacity
        self.head = 0  # slot the next transition goes to
        self.size = 0  # transitions retained

    def check_store(self, count: int) -> None:
        if count > self.capacity:
            raise ValueError(f"one store of {count} transitions does not fit max_size = {self.capacity}: the device "
                             "ring refuses a store larger than its capacity (the reference would keep its last "
                             "max_size rows); use max_size >= num_envs")

    def advance(self, count: int) -> None:
        """``count`` transitions appended (the oldest overwritten once full)."""
        self.head = (self.head + count) % self.capacity
        self.size = min(self.size + count, self.capacity)

    def check_sample(self) -> None:
        if self.size == 0:
            raise ValueError("cannot sample a mini-batch from an empty replay buffer (store transitions first)")

    def physical(self, indices):
        return physical_index(indices, self.head, self.size, self.capacity)

    def clear(self) -> None:
        self.head = self.size = 0


def check_transition(N: int, A: int, device, states, actions, rewards, next_states, dones):
    """Validated, flat views of one env step's transition: (s_src (N,), s_pos (N*A,), n_src, n_pos, actions (N*A,) f32
    or f64, rewards (N,) f64, dones (N,) int32).  Raises ValueError naming what is wrong."""
    device = torch.device(device)

    def descriptor(d, what):
        if isinstance(d, torch.Tensor):
            raise ValueError(f"{what} must be observation descriptors (obs_src (N,) int64, obs_pos (N, A) float64), not a "
                             "rendered observation: step the env with descriptors_out=(obs_src, obs_pos) and store that "
                             "pair (env.describe() gives the state after reset())")
        if not isinstance(d, (tuple, list)) or len(d) != 2:
            raise ValueError(f"{what} must be a pair (obs_src (N,) int64, obs_pos (N, A) float64)")
        src, pos = d
        if not isinstance(src, torch.Tensor) or src.dtype is not torch.int64 or tuple(src.shape) != (N,):
            raise ValueError(f"{what}[0] (obs_src) must be an int64 tensor of shape ({N},), got "
                             f"{getattr(src, 'dtype', type(src))} {tuple(getattr(src, 'shape', ()))}")
        if (not isinstance(pos, torch.Tensor) or pos.dtype is not torch.float64
                or tuple(pos.shape) not in ((N, A),) + (((N,),) if A == 1 else ())):
            raise ValueError(f"{what}[1] (obs_pos) must be a float64 tensor of shape ({N}, {A}), got "
                             f"{getattr(pos, 'dtype', type(pos))} {tuple(getattr(pos, 'shape', ()))}")
        return src, pos

    s_src, s_pos = descriptor(states, "states")
    n_src, n_pos = descriptor(next_states, "next_states")
    if not isinstance(actions, torch.Tensor) or actions.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"actions must be a float32 or float64 tensor, got {getattr(actions, 'dtype', type(actions))}")
    if tuple(actions.shape) not in ((N, A),) + (((N,),) if A == 1 else ()):
        raise ValueError(f"actions must have shape ({N}, {A}), got {tuple(actions.shape)}")
    if not isinstance(rewards, torch.Tensor) or rewards.dtype is not torch.float64 or tuple(rewards.shape) not in ((N,), (N, 1)):
        raise ValueError(f"rewards must be a float64 tensor of shape ({N},) (env.step's), got "
                         f"{getattr(rewards, 'dtype', type(rewards))} {tuple(getattr(rewards, 'shape', ()))}")
    if not isinstance(dones, torch.Tensor) or dones.dtype is not torch.int32 or tuple(dones.shape) not in ((N,), (N, 1)):
        raise ValueError(f"dones must be an int32 tensor of shape ({N},) (env.step's), got "
                         f"{getattr(dones, 'dtype', type(dones))} {tuple(getattr(dones, 'shape', ()))}")
    out = (s_src, s_pos, n_src, n_pos, actions, rewards, dones)
    for t in out:
        if t.device != device:
            raise ValueError(f"every transition field must be on the replay buffer's device {device}, got one on {t.device}")
    return tuple(t.contiguous().reshape(-1) for t in out)


# ---------------------------------------------------------------- the ring
class ReplayBuffer:
    """OPB's ``Buffer`` for a ``TimeSeriesEnv``: ``store`` / ``get_mini_batch`` / ``size`` with the reference's
    signatures; states are descriptor pairs ``(obs_src (N,) int64, obs_pos (N, A) float64)``.

    ``cursor=True``: the ring's ``head`` / ``size`` are mirrored into ``self.cursor`` ((4,) int64 on the device: head,
    size, draws, ticket) by every store (``fe_replay_append_c``) and ``draw`` samples from it; ``seed`` fixes the draw
    stream.  ``self.draws`` is the HOST's mirror of the draw counter, advanced by B per ``draw`` call: a replayed
    graph that contains a draw advances only the device's counter (``self.cursor[2]``)."""

    def __init__(self, env, max_size: int = 1_000_000, cursor: bool = False, seed: int = 0):
        self.env = env
        self.N, self.A, self.W = int(env.num_envs), int(env.num_assets), int(env.num_intervals)
        self._ring = RingIndex(max_size)
        self._ring.check_store(self.N)
        self.device = torch.device(env.device)
        if self.device.type != "cuda":
            raise RuntimeError("ReplayBuffer lives in HBM: the env must be on a GPU")
        self._lib = _lib.load()
        C_, A, dev = self._ring.capacity, self.A, self.device
        self.state_src = torch.zeros((C_,), dtype=torch.int64, device=dev)
        self.state_pos = torch.zeros((C_, A), dtype=torch.float64, device=dev)
        self.next_src = torch.zeros((C_,), dtype=torch.int64, device=dev)
        self.next_pos = torch.zeros((C_, A), dtype=torch.float64, device=dev)
        self.actions = torch.zeros((C_, A), dtype=torch.float32, device=dev)
        self.rewards = torch.zeros((C_,), dtype=torch.float32, device=dev)
        self.dones = torch.zeros((C_,), dtype=torch.float32, device=dev)
        self.errors = torch.zeros((1,), dtype=torch.int64, device=dev)  # out-of-range sample indices (fe_replay_sample)
        self._desc = _lib.FeReplayRing(
            C_, A, 0, self.state_src.data_ptr(), self.state_pos.data_ptr(), self.next_src.data_ptr(),
            self.next_pos.data_ptr(), self.actions.data_ptr(), self.rewards.data_ptr(), self.dones.data_ptr(),
            self.errors.data_ptr())
        self.cursor = torch.zeros((_lib.CURSOR_WORDS,), dtype=torch.int64, device=dev) if cursor else None
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.draws = 0

    # ---------------------------------------------------------------- bookkeeping
    @property
    def max_size(self) -> int:
        return self._ring.capacity

    @property
    def head(self) -> int:
        return self._ring.head

    def size(self) -> int:
        return self._ring.size

    def __len__(self) -> int:
        return self._ring.size

    def clear(self) -> None:
        self._ring.clear()
        if self.cursor is not None:  # head and size; the draw counter goes on
            self.cursor[:_lib.CURSOR_DRAWS].zero_()

    def physical(self, indices):
        """Ring slots of logical indices (see ``physical_index``)."""
        return self._ring.physical(indices)

    def _stream(self) -> int:
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        if _raw_stream is not None:
            return _raw_stream(idx)
        return torch.cuda.current_stream(self.device).cuda_stream

    # ---------------------------------------------------------------- store (OPB:33-66)
    def store(self, states: Tuple[torch.Tensor, torch.Tensor], actions: torch.Tensor, rewards: torch.Tensor,
              next_states: Tuple[torch.Tensor, torch.Tensor], dones: torch.Tensor) -> None:
        """One env step of all N envs (the eval env included, as TD3_agent.py:147-169 stores them), appended in env
        order.  ``states`` / ``next_states``: descriptor pairs; ``actions`` (N, A) f32 / f64 (stored as f32),
        ``rewards`` (N,) f64 and ``dones`` (N,) int32 as ``env.step`` returns them.  No host sync."""
        s_src, s_pos, n_src, n_pos, act, rew, done = check_transition(self.N, self.A, self.device, states, actions,
                                                                       rewards, next_states, dones)
        self._append(1, self.N, self.N, 0, self.N, s_src, s_pos, n_src, n_pos, act, rew, done)

    def extend(self, traj) -> None:
        """Append the filled steps of a ``TrajectoryBuffer(states=True)`` chunk -- the same transitions, in the same order,
        as one ``store`` per step (state = descriptor row t, next state = row t + 1) -- in one launch.  A chunk larger
        than the ring keeps its newest ``max_size`` transitions, as that many stores would."""
        if not getattr(traj, "has_states", False):
            raise ValueError("extend() needs a TrajectoryBuffer(states=True): the states are its descriptor rows")
        if traj.N != self.N or traj.A != self.A:
            raise ValueError(f"the trajectory holds {traj.N} envs x {traj.A} assets, this buffer's env {self.N} x {self.A}")
        if traj.obs_src.device != self.device:
            raise ValueError(f"the trajectory lives on {traj.obs_src.device}, this buffer on {self.device}")
        T = len(traj)
        if T == 0:
            return
        if not traj._begun:
            raise RuntimeError("the trajectory's state row 0 is not set (TrajectoryBuffer.begin)")
        total = T * self.N
        count = min(total, self.max_size)
        src, pos = traj.obs_src, traj.obs_pos  # (T + 1, N) / (T + 1, N, A) views, rows strided by the chunk's capacity
        self._append(T, self.N, traj.C, total - count, count, src[0], pos[0], src[1], pos[1], traj.actions[0],
                     traj.rewards[0], traj.dones[0])

    def _append(self, steps, N, ld, first, count, s_src, s_pos, n_src, n_pos, act, rew, done) -> None:
        # transitions before `first` would have been overwritten: the kept ones go to the slots they would occupy
        head = (self.head + first) % self.max_size
        args = (C.byref(self._desc), head, steps, N, ld, first, count, s_src.data_ptr(), s_pos.data_ptr(),
                n_src.data_ptr(), n_pos.data_ptr(), act.data_ptr(), int(act.dtype is torch.float64), rew.data_ptr(),
                done.data_ptr())
        if self.cursor is None:
            _lib.check(self._lib.fe_replay_append(*args, self._stream()), self._lib)
        else:  # the same launch leaves the new head and size in the cursor
            new_size = min(self.size() + first + count, self.max_size)
            _lib.check(self._lib.fe_replay_append_c(*args, self.cursor.data_ptr(), new_size, self._stream()), self._lib)
        self._ring.advance(first + count)

    # ---------------------------------------------------------------- the draw on the device
    def new_draw(self, size: int) -> ReplayDraw:
        """Uninitialised tensors of a ``size``-transition draw, for ``draw(size, out=)``: nothing is launched."""
        B, A, dev = int(size), self.A, self.device
        if B < 0:
            raise ValueError(f"cannot draw {B} transitions")
        return ReplayDraw(torch.empty((B,), dtype=torch.int64, device=dev),
                          torch.empty((B,), dtype=torch.int64, device=dev),
                          torch.empty((B, A), dtype=torch.float64, device=dev),
                          torch.empty((B,), dtype=torch.int64, device=dev),
                          torch.empty((B, A), dtype=torch.float64, device=dev),
                          torch.empty((B, A), dtype=torch.float32, device=dev),
                          torch.empty((B,), dtype=torch.float32, device=dev),
                          torch.empty((B,), dtype=torch.float32, device=dev))

    def draw(self, size: int, out: Optional[ReplayDraw] = None) -> ReplayDraw:
        """A mini-batch of ``size`` transitions drawn on the device, in one launch (``fe_ring_draw``): index b is
        ``draw_indices(self.seed, draws, size(), B)[b]`` with ``draws`` the device's counter, which the launch advances
        by B.  ``out``: a previous draw of the same B whose tensors are written again (what a captured graph needs).
        Capturable: nothing here reads ``head`` or ``size()`` on the host except the refusal of an empty ring."""
        if self.cursor is None:
            raise ValueError("draw() needs ReplayBuffer(cursor=True)")
        self._ring.check_sample()
        B, A, dev = int(size), self.A, self.device
        if B < 0:
            raise ValueError(f"cannot draw {B} transitions")
        if out is None:
            out = self.new_draw(B)
        elif not isinstance(out, ReplayDraw) or tuple(out.indices.shape) != (B,) or out.indices.device != dev:
            raise ValueError(f"out must be a ReplayDraw of {B} transitions on {dev}")
        _lib.check(self._lib.fe_ring_draw(
            C.byref(self._desc), self.cursor.data_ptr(), self.seed, B, out.indices.data_ptr(), out.state_src.data_ptr(),
            out.state_pos.data_ptr(), out.next_src.data_ptr(), out.next_pos.data_ptr(), out.actions.data_ptr(),
            out.rewards.data_ptr(), out.dones.data_ptr(), self._stream()), self._lib)
        self.draws += B
        return out

    # ---------------------------------------------------------------- sampling (OPB:68-77)
    def get_mini_batch(self, size: int, indices: Optional[torch.Tensor] = None, check: bool = False
                       ) -> Dict[str, torch.Tensor]:
        """OPB's mini-batch: {"states" (B, W, 5A), "actions" (B, A), "rewards" (B, 1), "next_states" (B, W, 5A),
        "dones" (B, 1)}, all float32, in one launch.  ``indices`` (B,) logical indices; by default the very draw OPB:69
        makes, ``torch.randint(0, self.size(), (size,), device=...)``, so the same torch seed picks the same transitions.
        An index outside [0, size()) yields NaN rows; ``check=True`` then raises (one host sync).  ``indices`` may be
        a ``ReplayDraw`` of this buffer: head and size are then read from the cursor (``fe_replay_sample_c``)."""
        draw = as_draw(self, indices, "get_mini_batch")
        self._ring.check_sample()
        if draw is not None:
            indices = draw.indices
        if indices is None:
            indices = torch.randint(0, self.size(), (int(size),), device=self.device)
        else:
            if not isinstance(indices, torch.Tensor) or indices.dtype.is_floating_point or indices.dtype.is_complex \
                    or indices.dtype is torch.bool:
                raise ValueError("indices must be an integer tensor of logical indices in [0, size())")
            if indices.device != self.device:
                raise ValueError(f"indices must be on the replay buffer's device {self.device}, got {indices.device}")
            indices = indices.reshape(-1).to(torch.int64).contiguous()
        B, A, W, dev = int(indices.numel()), self.A, self.W, self.device
        out = {
            "states": torch.empty((B, W, 5 * A), dtype=torch.float32, device=dev),
            "actions": torch.empty((B, A), dtype=torch.float32, device=dev),
            "rewards": torch.empty((B, 1), dtype=torch.float32, device=dev),
            "next_states": torch.empty((B, W, 5 * A), dtype=torch.float32, device=dev),
            "dones": torch.empty((B, 1), dtype=torch.float32, device=dev),
        }
        if check:
            self.errors.zero_()
        if B:
            outs = (out["states"].data_ptr(), out["next_states"].data_ptr(), out["actions"].data_ptr(),
                    out["rewards"].data_ptr(), out["dones"].data_ptr(), self._stream())
            if draw is None:
                _lib.check(self._lib.fe_replay_sample(
                    self.env._handle, C.byref(self._desc), self.head, self.size(), indices.data_ptr(), B, *outs), self._lib)
            else:
                _lib.check(self._lib.fe_replay_sample_c(
                    self.env._handle, C.byref(self._desc), self.cursor.data_ptr(), indices.data_ptr(), B, *outs), self._lib)
        if check:
            bad = int(self.errors.item())
            if bad:
                raise IndexError(f"{bad} of {B} sample indices lie outside [0, {self.size()}): their rows are NaN")
        return out
