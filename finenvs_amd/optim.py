"""The parameter side of a training step in one launch: Adam, the soft update and the packing into kernel layout.

``FusedAdam`` owns, for every network registered with it, the Adam moments, the packed buffers the fused kernels read
(``lstm_pack`` / ``pack_critic_weights`` / ``pack_sac_weights`` / ``lstm_fragment_major`` layout, for the network and for
its target) and a device-resident segment table.  ``step()`` is one launch of ``fe_net_update``
(include/finenvs_amd_optim.h): torch's single-tensor Adam, the reference's soft update ``target = target * (1 - rho) +
p * rho`` (SAC_agent.py:240, TD3_agent.py:263), the packed forms and the zeroing of the gradients, with the step count
kept on the device as the two running products ``b1^t`` and ``b2^t``.  Nothing is copied to the host.  The fused front
ends (``FusedLSTMHead``, ``FusedTwinCritic``, ``FusedSACRollout``) take such an optimizer as ``weights=`` and then read
its packed buffers instead of re-packing their modules at every call.

``reference_update`` restates the element-wise contract in plain torch, one f32 operation per rounding: what the kernel
is tested against bit for bit, on the CPU.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import _lib
from .rollout import lstm_row_order

# enum of include/finenvs_amd_optim.h
SEG_PLAIN, SEG_COPY, SEG_WHH, SEG_WHH_FRAGMENT, SEG_WL, SEG_WIH, SEG_BIAS_PAIR = range(7)
MODE_STEP, MODE_PACK, MODE_ZERO_GRAD = range(3)
BLOCK_ELEMS = 1024  # FE_OPTIM_BLOCK_ELEMS


def _f32(x: float) -> torch.Tensor:
    """A Python float rounded to f32 once, as a 0-dim tensor (so that an operation with it stays one f32 operation)."""
    return torch.tensor(float(x), dtype=torch.float32)


def initial_state() -> Dict[str, float]:
    """The step state before the first step: ``b1^0 = b2^0 = 1`` and ``step = 0``."""
    return {"beta1_pow": 1.0, "beta2_pow": 1.0, "step": 0}


def reference_update(params: Sequence[torch.Tensor], grads: Sequence[torch.Tensor], exp_avgs: Sequence[torch.Tensor],
                     exp_avg_sqs: Sequence[torch.Tensor], state: Dict[str, float], lr: float,
                     betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                     targets: Optional[Sequence[Optional[torch.Tensor]]] = None, rho=0.005, soft_update: bool = True,
                     zero_grad: bool = False) -> Dict[str, float]:
    """One ``FusedAdam.step`` in plain torch, in place on f32 tensors of any device (the CPU in the tests):

        m += (1 - b1) * (g - m);  v = v * b2 + ((1 - b2) * g) * g;  denom = sqrt(v) / bc2s + eps
        p += (-step_size) * (m / denom);  target = target * (1 - rho) + p * rho

    every operation a separate, correctly rounded f32 operation (no ``lerp``, ``addcmul`` or ``addcdiv``, which may fuse
    a multiply-add; the square root through f64), ``step_size = lr / (1 - b1^t)`` and ``bc2s = sqrt(1 - b2^t)`` formed in f64 from the running products
    of ``state`` and rounded to f32 once.  ``targets``: one tensor or None per parameter; ``rho``: one float, or one per
    parameter.  Returns the new state (``state`` itself is not modified)."""
    b1, b2 = float(betas[0]), float(betas[1])
    p1, p2 = state["beta1_pow"] * b1, state["beta2_pow"] * b2
    neg_step_size = -_f32(float(lr) / (1.0 - p1))
    bc2s = _f32(math.sqrt(1.0 - p2))
    omb1, b2f, omb2, epsf = _f32(1.0 - b1), _f32(b2), _f32(1.0 - b2), _f32(eps)
    with torch.no_grad():
        for i, (p, g, m, v) in enumerate(zip(params, grads, exp_avgs, exp_avg_sqs)):
            dev = p.device
            k = lambda t: t.to(dev)  # noqa: E731
            d = g - m
            d = d * k(omb1)
            m.copy_(m + d)
            gg = g * k(omb2)
            gg = gg * g
            v.copy_(v * k(b2f) + gg)
            # the correctly rounded f32 square root, as the kernel takes it: f64 holds more than 2 * 24 + 2 bits, so
            # rounding its square root once more changes nothing (torch's own f32 sqrt is a few in a thousand off by one
            # ulp in some CPU builds, and on the device)
            denom = v.double().sqrt().float() / k(bc2s)
            denom = denom + k(epsf)
            u = m / denom
            u = u * k(neg_step_size)
            p.copy_(p + u)
            t = targets[i] if targets is not None else None
            if soft_update and t is not None:
                r = float(rho[i] if isinstance(rho, (list, tuple)) else rho)
                a = t * k(_f32(1.0 - r))
                b = p * k(_f32(r))
                t.copy_(a + b)
            if zero_grad:
                g.zero_()
    return {"beta1_pow": p1, "beta2_pow": p2, "step": int(state["step"]) + 1}


# ---------------------------------------------------------------- the packed-destination maps (host restatement)
def packed_rows(H: int) -> torch.Tensor:
    """Packed row R of every torch row r = gate * H + unit: the inverse permutation of ``lstm_row_order``."""
    order = lstm_row_order(H)
    inv = torch.empty_like(order)
    inv[order] = torch.arange(4 * H)
    return inv


def fragment_index(R: torch.Tensor, c: torch.Tensor, cols: int) -> torch.Tensor:
    """[row tile][k group][k half][row & 31][4] of a (rows, cols) matrix (``lstm_fragment_major``, the actor's ``wl``)."""
    return (((R // 32) * (cols // 8) + c // 8) * 2 + (c % 8) // 4) * 128 + (R % 32) * 4 + c % 4


def packed_destinations(kind: int, H: int, cols: int, numel: int) -> Optional[torch.Tensor]:
    """Where the ``numel`` elements of a segment go in the flat packed buffer (int64, CPU): the map ``fe_net_update``
    computes per element.  None for ``SEG_PLAIN``.  For ``SEG_BIAS_PAIR`` the destination of the sum ``b_ih + b_hh``
    (slot 5 of the row); its zero slots are ``bias_pair_zero_destinations``."""
    e = torch.arange(numel)
    if kind == SEG_PLAIN:
        return None
    if kind == SEG_COPY:
        return e
    if kind == SEG_WL:
        return fragment_index(e // H, e % H, H)
    inv = packed_rows(H)
    if kind == SEG_WHH:
        return inv[e // H] * H + e % H
    if kind == SEG_WHH_FRAGMENT:
        return fragment_index(inv[e // H], e % H, H)
    if kind == SEG_WIH:
        c = e % cols
        return inv[e // cols] * 8 + torch.where(c < 5, c, torch.full_like(c, 6))
    if kind == SEG_BIAS_PAIR:
        return inv[e] * 8 + 5
    raise ValueError(f"unknown segment kind {kind}")


def bias_pair_zero_destinations(H: int, cols: int) -> torch.Tensor:
    """The slots of ``wx`` the bias-pair segment writes as zero: slot 7 of every row and, without an action column
    (``cols == 5``), slot 6."""
    rows = torch.arange(4 * H) * 8
    return torch.cat([rows + 7] + ([rows + 6] if cols == 5 else []))


class _Segment:
    """One row of the segment table: a parameter tensor (or the bias pair) and where it goes."""

    def __init__(self, name: str, kind: int, param, param2=None, dest: Optional[str] = None, H: int = 0, cols: int = 0):
        self.name, self.kind, self.param, self.param2, self.dest, self.H, self.cols = name, kind, param, param2, dest, H, cols
        self.target = self.target2 = None
        self.rho = 0.0

    @property
    def numel(self) -> int:
        return int(self.param.numel())


def network_kind(module: nn.Module) -> Tuple[str, int]:
    """("head" | "critic" | "actor", H) of a module ``FusedAdam.add`` takes: what ``check_head``,
    ``check_critic`` or ``check_actor`` (each with H up to 1024) accept; ValueError otherwise."""
    from .critic import check_critic
    from .lstm_head import check_head
    from .sac import check_actor

    lstm = getattr(module, "lstm", None)
    if not isinstance(lstm, nn.LSTM):
        raise ValueError("FusedAdam.add needs a module with an nn.LSTM `lstm` (an LSTM head, a critic or a SAC actor); "
                         "use add_tensor for a plain tensor")
    if hasattr(module, "mu_layer") and hasattr(module, "std_layer"):
        return "actor", check_actor(module, streamed=True)
    if lstm.input_size == 6:
        return "critic", check_critic(module, streamed=True)
    return "head", check_head(module, streamed=True)[0]


def network_segments(module: nn.Module) -> Tuple[str, int, List[_Segment], Dict[str, Tuple[int, ...]]]:
    """(kind, H, segments, packed shapes) of a network: its parameter tensors in ``head_parameters`` /
    ``critic_parameters`` / ``actor_parameters`` order, ``b_ih`` and ``b_hh`` as one segment."""
    kind, H = network_kind(module)
    lstm, last = module.lstm, module.last_layer[0]
    cols = 6 if kind == "critic" else 5
    segs = [
        _Segment("w_ih", SEG_WIH, lstm.weight_ih_l0, dest="wx", H=H, cols=cols),
        _Segment("w_hh", SEG_WHH_FRAGMENT if H > 128 else SEG_WHH, lstm.weight_hh_l0, dest="whh", H=H, cols=H),
        _Segment("b_ih+b_hh", SEG_BIAS_PAIR, lstm.bias_ih_l0, lstm.bias_hh_l0, dest="wx", H=H, cols=cols),
    ]
    shapes: Dict[str, Tuple[int, ...]] = {"whh": (4 * H, H), "wx": (4 * H, 8)}
    if kind == "actor":
        mu, std = module.mu_layer, module.std_layer
        segs += [_Segment("w_l", SEG_WL, last.weight, dest="wl", H=H, cols=H), _Segment("b_l", SEG_COPY, last.bias, dest="bl"),
                 _Segment("w_mu", SEG_COPY, mu.weight, dest="wmu"), _Segment("b_mu", SEG_COPY, mu.bias, dest="bmu"),
                 _Segment("w_std", SEG_COPY, std.weight, dest="wstd"), _Segment("b_std", SEG_COPY, std.bias, dest="bstd")]
        shapes.update(wl=(H, H), bl=(H,), wmu=(H,), bmu=(1,), wstd=(H,), bstd=(1,))
    else:
        segs += [_Segment("w_out", SEG_COPY, last.weight, dest="wout"), _Segment("b_out", SEG_COPY, last.bias, dest="bout")]
        shapes.update(wout=(H,), bout=(1,))
    return kind, H, segs, shapes


def scatter_packed(module: nn.Module) -> Dict[str, torch.Tensor]:
    """The packed buffers of ``module`` formed on the CPU through the destination maps, element by element as
    ``fe_net_update`` forms them.  From NaN-filled buffers, so a destination the maps miss shows."""
    _, H, segs, shapes = network_segments(module)
    out = {k: torch.full((math.prod(s),), float("nan"), dtype=torch.float32) for k, s in shapes.items()}
    for s in segs:
        x = s.param.detach().float().cpu().reshape(-1)
        if s.kind == SEG_BIAS_PAIR:
            x = x + s.param2.detach().float().cpu().reshape(-1)  # one f32 add
            out[s.dest][bias_pair_zero_destinations(H, s.cols)] = 0.0
        out[s.dest][packed_destinations(s.kind, s.H, s.cols, s.numel)] = x
    return {k: out[k].reshape(shapes[k]) for k in shapes}


# ---------------------------------------------------------------- the optimizer
class _Network:
    def __init__(self, module, target, kind, H, segments, shapes, rho):
        self.module, self.target, self.kind, self.H, self.segments, self.shapes, self.rho = module, target, kind, H, segments, shapes, rho
        self.packed: Dict[str, torch.Tensor] = {}
        self.packed_target: Dict[str, torch.Tensor] = {}


class FusedAdam:
    """``torch.optim.Adam(lr, betas, eps)`` (no weight decay, no amsgrad) for the fused front ends' networks, with the
    soft update of their targets and their packing into kernel layout, one launch per ``step()``.

        opt = FusedAdam(lr=3e-4)
        opt.add(critic_1, target=target_1, rho=0.005); opt.add(critic_2, target=target_2, rho=0.005)
        twin = FusedTwinCritic(env, critic_1, critic_2, weights=opt)
        target_twin = FusedTwinCritic(env, target_1, target_2, weights=opt)
        loss.backward(); opt.step()       # Adam, both soft updates, all four packed forms, gradients zeroed

    Every registered tensor must be float32, contiguous and on one HIP device.  ``add`` packs nothing yet: the first
    ``step`` / ``repack`` / ``packed`` builds the table.  After an in-place edit of a parameter outside ``step`` (a
    ``load_state_dict`` of a module, an initialisation) call ``repack()``."""

    def __init__(self, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8):
        if not lr >= 0.0 or not eps >= 0.0 or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError("FusedAdam needs lr >= 0, eps >= 0 and betas in [0, 1)")
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.networks: List[_Network] = []
        self.plain: List[_Segment] = []
        self._by_module: Dict[int, Tuple[_Network, bool]] = {}
        self._moments: Dict[int, Tuple[torch.Tensor, torch.Tensor]] = {}  # id(param) -> (exp_avg, exp_avg_sq)
        self.state: Optional[torch.Tensor] = None  # fe_optim_state as four f64 words
        self._table = self._table_host = self._pointers = None
        self._device = None
        self._num_blocks = 0
        self._lib = None
        self.version = 0  # counts the launches that rewrote packed buffers (step, repack)

    # ---- registration
    def _empty(self, shape, dtype=torch.float32) -> torch.Tensor:
        """Every buffer the optimizer owns is allocated here (the memory-contract tests place them between guard bands)."""
        return torch.empty(shape, dtype=dtype, device=self._device)

    def _check_tensor(self, p: torch.Tensor, what: str) -> None:
        if not isinstance(p, torch.Tensor) or p.dtype is not torch.float32:
            raise ValueError(f"{what} must be a float32 tensor (got {getattr(p, 'dtype', type(p))})")
        if p.device.type != "cuda":
            raise ValueError(f"{what} must live on the device (got {p.device}): fe_net_update has no host path")
        if self._device is None:
            self._device = p.device
        if p.device != self._device:
            raise ValueError(f"{what} lives on {p.device}, the optimizer's other tensors on {self._device}")
        if not p.is_contiguous():
            raise ValueError(f"{what} must be contiguous")

    def add(self, module: nn.Module, target: Optional[nn.Module] = None, rho: float = 0.005) -> None:
        """Register a network (an LSTM head, a critic or a SAC actor) and, optionally, the target network that follows
        it with ``target = target * (1 - rho) + p * rho`` at every ``step(soft_update=True)``."""
        if id(module) in self._by_module or (target is not None and id(target) in self._by_module):
            raise ValueError("the module is already registered with this optimizer")
        kind, H, segs, shapes = network_segments(module)
        for s in segs:
            for p in (s.param, s.param2):
                if p is not None:
                    self._check_tensor(p, f"{kind} parameter {s.name}")
        if target is not None:
            if target is module:
                raise ValueError("a network cannot be its own target")
            tk, tH, tsegs, _ = network_segments(target)
            if (tk, tH) != (kind, H):
                raise ValueError(f"the target is a {tk} of H = {tH}, the network a {kind} of H = {H}")
            if not 0.0 <= float(rho) <= 1.0:
                raise ValueError("rho must be in [0, 1]")
            for s, ts in zip(segs, tsegs):
                s.target, s.target2, s.rho = ts.param, ts.param2, float(rho)
                for p in (s.target, s.target2):
                    if p is not None:
                        self._check_tensor(p, f"target parameter {s.name}")
        net = _Network(module, target, kind, H, segs, shapes, float(rho))
        self.networks.append(net)
        self._by_module[id(module)] = (net, False)
        if target is not None:
            self._by_module[id(target)] = (net, True)
        self._table = None

    def add_tensor(self, p: torch.Tensor, target: Optional[torch.Tensor] = None, rho: float = 0.005) -> None:
        """Register a plain tensor with no packed form (``log_alpha``, PPO's ``log_standard_deviation``, a parameter of
        a network the fused kernels do not run), optionally with the target tensor that follows it."""
        self._check_tensor(p, "the tensor")
        if any(s.param is p for s in self.plain):
            raise ValueError("the tensor is already registered with this optimizer")
        seg = _Segment("tensor", SEG_PLAIN, p)
        if target is not None:
            self._check_tensor(target, "the target tensor")
            if target is p or tuple(target.shape) != tuple(p.shape):
                raise ValueError("the target must be another tensor of the parameter's shape")
            if not 0.0 <= float(rho) <= 1.0:
                raise ValueError("rho must be in [0, 1]")
            seg.target, seg.rho = target, float(rho)
        self.plain.append(seg)
        self._table = None

    def _segments(self) -> List[Tuple[Optional[_Network], _Segment]]:
        return [(n, s) for n in self.networks for s in n.segments] + [(None, s) for s in self.plain]

    def parameters(self) -> List[torch.Tensor]:
        """Every registered parameter tensor, in table order (``b_ih`` before ``b_hh``)."""
        return [p for _, s in self._segments() for p in (s.param, s.param2) if p is not None]

    def targets(self) -> List[Optional[torch.Tensor]]:
        """The target tensor of every entry of ``parameters()``, or None."""
        return [t for _, s in self._segments() for p, t in ((s.param, s.target), (s.param2, s.target2)) if p is not None]

    def rhos(self) -> List[float]:
        return [s.rho for _, s in self._segments() for p in (s.param, s.param2) if p is not None]

    def moments(self) -> Tuple[List[torch.Tensor], List[torch.Tensor]]:
        """(exp_avg, exp_avg_sq) of every entry of ``parameters()``."""
        self._ensure_table(need_grads=False)
        ms = [self._moments[id(p)] for p in self.parameters()]
        return [m for m, _ in ms], [v for _, v in ms]

    # ---- the device table
    def _ensure_table(self, need_grads: bool) -> None:
        segs = self._segments()
        if not segs:
            raise ValueError("nothing is registered with this optimizer")
        ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
        pointers = tuple(x for _, s in segs for x in (
            ptr(s.param), ptr(s.param2), ptr(s.target), ptr(s.target2),
            ptr(s.param.grad), ptr(None if s.param2 is None else s.param2.grad)))
        if need_grads:
            for _, s in segs:
                for p in (s.param, s.param2):
                    if p is not None and p.grad is None:
                        raise ValueError(f"a registered parameter ({s.name}, shape {tuple(p.shape)}) has no gradient: "
                                         "run backward() first, or zero the gradients with set_to_none=False")
        if self._table is not None and pointers == self._pointers:
            return  # the hot path: the tensors the table was built from (and checked for) are still the ones in use
        for _, s in segs:
            for p in (s.param, s.param2):
                if p is not None and p.grad is not None:
                    self._check_tensor(p.grad, f"the gradient of {s.name}")
        for _, s in segs:  # a module moved or re-created its tensors since add()
            for p, what in ((s.param, "parameter"), (s.param2, "parameter"), (s.target, "target"), (s.target2, "target")):
                if p is not None:
                    self._check_tensor(p, f"{what} {s.name}")
        if self._lib is None:
            self._lib = _lib.load()
        first = self.state is None
        if first:
            self.state = self._empty((4,), torch.float64)
            self.state.copy_(torch.tensor([1.0, 1.0, 0.0, 0.0], dtype=torch.float64), non_blocking=True)
        unpacked = False  # a network whose packed buffers are new: they are filled before anybody reads them
        for net in self.networks:
            if not net.packed:
                unpacked = True
                net.packed = {k: self._empty(shape) for k, shape in net.shapes.items()}
                if net.target is not None:
                    net.packed_target = {k: self._empty(shape) for k, shape in net.shapes.items()}
        rows = (_lib.FeOptimSegment * len(segs))()
        block = 0
        for row, (net, s) in zip(rows, segs):
            mom = []
            for p in (s.param, s.param2):
                if p is not None and id(p) not in self._moments:
                    m, v = self._empty(tuple(p.shape)), self._empty(tuple(p.shape))
                    m.zero_()
                    v.zero_()
                    self._moments[id(p)] = (m, v)
                mom.append(self._moments[id(p)] if p is not None else (None, None))
            row.param, row.grad, row.exp_avg, row.exp_avg_sq, row.target = (
                ptr(s.param), ptr(s.param.grad), ptr(mom[0][0]), ptr(mom[0][1]), ptr(s.target))
            if s.param2 is not None:
                row.param2, row.grad2, row.exp_avg2, row.exp_avg_sq2, row.target2 = (
                    ptr(s.param2), ptr(s.param2.grad), ptr(mom[1][0]), ptr(mom[1][1]), ptr(s.target2))
            if net is not None and s.dest is not None:
                row.packed = net.packed[s.dest].data_ptr()
                row.packed_target = net.packed_target[s.dest].data_ptr() if net.target is not None else 0
            row.numel, row.first_block = s.numel, block
            row.kind, row.H, row.cols = s.kind, s.H, s.cols
            row.one_minus_rho, row.rho = 1.0 - s.rho, s.rho  # ctypes rounds each to f32 once
            block += (s.numel + BLOCK_ELEMS - 1) // BLOCK_ELEMS
        self._num_blocks = block
        host = torch.frombuffer(bytearray(bytes(rows)), dtype=torch.uint8)
        if self._table is None or self._table.numel() != host.numel():
            self._table = self._empty((host.numel(),), torch.uint8)
        # ordered on the stream after every launch that read the old table; the source buffer stays alive in _table_host
        self._table_host = host.pin_memory()
        self._table.copy_(self._table_host, non_blocking=True)
        self._pointers = pointers
        if unpacked:
            self._launch(MODE_PACK)

    def _launch(self, mode: int, soft_update: bool = False, zero_grad: bool = False) -> None:
        b1, b2 = self.betas
        desc = _lib.FeOptimDesc(
            self._table.data_ptr(), self.state.data_ptr(), len(self._segments()), mode, self._num_blocks,
            int(bool(soft_update)), int(bool(zero_grad)), b1, b2, self.lr, 1.0 - b1, b2, 1.0 - b2, self.eps)
        if mode != MODE_ZERO_GRAD:
            self.version += 1
        stream = torch.cuda.current_stream(self._device).cuda_stream
        _lib.check(self._lib.fe_net_update(C.byref(desc), stream), self._lib)

    # ---- the three launches
    def step(self, soft_update: bool = True, zero_grad: bool = True) -> None:
        """Adam on every registered parameter from its ``.grad``; with ``soft_update`` the targets follow; the packed
        forms of what changed are rewritten; with ``zero_grad`` the gradients are zeroed (as
        ``zero_grad(set_to_none=False)``).  One launch, no host synchronisation."""
        self._ensure_table(need_grads=True)
        self._launch(MODE_STEP, soft_update, zero_grad)

    def zero_grad(self) -> None:
        """Zero every registered gradient in place (one launch), as ``zero_grad(set_to_none=False)``: a parameter that
        has no gradient yet is skipped."""
        self._ensure_table(need_grads=False)
        self._launch(MODE_ZERO_GRAD)

    def repack(self) -> None:
        """Rewrite every packed buffer from the modules' and targets' current parameters (one launch).  Moments, step
        state and gradients are left alone."""
        self._ensure_table(need_grads=False)
        self._launch(MODE_PACK)

    # ---- what the front ends read
    def packed(self, module: nn.Module) -> Dict[str, torch.Tensor]:
        """The packed buffers of a registered network or target, as ``pack_critic_weights`` / ``pack_sac_weights`` name
        them (an LSTM head: ``whh``, ``wx``, ``wout``, ``bout``).  The same tensors at every call: ``step`` writes them
        in place.  ValueError if the module is not registered here."""
        entry = self._by_module.get(id(module))
        if entry is None:
            raise ValueError("the module is not registered with this FusedAdam (add it, or add it as a target)")
        net, is_target = entry
        if not net.packed:  # allocated and filled once; step() keeps them current, so a call per forward costs a lookup
            self._ensure_table(need_grads=False)
        return net.packed_target if is_target else net.packed

    def check_version(self, version: int) -> None:
        """RuntimeError if a ``step`` or ``repack`` rewrote the packed buffers since ``version`` was read: a backward
        that recomputes its activations from them would differentiate another network than its forward ran."""
        if version != self.version:
            raise RuntimeError("the FusedAdam's packed weights were rewritten (step() or repack()) between this forward "
                               "and its backward(): run backward() before the optimizer step")

    def step_count(self) -> int:
        """The number of steps taken, read from the device (a copy to the host: for logs and tests, not the hot path)."""
        return 0 if self.state is None else int(self.state[2:3].view(torch.int64).item())

    # ---- resuming
    def state_dict(self) -> Dict[str, object]:
        """Hyper-parameters, the device step state and both moments of every parameter in ``parameters()`` order."""
        exp_avgs, exp_avg_sqs = self.moments()
        return {"lr": self.lr, "betas": self.betas, "eps": self.eps, "state": self.state.detach().clone(),
                "exp_avg": [m.detach().clone() for m in exp_avgs], "exp_avg_sq": [v.detach().clone() for v in exp_avg_sqs]}

    def load_state_dict(self, sd: Dict[str, object]) -> None:
        """Resume from ``state_dict()`` of an optimizer with the same registrations, then ``repack()`` (the modules'
        own ``load_state_dict`` is the caller's; do it first)."""
        exp_avgs, exp_avg_sqs = self.moments()
        if len(sd["exp_avg"]) != len(exp_avgs) or any(tuple(a.shape) != tuple(b.shape) for a, b in zip(sd["exp_avg"], exp_avgs)):
            raise ValueError("the state_dict does not describe this optimizer's registered parameters")
        self.lr, self.betas, self.eps = float(sd["lr"]), (float(sd["betas"][0]), float(sd["betas"][1])), float(sd["eps"])
        with torch.no_grad():
            self.state.copy_(sd["state"])
            self.state[3] = 0.0  # the workgroup ticket is 0 between launches
            for dst, src in zip(exp_avgs + exp_avg_sqs, list(sd["exp_avg"]) + list(sd["exp_avg_sq"])):
                dst.copy_(src)
        self.repack()
