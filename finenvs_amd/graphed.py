"""One fused update iteration -- draw, targets, both backward passes, optimizer steps -- as ONE hipGraph launch.

At the reference's batch sizes (B = 100 / 256) a fused SAC or TD3 update is host-bound: its ~160 launches are each a
few microseconds of device work.  ``GraphedUpdate`` captures one call of an update function into a
``torch.cuda.CUDAGraph`` (a hipGraph on ROCm); ``replay()`` runs it with one launch call.

What makes the update capturable is that nothing in it depends on a host integer that changes between replays:

* the front ends are built with ``weights=FusedAdam`` (finenvs_amd/optim.py): nothing is packed or copied to the host
  per call, gradients and moments live at fixed addresses, and the step counters are device memory;
* the replay buffer is a ``ReplayBuffer(cursor=True)`` sampled through ``buffer.draw(B, out=draw)`` with ``draw`` the
  tensors of an earlier draw: the ring's head, size and draw counter are read from device memory when the graph runs
  (include/finenvs_amd_replay_cursor.h), and the consumers take the ``ReplayDraw`` where they take indices;
* standard normals come from ``torch.randn`` inside ``fn`` (torch's generator is graph-aware) or from static tensors
  that the caller refills between replays;
* ``fn`` calls no ``.item()`` and nothing else that waits for the device, and allocates only through torch.

Stores into the buffer (``store`` / ``extend``) happen OUTSIDE the graph, between replays: they mirror the new head and
size into the cursor, and the next replay samples from the ring as it then stands.  That is the point of the cursor.
The host's ``buffer.draws`` is advanced by ``draw`` calls only, so a replay advances the device's counter alone.
"""
from __future__ import annotations

from typing import Callable, Optional

import torch


class GraphedUpdate:
    """``fn`` captured once and replayed.

    ``fn()`` runs ``warmup`` times on a side stream first, as ``torch.cuda.graph`` requires (allocator and lazy
    initialisation, ``FusedAdam``'s segment table, the gradients' addresses).  These are REAL updates: parameters,
    moments, targets and the draw counter move ``warmup`` times before the first ``replay()``.  ``between``, if given,
    is called after each warm-up call (the stores and noise refills a training loop does between its updates).  The
    capture itself executes nothing.

    ``replay()`` launches the graph and returns what ``fn`` returned at capture: tensors that every replay overwrites
    (clone what must outlive the next one)."""

    def __init__(self, fn: Callable[[], object], warmup: int = 3, between: Optional[Callable[[], None]] = None,
                 device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("GraphedUpdate captures a GPU graph: no GPU is visible")
        if int(warmup) < 1:
            raise ValueError("warmup must be >= 1: a capture without a warmed-up allocator and optimizer table fails")
        self.fn = fn
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            for _ in range(int(warmup)):
                fn()
                if between is not None:
                    between()
        torch.cuda.current_stream(dev).wait_stream(s)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        # thread-local capture mode, as GraphedRollout: only this thread's calls are held to the capture rules, so a
        # process group's watchdog thread polling its events during the capture does not abort the process
        with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            self.outputs = fn()
        self.replays = 0

    def replay(self):
        """One captured iteration; returns ``fn``'s outputs (static tensors)."""
        self.graph.replay()
        self.replays += 1
        return self.outputs
