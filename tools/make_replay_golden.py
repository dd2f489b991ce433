#!/usr/bin/env python3
"""Write tests/golden/replay_buffer.npz by RUNNING THE REFERENCE's off-policy buffer (test infrastructure, not the product).

Runs only where a checkout of the reference is available: its Python is imported the way tools/make_evo_golden.py does it
(a scratch copy of its package on sys.path; nothing of it is written here).  The reference's Buffer (on the CPU,
device_id=-1) receives STORES stores of N transitions, max_size = CAPACITY (not a multiple of N, so that partial steps are
retained and the ring wraps mid-step).  Every field carries its transition's id (id = store * N + env, below 2^24):
states = id, actions = id + 0.25, rewards = id + 0.125, next_states = id + 0.5, dones = id.  The fixture holds arrays only:
  sizes     (STORES,) Buffer.size() after each store
  at        (K,) the stores after which the buffer is inspected
  retained  (K, CAPACITY) the ids of the retained transitions in the buffer's row order (-1 past size())
  indices   (K, BATCH) the indices get_mini_batch drew (torch seed 100 + k before each draw)
  states, actions, rewards, next_states, dones   (K, BATCH, ...) what get_mini_batch returned

    python tools/make_replay_golden.py <reference checkout>
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
N, CAPACITY, STORES, BATCH = 48, 1000, 60, 64
AT = (0, 1, 19, 20, 21, 22, 41, 42, 59)  # before the first wrap, at it, and around later ones


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "finenvs")):
        sys.exit("usage: python tools/make_replay_golden.py <reference checkout>")
    from make_evo_golden import setup_reference

    setup_reference(sys.argv[1])
    from finenvs.agents.off_policy_buffer import Buffer

    buf = Buffer(max_size=CAPACITY, device_id=-1)
    sizes, retained, indices = [], [], []
    fields = {k: [] for k in ("states", "actions", "rewards", "next_states", "dones")}
    for s in range(STORES):
        ids = torch.arange(s * N, (s + 1) * N, dtype=torch.int64)
        x = ids.double()
        buf.store(x.reshape(N, 1, 1).expand(N, 1, 2), (x + 0.25).float().reshape(N, 1), x + 0.125,
                  (x + 0.5).reshape(N, 1, 1).expand(N, 1, 2), ids.int())
        sizes.append(buf.size())
        if s in AT:
            row = np.full(CAPACITY, -1, dtype=np.int64)
            row[: buf.size()] = buf.container["states"][:, 0, 0].numpy().astype(np.int64)
            retained.append(row)
            torch.manual_seed(100 + s)
            batch = buf.get_mini_batch(BATCH)
            torch.manual_seed(100 + s)
            indices.append(torch.randint(0, buf.size(), (BATCH,)).numpy())
            for k in fields:
                fields[k].append(batch[k].numpy())
    out = os.path.join(REPO, "tests", "golden", "replay_buffer.npz")
    np.savez_compressed(out, sizes=np.array(sizes, dtype=np.int64), at=np.array(AT, dtype=np.int64),
                        retained=np.stack(retained), indices=np.stack(indices),
                        meta=np.array([N, CAPACITY, STORES, BATCH], dtype=np.int64),
                        **{k: np.stack(v) for k, v in fields.items()})
    print("wrote", out)


if __name__ == "__main__":
    main()
