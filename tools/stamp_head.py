#!/usr/bin/env python3
"""GPU box: the start-up chain of the SINGLE-asset step kernel at config 2, stamped (diagnostic; needs the TEMPORARY stamp build).

    python tools/stamp_head.py [variant tag, default stamp1]

Needs finenvs_amd/csrc/variants/libfinenvs_amd.<tag>.so: the product source with profiles/launch_head/head_stamps.patch applied,
compiled with -DFE_STAMP=1 (the patch says how).  Thread 0 of every workgroup writes s_memrealtime stamps (100 MHz: 10 ns steps,
so single values are coarse and the medians over 1 024 workgroups x 30 launches are what to read) into 8 words of its own:
[0] entry, [1] index loads back (the bar gather has just been issued), [2] bar gather + NaN probe back, [3] first tile accounted
(LDS published, barrier passed), [4] first observation store of the workgroup about to be issued, [5] workgroup done, [6] XCC id.
Back-to-back launches use one stamp buffer each.  Two forms: FORM 2 through fe_env_step_traj_notify (what bench.py's headline
launches) and FORM 0 through fe_env_step_traj."""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import finenvs_amd  # noqa: E402
from bench import CONFIGS, make_series  # noqa: E402
from finenvs_amd import _lib  # noqa: E402

TICK_US = 0.01
tag = sys.argv[1] if len(sys.argv) > 1 else "stamp1"
native = _lib.load(os.path.join(os.path.dirname(_lib.LIB_PATH), "variants", f"libfinenvs_amd.{tag}.so"))
_, N, A, W = CONFIGS[2]
prices, day_id, _ = make_series(A)
env = finenvs_amd.TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=W, num_envs=N, redraw="torch", seed=1, obs_buffers=2, _native=native)
grid = env.launch_info()["grid"]
g = torch.Generator(device="cuda:0").manual_seed(7)
acts = [(torch.rand((N, A), generator=g, device="cuda:0") * 2 - 1).float() for _ in range(8)]
rew = torch.empty((N,), dtype=torch.float64, device="cuda:0")
done = torch.empty((N,), dtype=torch.int32, device="cuda:0")
act = torch.empty((N, A), dtype=torch.float32, device="cuda:0")
lib, h, hv, st = env._lib, env._handle, env._handle_v, torch.cuda.current_stream().cuda_stream
obs = [t.data_ptr() for t in env._obs_ring]
K, SKIP = 40, 10
seq = 0


def med(x):
    return f"median {np.median(x):5.2f}  p10 {np.percentile(x, 10):5.2f}  p90 {np.percentile(x, 90):5.2f}"


for form in ("FORM 2 (fe_env_step_traj_notify: the headline)", "FORM 0 (fe_env_step_traj)"):
    stamps = [torch.zeros((grid, 8), dtype=torch.int64, device="cuda:0") for _ in range(K)]
    _lib.check(lib.fe_env_bind_stats(h, None, None, None))
    for i in range(400):  # settle, unstamped
        seq += 1
        if form.startswith("FORM 2"):
            lib.fe_env_step_traj_notify(hv, acts[i % 8].data_ptr(), obs[i % 2], rew.data_ptr(), done.data_ptr(), act.data_ptr(), None, None, env._flag, seq, st)
        else:
            lib.fe_env_step_traj(hv, acts[i % 8].data_ptr(), obs[i % 2], rew.data_ptr(), done.data_ptr(), act.data_ptr(), None, None, st)
    for i in range(K):
        _lib.check(lib.fe_env_bind_stats(h, None, None, C.c_void_p(stamps[i].data_ptr())))
        seq += 1
        if form.startswith("FORM 2"):
            _lib.check(lib.fe_env_step_traj_notify(hv, acts[i % 8].data_ptr(), obs[i % 2], rew.data_ptr(), done.data_ptr(), act.data_ptr(), None, None,
                                                   env._flag, seq, st))
        else:
            _lib.check(lib.fe_env_step_traj(hv, acts[i % 8].data_ptr(), obs[i % 2], rew.data_ptr(), done.data_ptr(), act.data_ptr(), None, None, st))
    torch.cuda.synchronize()
    _lib.check(lib.fe_env_bind_stats(h, None, None, None))
    S = [s.cpu().numpy().astype(np.int64) for s in stamps]
    stages = {k: [] for k in ("entry -> index loads back", "index loads back -> bar gather back", "bar gather back -> accounted",
                              "accounted -> first store issued", "entry -> first store issued")}
    gaps, spans, first_store_launch = [], [], []
    for i in range(SKIP, K):
        s = S[i]
        stages["entry -> index loads back"].append((s[:, 1] - s[:, 0]) * TICK_US)
        stages["index loads back -> bar gather back"].append((s[:, 2] - s[:, 1]) * TICK_US)
        stages["bar gather back -> accounted"].append((s[:, 3] - s[:, 2]) * TICK_US)
        stages["accounted -> first store issued"].append((s[:, 4] - s[:, 3]) * TICK_US)
        stages["entry -> first store issued"].append((s[:, 4] - s[:, 0]) * TICK_US)
        gaps.append((s[:, 0].min() - S[i - 1][:, 5].max()) * TICK_US)
        spans.append((s[:, 5].max() - s[:, 0].min()) * TICK_US)
        first_store_launch.append((s[:, 4].min() - s[:, 0].min()) * TICK_US)
    print(f"\n## {form}, config 2, grid {grid}, launches {SKIP}..{K - 1} of a back-to-back train (us)")
    for k, v in stages.items():
        print(f"  {k:38s} per workgroup: {med(np.concatenate(v))}")
    print(f"  previous launch's last workgroup out -> this launch's first in: median {np.median(gaps):5.2f}")
    print(f"  this launch's first in -> its FIRST store issued by any workgroup: median {np.median(first_store_launch):5.2f}")
    print(f"  this launch's first in -> last out: median {np.median(spans):5.2f}")
