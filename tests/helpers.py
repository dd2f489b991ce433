"""Shared helpers for the parity tests (test infrastructure)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    with np.load(os.path.join(GOLDEN, name)) as z:
        return {k: z[k] for k in z.files}


def _canon(a):
    """Bytes of an array with every NaN mapped to one canonical NaN: a NaN's sign and payload are
    not part of the contract (x86 and gfx950 generate different default NaNs); everything else,
    including the sign of zero, is."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        a = a.copy()
        a[np.isnan(a)] = np.nan
    return a


def bits_equal(a, b):
    """Bit-for-bit equality (any NaN == any NaN, +0 != -0)."""
    a, b = _canon(a), _canon(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return a.tobytes() == b.tobytes()


def assert_bits(a, b, what=""):
    a, b = _canon(a), _canon(b)
    assert a.shape == b.shape, f"{what}: shape {a.shape} vs {b.shape}"
    assert a.dtype == b.dtype, f"{what}: dtype {a.dtype} vs {b.dtype}"
    if a.tobytes() != b.tobytes():
        ai = a.view(f"u{a.dtype.itemsize}") if a.dtype.kind == "f" else a
        bi = b.view(f"u{b.dtype.itemsize}") if b.dtype.kind == "f" else b
        bad = np.argwhere(ai != bi)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} mismatching elements, first at {i}: {a[i]!r} vs {b[i]!r}")


def crafted_descriptors(D, L, W, B, seed, pos_scale=0.5):
    """``(src int64 (B,), pos float64 (B, 1))`` on the CPU: B observation descriptors of a one-asset log-return table of D
    days x L rows (``row_elems = 4``), drawn without an env -- windows the env's own reset states never hold, and
    positions that are not zero.

    A window is ``(day d, start s)`` with ``0 <= s <= L - W``; ``src = (d * L + s) * 4`` (what ``fe_check_descriptors_kernel``
    admits: the last one ends on the table's last row).  The windows are drawn without replacement while
    ``B <= D * (L - W + 1)``, otherwise as random permutations of all of them one after the other, the first of which is
    complete.  Index 0 holds window ``(0, 0)`` and, when ``B >= 2``, index ``B - 1`` the last valid window
    ``(D - 1, L - W)``: the pair whose descriptor a ragged tile's padding pairs duplicate.  ``pos ~ U(-pos_scale, pos_scale)``
    in float64, as drawn (not rounded to f32); ``pos[1]`` takes the sign ``pos[0]`` does not have, so both signs occur."""
    import torch

    per_day = L - W + 1
    assert D >= 1 and W >= 1 and per_day >= 1 and B >= 1, (D, L, W, B)
    total = D * per_day
    gen = torch.Generator().manual_seed(seed)
    if B == 1:
        ids = torch.zeros((1,), dtype=torch.int64)
    elif B <= total:
        middle = 1 + torch.randperm(total - 2, generator=gen)[:B - 2]
        ids = torch.cat([torch.zeros((1,), dtype=torch.int64), middle, torch.full((1,), total - 1, dtype=torch.int64)])
    else:  # repeats: the first permutation holds every window once, window (0, 0) first
        blocks = [torch.cat([torch.zeros((1,), dtype=torch.int64), 1 + torch.randperm(total - 1, generator=gen)])]
        while sum(b.numel() for b in blocks) < B:
            blocks.append(torch.randperm(total, generator=gen))
        ids = torch.cat(blocks)[:B].clone()
        ids[B - 1] = total - 1
    d, s = ids // per_day, ids % per_day
    src = (d * L + s) * 4
    pos = (torch.rand((B, 1), generator=gen, dtype=torch.float64) * 2 - 1) * pos_scale
    if B >= 2 and float(pos[0, 0]) * float(pos[1, 0]) > 0:
        pos[1, 0] = -pos[1, 0]
    return src, pos


def crafted_descriptors_for(env, B, seed, pos_scale=0.5):
    """``crafted_descriptors`` for a one-asset env's own table (``env.geometry()``), on the env's device, checked once by
    ``env.check_descriptors``."""
    D, L, W, A = (int(x) for x in env.geometry())
    assert A == 1, A
    src, pos = crafted_descriptors(D, L, W, B, seed, pos_scale)
    src, pos = src.to(env._dev), pos.to(env._dev)
    env.check_descriptors(src)
    return src, pos


def econ_kwargs(g):
    return dict(
        max_shares=int(g["max_shares"]),
        starting_balance=float(g["starting_balance"]),
        per_share_commission=float(g["commission"]),
        initial_margin_requirement=float(g["imr"]),
        maintenance_margin_requirement=float(g["mmr"]),
    )
