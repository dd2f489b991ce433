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


_PHILOX_M0, _PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_U32 = np.uint64(0xFFFFFFFF)
_SHIFT32 = np.uint64(32)
EVO_DOMAIN_Z, EVO_DOMAIN_ACT = 0x45565A00, 0x45564100  # word c3 of the two counters (include/finenvs_amd_evo.h)


def philox4x32_10(key, c0, c1, c2, c3):
    """Philox4x32-10 (Salmon et al., SC'11; the Random123 recurrence), all four output words, vectorised: the counter
    words broadcast against each other, the result is four uint32 arrays of the broadcast shape.  ``key`` is the pair
    ``(k0, k1)`` or one integer below 2^64 whose low half is ``k0`` (how the library keys its streams with a seed)."""
    if isinstance(key, (tuple, list)):
        k0, k1 = (int(k) & 0xFFFFFFFF for k in key)
    else:
        k0, k1 = int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF
    c = [np.asarray(x).astype(np.uint64) & _U32 for x in np.broadcast_arrays(c0, c1, c2, c3)]
    for _ in range(10):
        p0, p1 = _PHILOX_M0 * c[0], _PHILOX_M1 * c[2]  # 32 x 32 bits: below 2^64
        c = [(p1 >> _SHIFT32) ^ c[1] ^ np.uint64(k0), p1 & _U32, (p0 >> _SHIFT32) ^ c[3] ^ np.uint64(k1), p0 & _U32]
        k0, k1 = (k0 + _PHILOX_W0) & 0xFFFFFFFF, (k1 + _PHILOX_W1) & 0xFFFFFFFF
    return tuple(x.astype(np.uint32) for x in c)


def box_muller_radius(w):
    """``(u, r)`` of a uint32 word in f64: ``u = ((w >> 8) + 1) / 2^24`` in (0, 1], ``r = sqrt(-2 ln u)``."""
    u = ((np.asarray(w).astype(np.uint64) >> np.uint64(8)).astype(np.float64) + 1.0) / 2.0 ** 24
    return u, np.sqrt(-2.0 * np.log(u))


def box_muller4(w0, w1, w2, w3):
    """The Box-Muller transform of include/finenvs_amd_evo.h on four Philox words, evaluated in f64: the radius from the
    top 24 bits of ``w0`` (``w2``), the angle ``(w1 >> 8) / 2^24`` (``w3``) in revolutions; normals 0 and 1 are
    ``r0 cos``, ``r0 sin``, normals 2 and 3 the same from ``(w2, w3)``.  Returns an array with a last axis of 4."""
    out = []
    for wu, wt in ((w0, w1), (w2, w3)):
        _, r = box_muller_radius(wu)
        t = (np.asarray(wt).astype(np.uint64) >> np.uint64(8)).astype(np.float64) / 2.0 ** 24
        out += [r * np.cos(2.0 * np.pi * t), r * np.sin(2.0 * np.pi * t)]
    return np.stack(out, axis=-1)


def evo_z_reference(seed, g, pairs, P):
    """``z_{g,p,j}`` of include/finenvs_amd_evo.h for ``p`` in ``pairs`` and ``j < P``, ``(len(pairs), P)`` f64: word
    ``j % 4`` of the transform of Philox(key = seed, counter = (j / 4, p, g, 0x45565a00)).  Written from the header's
    text; the device code is not consulted."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1)
    q = np.arange((int(P) + 3) // 4, dtype=np.int64)
    z = box_muller4(*philox4x32_10(seed, q[None, :], pairs[:, None], int(g), EVO_DOMAIN_Z))
    return z.reshape(pairs.size, -1)[:, :int(P)]


def evo_action_noise_reference(seed, g, step, n, a):
    """The action noise ``xi`` of env ``n``, asset ``a`` at step ``step`` of generation ``g`` (the four broadcast), f64: word
    ``a % 4`` of the transform of Philox(key = seed, counter = (n, step, g, 0x45564100 | a / 4))."""
    step, n, a = np.broadcast_arrays(np.asarray(step, dtype=np.int64), np.asarray(n, dtype=np.int64),
                                     np.asarray(a, dtype=np.int64))
    z = box_muller4(*philox4x32_10(seed, n, step, int(g), EVO_DOMAIN_ACT | (a // 4)))
    return np.take_along_axis(z, (a % 4)[..., None], axis=-1)[..., 0]


PPO_PERM_SALT = 0x50504F5045524D31  # FE_PPO_PERM_SALT of include/finenvs_amd_ppo.h (pinned by tests/test_ppo_update_host.py)
PHILOX_U32_DOMAIN = 0x46454E56      # word c2 of the project's one-word generator (pinned by tests/test_evo_streams_host.py)


def ppo_permute_reference(seed, epoch, n, positions):
    """``pi_epoch`` of include/finenvs_amd_ppo.h on a whole array of positions, written from the header's text on
    ``philox4x32_10``; neither ``rng.ppo_permute`` nor the device code is consulted.  One pass of the four-round Feistel
    network over all positions, then again over those whose value is still ``>= n`` only, until none is left.  Returns
    ``(samples int64 of positions' shape, passes)``, ``passes`` the number of passes the longest walk took."""
    n, m64 = int(n), (1 << 64) - 1
    x = np.array(positions, dtype=np.int64)
    if not 1 <= n < 1 << 32 or x.size == 0 or int(x.min()) < 0 or int(x.max()) >= n:
        raise ValueError(f"need 1 <= n < 2**32 and positions in [0, n) (got n = {n})")
    shape, x = x.shape, x.reshape(-1).astype(np.uint64)
    hb = (max(1, (n - 1).bit_length()) + 1) // 2
    shift, mask = np.uint64(hb), np.uint64((1 << hb) - 1)
    key = (int(seed) ^ PPO_PERM_SALT) & m64
    rounds = [(((int(epoch) * 4 + r) & m64) << 16) & m64 for r in range(4)]  # 64-bit arithmetic, as the device's
    walking, passes = np.arange(x.size), 0
    while walking.size:
        if passes >= 1 << (2 * hb):
            raise AssertionError("a walk longer than the domain: the pass is no bijection")
        passes += 1
        left, right = x[walking] >> shift, x[walking] & mask
        for base in rounds:  # right < 2^16 and base's low 16 bits are clear: the counter's low word is (base | right) & 2^32 - 1
            low = np.uint64(base & 0xFFFFFFFF) | right
            word = philox4x32_10(key, low, base >> 32, PHILOX_U32_DOMAIN, 0)[0].astype(np.uint64)
            left, right = right, left ^ (word & mask)
        x[walking] = (left << shift) | right
        walking = walking[x[walking] >= np.uint64(n)]
    return x.astype(np.int64).reshape(shape), passes


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


# ----------------------------------------------------------------------------------------------- saturated ("hot") modules
def cpu_states(days, bars, W, seed, src, pos):
    """``env.render(src, pos)`` of the one-asset env the gradient suites build (``synthetic_series(days, 1, bars, seed, 0)``)
    without a GPU: ``(B, W, 5)`` f64 on the CPU, rows ``src / 4 + j`` of the oracle's log-return table and the position in
    column 4.  Also returns the table's ``(D, L)``."""
    import torch

    from finenvs_amd.data import synthetic
    from oracle import fe_oracle

    fe_oracle.build()
    prices, day_id, _ = synthetic.synthetic_series(days, 1, bars, seed, 0.0)
    _, LR, *_ = fe_oracle.tables_from_series(prices, day_id, W)
    D, L, _ = LR.shape
    table = torch.from_numpy(np.ascontiguousarray(LR, dtype=np.float64)).reshape(D * L, 4)
    rows = (src.cpu().reshape(-1, 1) // 4) + torch.arange(W).reshape(1, W)
    states = torch.cat([table[rows], pos.cpu().double().reshape(-1, 1, 1).expand(-1, W, 1)], dim=2)
    assert not bool(torch.isnan(states).any())
    return states, (D, L)


class modules_on_cpu:
    """Inside the block ``nn.Module.cuda()`` returns the module as it is, so that the GPU suites' own module builders
    (``_module``, ``_critic``, ``_actor``: they draw on the CPU and end in ``.cuda()``) can be called without a GPU.  For
    the CPU tests of conditions on those builders; nothing inside may launch a kernel."""

    def __enter__(self):
        import torch

        self._cuda = torch.nn.Module.cuda
        torch.nn.Module.cuda = lambda module, device=None: module

    def __exit__(self, *exc):
        import torch

        torch.nn.Module.cuda = self._cuda


def heat(module, gate_scale, out_scale):
    """Make a family's module "hot", in place: the recurrent layer of an LSTM module (``weight_ih``, ``weight_hh``, both
    biases) or the first layer and its bias of an MLP module (``network``) times ``gate_scale``; the layer that feeds the
    output (``last_layer[0]`` of the LSTM head and critic, ``mu_layer`` of the SAC actor, the last ``Linear`` of an MLP)
    times ``out_scale``.  Returns the module."""
    import torch

    with torch.no_grad():
        if hasattr(module, "lstm"):
            for name in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
                getattr(module.lstm, name).mul_(gate_scale)
            out = module.mu_layer if hasattr(module, "mu_layer") else module.last_layer[0]
        else:
            linear = [m for m in module.network if isinstance(m, torch.nn.Linear)]
            linear[0].weight.mul_(gate_scale)
            linear[0].bias.mul_(gate_scale)
            out = linear[-1]
        out.weight.mul_(out_scale)
        out.bias.mul_(out_scale)
    return module


def hot_preactivations(module, states, actions=None, eps=None):
    """``(z, p)`` of the f64 copy of a family's module on rendered ``states`` (``actions``: the critics' second input;
    ``eps``: the SAC actor's noise): ``z`` every gate pre-activation of the LSTM at every step, ``(B, W, 4H)``, or every
    pre-activation of the MLP's first hidden layer, ``(B, H)``; ``p`` the pre-activation of the output ``(B, 1)`` (the
    SAC actor: ``u = mu + eps s``)."""
    import copy

    import torch

    m = copy.deepcopy(module).double()
    x = states.double()
    B = x.shape[0]
    with torch.no_grad():
        if hasattr(m, "lstm"):
            if actions is not None:
                x = torch.cat([x, actions.double().reshape(B, 1, 1).expand(-1, x.shape[1], 1)], dim=2)
            H = m.lstm.hidden_size
            h, c, zs = x.new_zeros((B, H)), x.new_zeros((B, H)), []
            for t in range(x.shape[1]):
                z = x[:, t] @ m.lstm.weight_ih_l0.t() + m.lstm.bias_ih_l0 + h @ m.lstm.weight_hh_l0.t() + m.lstm.bias_hh_l0
                i, f, g, o = z.chunk(4, dim=1)
                c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
                h = torch.sigmoid(o) * torch.tanh(c)
                zs.append(z)
            assert float((h - m.lstm(x)[0][:, -1]).abs().max()) < 1e-9  # the recurrence written out is nn.LSTM's
            z = torch.stack(zs, dim=1)
            if hasattr(m, "mu_layer"):
                hid = m.last_layer(h)
                p = m.mu_layer(hid) + eps.double() * torch.nn.functional.softplus(m.std_layer(hid))
            else:
                p = m.last_layer[0](h)
        else:
            x = x.reshape(B, -1)
            if actions is not None:
                x = torch.cat([x, actions.double().reshape(B, 1)], dim=1)
            z = m.network[0](x)
            p = m.network[:-1](x)
    return z, p


def hot_shares(z, p, lstm, tanh_output):
    """The saturated shares of ``hot_preactivations``' result, asserted against the conditions a hot case rests on
    (conditions on the f64 reference, not measurements); returns them as a dict."""
    def share(mask):
        return float(mask.double().mean())

    s = {"z>17": share(z.abs() > 17), "z>60": share(z.abs() > 60), "z<2": share(z.abs() < 2)}
    assert s["z>17"] >= 0.10 and s["z<2"] >= 0.03, s
    if lstm:
        assert s["z>60"] >= 0.01, s  # the clamp of the exponential's argument
    if tanh_output:
        a = p.abs()
        s.update({"p<2": share(a < 2), "p4-9": share((a > 4) & (a < 9)), "p>9.1": share(a > 9.1)})
        assert s["p<2"] >= 0.20 and s["p4-9"] >= 0.20 and s["p>9.1"] >= 0.05, s
    return s
