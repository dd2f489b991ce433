"""CPU: the host mirror of the two ES noise streams (tests/helpers.py), which tests/test_evo_shapes_gpu.py holds the kernels to.

The mirror is written from the text of include/finenvs_amd_evo.h (Philox4x32-10, the two counter layouts, the Box-Muller
transform), not from the device code, so here it is pinned on its own: the Random123 known-answer vectors, the project's
one-word host generator ``finenvs_amd.rng.philox_u32`` as a special case, the edges of the transform, and the layout of the
two streams restated with scalar arithmetic.
"""
import math

import numpy as np

from tests.helpers import (EVO_DOMAIN_ACT, EVO_DOMAIN_Z, box_muller4, box_muller_radius, evo_action_noise_reference,
                           evo_z_reference, philox4x32_10)

F = 0xFFFFFFFF
KNOWN_ANSWERS = [  # Random123's kat_vectors for philox4x32 with 10 rounds: (key, counter, output)
    ((0, 0), (0, 0, 0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((F, F), (F, F, F, F), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0xA4093822, 0x299F31D0), (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def test_philox_reproduces_the_known_answer_vectors():
    for key, counter, want in KNOWN_ANSWERS:
        got = philox4x32_10(key, *counter)
        assert all(w.dtype == np.uint32 for w in got)
        assert tuple(int(w) for w in got) == want, (key, counter, [hex(int(w)) for w in got])
        # the key as one 64-bit integer, low half first
        assert tuple(int(w) for w in philox4x32_10(key[0] | key[1] << 32, *counter)) == want
    # vectorised: the three vectors in one call per key-independent part
    for key, counter, want in KNOWN_ANSWERS:
        c = [np.array([x, x, 0]) for x in counter]
        got = philox4x32_10(key, *c)
        assert [tuple(int(w[i]) for w in got) for i in (0, 1)] == [want, want]


def test_first_word_equals_the_one_word_host_generator():
    from finenvs_amd.rng import philox_u32

    rng = np.random.default_rng(7)
    seeds = rng.integers(0, 2 ** 64, size=1000, dtype=np.uint64)
    counters = rng.integers(0, 2 ** 64, size=1000, dtype=np.uint64)
    for s, c in zip(seeds.tolist(), counters.tolist()):
        assert int(philox4x32_10(s, c & F, c >> 32, 0x46454E56, 0)[0]) == philox_u32(s, c)
    # one seed, the 1 000 counters in one vectorised call
    s = int(seeds[0])
    got = philox4x32_10(s, counters & np.uint64(F), counters >> np.uint64(32), 0x46454E56, 0)[0]
    assert got.tolist() == [philox_u32(s, c) for c in counters.tolist()]


def test_transform_edges():
    u, r = box_muller_radius(np.array([0, 0xFF, 0x100, F - 0xFF, F], dtype=np.uint32))
    assert u.min() > 0 and u.max() == 1.0 and bool(np.isfinite(r).all())
    assert u[0] == u[1] == 2.0 ** -24 and u[2] == 2.0 ** -23  # only the top 24 bits count
    assert abs(r[0] - math.sqrt(48 * math.log(2))) < 1e-14 and abs(r[0] - 5.768) < 1e-3  # the largest radius
    assert r[4] == 0.0 and r[3] == 0.0
    z = box_muller4(0, 0, 0, 1 << 30)  # angle 0 and a quarter revolution
    assert z.shape == (4,)
    assert z[0] == r[0] and z[1] == 0.0 and abs(z[2]) < 1e-15 and abs(z[3] - r[0]) < 1e-14
    z = box_muller4(F, 12345, 1 << 31, 3 << 29)  # u = 1: both normals 0; u = 1/2 + 2^-24 at 3/8 of a revolution
    assert z[0] == 0.0 and z[1] == 0.0
    r2 = math.sqrt(-2 * math.log(0.5 + 2.0 ** -24))
    assert np.allclose(z[2:], [r2 * math.cos(0.75 * math.pi), r2 * math.sin(0.75 * math.pi)], rtol=1e-14, atol=0)


def _scalar_normal(words, m):
    wu, wt = (words[0], words[1]) if m < 2 else (words[2], words[3])
    r = math.sqrt(-2 * math.log(((wu >> 8) + 1) / 2 ** 24))
    t = 2 * math.pi * ((wt >> 8) / 2 ** 24)
    return r * (math.cos(t) if m % 2 == 0 else math.sin(t))


def test_stream_layouts_restated_with_scalars():
    seed, g, P = 0xFEDCBA9876543210, 3, 23  # P is no multiple of 4
    pairs = [5, 0, 2 ** 31 + 1]
    z = evo_z_reference(seed, g, pairs, P)
    assert z.shape == (3, P) and z.dtype == np.float64
    for i, p in enumerate(pairs):
        for j in (0, 1, 2, 3, 4, 7, 21, 22):
            words = [int(w) for w in philox4x32_10(seed, j // 4, p, g, EVO_DOMAIN_Z)]
            assert abs(z[i, j] - _scalar_normal(words, j % 4)) <= 1e-14, (p, j)  # numpy's and libm's cos differ by ulps
    # the four counter slots and the key are all live
    base = evo_z_reference(seed, g, [5], P)
    assert not np.array_equal(evo_z_reference(seed, g + 1, [5], P), base)
    assert not np.array_equal(evo_z_reference(seed ^ 1, g, [5], P), base)
    assert not np.array_equal(evo_z_reference(seed ^ (1 << 32), g, [5], P), base)
    assert not np.array_equal(evo_z_reference(seed, g, [6], P), base)

    step, n, a = np.arange(3)[:, None, None], np.arange(4)[None, :, None], np.arange(9)[None, None, :]
    xi = evo_action_noise_reference(seed, g, step, n, a)
    assert xi.shape == (3, 4, 9) and xi.dtype == np.float64
    for k, i, j in ((0, 0, 0), (2, 3, 1), (1, 2, 3), (1, 0, 4), (2, 1, 7), (0, 3, 8)):
        words = [int(w) for w in philox4x32_10(seed, i, k, g, EVO_DOMAIN_ACT | (j // 4))]
        assert abs(xi[k, i, j] - _scalar_normal(words, j % 4)) <= 1e-14, (k, i, j)
    flat = xi.reshape(-1)
    assert np.unique(flat).size == flat.size  # every (step, env, asset) draws its own value
    assert not np.array_equal(evo_action_noise_reference(seed, g + 1, step, n, a), xi)
    assert float(evo_action_noise_reference(seed, g, 2, 3, 1)) == xi[2, 3, 1]


def test_streams_are_standard_normal():
    z = evo_z_reference(0x0123456789ABCDEF, 0, np.arange(64), 4097)
    assert abs(z.mean()) < 1e-2 and abs(z.var() - 1.0) < 1e-2 and abs((z ** 4).mean() - 3.0) < 0.1
