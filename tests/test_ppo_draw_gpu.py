"""GPU: ``fe_ppo_minibatch`` (include/finenvs_amd_ppo.h) beyond one asset and one workgroup.

tests/test_ppo_update_gpu.py draws with A = 1, B <= 30, n <= 120 (a Feistel half-width hb <= 4), four columns and a base
epoch of 0 or 2.  Here the same launch runs

* with A = 3 and A = 2: ``b = i / A``, ``a = i - b * A``, ``row * A + a``, the scalar fields stored by lane ``a == 0``;
* in 11 workgroups (B * A = 2 700) and with a second trip of the grid-stride loop (B * A = 540 000 > 2 048 x 256);
* at n = 65 536 (hb = 8, no walk), n = 65 537 (hb = 9: three of four outputs of a pass fall outside [0, n), the longest
  walk takes 39 passes) and n = 2^22 + 1 (hb = 12, the round counter's 16-bit field three quarters full);
* with two columns, with none and a null ``columns_out``;
* with a base epoch of 2^20 + 3 in the cursor (the counter's high word is not zero then).

The chunks are plain tensors of the documented shapes, ``obs_src`` and ``obs_pos`` encode ``(step, env, asset)``, the rows
between N and the capacity C hold -99.  The expected values are ``helpers.ppo_permute_reference`` (numpy, from the header's
text) and plain torch indexing with ``env = s // T``, ``step = s % T``: the library's host mirror is not consulted."""
import types

import numpy as np
import pytest
import torch

from tests.helpers import assert_bits, ppo_permute_reference
from tests.test_ppo_update_gpu import FIELDS, _banded, _bands_intact, _draw

pytestmark = pytest.mark.gpu

SEED = 1234567
COLS = ("col0", "col1", "col2", "col3")


@pytest.fixture(scope="module")
def lib():
    import finenvs_amd  # noqa: F401
    from finenvs_amd import _lib

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load()


def _chunk(T, N, C, A, seed=3):
    """obs_src (T + 1, C), obs_pos (T + 1, C, A), actions (T, C, A), four columns (T, N).  ``obs_src[t, e]`` is
    ``(t << 40) | (e + 1)`` and ``obs_pos[t, e, a]`` is ``((t * C + e) * A + a) + 0.25``, exact in their types, so a
    wrong row or asset is a different number; the actions and columns are seeded normal draws."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.arange(T + 1, device="cuda", dtype=torch.int64).reshape(T + 1, 1)
    e = torch.arange(C, device="cuda", dtype=torch.int64).reshape(1, C)
    obs_src = (t << 40) | (e + 1)
    a = torch.arange(A, device="cuda", dtype=torch.int64).reshape(1, 1, A)
    obs_pos = (((t * C + e).reshape(T + 1, C, 1) * A + a).double() + 0.25)
    actions = torch.randn((T, C, A), generator=gen, device="cuda")
    if C > N:  # the padding of a chunk's rows: never a sample
        obs_src[:, N:], obs_pos[:, N:], actions[:, N:] = -99, -99.0, -99.0
    columns = [torch.randn((T, N), generator=gen, device="cuda") for _ in range(4)]
    chunk = types.SimpleNamespace(obs_src=obs_src.contiguous(), obs_pos=obs_pos.contiguous(), actions=actions, T=T, N=N, C=C, A=A)
    return chunk, columns


def _reference(chunk, columns, seed, epoch, M, m):
    """What the header says mini-batch m of M of ``epoch`` holds, and the longest walk of its positions."""
    T, n = chunk.T, chunk.T * chunk.N
    B = n // M
    s, passes = ppo_permute_reference(seed, epoch, n, np.arange(m * B, (m + 1) * B))
    idx = torch.from_numpy(s).cuda()
    env, step = idx // T, idx % T
    want = {"indices": idx, "obs_src": chunk.obs_src[step, env], "obs_pos": chunk.obs_pos[step, env].reshape(-1),
            "actions": chunk.actions[step, env].reshape(-1)}
    for i, c in enumerate(columns):
        want[f"col{i}"] = c[step, env]
    return want, passes


def _check(lib, chunk, columns, cursor, epoch, offset, M, m, skip=(), **draw):
    """One draw between guard bands against the reference, bit for bit; returns the outputs."""
    B, A = (chunk.T * chunk.N) // M, chunk.A
    big, win = _banded(B, A)
    _draw(lib, chunk, columns, cursor, SEED, offset, M, m, win, skip, A=A, **draw)
    _bands_intact(big, B, skip, A=A)
    want, _ = _reference(chunk, columns, SEED, epoch, M, m)
    for k in FIELDS:
        if k not in skip:
            assert_bits(win[k].cpu().numpy(), want[k].cpu().numpy(), f"{k} (epoch {epoch}, mini-batch {m} of {M})")
    return {k: v.clone() for k, v in win.items()}


def _cursor(epoch=0):
    return torch.tensor([epoch, 0], dtype=torch.int64, device="cuda")


def test_three_assets_every_minibatch_with_and_without_null_outputs(lib):
    """A = 3, N = 24, T = 5, C = 32, M = 4: B = 30 samples, 90 lanes."""
    chunk, columns = _chunk(5, 24, 32, 3)
    cursor, M = _cursor(), 4
    skip = ("obs_src", "obs_pos", "col1", "col3")
    for offset in (0, 1):
        for m in range(M):
            full = _check(lib, chunk, columns, cursor, offset, offset, M, m)
            assert full["obs_pos"].reshape(30, 3).shape == full["actions"].reshape(30, 3).shape == (30, 3)
            some = _check(lib, chunk, columns, cursor, offset, offset, M, m, skip)
            for k in FIELDS:
                if k not in skip:
                    assert_bits(some[k].cpu().numpy(), full[k].cpu().numpy(), f"{k} next to null outputs")
    assert cursor.tolist() == [0, 0]


@pytest.mark.parametrize("num_columns,columns_out", [(2, True), (0, False)])
def test_fewer_columns_leave_the_absent_ones_alone(lib, num_columns, columns_out):
    """A = 2 with two columns, then with none and ``columns_out`` null.  The tails of both pointer arrays name real
    buffers: a launch that looked at them would write into a guarded window, and ``_bands_intact`` would say so."""
    chunk, columns = _chunk(5, 24, 32, 2)
    cursor, M = _cursor(), 4
    absent = COLS[num_columns:]
    for offset in (0, 1):
        for m in range(M):
            _check(lib, chunk, columns, cursor, offset, offset, M, m, absent, num_columns=num_columns, columns_out=columns_out)
    assert cursor.tolist() == [0, 0]


def test_eleven_workgroups_draw_a_bijection(lib):
    """N = 300, T = 3, C = 300, A = 3, M = 1: B = 900, 2 700 lanes in 11 workgroups; one epoch is a permutation."""
    chunk, columns = _chunk(3, 300, 300, 3)
    cursor = _cursor()
    assert -(-900 * 3 // 256) == 11
    out = _check(lib, chunk, columns, cursor, 0, 0, 1, 0)
    assert torch.equal(out["indices"].sort().values, torch.arange(900, device="cuda"))
    assert cursor.tolist() == [0, 0]


@pytest.fixture(scope="module")
def chunk_65537():
    return _chunk(1, 65537, 65537, 1)


def test_long_walks_whole_epoch(lib, chunk_65537):
    """n = 65 537 (hb = 9), M = 1: every position, the longest walk among them (39 passes with this seed and epoch)."""
    chunk, columns = chunk_65537
    cursor = _cursor()
    _, passes = _reference(chunk, columns, SEED, 1, 1, 0)
    print(f"n = 65537: the longest walk takes {passes} passes")
    assert passes > 8
    out = _check(lib, chunk, columns, cursor, 1, 1, 1, 0)
    assert torch.equal(out["indices"].sort().values, torch.arange(65537, device="cuda"))
    assert cursor.tolist() == [0, 0]  # no walk without an end


def test_long_walks_in_four_minibatches(lib, chunk_65537):
    """n = 65 537, M = 4: B = 16 384; the mini-batches are disjoint and leave exactly one sample out."""
    chunk, columns = chunk_65537
    cursor = _cursor()
    drawn = torch.cat([_check(lib, chunk, columns, cursor, 0, 0, 4, m)["indices"] for m in range(4)])
    assert drawn.numel() == 65536 and torch.unique(drawn).numel() == 65536
    assert int(drawn.min()) >= 0 and int(drawn.max()) < 65537
    assert cursor.tolist() == [0, 0]


def test_a_power_of_four_needs_no_walk(lib):
    """n = 65 536 (hb = 8): the domain is [0, n) itself."""
    chunk, columns = _chunk(1, 65536, 65536, 1)
    cursor = _cursor()
    _, passes = _reference(chunk, columns, SEED, 0, 1, 0)
    assert passes == 1
    out = _check(lib, chunk, columns, cursor, 0, 0, 1, 0)
    assert torch.equal(out["indices"].sort().values, torch.arange(65536, device="cuda"))
    assert cursor.tolist() == [0, 0]


def test_the_grid_stride_loop_takes_a_second_trip(lib):
    """T = 3, N = 60 000, C = 60 001, A = 3, M = 1: B * A = 540 000 lanes' worth of work on the capped grid of 2 048
    workgroups, so 15 712 lanes take a second element."""
    chunk, columns = _chunk(3, 60000, 60001, 3)
    B = 3 * 60000
    assert B * 3 > 2048 * 256 and B * 3 - 2048 * 256 == 15712
    cursor = _cursor()
    out = _check(lib, chunk, columns, cursor, 0, 0, 1, 0)
    assert torch.equal(out["indices"].sort().values, torch.arange(B, device="cuda"))
    assert cursor.tolist() == [0, 0]


def test_half_width_twelve(lib):
    """n = 2^22 + 1 (T = 1), hb = 12, M = 64, no columns, mini-batches 0 and 63.  The widest half-width whose chunk
    (about 150 MB with both descriptor arrays) is filled in well under a second; hb = 13 .. 16 need chunks of gigabytes
    and are not run."""
    n = (1 << 22) + 1
    assert (max(1, (n - 1).bit_length()) + 1) // 2 == 12
    chunk, columns = _chunk(1, n, n, 1)
    cursor = _cursor()
    for m in (0, 63):
        out = _check(lib, chunk, columns, cursor, 0, 0, 64, m, COLS, num_columns=0, columns_out=False)
        assert out["indices"].numel() == 65536 and torch.unique(out["indices"]).numel() == 65536
    assert cursor.tolist() == [0, 0]


def test_a_base_epoch_with_many_bits(lib):
    """``cursor[0] = 2^20 + 3`` written by the host: ``(epoch * 4 + round) << 16`` then reaches bit 38, the counter's high
    word.  Offsets 0 and 1 are epochs 2^20 + 3 and 2^20 + 4; after ``fe_ppo_epochs_advance(cursor, 5)`` offset 0 is
    epoch 2^20 + 8."""
    from finenvs_amd import _lib

    base = (1 << 20) + 3
    chunk, columns = _chunk(5, 24, 32, 1)
    cursor, M = _cursor(base), 4
    first = {}
    for offset in (0, 1):
        for m in range(M):
            first[offset, m] = _check(lib, chunk, columns, cursor, base + offset, offset, M, m)["indices"]
    assert not torch.equal(first[0, 0], first[1, 0])
    assert cursor.tolist() == [base, 0]
    _lib.check(lib.fe_ppo_epochs_advance(cursor.data_ptr(), 5, torch.cuda.current_stream().cuda_stream), lib)
    _check(lib, chunk, columns, cursor, base + 5, 0, M, 0)
    assert cursor.tolist() == [base + 5, 0]
