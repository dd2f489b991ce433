"""CPU: the replay cursor's C ABI surface (include/finenvs_amd_replay_cursor.h) against the built library and the ctypes
table, the host mirror of the device draw's index rule, and the refusal of a ``ReplayDraw`` on a buffer without a
cursor (before any device work)."""
import ctypes
import os
from types import SimpleNamespace

import pytest

from tests.test_cabi import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "finenvs_amd_replay_cursor.h")
EXPECTED = ["fe_replay_append_c", "fe_replay_sample_c", "fe_ring_draw", "fe_twin_q_target_c"]


@pytest.fixture(scope="module")
def lib():
    from finenvs_amd.csrc import build as hip_build

    if not os.path.exists(hip_build.LIB) and not os.path.exists(hip_build.HIPCC):
        pytest.skip("no built library and no hipcc")
    return ctypes.CDLL(hip_build.build())


def test_header_symbols_are_exported_and_bound(lib):
    from finenvs_amd import _lib

    names = declared_symbols(HEADER)
    assert names == EXPECTED
    for name in names:
        assert hasattr(lib, name), f"{name} is declared in the header but not exported by the library"
        assert name in _lib.REPLAY_CURSOR_SIGNATURES, f"{name} has no ctypes signature"


def test_signature_table_equals_the_header():
    from finenvs_amd import _lib

    assert sorted(_lib.REPLAY_CURSOR_SIGNATURES) == declared_symbols(HEADER)
    # argument counts, from the declarations themselves
    import re

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, (res, args) in _lib.REPLAY_CURSOR_SIGNATURES.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
        assert decl, name
        assert len(args) == len(decl.group(1).split(",")), name
        assert res is ctypes.c_int
    # the siblings differ from the by-value entries as the header says
    assert len(_lib.REPLAY_CURSOR_SIGNATURES["fe_replay_append_c"][1]) == len(_lib.REPLAY_SIGNATURES["fe_replay_append"][1]) + 2
    assert len(_lib.REPLAY_CURSOR_SIGNATURES["fe_replay_sample_c"][1]) == len(_lib.REPLAY_SIGNATURES["fe_replay_sample"][1]) - 1
    assert len(_lib.REPLAY_CURSOR_SIGNATURES["fe_twin_q_target_c"][1]) == len(_lib.CRITIC_SIGNATURES["fe_twin_q_target"][1]) - 1
    assert (_lib.CURSOR_HEAD, _lib.CURSOR_SIZE, _lib.CURSOR_DRAWS, _lib.CURSOR_TICKET, _lib.CURSOR_WORDS) == (0, 1, 2, 3, 4)
    for word, value in (("HEAD", 0), ("SIZE", 1), ("DRAWS", 2), ("TICKET", 3), ("WORDS", 4)):
        assert re.search(rf"#define FE_CURSOR_{word} {value}\b", text)


@pytest.mark.parametrize("size", [1, 2, 7, 40, 2 ** 31])
def test_draw_indices_rule_and_range(size):
    from finenvs_amd.replay import draw_indices
    from finenvs_amd.rng import philox_u32

    seed, c, count = 0x1234_5678_9ABC_DEF0, 2 ** 32 - 3, 64  # the counter crosses its low word
    got = draw_indices(seed, c, size, count)
    assert got == [(philox_u32(seed, c + b) * size) >> 32 for b in range(count)]
    assert all(0 <= k < size for k in got)
    if size == 1:
        assert got == [0] * count
    if size >= 40:
        assert len(set(got)) > 1


def test_draw_indices_is_one_stream():
    from finenvs_amd.replay import draw_indices

    seed, first, size = 9, 1000, 40
    assert draw_indices(seed, first, size, 5) + draw_indices(seed, first + 5, size, 9) == draw_indices(seed, first, size, 14)
    assert draw_indices(seed, first, size, 0) == []
    with pytest.raises(ValueError):
        draw_indices(seed, first, 0, 3)


def test_a_replay_draw_needs_a_cursor_buffer():
    """Every consumer refuses a ``ReplayDraw`` on a buffer that keeps head and size on the host only, first thing: the
    stubs below have nothing else a consumer could touch."""
    from finenvs_amd.critic import FusedTwinCritic
    from finenvs_amd.lstm_head import td3_actor_loss
    from finenvs_amd.replay import ReplayBuffer, ReplayDraw, as_draw
    from finenvs_amd.sac import FusedSACRollout

    draw = ReplayDraw(*([None] * 8))
    plain = SimpleNamespace(cursor=None)
    stub = SimpleNamespace()
    with pytest.raises(ValueError, match="cursor=True"):
        ReplayBuffer.get_mini_batch(plain, 4, indices=draw)
    with pytest.raises(ValueError, match="cursor=True"):
        ReplayBuffer.draw(plain, 4)
    with pytest.raises(ValueError, match="cursor=True"):
        FusedTwinCritic.sac_targets(stub, plain, draw, None)
    with pytest.raises(ValueError, match="cursor=True"):
        FusedTwinCritic.td3_targets(stub, plain, draw, None)
    with pytest.raises(ValueError, match="cursor=True"):
        FusedTwinCritic.critic_loss(stub, plain, draw, None)
    with pytest.raises(ValueError, match="cursor=True"):
        FusedSACRollout.actor_losses(stub, plain, draw, None)
    with pytest.raises(ValueError, match="cursor=True"):
        td3_actor_loss(stub, plain, draw, None)
    # indices that are no draw pass through, and a cursor buffer admits the draw
    assert as_draw(plain, None, "x") is None and as_draw(plain, [1, 2], "x") is None
    assert as_draw(SimpleNamespace(cursor=object()), draw, "x") is draw
