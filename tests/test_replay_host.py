"""CPU: the replay ring's host bookkeeping (finenvs_amd/replay.py) against the reference's own buffer
(tests/golden/replay_buffer.npz, written by tools/make_replay_golden.py from finenvs/agents/off_policy_buffer.py), and the
refusals that need no device."""
import numpy as np
import pytest
import torch

from tests.helpers import assert_bits, load_golden


@pytest.fixture(scope="module")
def gold():
    return load_golden("replay_buffer.npz")


def _replay_the_stores(gold):
    """The golden's stores on a ring of transition ids: store k writes ids k*N .. k*N + N - 1 to slots (head + j) mod C,
    as fe_replay_append does; yields (store, ring index, ring of ids)."""
    from finenvs_amd.replay import RingIndex

    N, C, S, _ = (int(x) for x in gold["meta"])
    ring, ids = RingIndex(C), np.full(C, -1, dtype=np.int64)
    for s in range(S):
        ring.check_store(N)
        ids[(ring.head + np.arange(N)) % C] = s * N + np.arange(N)
        ring.advance(N)
        yield s, ring, ids


def test_sizes_follow_the_reference(gold):
    sizes = [ring.size for _, ring, _ in _replay_the_stores(gold)]
    assert sizes == gold["sizes"].tolist()
    assert max(sizes) == int(gold["meta"][1]) and int(gold["meta"][1]) % int(gold["meta"][0]) != 0


def test_index_map_reproduces_retained_and_sampled_ids(gold):
    at = gold["at"].tolist()
    checked = 0
    for s, ring, ids in _replay_the_stores(gold):
        if s not in at:
            continue
        k = at.index(s)
        retained = ids[ring.physical(np.arange(ring.size))]
        assert retained.tolist() == gold["retained"][k][: ring.size].tolist(), f"retained ids after store {s}"
        assert (gold["retained"][k][ring.size:] == -1).all()
        drawn = ids[ring.physical(gold["indices"][k])]
        x = drawn.astype(np.float64)
        # every field of the reference's mini-batch carries the id of the transition it was drawn from
        assert_bits(gold["states"][k][:, 0, 0], x.astype(np.float32), f"states ids after store {s}")
        assert_bits(gold["next_states"][k][:, 0, 0], (x + 0.5).astype(np.float32), f"next_states ids after store {s}")
        assert_bits(gold["actions"][k][:, 0], (x + 0.25).astype(np.float32), f"actions ids after store {s}")
        assert_bits(gold["rewards"][k][:, 0], (x + 0.125).astype(np.float32), f"rewards ids after store {s}")
        assert_bits(gold["dones"][k][:, 0], x.astype(np.float32), f"dones ids after store {s}")
        checked += 1
    assert checked == len(at)


def test_physical_index_on_ints_numpy_and_torch():
    from finenvs_amd.replay import physical_index

    assert physical_index(0, 3, 5, 10) == 8 and physical_index(4, 3, 5, 10) == 2
    assert physical_index(np.arange(3), 0, 10, 10).tolist() == [0, 1, 2]
    assert physical_index(torch.arange(4), 2, 7, 7).tolist() == [2, 3, 4, 5]


def test_default_draw_is_the_reference_call():
    """get_mini_batch draws with torch.randint(0, size, (B,)) on the buffer's device: the reference's generator stream."""
    import inspect

    from finenvs_amd.replay import ReplayBuffer

    assert "torch.randint(0, self.size(), (int(size),), device=self.device)" in inspect.getsource(ReplayBuffer.get_mini_batch)


def test_refusals_without_a_device():
    from types import SimpleNamespace

    from finenvs_amd.replay import ReplayBuffer, RingIndex

    with pytest.raises(ValueError, match="max_size must be >= 1"):
        RingIndex(0)
    with pytest.raises(ValueError, match="empty replay buffer"):
        RingIndex(10).check_sample()
    env = SimpleNamespace(num_envs=48, num_assets=1, num_intervals=4, device="cpu")
    with pytest.raises(ValueError, match="does not fit max_size = 47"):
        ReplayBuffer(env, max_size=47)  # N > max_size: the one divergence from the reference
    with pytest.raises(RuntimeError, match="lives in HBM"):
        ReplayBuffer(env, max_size=48)


def _transition(N, A, device="cpu"):
    s = (torch.zeros(N, dtype=torch.int64, device=device), torch.zeros((N, A), dtype=torch.float64, device=device))
    n = (torch.zeros(N, dtype=torch.int64, device=device), torch.zeros((N, A), dtype=torch.float64, device=device))
    return dict(states=s, actions=torch.zeros((N, A), device=device), rewards=torch.zeros(N, dtype=torch.float64, device=device),
                next_states=n, dones=torch.zeros(N, dtype=torch.int32, device=device))


@pytest.mark.parametrize("field,value,match", [
    ("states", torch.zeros((5, 4, 15), dtype=torch.float64), "descriptors_out"),   # a rendered observation
    ("next_states", torch.zeros((5, 4, 15), dtype=torch.float32), "descriptors_out"),
    ("states", (torch.zeros(5, dtype=torch.int32), torch.zeros((5, 3), dtype=torch.float64)), "obs_src"),
    ("states", (torch.zeros(6, dtype=torch.int64), torch.zeros((6, 3), dtype=torch.float64)), "obs_src"),   # N mismatch
    ("next_states", (torch.zeros(5, dtype=torch.int64), torch.zeros((5, 2), dtype=torch.float64)), "obs_pos"),  # A mismatch
    ("next_states", (torch.zeros(5, dtype=torch.int64), torch.zeros((5, 3), dtype=torch.float32)), "obs_pos"),
    ("states", (torch.zeros(5, dtype=torch.int64),), "pair"),
    ("actions", torch.zeros((5, 3), dtype=torch.float16), "actions must be a float32 or float64"),
    ("actions", torch.zeros((5, 2)), "actions must have shape"),
    ("rewards", torch.zeros(5, dtype=torch.float32), "rewards must be a float64"),
    ("rewards", torch.zeros(4, dtype=torch.float64), "rewards must be a float64"),
    ("dones", torch.zeros(5, dtype=torch.bool), "dones must be an int32"),
])
def test_store_refuses_malformed_transitions(field, value, match):
    from finenvs_amd.replay import check_transition

    kw = _transition(5, 3)
    check_transition(5, 3, "cpu", **kw)  # the well-formed one passes
    kw[field] = value
    with pytest.raises(ValueError, match=match):
        check_transition(5, 3, "cpu", **kw)


def test_store_refuses_a_foreign_device():
    from finenvs_amd.replay import check_transition

    with pytest.raises(ValueError, match="device"):
        check_transition(5, 1, "cuda:0", **_transition(5, 1))
