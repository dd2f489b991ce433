"""CPU: ``tests/helpers.py::crafted_descriptors``, the descriptor generator of tests/test_grad_descriptors_gpu.py, meets
the conditions those tests rest on -- conditions on the input alone, checked without a GPU."""
import pytest
import torch

from tests.helpers import crafted_descriptors


# the last eight: the twin MLP critics' cases, their targets' batch of 513 and the rings' 520 slots (D = 12, L = max(60, W + 40))
@pytest.mark.parametrize("D,L,W,B", [(12, 60, 4, 33), (12, 60, 1, 1), (12, 430, 390, 33), (12, 60, 4, 1057),
                                     (12, 60, 1, 33), (12, 60, 7, 33), (12, 60, 16, 257), (12, 80, 40, 33),
                                     (12, 60, 7, 513), (12, 60, 7, 520), (12, 60, 16, 520), (12, 60, 1, 520)])
def test_crafted_descriptors_meet_their_conditions(D, L, W, B):
    src, pos = crafted_descriptors(D, L, W, B, seed=5)
    assert src.dtype is torch.int64 and tuple(src.shape) == (B,) and src.device.type == "cpu"
    assert pos.dtype is torch.float64 and tuple(pos.shape) == (B, 1) and pos.device.type == "cpu"
    # the rule of fe_check_descriptors_kernel, row_elems = 4, rows = D * L
    assert bool((src >= 0).all()) and bool((src % 4 == 0).all()) and bool((src // 4 + W <= D * L).all())
    # ... and a window never crosses from one day's rows into the next's
    start = (src // 4) % L
    assert bool((start + W <= L).all())
    # both extremes, where the tests expect them
    assert int(src[0]) == 0
    if B >= 2:
        assert int(src[B - 1]) == ((D - 1) * L + (L - W)) * 4 == (D * L - W) * 4
    total = D * (L - W + 1)
    assert int(torch.unique(src).numel()) == min(B, total)
    if B > total:  # the first permutation is complete
        assert int(torch.unique(src[:total]).numel()) == total
    # positions: never zero, inside the scale, both signs, not representable in f32
    assert bool((pos != 0).all()) and float(pos.abs().max()) < 0.5
    if B >= 8:
        assert bool((pos > 0).any()) and bool((pos < 0).any())
    assert float((pos.float().double() != pos).double().mean()) > 0.9
    # the same seed gives the same batch, another seed another
    again = crafted_descriptors(D, L, W, B, seed=5)
    assert torch.equal(again[0], src) and torch.equal(again[1], pos)
    if B > 2:
        other = crafted_descriptors(D, L, W, B, seed=6)
        assert not torch.equal(other[0], src) and not torch.equal(other[1], pos)


def test_pos_scale_and_the_smallest_tables():
    src, pos = crafted_descriptors(3, 10, 4, 16, seed=1, pos_scale=2.0)
    assert 0.5 < float(pos.abs().max()) < 2.0
    src, pos = crafted_descriptors(1, 4, 4, 5, seed=1)  # one window in the whole table: every descriptor is that one
    assert src.tolist() == [0] * 5 and bool((pos != 0).all())
    src, _ = crafted_descriptors(1, 5, 4, 2, seed=1)  # two windows, two descriptors
    assert src.tolist() == [0, 4]
