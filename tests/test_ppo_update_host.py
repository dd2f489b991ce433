"""CPU: the host side of the capturable PPO update (include/finenvs_amd_ppo.h, finenvs_amd/rng.py, finenvs_amd/ppo.py).

* ``rng.ppo_permute`` is a bijection of ``[0, n)`` that depends on the epoch and on the seed;
* the mini-batch arithmetic: ``B = n // M``, the remainder dropped, the mini-batches of an epoch disjoint;
* every ``FE_ERR_ARG`` case of ``fe_ppo_minibatch`` and its siblings comes back through ctypes without a GPU;
* ``PPO_SIGNATURES`` is the header's list of functions;
* ``PPOUpdate`` refuses heads that are not capturable."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.test_cabi import declared_symbols

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PPO_HEADER = os.path.join(REPO, "include", "finenvs_amd_ppo.h")
SIZES = (1, 2, 3, 5, 16, 17, 35, 120, 255, 256, 257, 1000)


@pytest.fixture(scope="module")
def lib():
    from finenvs_amd import _lib

    return _lib.load()


@pytest.mark.parametrize("n", SIZES)
def test_permutation_is_a_bijection(n):
    from finenvs_amd.rng import ppo_permute

    perms = {(seed, epoch): [ppo_permute(seed, epoch, n, i) for i in range(n)] for seed, epoch in ((7, 0), (7, 1), (8, 0))}
    for key, p in perms.items():
        assert sorted(p) == list(range(n)), key
    if n >= 16:
        assert perms[7, 0] != perms[7, 1], "epochs 0 and 1 shuffle alike"
        assert perms[7, 0] != perms[8, 0], "two seeds shuffle alike"


BIG_SIZES = (65536, 65537, 200003)  # hb = 8 without a walk; hb = 9 just above a power of 4; an odd size in between


@pytest.mark.parametrize("n", SIZES)
def test_vectorised_reference_equals_the_scalar_mirror(n):
    """``helpers.ppo_permute_reference`` (numpy, from the header's text) against ``rng.ppo_permute``, element for element."""
    from finenvs_amd.rng import ppo_permute
    from tests.helpers import ppo_permute_reference

    for seed in (7, 0xFEDCBA9876543210):
        for epoch in (0, (1 << 20) + 3):
            got, passes = ppo_permute_reference(seed, epoch, n, np.arange(n))
            assert got.dtype == np.int64 and got.shape == (n,) and passes >= 1
            assert got.tolist() == [ppo_permute(seed, epoch, n, i) for i in range(n)], (seed, epoch)


@pytest.fixture(scope="module")
def big_permutations():
    from tests.helpers import ppo_permute_reference

    return {n: ppo_permute_reference(1234567, 1, n, np.arange(n)) for n in BIG_SIZES}


@pytest.mark.parametrize("n", BIG_SIZES)
def test_vectorised_reference_at_large_sizes(big_permutations, n):
    """A bijection of ``[0, n)`` at the sizes the device tests draw from, equal to the scalar mirror on the first 40
    positions and the last.  Longest walks measured with seed 1234567, epoch 1: 1 pass at n = 65 536 (the domain is
    [0, n) itself), 39 passes at n = 65 537 (three of four outputs of a pass fall outside), 10 at n = 200 003."""
    from finenvs_amd.rng import ppo_permute

    got, passes = big_permutations[n]
    assert np.array_equal(np.sort(got), np.arange(n))
    for i in list(range(40)) + [n - 1]:
        assert int(got[i]) == ppo_permute(1234567, 1, n, i), i
    print(f"n = {n}: longest walk {passes} passes")
    if n == 65536:
        assert passes == 1
    if n == 65537:
        assert passes > 8


def test_vectorised_reference_refuses_positions_outside():
    from tests.helpers import ppo_permute_reference

    for n, positions in ((0, [0]), (1 << 32, [0]), (5, [5]), (5, [-1]), (5, [])):
        with pytest.raises(ValueError):
            ppo_permute_reference(0, 0, n, positions)
    got, passes = ppo_permute_reference(3, 9, 1, [[0]])
    assert got.tolist() == [[0]] and passes >= 1  # (n = 1 has a domain of four: a walk there may take several passes)


def test_permutation_refuses_what_the_device_refuses():
    from finenvs_amd.rng import ppo_permute

    for n, i in ((0, 0), (1 << 32, 0), (5, 5), (5, -1)):
        with pytest.raises(ValueError):
            ppo_permute(0, 0, n, i)
    assert ppo_permute(3, 9, 1, 0) == 0


def test_the_salt_is_the_headers():
    from finenvs_amd import _lib, rng

    text = open(PPO_HEADER).read()
    assert f"#define FE_PPO_PERM_SALT 0x{rng.PPO_PERM_SALT:016X}ull" in text
    assert _lib.PPO_PERM_SALT == rng.PPO_PERM_SALT
    for name, value in (("EPOCH", _lib.PPO_CURSOR_EPOCH), ("ERRORS", _lib.PPO_CURSOR_ERRORS), ("WORDS", _lib.PPO_CURSOR_WORDS)):
        assert f"#define FE_PPO_CURSOR_{name} {value}\n" in text
    assert f"#define FE_PPO_MAX_COLUMNS {_lib.PPO_MAX_COLUMNS}\n" in text


def test_minibatch_arithmetic_drops_the_remainder():
    from finenvs_amd.ppo import minibatch_indices, minibatch_size

    N, T, M = 7, 5, 4
    n = N * T
    assert minibatch_size(n, M) == 8
    for epoch in (0, 1):
        batches = [minibatch_indices(11, epoch, n, M, m) for m in range(M)]
        assert all(len(b) == 8 for b in batches)
        seen = [s for b in batches for s in b]
        assert len(set(seen)) == 32 and all(0 <= s < n for s in seen)  # disjoint, and three samples dropped
        assert len(set(range(n)) - set(seen)) == 3
    with pytest.raises(ValueError):
        minibatch_size(3, 4)
    with pytest.raises(ValueError):
        minibatch_indices(11, 0, n, M, M)


def test_argument_errors_do_not_need_a_gpu(lib):
    from finenvs_amd import _lib

    P = 8  # any non-null address: an argument error returns before a pointer is looked at
    cols = (C.c_void_p * 4)(P, P, P, P)
    five = (C.c_void_p * 5)(P, P, P, P, P)
    good = dict(src=P, pos=P, act=P, T=5, N=7, Cap=7, A=1, cols=cols, outs=cols, ncols=4, cursor=P, seed=0, off=0, M=4, m=0,
                idx=P)

    def call(**kw):
        a = {**good, **kw}
        return lib.fe_ppo_minibatch(a["src"], a["pos"], a["act"], a["T"], a["N"], a["Cap"], a["A"], a["cols"], a["outs"],
                                    a["ncols"], a["cursor"], a["seed"], a["off"], a["M"], a["m"], a["idx"], None, None, None,
                                    None)

    bad = [dict(src=None), dict(pos=None), dict(act=None), dict(cursor=None), dict(idx=None),
           dict(T=0), dict(N=0), dict(Cap=6), dict(A=0),
           dict(T=1 << 16, N=1 << 16, Cap=1 << 16), dict(T=1 << 33, N=1, Cap=1), dict(T=1, N=1 << 33, Cap=1 << 33),
           dict(M=0), dict(M=36), dict(m=-1), dict(m=4),
           dict(off=-1),
           dict(cols=five, outs=five, ncols=5), dict(ncols=-1), dict(cols=None), dict(cols=(C.c_void_p * 4)(P, None, P, P))]
    for kw in bad:
        assert call(**kw) == _lib.FE_ERR_ARG, kw
        assert b"fe_ppo_minibatch" in lib.fe_last_error()
    assert lib.fe_ppo_epochs_advance(None, 1, None) == _lib.FE_ERR_ARG
    assert lib.fe_ppo_epochs_advance(P, -1, None) == _lib.FE_ERR_ARG
    assert lib.fe_ppo_loss_workspace_doubles(0) == -1
    assert lib.fe_ppo_loss_workspace_doubles(1) == 3 and lib.fe_ppo_loss_workspace_doubles(257) == 5
    assert lib.fe_ppo_loss_workspace_doubles(1 << 40) == 1 + 2 * 256  # the grid is capped: the workspace is bounded
    actor = [P] * 5 + [61, 0.2, 0.01] + [P] * 4 + [None]
    for i in (0, 1, 2, 3, 4, 8, 9, 10, 11):
        a = list(actor)
        a[i] = None
        assert lib.fe_ppo_actor_loss(*a) == _lib.FE_ERR_ARG, i
    for i, v in ((5, 0), (6, -0.1), (6, float("nan"))):
        a = list(actor)
        a[i] = v
        assert lib.fe_ppo_actor_loss(*a) == _lib.FE_ERR_ARG, (i, v)
    value = [P, P, 61, P, P, P, None]
    for i in (0, 1, 3, 4, 5):
        a = list(value)
        a[i] = None
        assert lib.fe_ppo_value_loss(*a) == _lib.FE_ERR_ARG, i
    assert lib.fe_ppo_value_loss(P, P, 0, P, P, P, None) == _lib.FE_ERR_ARG


def test_signatures_match_the_header(lib):
    from finenvs_amd import _lib

    names = declared_symbols(PPO_HEADER)
    assert names == sorted(_lib.PPO_SIGNATURES)
    assert names == ["fe_ppo_actor_loss", "fe_ppo_epochs_advance", "fe_ppo_loss_workspace_doubles", "fe_ppo_minibatch",
                     "fe_ppo_value_loss"]
    for n in names:
        fn = getattr(lib, n)  # exported
        assert fn.restype is _lib.PPO_SIGNATURES[n][0] and list(fn.argtypes) == _lib.PPO_SIGNATURES[n][1]
    every_other = {**_lib.SIGNATURES, **_lib.EXT_SIGNATURES, **_lib.REPLAY_CURSOR_SIGNATURES, **_lib.OPTIM_SIGNATURES}
    assert not set(names) & set(every_other)
    # the argument lists: one ctypes entry per C parameter
    text = open(PPO_HEADER).read()
    import re

    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in names:
        params = re.search(rf"\b{n}\s*\(([^)]*)\)", text).group(1)
        assert len(params.split(",")) == len(_lib.PPO_SIGNATURES[n][1]), n


def test_integration_doc_names_the_entry_points():
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    assert not [n for n in declared_symbols(PPO_HEADER) if n not in doc]


def test_update_refuses_heads_that_are_not_capturable():
    from finenvs_amd.lstm_head import FusedLSTMHead
    from finenvs_amd.optim import FusedAdam
    from finenvs_amd.ppo import PPOUpdate

    def head(weights):  # the one attribute the check reads: no GPU is needed to be refused
        h = FusedLSTMHead.__new__(FusedLSTMHead)
        h.weights = weights
        return h

    opt_a, opt_c = FusedAdam(lr=3e-4), FusedAdam(lr=3e-4)
    log_std = torch.nn.Parameter(torch.zeros(1))
    with pytest.raises(ValueError, match="weights="):
        PPOUpdate(None, None, head(None), head(opt_c), log_std, opt_a, opt_c)
    with pytest.raises(ValueError, match="weights="):
        PPOUpdate(None, None, head(opt_a), head(None), log_std, opt_a, opt_c)
    with pytest.raises(ValueError, match="weights="):  # the other optimizer's head
        PPOUpdate(None, None, head(opt_c), head(opt_c), log_std, opt_a, opt_c)
    with pytest.raises(ValueError, match="FusedLSTMHead"):
        PPOUpdate(None, None, object(), head(opt_c), log_std, opt_a, opt_c)
    with pytest.raises(ValueError, match="add_tensor"):
        PPOUpdate(None, None, head(opt_a), head(opt_c), log_std, opt_a, opt_c)
