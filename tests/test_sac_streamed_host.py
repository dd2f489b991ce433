"""CPU: the SAC LSTM actor at H = 256 / 512 / 1024 -- the C ABI surface of include/finenvs_amd_sac_streamed.h with the
argument checks that need no device (and their order), the workspace size, ``check_actor``'s ``streamed`` opt-in and the
packed layout ``pack_sac_weights`` and ``FusedAdam`` keep for such an actor."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "finenvs_amd_sac_streamed.h")
SIZES = (256, 512, 1024)


def test_header_declares_exactly_the_four_signatures_and_the_library_exports_them():
    from finenvs_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(fe_[a-z0-9_]+)\s*\(", text))) == sorted(_lib.SAC_STREAMED_SIGNATURES)
    assert sorted(_lib.SAC_STREAMED_SIGNATURES) == ["fe_env_rollout_sac_streamed", "fe_sac_backward_streamed",
                                                    "fe_sac_forward_streamed", "fe_sac_streamed_grad_workspace_floats"]
    others = (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.SAC_SIGNATURES) | set(_lib.SAC_GRAD_SIGNATURES)
              | set(_lib.CRITIC_STREAMED_SIGNATURES) | set(_lib.LSTM_STREAMED_GRAD_SIGNATURES) | set(_lib.OPTIM_SIGNATURES)
              | set(_lib.REPLAY_CURSOR_SIGNATURES))
    assert not set(_lib.SAC_STREAMED_SIGNATURES) & others
    lib = _lib.load()
    for name, (res, args) in _lib.SAC_STREAMED_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    # each entry takes the argument list of its register-resident namesake with the biases in device memory
    s = _lib.SAC_STREAMED_SIGNATURES
    assert s["fe_env_rollout_sac_streamed"] == _lib.OPTIM_SIGNATURES["fe_env_rollout_sac_p"]
    assert s["fe_sac_forward_streamed"] == _lib.OPTIM_SIGNATURES["fe_sac_forward_p"]
    assert s["fe_sac_backward_streamed"] == _lib.OPTIM_SIGNATURES["fe_sac_backward_p"]
    assert s["fe_sac_streamed_grad_workspace_floats"] == _lib.SAC_GRAD_SIGNATURES["fe_sac_grad_workspace_floats"]
    assert lib.fe_version() == _lib.FE_ABI_VERSION == 5


def test_workspace_size_is_monotone_and_constant_from_the_chunk_on():
    from finenvs_amd import _lib

    lib = _lib.load()
    floats = lib.fe_sac_streamed_grad_workspace_floats
    for H, W, n in ((32, 4, 1), (128, 4, 1), (300, 4, 1), (2048, 4, 1), (256, 0, 1), (256, 4, -1)):
        assert floats(H, W, n) == -1, (H, W, n)
    for H in SIZES:
        for W in (4, 7):
            chunk = lib.fe_lstm_streamed_grad_chunk_pairs(H, W)
            counts = (0, 1, 31, 32, 33, 256, 4097, chunk, chunk + 33, 1 << 20)
            assert list(counts) == sorted(counts)
            sizes = [floats(H, W, n) for n in counts]
            assert all(s > 0 for s in sizes), (H, W, sizes)
            assert all(b >= a for a, b in zip(sizes, sizes[1:])), (H, W, sizes)
            assert sizes[1] > sizes[0] and sizes[4] > sizes[3] and sizes[6] < sizes[7], (H, W, sizes)
            assert sizes[7] == sizes[8] == sizes[9], (H, W, sizes)
            # the LSTM pass's workspace, W_l^T, at least one split sum of d W_l, and z and dz of every pair of a pass
            lstm = [lib.fe_lstm_streamed_grad_workspace_floats(H, W, n) for n in counts]
            padded = [min(chunk, (n + 31) // 32 * 32) for n in counts]
            assert all(s >= l + 2 * H * H + 2 * p * H for s, l, p in zip(sizes, lstm, padded)), (H, W)
            assert all(s % 4 == 0 for s in sizes)
            assert 4 * sizes[-1] <= (1 << 31) + (1 << 29)


_ROLLOUT = ("env", "lr32", "whh", "wx", "wl", "bl", "wmu", "bmu", "wstd", "bstd", "src", "pos", "rewards", "dones")
_FORWARD = ("env", "lr32", "whh", "wx", "wl", "bl", "wmu", "bmu", "wstd", "bstd", "src", "pos")
_BACKWARD = _FORWARD + ("noise", "actions", "stds", "workspace")


def _rollout(lib, H=256, K=4, traj_src=None, traj_pos=None, **null):
    p = {k: 16 for k in _ROLLOUT}
    p.update(null)
    return lib.fe_env_rollout_sac_streamed(p["env"], p["lr32"], p["whh"], p["wx"], p["wl"], p["bl"], p["wmu"], p["bmu"],
                                           p["wstd"], p["bstd"], H, K, p["src"], p["pos"], None, None, None, None,
                                           p["rewards"], p["dones"], traj_src, traj_pos, None)


def _forward(lib, H=256, count=4, noise=None, actions=None, **null):
    p = {k: 16 for k in _FORWARD}
    p.update(null)
    return lib.fe_sac_forward_streamed(p["env"], p["lr32"], p["whh"], p["wx"], p["wl"], p["bl"], p["wmu"], p["bmu"],
                                       p["wstd"], p["bstd"], H, p["src"], p["pos"], count, noise, actions, None, 16, 16, None)


def _backward(lib, H=256, count=4, d_actions=16, d_log_probs=16, grads="ok", **null):
    from finenvs_amd import _lib

    p = {k: 16 for k in _BACKWARD}
    p.update(null)
    grads = _lib.FeSacGrads(*([16] * 10)) if grads == "ok" else grads
    return lib.fe_sac_backward_streamed(p["env"], p["lr32"], p["whh"], p["wx"], p["wl"], p["bl"], p["wmu"], p["bmu"],
                                        p["wstd"], p["bstd"], H, p["src"], p["pos"], count, p["noise"], p["actions"],
                                        p["stds"], d_actions, d_log_probs, p["workspace"],
                                        None if grads is None else C.byref(grads), None)


def test_the_new_entries_refuse_without_a_device_in_the_stated_order():
    """Made-up non-null pointers, never dereferenced: every case here is refused first."""
    from finenvs_amd import _lib

    lib = _lib.load()
    err = lambda: lib.fe_last_error()  # noqa: E731
    # acting
    for name in _ROLLOUT:
        assert _rollout(lib, **{name: None}) == _lib.FE_ERR_ARG, name
        assert err().startswith(b"fe_env_rollout_sac_streamed: bad argument"), name
    assert _rollout(lib, K=0) == _lib.FE_ERR_ARG and err().startswith(b"fe_env_rollout_sac_streamed: bad argument")
    assert _rollout(lib, traj_src=16) == _lib.FE_ERR_ARG
    assert err().startswith(b"fe_env_rollout_sac_streamed: states_src_out and states_pos_out go together")
    for H in (32, 128, 300, 2048):
        assert _rollout(lib, H=H) == _lib.FE_ERR_ARG
        assert err().startswith(b"fe_env_rollout_sac_streamed: H must be 256, 512 or 1024"), err()
        assert b"fe_env_rollout_sac runs H = 32, 64 and 128" in err(), err()
    assert _rollout(lib, H=128, bmu=None) == _lib.FE_ERR_ARG and b"bad argument" in err()  # nulls come before H
    # forward
    for name in _FORWARD:
        assert _forward(lib, **{name: None}) == _lib.FE_ERR_ARG, name
        assert err().startswith(b"fe_sac_forward_streamed: bad argument"), name
    assert _forward(lib, count=-1) == _lib.FE_ERR_ARG and err().startswith(b"fe_sac_forward_streamed: bad argument")
    assert _forward(lib, actions=16) == _lib.FE_ERR_ARG
    assert err().startswith(b"fe_sac_forward_streamed: actions_out and log_probs_out need noise")
    for H in (32, 128, 300, 2048):
        assert _forward(lib, H=H) == _lib.FE_ERR_ARG
        assert err().startswith(b"fe_sac_forward_streamed: H must be 256, 512 or 1024"), err()
        assert b"fe_sac_forward runs H = 32, 64 and 128" in err(), err()
    assert _forward(lib, H=128, count=-1) == _lib.FE_ERR_ARG and b"bad argument" in err()
    # backward
    for name in _BACKWARD:
        assert _backward(lib, **{name: None}) == _lib.FE_ERR_ARG, name
        assert err().startswith(b"fe_sac_backward_streamed: bad argument"), name
    for kw in (dict(count=-1), dict(grads=None), dict(d_actions=None, d_log_probs=None)):
        assert _backward(lib, **kw) == _lib.FE_ERR_ARG, kw
        assert err().startswith(b"fe_sac_backward_streamed: bad argument"), kw
    for k in range(10):  # every field of fe_sac_grads is required
        ptrs = [16] * 10
        ptrs[k] = None
        assert _backward(lib, grads=_lib.FeSacGrads(*ptrs)) == _lib.FE_ERR_ARG, k
        assert err().startswith(b"fe_sac_backward_streamed: bad argument"), k
    for H in (32, 128, 300, 2048):
        assert _backward(lib, H=H) == _lib.FE_ERR_ARG
        assert err().startswith(b"fe_sac_backward_streamed: H must be 256, 512 or 1024"), err()
        assert b"fe_sac_backward runs H = 32, 64 and 128" in err(), err()
    assert _backward(lib, H=128, count=-1) == _lib.FE_ERR_ARG and b"bad argument" in err()


def test_the_old_entries_still_refuse_256():
    from finenvs_amd import _lib

    lib = _lib.load()
    g = _lib.FeSacGrads(*([16] * 10))
    assert lib.fe_sac_forward(16, 16, 16, 16, 16, 16, 16, 0.0, 16, 0.0, 256, 16, 16, 4, None, None, None, 16, 16,
                              None) == _lib.FE_ERR_ARG
    assert b"fe_sac_forward: H must be 32, 64 or 128 (got 256): the SAC head has no streamed or split kernel" \
        in lib.fe_last_error()
    assert lib.fe_sac_forward_p(16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 256, 16, 16, 4, None, None, None, 16, 16,
                                None) == _lib.FE_ERR_ARG
    assert b"fe_sac_forward: H must be 32, 64 or 128" in lib.fe_last_error()
    for entry, bias in ((lib.fe_sac_backward, 0.0), (lib.fe_sac_backward_p, 16)):
        assert entry(16, 16, 16, 16, 16, 16, 16, bias, 16, bias, 256, 16, 16, 4, 16, 16, 16, 16, 16, 16, C.byref(g),
                     None) == _lib.FE_ERR_ARG
        assert b"fe_sac_backward: H must be 32, 64 or 128 (got 256)" in lib.fe_last_error()
    assert lib.fe_sac_grad_workspace_floats(256, 4, 33) == -1


def test_check_actor_admits_the_large_sizes_only_when_asked():
    from finenvs_amd.sac import SACActorLSTM, check_actor

    with pytest.raises(ValueError, match="256.*streamed=True"):
        check_actor(SACActorLSTM(H=256, W=4))
    assert check_actor(SACActorLSTM(H=256, W=4), streamed=True) == 256
    assert check_actor(SACActorLSTM(H=1024, W=4), streamed=True) == 1024
    assert check_actor(SACActorLSTM(H=64, W=4), streamed=True) == 64  # the small sizes go the register-resident way
    for H in (2048, 48):
        with pytest.raises(ValueError, match=str(H)):
            check_actor(SACActorLSTM(H=H, W=4), streamed=True)
        with pytest.raises(ValueError, match=str(H)):
            check_actor(SACActorLSTM(H=H, W=4))
    with pytest.raises(ValueError, match="mu_layer"):
        check_actor(SACActorLSTM(H=256, W=4, A=2), streamed=True)


def test_a_large_actor_is_packed_fragment_major_by_pack_sac_weights_and_by_the_optimizer():
    from finenvs_amd import optim
    from finenvs_amd.rollout import lstm_fragment_major, lstm_pack
    from finenvs_amd.sac import SACActorLSTM, pack_sac_weights, unpack_last_layer

    torch.manual_seed(5)
    actor = SACActorLSTM(H=256, W=4)
    kind, H, segs, shapes = optim.network_segments(actor)
    assert (kind, H) == ("actor", 256)
    assert {s.name: s.kind for s in segs}["w_hh"] == optim.SEG_WHH_FRAGMENT
    assert {s.name: s.kind for s in segs}["w_l"] == optim.SEG_WL
    packed, scattered = pack_sac_weights(actor), optim.scatter_packed(actor)
    assert sorted(packed) == sorted(scattered) == ["bl", "bmu", "bstd", "whh", "wl", "wmu", "wstd", "wx"]
    for k in packed:
        assert packed[k].shape == scattered[k].shape == shapes[k], k
        assert torch.equal(packed[k], scattered[k]), k
    lstm = actor.lstm
    whh, _ = lstm_pack(lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0, 256)
    assert torch.equal(packed["whh"], lstm_fragment_major(whh, 256)) and not torch.equal(packed["whh"], whh)
    assert torch.equal(unpack_last_layer(packed["wl"]), actor.last_layer[0].weight.detach())
    # the small sizes keep the row-major form
    small = SACActorLSTM(H=64, W=4)
    lstm = small.lstm
    whh, _ = lstm_pack(lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0, 64)
    assert torch.equal(pack_sac_weights(small)["whh"], whh)
