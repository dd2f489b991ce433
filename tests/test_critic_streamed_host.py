"""CPU: the twin LSTM critics at H = 256 / 512 / 1024 -- the C ABI surface of include/finenvs_amd_critic_streamed.h
with the argument checks that need no device, the workspace size, ``check_critic``'s ``streamed`` opt-in and the packed
layout ``FusedAdam`` keeps for such a critic."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "finenvs_amd_critic_streamed.h")
SIZES = (256, 512, 1024)


def test_header_declares_exactly_the_streamed_signatures_and_the_library_exports_them():
    from finenvs_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(fe_[a-z0-9_]+)\s*\(", text))) == sorted(_lib.CRITIC_STREAMED_SIGNATURES)
    assert len(_lib.CRITIC_STREAMED_SIGNATURES) == 5
    others = (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.CRITIC_SIGNATURES) | set(_lib.CRITIC_GRAD_SIGNATURES)
              | set(_lib.LSTM_GRAD_SIGNATURES) | set(_lib.LSTM_STREAMED_GRAD_SIGNATURES) | set(_lib.OPTIM_SIGNATURES)
              | set(_lib.REPLAY_CURSOR_SIGNATURES))
    assert not set(_lib.CRITIC_STREAMED_SIGNATURES) & others
    lib = _lib.load()
    for name, (res, args) in _lib.CRITIC_STREAMED_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    # each entry takes the argument list of its register-resident namesake
    s = _lib.CRITIC_STREAMED_SIGNATURES
    assert s["fe_twin_q_forward_streamed"] == _lib.CRITIC_SIGNATURES["fe_twin_q_forward"]
    assert s["fe_twin_q_target_streamed"] == _lib.CRITIC_SIGNATURES["fe_twin_q_target"]
    assert s["fe_twin_q_target_streamed_c"] == _lib.REPLAY_CURSOR_SIGNATURES["fe_twin_q_target_c"]
    assert s["fe_twin_q_backward_streamed"] == _lib.CRITIC_GRAD_SIGNATURES["fe_twin_q_backward"]
    assert s["fe_twin_q_streamed_grad_workspace_floats"] == _lib.CRITIC_GRAD_SIGNATURES["fe_twin_q_grad_workspace_floats"]
    assert lib.fe_version() == _lib.FE_ABI_VERSION == 5


def test_workspace_size_is_monotone_and_its_stash_constant_from_the_chunk_on():
    from finenvs_amd import _lib

    lib = _lib.load()
    floats = lib.fe_twin_q_streamed_grad_workspace_floats
    for H, W, n in ((32, 4, 1), (128, 4, 1), (300, 4, 1), (256, 0, 1), (256, 4, -1)):
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
            # d_actions is written in place: nothing per pair past the chunk, and the stash is one critic's, not two
            assert sizes[7] == sizes[8] == sizes[9], (H, W, sizes)
            assert sizes == [lib.fe_lstm_streamed_grad_workspace_floats(H, W, n) for n in counts]
            assert 4 * sizes[-1] <= (1 << 31) + (1 << 29)


def _weights(**null):
    from finenvs_amd import _lib

    f = dict(whh=16, wx=16, wout=16, bout=16)
    f.update(null)
    return _lib.FeCriticWeights(f["whh"], f["wx"], f["wout"], f["bout"])


def _ring(**kw):
    from finenvs_amd import _lib

    f = dict(capacity=64, num_assets=1, reserved=0, state_src=16, state_pos=16, next_src=16, next_pos=16, actions=16,
             rewards=16, dones=16, errors=16)
    f.update(kw)
    return _lib.FeReplayRing(*(f[k] for k, _ in _lib.FeReplayRing._fields_))


def _forward(lib, H=256, count=4, c1=None, c2=None, **null):
    p = {k: 16 for k in ("env", "lr32", "src", "pos", "actions", "q1", "q2")}
    p.update(null)
    c1, c2 = c1 or _weights(), c2 or _weights()
    return lib.fe_twin_q_forward_streamed(p["env"], p["lr32"], C.byref(c1), C.byref(c2), H, p["src"], p["pos"],
                                          p["actions"], count, p["q1"], p["q2"], None)


def _target(lib, H=256, count=4, cursor=False, ring=None, head=8, size=8, noise=None, log_probs=None, alpha=None, **null):
    p = {k: 16 for k in ("env", "lr32", "indices", "next_actions", "y", "q1", "q2")}
    p.update(null)
    c1, c2, ring = _weights(), _weights(), ring or _ring()
    tail = (p["indices"], count, p["next_actions"], noise, 0.2, 0.5, log_probs, alpha, 0.99, 1.0, p["y"], p["q1"], p["q2"], None)
    if cursor is not False:
        return lib.fe_twin_q_target_streamed_c(p["env"], p["lr32"], C.byref(c1), C.byref(c2), H, C.byref(ring), cursor, *tail)
    return lib.fe_twin_q_target_streamed(p["env"], p["lr32"], C.byref(c1), C.byref(c2), H, C.byref(ring), head, size, *tail)


def _backward(lib, H=256, count=4, c1="ok", g1="ok", g2="ok", dq1=16, dq2=16, da=16, **null):
    from finenvs_amd import _lib

    p = {k: 16 for k in ("env", "lr32", "src", "pos", "actions", "workspace")}
    p.update(null)
    c1 = _weights() if c1 == "ok" else c1
    c2 = _weights()
    g1 = _lib.FeCriticGrads(*([16] * 6)) if g1 == "ok" else g1
    g2 = _lib.FeCriticGrads(*([16] * 6)) if g2 == "ok" else g2
    ref = lambda x: None if x is None else C.byref(x)  # noqa: E731
    return lib.fe_twin_q_backward_streamed(p["env"], p["lr32"], ref(c1), C.byref(c2), H, p["src"], p["pos"], p["actions"],
                                           count, dq1, dq2, p["workspace"], ref(g1), ref(g2), da, None)


def test_the_new_entries_refuse_without_a_device():
    """Made-up non-null pointers, never dereferenced: every case here is refused first."""
    from finenvs_amd import _lib

    lib = _lib.load()
    err = lambda: lib.fe_last_error()  # noqa: E731
    # forward
    for name in ("env", "lr32", "src", "pos", "actions", "q1", "q2"):
        assert _forward(lib, **{name: None}) == _lib.FE_ERR_ARG, name
        assert err().startswith(b"fe_twin_q_forward_streamed: bad argument"), name
    assert _forward(lib, count=-1) == _lib.FE_ERR_ARG
    assert _forward(lib, c2=_weights(bout=None)) == _lib.FE_ERR_ARG and b"bad argument" in err()
    for H in (32, 128, 300, 2048):
        assert _forward(lib, H=H) == _lib.FE_ERR_ARG
        assert err().startswith(b"fe_twin_q_forward_streamed: H must be 256, 512 or 1024"), err()
    # targets, by value and by cursor
    for cursor in (False, 16):
        for name in ("env", "lr32", "indices", "next_actions", "y", "q1", "q2"):
            assert _target(lib, cursor=cursor, **{name: None}) == _lib.FE_ERR_ARG, name
            assert err().startswith(b"fe_twin_q_target_streamed: bad argument"), name
        assert _target(lib, cursor=cursor, ring=_ring(next_src=None)) == _lib.FE_ERR_ARG
        assert _target(lib, cursor=cursor, noise=16, log_probs=16, alpha=16) == _lib.FE_ERR_ARG
        assert err().startswith(b"fe_twin_q_target_streamed: smooth_noise (TD3) and log_probs (SAC) are exclusive")
        assert _target(lib, cursor=cursor, log_probs=16) == _lib.FE_ERR_ARG
        assert err().startswith(b"fe_twin_q_target_streamed: log_probs (SAC) need alpha")
        assert _target(lib, cursor=cursor, H=128) == _lib.FE_ERR_ARG
        assert err().startswith(b"fe_twin_q_target_streamed: H must be 256, 512 or 1024"), err()
    assert _target(lib, cursor=None) == _lib.FE_ERR_ARG and err().startswith(b"fe_twin_q_target_streamed_c: null cursor")
    # backward
    for name in ("env", "lr32", "src", "pos", "actions", "workspace"):
        assert _backward(lib, **{name: None}) == _lib.FE_ERR_ARG, name
        assert err().startswith(b"fe_twin_q_backward_streamed: bad argument"), name
    for kw in (dict(count=-1), dict(c1=None), dict(c1=_weights(wx=None)), dict(g1=None, da=None), dict(g2=None, da=None)):
        assert _backward(lib, **kw) == _lib.FE_ERR_ARG, kw
        assert err().startswith(b"fe_twin_q_backward_streamed: bad argument"), kw
    for k in range(6):  # every field of a given fe_critic_grads is required
        ptrs = [16] * 6
        ptrs[k] = None
        assert _backward(lib, g1=_lib.FeCriticGrads(*ptrs)) == _lib.FE_ERR_ARG, k
    for H in (32, 128, 300):
        assert _backward(lib, H=H) == _lib.FE_ERR_ARG
        assert err().startswith(b"fe_twin_q_backward_streamed: H must be 256, 512 or 1024"), err()


def test_the_old_entries_still_refuse_the_large_sizes():
    from finenvs_amd import _lib

    lib = _lib.load()
    w, g = _weights(), _lib.FeCriticGrads(*([16] * 6))
    assert lib.fe_twin_q_forward(16, 16, C.byref(w), C.byref(w), 256, 16, 16, 16, 4, 16, 16, None) == _lib.FE_ERR_ARG
    assert b"fe_twin_q_forward: H must be 32, 64 or 128 (got 256): the twin critic has no streamed or split kernel" \
        in lib.fe_last_error()
    ring = _ring()
    assert lib.fe_twin_q_target(16, 16, C.byref(w), C.byref(w), 256, C.byref(ring), 8, 8, 16, 4, 16, None, 0.2, 0.5, None,
                                None, 0.99, 1.0, 16, 16, 16, None) == _lib.FE_ERR_ARG
    assert b"fe_twin_q_target: H must be 32, 64 or 128" in lib.fe_last_error()
    assert lib.fe_twin_q_backward(16, 16, C.byref(w), C.byref(w), 256, 16, 16, 16, 4, 16, 16, 16, C.byref(g), C.byref(g), 16,
                                  None) == _lib.FE_ERR_ARG
    assert b"fe_twin_q_backward: H must be 32, 64 or 128" in lib.fe_last_error()
    assert lib.fe_twin_q_grad_workspace_floats(256, 4, 33) == -1


def test_check_critic_admits_the_large_sizes_only_when_asked():
    from finenvs_amd.critic import CriticLSTM, check_critic

    with pytest.raises(ValueError, match="256.*streamed=True"):
        check_critic(CriticLSTM(256, 4))
    assert check_critic(CriticLSTM(256, 4), streamed=True) == 256
    assert check_critic(CriticLSTM(1024, 4), streamed=True) == 1024
    assert check_critic(CriticLSTM(64, 4), streamed=True) == 64  # the small sizes go the register-resident way
    for H in (2048, 48):
        with pytest.raises(ValueError, match=str(H)):
            check_critic(CriticLSTM(H, 4), streamed=True)


def test_a_large_critic_is_packed_fragment_major_by_the_optimizer_and_by_pack_critic_weights():
    from finenvs_amd import optim
    from finenvs_amd.critic import CriticLSTM, pack_critic_weights
    from finenvs_amd.rollout import lstm_fragment_major, lstm_pack

    torch.manual_seed(5)
    critic = CriticLSTM(256, 4)
    kind, H, segs, shapes = optim.network_segments(critic)
    assert (kind, H) == ("critic", 256)
    assert {s.name: s.kind for s in segs}["w_hh"] == optim.SEG_WHH_FRAGMENT
    assert {s.name: s.cols for s in segs}["w_ih"] == 6
    packed, scattered = pack_critic_weights(critic), optim.scatter_packed(critic)
    assert sorted(packed) == sorted(scattered) == ["bout", "whh", "wout", "wx"]
    for k in packed:
        assert packed[k].shape == scattered[k].shape == shapes[k], k
        assert torch.equal(packed[k], scattered[k]), k
    lstm = critic.lstm
    whh, _ = lstm_pack(lstm.weight_ih_l0[:, :5], lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0, 256)
    assert torch.equal(packed["whh"], lstm_fragment_major(whh, 256)) and not torch.equal(packed["whh"], whh)
    # the small sizes keep the row-major form
    small = CriticLSTM(64, 4)
    lstm = small.lstm
    whh, _ = lstm_pack(lstm.weight_ih_l0[:, :5], lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0, 64)
    assert torch.equal(pack_critic_weights(small)["whh"], whh)
