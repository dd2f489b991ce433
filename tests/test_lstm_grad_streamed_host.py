"""CPU: the gradient half of the one-output LSTM head at H = 256 / 512 / 1024 -- the C ABI surface of
include/finenvs_amd_lstm_grad_streamed.h with the argument checks that need no device, the chunk size, the workspace
size, and ``check_head``'s ``streamed`` opt-in."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "finenvs_amd_lstm_grad_streamed.h")
SIZES = (256, 512, 1024)
WHO = b"fe_lstm_backward_streamed: "


def test_header_declares_exactly_the_streamed_signatures_and_the_library_exports_them():
    from finenvs_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(fe_[a-z0-9_]+)\s*\(", text))) == sorted(_lib.LSTM_STREAMED_GRAD_SIGNATURES)
    assert len(_lib.LSTM_STREAMED_GRAD_SIGNATURES) == 3
    others = (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.EVO_SIGNATURES) | set(_lib.REPLAY_SIGNATURES)
              | set(_lib.SAC_SIGNATURES) | set(_lib.CRITIC_SIGNATURES) | set(_lib.CRITIC_GRAD_SIGNATURES)
              | set(_lib.SAC_GRAD_SIGNATURES) | set(_lib.LSTM_GRAD_SIGNATURES))
    assert not set(_lib.LSTM_STREAMED_GRAD_SIGNATURES) & others
    lib = _lib.load()
    for name in _lib.LSTM_STREAMED_GRAD_SIGNATURES:
        assert hasattr(lib, name)
    assert lib.fe_version() == _lib.FE_ABI_VERSION == 5
    # the argument list of fe_lstm_backward exactly
    assert _lib.LSTM_STREAMED_GRAD_SIGNATURES["fe_lstm_backward_streamed"] == _lib.LSTM_GRAD_SIGNATURES["fe_lstm_backward"]


POINTERS = ("env", "lr32", "whh", "wx", "wout", "src", "pos", "outputs", "d_outputs", "workspace")


def _backward(lib, H=256, act=0, count=4, grads="ok", **null):
    """fe_lstm_backward_streamed on made-up non-null pointers (never dereferenced: every case here is refused first)."""
    from finenvs_amd import _lib

    p = {k: 16 for k in POINTERS}
    p.update(null)
    g = _lib.FeLstmGrads(*([16] * 6)) if grads == "ok" else grads
    return lib.fe_lstm_backward_streamed(p["env"], p["lr32"], p["whh"], p["wx"], p["wout"], H, act, p["src"], p["pos"],
                                         count, p["outputs"], p["d_outputs"], p["workspace"],
                                         None if g is None else C.byref(g), None)


def test_argument_checks_need_no_device():
    from finenvs_amd import _lib

    lib = _lib.load()
    for name in POINTERS:
        if name == "outputs":
            continue  # may be null without an activation; refused with tanh below
        assert _backward(lib, **{name: None}) == _lib.FE_ERR_ARG, name
        assert lib.fe_last_error().startswith(WHO + b"bad argument"), name
    for kw in (dict(grads=None), dict(count=-1)):
        assert _backward(lib, **kw) == _lib.FE_ERR_ARG, kw
        assert lib.fe_last_error().startswith(WHO + b"bad argument")
    for k in range(6):  # every field of fe_lstm_grads is required
        ptrs = [16] * 6
        ptrs[k] = None
        assert _backward(lib, grads=_lib.FeLstmGrads(*ptrs)) == _lib.FE_ERR_ARG, k
        assert lib.fe_last_error().startswith(WHO + b"bad argument")
    for H in (32, 128, 48, 2048):
        for act in (0, 2):
            assert _backward(lib, H=H, act=act) == _lib.FE_ERR_ARG
            msg = lib.fe_last_error()
            assert msg.startswith(WHO + b"H must be 256, 512 or 1024"), msg
            assert b"fe_lstm_backward " in msg, msg  # where the small sizes go
    for act in (1, -1, 3):  # clamp has no gradient to train on
        assert _backward(lib, act=act) == _lib.FE_ERR_ARG
        assert lib.fe_last_error().startswith(WHO + b"out_activation must be 0 (tanh) or 2 (none)")
    assert _backward(lib, act=0, outputs=None) == _lib.FE_ERR_ARG
    msg = lib.fe_last_error()
    assert msg.startswith(WHO) and b"needs outputs" in msg, msg
    # the order of fe_lstm_backward: the activation is judged before H
    assert _backward(lib, H=32, act=1) == _lib.FE_ERR_ARG
    assert b"out_activation" in lib.fe_last_error()


def test_chunk_pairs_is_a_function_of_h_and_w():
    from finenvs_amd import _lib

    lib = _lib.load()
    for H in SIZES:
        chunks = [lib.fe_lstm_streamed_grad_chunk_pairs(H, W) for W in (1, 4, 16, 390)]
        assert all(c > 0 and c % 32 == 0 for c in chunks), (H, chunks)
        assert all(b <= a for a, b in zip(chunks, chunks[1:])), (H, chunks)
        for W, c in zip((1, 4, 16, 390), chunks):  # the rule the header states
            stash = 4 * W * (6 * H + 32)
            assert c % 256 == 0 and c == max(256, (1 << 31) // stash // 256 * 256), (H, W, c)
    assert lib.fe_lstm_streamed_grad_chunk_pairs(1024, 4) == 21504
    for H, W in ((128, 4), (256, 0), (2048, 4), (48, 4), (256, -1)):
        assert lib.fe_lstm_streamed_grad_chunk_pairs(H, W) == -1, (H, W)


def test_workspace_size_is_monotone_and_constant_from_the_chunk_on():
    from finenvs_amd import _lib

    lib = _lib.load()
    floats = lib.fe_lstm_streamed_grad_workspace_floats
    for H in SIZES:
        for W in (4, 16):
            chunk = lib.fe_lstm_streamed_grad_chunk_pairs(H, W)
            counts = (0, 1, 31, 32, 33, chunk - 32, chunk, chunk + 1, 1 << 24)
            sizes = [floats(H, W, n) for n in counts]
            assert all(s > 0 for s in sizes)
            assert all(b >= a for a, b in zip(sizes, sizes[1:])), (H, W, sizes)
            assert sizes[6] == sizes[7] == sizes[8] and sizes[5] < sizes[6], (H, W, sizes)
            assert sizes[1] > sizes[0] and sizes[4] > sizes[3]
            # the stash stays within 2 GiB, and the whole workspace within 2.5 GiB
            assert 4 * chunk * W * (6 * H + 32) <= 1 << 31
            assert 4 * sizes[-1] <= (1 << 31) + (1 << 29)
        assert floats(H, 16, 1000) > floats(H, 4, 1000)
    for H, W, n in ((128, 4, 1), (48, 4, 1), (2048, 4, 1), (256, 0, 1), (256, 4, -1)):
        assert floats(H, W, n) == -1, (H, W, n)


def test_check_head_admits_the_large_sizes_only_when_asked():
    from finenvs_amd.lstm_head import LSTMHead, check_head

    with pytest.raises(ValueError, match="256"):
        check_head(LSTMHead(256, 4))
    assert check_head(LSTMHead(256, 4), streamed=True) == (256, "tanh")
    assert check_head(LSTMHead(1024, 4, "none"), streamed=True) == (1024, "none")
    assert check_head(LSTMHead(64, 4), streamed=True) == (64, "tanh")  # the small sizes go the register-resident way
    for H in (2048, 48):
        with pytest.raises(ValueError, match=str(H)):
            check_head(LSTMHead(H, 4), streamed=True)
