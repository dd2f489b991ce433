"""CPU: the SAC MLP actor -- the C ABI surface of include/finenvs_amd_mlp_sac.h with the argument checks that need no
device, the workspace size against the formula the header states, the window constants against the LDS rule, the fold
and the rank-two backward algebra against f64 torch, the module's ``state_dict`` keys, and the batch conditions of the
gradient cases of tests/test_mlp_sac_gpu.py (decided in tests/mlp_sac_cases.py from the f64 copy alone, for the seeds the
GPU file uses).  The refusals that read the env (A != 1, the window) are tests/test_mlp_sac_gpu.py's."""
import copy
import ctypes as C
import os
import re

import pytest
import torch

from tests import mlp_sac_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "finenvs_amd_mlp_sac.h")
P = 16  # a made-up non-null pointer, never dereferenced: every case here is refused first
F64 = torch.float64


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_exactly_the_mlp_sac_signatures_and_the_library_exports_them():
    from finenvs_amd import _lib
    from finenvs_amd.mlp_sac import MLP_SAC_GRAD_KEYS

    text = _header()
    assert sorted(set(re.findall(r"\b(fe_[a-z0-9_]+)\s*\(", text))) == sorted(_lib.MLP_SAC_SIGNATURES)
    assert sorted(_lib.MLP_SAC_SIGNATURES) == ["fe_env_rollout_mlp_sac", "fe_mlp_sac_backward", "fe_mlp_sac_forward",
                                               "fe_mlp_sac_grad_workspace_floats", "fe_mlp_sac_pack"]
    others = set()
    for name in dir(_lib):
        if name.endswith("SIGNATURES") and name != "MLP_SAC_SIGNATURES":
            others |= set(getattr(_lib, name))
    assert len(others) > 50 and not set(_lib.MLP_SAC_SIGNATURES) & others
    lib = _lib.load()
    for name, (_, args) in _lib.MLP_SAC_SIGNATURES.items():
        assert hasattr(lib, name)
        decl = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert len(decl.split(",")) == len(args), name  # one binding argument per declared parameter
    fields = re.search(r"typedef struct fe_mlp_sac_grads \{(.*?)\} fe_mlp_sac_grads;", text, flags=re.S).group(1)
    assert re.findall(r"\*(\w+);", fields) == [f for f, _ in _lib.FeMlpSacGrads._fields_] == list(MLP_SAC_GRAD_KEYS)
    fields = re.search(r"typedef struct fe_mlp_sac_weights \{(.*?)\} fe_mlp_sac_weights;", text, flags=re.S).group(1)
    assert re.findall(r"\*(\w+);", fields) == [f for f, _ in _lib.FeMlpSacWeights._fields_]
    assert int(re.search(r"#define FE_MLP_SAC_GRAD_CHUNK_PAIRS (\d+)", text).group(1)) == _lib.MLP_SAC_GRAD_CHUNK_PAIRS == 512
    assert int(re.search(r"#define FE_MLP_SAC_GRAD_MAX_GROUPS (\d+)", text).group(1)) == _lib.MLP_SAC_GRAD_MAX_GROUPS
    for H, W in _lib.MLP_SAC_MAX_WINDOW.items():
        assert int(re.search(rf"#define FE_MLP_SAC_MAX_WINDOW_H{H} (\d+)", text).group(1)) == W
    cites = open(HEADER).read()
    for ref in ("SAC/SAC_agent.py:244-279", "SAC/actor.py:106-120", "SAC/actor.py:51-61"):
        assert ref in cites, ref  # the reference lines the entries replace


def _weights(**null):
    from finenvs_amd import _lib

    p = {k: P for k, _ in _lib.FeMlpSacWeights._fields_}
    p.update(null)
    return _lib.FeMlpSacWeights(*(p[k] for k, _ in _lib.FeMlpSacWeights._fields_))


def _ref(x):
    return None if x is None else C.byref(x)


def _rollout(lib, H=32, act=0, K=2, w="ok", **over):
    p = {k: P for k in ("env", "lr32", "src", "pos", "rewards", "dones")}
    p.update(noise=None, actions=None, means=None, stds=None, src_out=None, pos_out=None)
    p.update(over)
    w = _weights() if w == "ok" else w
    return lib.fe_env_rollout_mlp_sac(p["env"], p["lr32"], _ref(w), H, act, K, p["src"], p["pos"], p["noise"], p["actions"],
                                      p["means"], p["stds"], p["rewards"], p["dones"], p["src_out"], p["pos_out"], None)


def _forward(lib, H=32, act=0, count=4, w="ok", **over):
    p = {k: P for k in ("env", "lr32", "src", "pos")}
    p.update(noise=None, actions=None, logp=None, means=P, stds=P)
    p.update(over)
    w = _weights() if w == "ok" else w
    return lib.fe_mlp_sac_forward(p["env"], p["lr32"], _ref(w), H, act, p["src"], p["pos"], count, p["noise"], p["actions"],
                                  p["logp"], p["means"], p["stds"], None)


def _backward(lib, H=32, act=0, count=4, w="ok", g="ok", **over):
    from finenvs_amd import _lib

    p = {k: P for k in ("env", "lr32", "src", "pos", "noise", "actions", "stds", "d_actions", "d_logp", "workspace")}
    p.update(over)
    w = _weights() if w == "ok" else w
    g = _lib.FeMlpSacGrads(*([P] * 8)) if g == "ok" else g
    return lib.fe_mlp_sac_backward(p["env"], p["lr32"], _ref(w), H, act, p["src"], p["pos"], count, p["noise"], p["actions"],
                                   p["stds"], p["d_actions"], p["d_logp"], p["workspace"], _ref(g), None)


def _pack(lib, H=32, W=4, **over):
    names = ("weight1", "w2", "b2", "wmu", "bmu", "wstd", "bstd", "w1t", "wpos", "vmu", "vstd", "cfold")
    p = {k: P for k in names}
    p.update(over)
    return lib.fe_mlp_sac_pack(*(p[k] for k in names[:7]), H, W, *(p[k] for k in names[7:]), None)


def test_argument_checks_need_no_device_and_come_in_the_documented_order():
    from finenvs_amd import _lib

    lib = _lib.load()
    ERR = _lib.FE_ERR_ARG
    calls = {"fe_env_rollout_mlp_sac": (_rollout, ("env", "lr32", "src", "pos", "rewards", "dones")),
             "fe_mlp_sac_forward": (_forward, ("env", "lr32", "src", "pos")),
             "fe_mlp_sac_backward": (_backward, ("env", "lr32", "src", "pos", "noise", "actions", "stds", "workspace"))}
    for name, (call, required) in calls.items():
        who = name.encode()
        for ptr in required:
            assert call(lib, **{ptr: None}) == ERR, (name, ptr)
            assert lib.fe_last_error() == who + b": bad argument", (name, ptr)
        assert call(lib, w=None) == ERR and lib.fe_last_error() == who + b": bad argument"
        for field, _ in _lib.FeMlpSacWeights._fields_:
            assert call(lib, w=_weights(**{field: None})) == ERR, (name, field)
            assert lib.fe_last_error() == who + b": bad argument"
        for H in (16, 48, 256):
            assert call(lib, H=H) == ERR
            assert lib.fe_last_error() == who + b": H must be 32, 64 or 128 (got %d)" % H
        for act in (-1, 3):
            assert call(lib, act=act) == ERR
            assert lib.fe_last_error() == who + b": activation must be 0 (ELU), 1 (ReLU) or 2 (tanh)"
        # the order: a null pointer before H, H before the activation, the activation before the count
        assert call(lib, H=48, **{required[-1]: None}) == ERR and b"bad argument" in lib.fe_last_error()
        assert call(lib, H=48, act=7) == ERR and b"H must be" in lib.fe_last_error()
        small = {"K": 0} if call is _rollout else {"count": -1}
        assert call(lib, act=7, **small) == ERR and b"activation must be" in lib.fe_last_error()
        assert call(lib, **small) == ERR and who + b": bad argument" in lib.fe_last_error()
    # the rollout: K < 1 before the states_*_out pair
    who = b"fe_env_rollout_mlp_sac"
    assert _rollout(lib, K=0, src_out=P) == ERR and who + b": bad argument" in lib.fe_last_error()
    for one in ("src_out", "pos_out"):
        assert _rollout(lib, **{one: P}) == ERR
        assert lib.fe_last_error() == who + b": states_src_out and states_pos_out go together"
    # the forward: count < 0 before the outputs that need noise
    who = b"fe_mlp_sac_forward"
    assert _forward(lib, count=-1, actions=P) == ERR and who + b": bad argument" in lib.fe_last_error()
    for out in ("actions", "logp"):
        assert _forward(lib, **{out: P}) == ERR
        assert lib.fe_last_error() == who + b": actions_out / log_probs_out need noise"
    # the backward: its gradient struct, then both upstream gradients null
    who = b"fe_mlp_sac_backward"
    assert _backward(lib, g=None) == ERR and lib.fe_last_error() == who + b": bad argument"
    for k in range(8):
        ptrs = [P] * 8
        ptrs[k] = None
        assert _backward(lib, g=_lib.FeMlpSacGrads(*ptrs)) == ERR and lib.fe_last_error() == who + b": bad argument", k
    assert _backward(lib, d_actions=None, d_logp=None) == ERR
    assert lib.fe_last_error() == who + b": d_actions and d_log_probs are both null: nothing to compute"
    assert _backward(lib, d_actions=None, d_logp=None, count=-1) == ERR and who + b": bad argument" in lib.fe_last_error()
    # the pack
    who = b"fe_mlp_sac_pack"
    for ptr in ("weight1", "w2", "b2", "wmu", "bmu", "wstd", "bstd", "w1t", "wpos", "vmu", "vstd", "cfold"):
        assert _pack(lib, **{ptr: None}) == ERR and lib.fe_last_error() == who + b": bad argument", ptr
    assert _pack(lib, H=48) == ERR and lib.fe_last_error() == who + b": H must be 32, 64 or 128 (got 48)"
    assert _pack(lib, W=0) == ERR and lib.fe_last_error() == who + b": W must be >= 1 (got 0)"


def test_the_three_translation_units_write_one_error_buffer():
    from finenvs_amd import _lib

    lib = _lib.load()
    assert _forward(lib, H=48) == _lib.FE_ERR_ARG  # set by fe_mlp_sac.hip
    assert lib.fe_last_error() == b"fe_mlp_sac_forward: H must be 32, 64 or 128 (got 48)"
    assert lib.fe_mlp2_forward(None, P, None, 32, 0, 0, P, P, 4, P, None) == _lib.FE_ERR_ARG  # then one set by fe_env.hip
    assert lib.fe_last_error() == b"fe_mlp2_forward: bad argument"
    assert _backward(lib, count=-1) == _lib.FE_ERR_ARG  # and back
    assert lib.fe_last_error() == b"fe_mlp_sac_backward: bad argument (count must be >= 0)"


def _formula(H, W, count):
    """The workspace size as include/finenvs_amd_mlp_sac.h states it."""
    if count == 0:
        return 0
    blocks, splits, F = -(-count // 32), -(-count // 512), 32 * -(-(4 * W + 2) // 32)
    waves = 4 * min(-(-blocks // 4), 256)
    return 32 * blocks * H + splits * H * F + waves * 2 * (H + 4)


def test_workspace_size_equals_the_header_formula_up_to_2_to_the_40():
    from finenvs_amd import _lib

    lib = _lib.load()
    counts = (0, 1, 31, 32, 33, 256, 511, 512, 513, 1023, 1024, 1025, 4097, 32767, 32768, 32769, 65536, 65537, 70001, 1 << 20,
              1 << 24, (1 << 31) + 5, 1 << 40)
    for H in (32, 64, 128):
        for W in (1, 4, 7, 8, 16, 40, 72, 144, 304):
            sizes = [lib.fe_mlp_sac_grad_workspace_floats(H, W, n) for n in counts]
            assert sizes == [_formula(H, W, n) for n in counts], (H, W)
            assert all(b >= a for a, b in zip(sizes, sizes[1:])), (H, W, sizes)
            assert sizes[0] == 0 < sizes[1]
            # one H-float row per pair, not the two-layer head's three
            n = 1 << 20
            assert lib.fe_mlp2_grad_workspace_floats(H, W, n) - lib.fe_mlp_sac_grad_workspace_floats(H, W, n) >= 2 * n * H
    for H, W, n in ((48, 4, 1), (16, 4, 1), (256, 4, 1), (32, 0, 1), (32, 4, -1)):
        assert lib.fe_mlp_sac_grad_workspace_floats(H, W, n) == -1
    assert "32 blocks H   +   splits H F   +   waves 2 (H + 4)" in open(HEADER).read()
    assert "F = 32 ceil((4W + 2) / 32)" in open(HEADER).read()


def _lds_bytes(W, H, pairs=128):
    """The LDS rule written out (csrc/fe_rollout_kernels.h::mlp_lds_bytes at one asset, plus v_s and the two constants
    padded to 16 bytes): the tile's state, the redrawn day and the action per pair, then the weight image."""
    kp = -(-(4 * W) // 32) * 32 + 4
    tile = pairs * 8 + pairs * 8 + pairs * 8 + pairs * 4 + pairs * 4 + pairs * 4
    b = (tile + 7) // 8 * 8 + pairs * 8 + pairs * 4
    b = (b + 15) // 16 * 16 + H * kp * 4 + 3 * H * 4
    return (b + 15) // 16 * 16 + (H + 4) * 4


def test_the_window_constants_are_the_lds_rule():
    from finenvs_amd import _lib

    for H, W in _lib.MLP_SAC_MAX_WINDOW.items():
        assert _lds_bytes(W, H) <= 160 * 1024 < _lds_bytes(W + 1, H), (H, W, _lds_bytes(W, H), _lds_bytes(W + 1, H))
    assert _lib.MLP_SAC_MAX_WINDOW[128] == 72 > _lib.MLP2_MAX_WINDOW[128]  # wider than the twin critics' limit of 40


def test_state_dict_keys_are_the_references():
    from finenvs_amd.mlp_sac import MLP_SAC_STATE_DICT_KEYS, SACActorMLP, check_mlp_sac_actor, mlp_sac_parameters

    a = SACActorMLP(64, 7, "tanh", starting_alpha=0.5)
    assert list(a.state_dict()) == ["network.0.weight", "network.0.bias", "network.2.weight", "network.2.bias",
                                    "mu_layer.weight", "mu_layer.bias", "std_layer.weight", "std_layer.bias"]
    assert list(a.state_dict()) == list(MLP_SAC_STATE_DICT_KEYS) == [n for n, _ in a.named_parameters()]
    assert [tuple(p.shape) for p in mlp_sac_parameters(a)] == [(64, 35), (64,), (64, 64), (64,), (1, 64), (1,), (1, 64), (1,)]
    assert check_mlp_sac_actor(a) == (64, 7, "tanh")
    assert isinstance(a.network[3], torch.nn.Identity) and len(a.network) == 4
    assert abs(float(a.log_alpha.detach().exp()) - 0.5) < 1e-7 and a.log_alpha.requires_grad and a.target_entropy == -1.0
    assert "log_alpha" not in dict(a.named_parameters())
    b = SACActorMLP(64, 7, "tanh")
    b.load_state_dict(a.state_dict())
    x = torch.randn(5, 7, 5)
    assert torch.equal(a(x), b(x)) and torch.equal(a(x), a(x.reshape(5, 35)))
    eps = torch.randn(5, 1)
    assert torch.equal(a.step_actions(x, eps)[:-1], a.get_actions_and_log_probs(x, eps)[0][:-1].detach())
    assert torch.equal(a.step_actions(x, eps)[-1], a.get_distribution(x).loc[-1].detach())
    bad = SACActorMLP(64, 7)
    bad.network[3] = torch.nn.Tanh()
    with pytest.raises(ValueError, match="no activation"):
        check_mlp_sac_actor(bad)


@pytest.mark.parametrize("H,W", [(32, 4), (64, 7), (128, 40), (128, 4)])
def test_fold_head_against_the_layer_by_layer_f64_module(H, W):
    from finenvs_amd.mlp_sac import SACActorMLP, fold_head

    torch.manual_seed(H + W)
    a = SACActorMLP(H, W).double()
    x = torch.randn(257, 5 * W, dtype=F64)
    with torch.no_grad():
        a1 = a.network[1](a.network[0](x))
        z = a.network(x)
        mu, q = a.mu_layer(z).reshape(-1), a.std_layer(z).reshape(-1)
        f = fold_head(a)
        assert all(t.dtype is F64 for t in f.values())
        mu_f, q_f = f["c_mu"] + a1 @ f["v_mu"], f["c_s"] + a1 @ f["v_s"]
    for got, want in ((mu_f, mu), (q_f, q)):
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    f32 = fold_head(copy.deepcopy(a).float())  # formed in f64 from the f32 parameters, rounded once
    assert all(t.dtype is torch.float32 for t in f32.values())
    a32 = copy.deepcopy(a).float().double()
    assert torch.equal(f32["v_mu"], fold_head(a32)["v_mu"].float())


@pytest.mark.parametrize("activation", ["elu", "relu", "tanh"])
def test_reference_backward_against_f64_autograd(activation):
    from finenvs_amd.mlp_sac import SACActorMLP, mlp_sac_parameters, reference_backward

    H, W, B = 32, 4, 129
    torch.manual_seed(11)
    a = SACActorMLP(H, W, activation).double()
    with torch.no_grad():
        a.std_layer.bias.add_(-0.5)
    x = torch.randn(B, W, 5, dtype=F64)
    eps, c = torch.randn(B, 1, dtype=F64), torch.rand(B, 1, dtype=F64) + 0.5
    for kind in cases.KINDS:
        for p in a.parameters():
            p.grad = None
        actions, log_probs = a.get_actions_and_log_probs(x, eps)
        if kind == "chained":  # a stand-in critic: any smooth function of the actions
            loss = -((torch.sin(actions) * c).sum() - 0.7 * log_probs.sum()) / B
        elif kind == "log_probs":
            loss = (log_probs * c).sum()
        else:
            loss = actions.sum()
        ga, gl = torch.autograd.grad(loss, (actions, log_probs), retain_graph=True, allow_unused=True)
        loss.backward()
        got = reference_backward(a, x, eps, ga, gl)
        for name, g, p in zip(cases.NAMES, got, mlp_sac_parameters(a)):
            assert g.shape == p.grad.shape, name
            assert float((g - p.grad).abs().max()) <= 1e-10 * float(p.grad.abs().max()), (kind, name)


@pytest.mark.parametrize("H,W,B,activation", cases.SHAPES)
def test_the_gpu_gradient_cases_meet_their_batch_conditions(H, W, B, activation):
    """Every condition is asserted inside ``cases.conditioned``; here: the seed search ends, and what it returns is what
    the GPU file expects."""
    case = cases.conditioned(H, W, B, activation)
    assert tuple(case["states"].shape) == (B, W, 5) and case["states"].dtype is F64
    assert all(p.device.type == "cpu" for m in (case["actor"],) + case["critics"] for p in m.parameters())
    for kind in cases.KINDS:
        keep = case["keep"][kind]
        assert tuple(keep.shape) == (B, 1) and float(keep.sum()) >= 0.98 * B
        assert len(case["g64"][kind][1]) == 8 and all(g.dtype is F64 for g in case["g64"][kind][1])
    print(f"({H}, {W}, {B}, {activation}): seed {case['seed']}, dropped {B - int(case['keep']['chained'].sum())} samples")
