"""CPU: what the six descriptor front ends -- ``FusedSACRollout`` / ``FusedMLPSACRollout``, ``FusedTwinCritic`` /
``FusedTwinMLPCritic``, ``FusedLSTMHead`` / ``FusedMLPHead`` / ``FusedMLP2Head`` -- hand to the C ABI, and what they refuse
and in which order, without a device: a recording object stands in for ``env._lib`` and the env is a namespace on the CPU.

A trace is the list of native calls one Python call made, one string per call: the entry's name, then one word per
argument -- an integer or float scalar as its value (a by-value bias as the name of the parameter it equals), a null
pointer as ``None``, a struct passed by reference as ``&`` and its ctypes class, a pointer as the name of the tensor of
the test whose ``data_ptr()`` it is (``p``: some other buffer, e.g. packed weights or a workspace).  The expected traces
are literals: a front end that reorders, drops or re-types an argument, launches where it must not (an empty batch, a
frozen critic, an unused output) or picks another entry fails here.  In the empty-batch cases the sizing queries
(``*_workspace_floats``: host arithmetic, no launch) are left out of the trace: the rule is that nothing launches."""
import ctypes as C
import types

import pytest
import torch

from finenvs_amd import _lib

SIGNATURES = {}
for _name in dir(_lib):
    if _name.endswith("SIGNATURES"):
        SIGNATURES.update(getattr(_lib, _name))

H, W, B, K, N = 32, 4, 5, 2, 3
WORKSPACE_FLOATS = 64


class RecordingLib:
    """Stands in for the loaded library: accepts exactly the bound entries, checks the argument count against the
    binding, records the call and reports success."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name not in SIGNATURES:
            raise AttributeError(name)
        argtypes = SIGNATURES[name][1]

        def entry(*args):
            assert len(args) == len(argtypes), f"{name}: {len(args)} arguments for {len(argtypes)} parameters"
            self.calls.append((name, args))
            return WORKSPACE_FLOATS if name.endswith("_workspace_floats") else 0

        return entry


def make_env(A=1, evaluate=False):
    env = types.SimpleNamespace(
        num_envs=N, num_assets=A, num_intervals=W, _dev=torch.device("cpu"), _lib=RecordingLib(), _handle=1,
        _stream=lambda: None, redraw="device", evaluate=evaluate, _binding_epoch=0, _generation=0,
        _sync_public_views=lambda: None, _log_return_f32=torch.zeros(8))
    # what evaluate_returns reads: every env has finished
    env._counters = torch.tensor([N])
    env.episode_returns = torch.arange(N, dtype=torch.float64)
    env.reset_evaluation_metrics = lambda: None
    return env


def normalise(calls, labels, skip_sizing=False):
    pointers = {t.data_ptr(): k for k, t in labels.items() if isinstance(t, torch.Tensor) and t.numel()}
    floats = {float(v): k for k, v in labels.items() if isinstance(v, float)}
    pointers[1] = "env"
    out = []
    for name, args in calls:
        if skip_sizing and name.endswith("_workspace_floats"):
            continue
        words = []
        for a, t in zip(args, SIGNATURES[name][1]):
            if a is None:
                words.append("None")
            elif t is C.c_void_p:
                assert isinstance(a, int), (name, a)
                words.append(pointers.get(a, "p"))
            elif t in (C.c_float, C.c_double):
                assert isinstance(a, float), (name, a)
                words.append(floats.get(a, repr(a)))
            elif t in (C.c_int32, C.c_int64, C.c_uint64, C.c_int):
                assert isinstance(a, int) and not isinstance(a, bool), (name, a)
                words.append(str(a))
            else:  # a struct by reference
                words.append("&" + type(a._obj).__name__)
        out.append(name + ": " + " ".join(words))
    return out


def traced(env, fn, labels=lambda out: {}, skip_sizing=False):
    env._lib.calls.clear()
    out = fn()
    named = dict(labels(out), lr32=env._log_return_f32)
    return normalise(env._lib.calls, named, skip_sizing), out


def descriptors(count=B, A=1):
    return torch.arange(count, dtype=torch.int64), torch.zeros((count, A), dtype=torch.float64)


# ---------------------------------------------------------------- SAC actors
def lstm_sac(env, H=H):
    from finenvs_amd.sac import FusedSACRollout, SACActorLSTM

    torch.manual_seed(0)
    actor = SACActorLSTM(H=H, W=W)
    return actor, FusedSACRollout(env, actor, streamed=H > 128)


def mlp_sac(env):
    from finenvs_amd.mlp_sac import FusedMLPSACRollout, SACActorMLP

    torch.manual_seed(0)
    actor = SACActorMLP(H, W)
    return actor, FusedMLPSACRollout(env, actor)


def sac_labels(actor, roll, **more):
    named = dict(more, obs_src=roll.obs_src, obs_pos=roll.obs_pos, bmu=float(actor.mu_layer.bias.detach()),
                 bstd=float(actor.std_layer.bias.detach()))
    if roll.means is not None:
        named["means"] = roll.means
    if roll.stds is not None:
        named["stds"] = roll.stds
    return named


def sample_and_backward(roll, src, pos, noise):
    actions, log_probs = roll.sample(src, pos, noise)
    (actions.sum() + log_probs.sum()).backward()
    return actions, log_probs


LSTM_SAC_WEIGHTS = "env lr32 p p p p p bmu p bstd 32"
MLP_SAC_WEIGHTS = "env lr32 &FeMlpSacWeights 32 0"
MLP_SAC_PACK = "fe_mlp_sac_pack: p p p p p p p 32 4 p p p p p None"


def test_sac_lstm_traces():
    env = make_env()
    assert env._lib.calls == []
    actor, roll = lstm_sac(env)
    assert normalise(env._lib.calls, sac_labels(actor, roll)) == ["fe_env_describe: env obs_src obs_pos None"]
    src, pos = descriptors()
    noise = torch.randn((B, 1))

    trace, (actions, log_probs) = traced(
        env, lambda: sample_and_backward(roll, src, pos, noise),
        lambda out: sac_labels(actor, roll, src=src, pos=pos, noise=noise, actions=out[0], log_probs=out[1],
                               last_means=roll.last["means"], last_stds=roll.last["stds"]))
    assert trace == [
        f"fe_sac_forward: {LSTM_SAC_WEIGHTS} src pos 5 noise actions log_probs last_means last_stds None",
        "fe_sac_grad_workspace_floats: 32 4 5",
        f"fe_sac_backward: {LSTM_SAC_WEIGHTS} src pos 5 noise actions last_stds p p p &FeSacGrads None",
    ]
    assert actions.shape == log_probs.shape == (B, 1)
    assert all(p.grad is not None for p in actor.parameters())

    trace, out = traced(env, lambda: roll.forward(src, pos),
                        lambda out: sac_labels(actor, roll, src=src, pos=pos, fwd_means=out[2], fwd_stds=out[3]))
    assert trace == [f"fe_sac_forward: {LSTM_SAC_WEIGHTS} src pos 5 None None None fwd_means fwd_stds None"]
    assert out[0] is None and out[1] is None

    rollout_noise = torch.randn((K, N, 1))
    trace, _ = traced(env, lambda: roll.run(K, noise=rollout_noise),
                      lambda out: sac_labels(actor, roll, noise=rollout_noise, actions=out[0], rewards=out[1], dones=out[2]))
    assert trace == [f"fe_env_rollout_sac: {LSTM_SAC_WEIGHTS} 2 obs_src obs_pos noise actions None None rewards dones None "
                     "None None"]
    trace, _ = traced(env, lambda: roll.run(K),
                      lambda out: sac_labels(actor, roll, actions=out[0], rewards=out[1], dones=out[2]))
    assert trace == [f"fe_env_rollout_sac: {LSTM_SAC_WEIGHTS} 2 obs_src obs_pos None actions None None rewards dones None "
                     "None None"]
    trace, _ = traced(env, lambda: roll.run(K, record_means=True, record_stds=True),
                      lambda out: sac_labels(actor, roll, actions=out[0], rewards=out[1], dones=out[2]))
    assert trace == [f"fe_env_rollout_sac: {LSTM_SAC_WEIGHTS} 2 obs_src obs_pos None actions means stds rewards dones None "
                     "None None"]
    assert roll.means.shape == roll.stds.shape == (K, N, 1)
    assert env._generation == 3

    # an empty batch packs nothing and launches nothing, in either direction
    empty_src, empty_pos = descriptors(0)
    trace, (actions, _) = traced(env, lambda: sample_and_backward(roll, empty_src, empty_pos, torch.zeros((0, 1))),
                                 skip_sizing=True)
    assert trace == [] and actions.shape == (0, 1)


def test_sac_lstm_streamed_traces():
    """H = 256: the ``_streamed`` entries, with both output biases read on the device."""
    env = make_env()
    actor, roll = lstm_sac(env, H=256)
    src, pos = descriptors()
    noise = torch.randn((B, 1))
    weights = "env lr32 p p p p p p p p 256"
    trace, _ = traced(
        env, lambda: sample_and_backward(roll, src, pos, noise),
        lambda out: sac_labels(actor, roll, src=src, pos=pos, noise=noise, actions=out[0], log_probs=out[1],
                               last_means=roll.last["means"], last_stds=roll.last["stds"]))
    assert trace == [
        f"fe_sac_forward_streamed: {weights} src pos 5 noise actions log_probs last_means last_stds None",
        "fe_sac_streamed_grad_workspace_floats: 256 4 5",
        f"fe_sac_backward_streamed: {weights} src pos 5 noise actions last_stds p p p &FeSacGrads None",
    ]
    trace, _ = traced(env, lambda: roll.run(K),
                      lambda out: sac_labels(actor, roll, actions=out[0], rewards=out[1], dones=out[2]))
    assert trace == [f"fe_env_rollout_sac_streamed: {weights} 2 obs_src obs_pos None actions None None rewards dones None "
                     "None None"]


def test_sac_mlp_traces():
    env = make_env()
    actor, roll = mlp_sac(env)
    assert normalise(env._lib.calls, sac_labels(actor, roll)) == ["fe_env_describe: env obs_src obs_pos None"]
    src, pos = descriptors()
    noise = torch.randn((B, 1))

    trace, (actions, log_probs) = traced(
        env, lambda: sample_and_backward(roll, src, pos, noise),
        lambda out: sac_labels(actor, roll, src=src, pos=pos, noise=noise, actions=out[0], log_probs=out[1],
                               last_means=roll.last["means"], last_stds=roll.last["stds"]))
    assert trace == [
        MLP_SAC_PACK,
        f"fe_mlp_sac_forward: {MLP_SAC_WEIGHTS} src pos 5 noise actions log_probs last_means last_stds None",
        "fe_mlp_sac_grad_workspace_floats: 32 4 5",
        f"fe_mlp_sac_backward: {MLP_SAC_WEIGHTS} src pos 5 noise actions last_stds p p p &FeMlpSacGrads None",
    ]
    assert actions.shape == log_probs.shape == (B, 1)
    assert all(p.grad is not None for p in actor.parameters())

    trace, out = traced(env, lambda: roll.forward(src, pos),
                        lambda out: sac_labels(actor, roll, src=src, pos=pos, fwd_means=out[2], fwd_stds=out[3]))
    assert trace == [MLP_SAC_PACK, f"fe_mlp_sac_forward: {MLP_SAC_WEIGHTS} src pos 5 None None None fwd_means fwd_stds None"]
    assert out[0] is None and out[1] is None

    rollout_noise = torch.randn((K, N, 1))
    trace, _ = traced(env, lambda: roll.run(K, noise=rollout_noise),
                      lambda out: sac_labels(actor, roll, noise=rollout_noise, actions=out[0], rewards=out[1], dones=out[2]))
    assert trace == [MLP_SAC_PACK, f"fe_env_rollout_mlp_sac: {MLP_SAC_WEIGHTS} 2 obs_src obs_pos noise actions None None "
                                   "rewards dones None None None"]
    trace, _ = traced(env, lambda: roll.run(K),
                      lambda out: sac_labels(actor, roll, actions=out[0], rewards=out[1], dones=out[2]))
    assert trace == [MLP_SAC_PACK, f"fe_env_rollout_mlp_sac: {MLP_SAC_WEIGHTS} 2 obs_src obs_pos None actions None None "
                                   "rewards dones None None None"]
    trace, _ = traced(env, lambda: roll.run(K, record_means=True, record_stds=True),
                      lambda out: sac_labels(actor, roll, actions=out[0], rewards=out[1], dones=out[2]))
    assert trace == [MLP_SAC_PACK, f"fe_env_rollout_mlp_sac: {MLP_SAC_WEIGHTS} 2 obs_src obs_pos None actions means stds "
                                   "rewards dones None None None"]
    trace, out = traced(env, lambda: roll.run(K, record_actions=False),
                        lambda out: sac_labels(actor, roll, rewards=out[1], dones=out[2]))
    assert trace == [MLP_SAC_PACK, f"fe_env_rollout_mlp_sac: {MLP_SAC_WEIGHTS} 2 obs_src obs_pos None None None None "
                                   "rewards dones None None None"]
    assert out[0] is None

    empty_src, empty_pos = descriptors(0)
    trace, (actions, _) = traced(env, lambda: sample_and_backward(roll, empty_src, empty_pos, torch.zeros((0, 1))),
                                 skip_sizing=True)
    assert trace == [] and actions.shape == (0, 1)


def test_another_rollout_object_in_between_needs_sync_from_env():
    env = make_env()
    _, first = lstm_sac(env)
    actor, second = mlp_sac(env)
    first.run(K)
    with pytest.raises(RuntimeError, match="stepped by someone else"):
        second.run(K)
    second.sync_from_env()
    trace, _ = traced(env, lambda: second.run(K),
                      lambda out: sac_labels(actor, second, actions=out[0], rewards=out[1], dones=out[2]))
    assert trace[1].startswith("fe_env_rollout_mlp_sac: ")


def test_sac_lstm_run_without_actions_and_evaluate_returns():
    """THE FIX of sharing ``run``: ``FusedSACRollout.run`` takes ``record_actions`` as ``FusedMLPSACRollout.run`` does, so
    the inherited ``evaluate_returns`` (which passes ``record_actions=False``) works; before, it raised TypeError.  The
    entry documents a null ``actions_out`` as not written."""
    env = make_env(evaluate=True)
    actor, roll = lstm_sac(env)
    expected = [f"fe_env_rollout_sac: {LSTM_SAC_WEIGHTS} 2 obs_src obs_pos None None None None rewards dones None None None"]
    trace, out = traced(env, lambda: roll.run(K, record_actions=False),
                        lambda out: sac_labels(actor, roll, rewards=out[1], dones=out[2]))
    assert trace == expected and out[0] is None
    trace, returns = traced(env, lambda: roll.evaluate_returns(chunk=K), lambda out: sac_labels(actor, roll))
    assert trace == [expected[0].replace("rewards dones", "p p")]
    assert torch.equal(returns, env.episode_returns)


def refusals(call, steps):
    """``steps``: (expected message, the repair that removes its cause), in the order the front end checks: with every
    cause present the first message is raised, and each repair uncovers the next."""
    for message, repair in steps:
        with pytest.raises(ValueError) as info:
            call()
        assert str(info.value) == message
        repair()
    call()


@pytest.mark.parametrize("family", ["lstm", "mlp"])
def test_sac_sample_refusals_in_order(family):
    from finenvs_amd.critic import CriticLSTM, FusedTwinCritic
    from finenvs_amd.mlp_critic import FusedTwinMLPCritic, MLPCritic

    env = make_env()
    actor, roll = (lstm_sac if family == "lstm" else mlp_sac)(env)
    src, pos = descriptors()
    a = types.SimpleNamespace(src=[0, 1], pos=pos, noise=None)
    env.num_assets = 2
    actor.double()
    dtype = {"lstm": "the fused actor's gradient needs float32 parameters",
             "mlp": "the fused SAC MLP actor needs float32 parameters"}[family]
    refusals(lambda: roll.sample(a.src, a.pos, a.noise), [
        ("the fused actor gradient runs one asset (the env has 2): its consumer, the fused twin critic, does",
         lambda: setattr(env, "num_assets", 1)),
        ("obs_src / obs_pos must be tensors of observation descriptors", lambda: setattr(a, "src", src)),
        ("sample needs noise: a (5, 1) float32 tensor of standard normals on cpu",
         lambda: setattr(a, "noise", torch.zeros((4, 1)))),
        ("noise must be a (5, 1) float32 tensor of standard normals on cpu, got torch.float32 (4, 1) on cpu",
         lambda: setattr(a, "noise", torch.zeros((B, 1), dtype=torch.float64))),
        ("noise must be a (5, 1) float32 tensor of standard normals on cpu, got torch.float64 (5, 1) on cpu",
         lambda: setattr(a, "noise", torch.zeros((B, 1), device="meta"))),
        ("noise must be a (5, 1) float32 tensor of standard normals on cpu, got torch.float32 (5, 1) on meta",
         lambda: setattr(a, "noise", torch.zeros((B, 1)))),
        (dtype, lambda: actor.float()),
    ])
    # parameters on another device: the LSTM family checks the dtype first, the MLP family the device
    actor.double()
    actor.to("meta")
    device = "the actor's parameters must live on the env's device cpu"
    with pytest.raises(ValueError) as info:
        roll.sample(src, pos, a.noise)
    assert str(info.value) == (dtype if family == "lstm" else device)
    actor.float()
    with pytest.raises(ValueError) as info:
        roll.sample(src, pos, a.noise)
    assert str(info.value) == device

    # actor_losses: the other family's twin, and a twin of another env
    torch.manual_seed(1)
    lstm_twin = lambda e: FusedTwinCritic(e, CriticLSTM(H, W), CriticLSTM(H, W))  # noqa: E731
    mlp_twin = lambda e: FusedTwinMLPCritic(e, MLPCritic(H, W), MLPCritic(H, W))  # noqa: E731
    own, other = (lstm_twin, mlp_twin) if family == "lstm" else (mlp_twin, lstm_twin)
    message = {"lstm": "twin must be a FusedTwinCritic of this rollout's env",
               "mlp": "twin must be a FusedTwinMLPCritic of this rollout's env"}[family]
    for twin in (other(env), own(make_env()), None):
        with pytest.raises(ValueError) as info:
            roll.actor_losses(None, torch.arange(B), twin)
        assert str(info.value) == message
    with pytest.raises(ValueError) as info:
        roll.actor_losses(None, None, own(env))
    assert str(info.value) == "actor_losses needs the indices of the sampled transitions"


# ---------------------------------------------------------------- twin critics
def lstm_twin(env, H=H):
    from finenvs_amd.critic import CriticLSTM, FusedTwinCritic

    torch.manual_seed(0)
    c1, c2 = CriticLSTM(H, W), CriticLSTM(H, W)
    return c1, c2, FusedTwinCritic(env, c1, c2, streamed=H > 128)


def mlp_twin(env):
    from finenvs_amd.mlp_critic import FusedTwinMLPCritic, MLPCritic

    torch.manual_seed(0)
    c1, c2 = MLPCritic(H, W), MLPCritic(H, W)
    return c1, c2, FusedTwinMLPCritic(env, c1, c2)


TWIN = {
    "lstm": dict(make=lstm_twin, pack=[], forward="fe_twin_q_forward", backward="fe_twin_q_backward",
                 workspace="fe_twin_q_grad_workspace_floats", weights="env lr32 &FeCriticWeights &FeCriticWeights 32",
                 grads="&FeCriticGrads", dtype="the fused critic's gradient needs float32 parameters"),
    "mlp": dict(make=mlp_twin, pack=["fe_mlp_pack: p 32 4 p p None"] * 2, forward="fe_twin_mlpq_forward",
                backward="fe_twin_mlpq_backward", workspace="fe_twin_mlpq_grad_workspace_floats",
                weights="env lr32 &FeMlpqWeights &FeMlpqWeights 32 0", grads="&FeMlpqGrads",
                dtype="the fused MLP critic's gradient needs float32 parameters"),
}


@pytest.mark.parametrize("family", ["lstm", "mlp"])
def test_twin_critic_traces(family):
    f = TWIN[family]
    env = make_env()
    c1, c2, twin = f["make"](env)
    assert env._lib.calls == []
    src, pos = descriptors()
    actions = torch.randn((B, 1))
    forward = f"{f['forward']}: {f['weights']} src pos actions 5 q1 q2 None"
    workspace = f"{f['workspace']}: 32 4 5"

    def q_and_backward(act):
        q1, q2 = twin.q(src, pos, act)
        (q1.sum() + 2 * q2.sum()).backward()
        return q1, q2

    def labels(act):
        return lambda out: dict(src=src, pos=pos, actions=act, q1=out[0], q2=out[1])

    trace, (q1, q2) = traced(env, lambda: twin.forward(src, pos, actions), labels(actions))
    assert trace == f["pack"] + [forward]
    assert q1.shape == q2.shape == (B, 1)
    trace, _ = traced(env, lambda: twin(src, pos, actions), labels(actions))
    assert trace == f["pack"] + [forward]

    # every parameter trainable: both weight reductions, no dQ/da
    trace, _ = traced(env, lambda: q_and_backward(actions), labels(actions))
    assert trace == f["pack"] + [forward, workspace,
                                 f"{f['backward']}: {f['weights']} src pos actions 5 p p p {f['grads']} {f['grads']} None None"]
    assert all(p.grad is not None for c in (c1, c2) for p in c.parameters())

    # critic 2 frozen and the actions constant: its output's gradient has nowhere to go, so it does not run
    c2.requires_grad_(False)
    trace, _ = traced(env, lambda: q_and_backward(actions), labels(actions))
    assert trace == f["pack"] + [forward, workspace,
                                 f"{f['backward']}: {f['weights']} src pos actions 5 p None p {f['grads']} None None None"]

    # critic 2 frozen, the actions a leaf: it runs for dQ/da without a weight reduction
    leaf = actions.clone().requires_grad_(True)
    trace, _ = traced(env, lambda: q_and_backward(leaf), labels(leaf))
    assert trace == f["pack"] + [forward, workspace,
                                 f"{f['backward']}: {f['weights']} src pos actions 5 p p p {f['grads']} None p None"]
    assert leaf.grad.shape == (B, 1)

    # only the actions need a gradient
    c1.requires_grad_(False)
    leaf = actions.clone().requires_grad_(True)
    trace, _ = traced(env, lambda: q_and_backward(leaf), labels(leaf))
    assert trace == f["pack"] + [forward, workspace, f"{f['backward']}: {f['weights']} src pos actions 5 p p p None None p None"]
    assert leaf.grad.shape == (B, 1)

    # an unused output: its critic does not run
    c1.requires_grad_(True), c2.requires_grad_(True)

    def first_only():
        q1, _ = twin.q(src, pos, actions)
        q1.sum().backward()

    trace, _ = traced(env, first_only, lambda out: dict(src=src, pos=pos, actions=actions))
    assert trace[-1] == f"{f['backward']}: {f['weights']} src pos actions 5 p None p {f['grads']} None None None"

    # B = 0: no launch, zeros
    for c in (c1, c2):
        c.zero_grad(set_to_none=True)
    empty_src, empty_pos = descriptors(0)
    empty = torch.zeros((0, 1), requires_grad=True)
    trace, (q1, _) = traced(env, lambda: twin.forward(empty_src, empty_pos, empty.detach()))
    assert trace == [] and q1.shape == (0, 1)

    def empty_q():
        q1, q2 = twin.q(empty_src, empty_pos, empty)
        (q1.sum() + q2.sum()).backward()

    trace, _ = traced(env, empty_q, skip_sizing=True)
    assert trace == []
    assert all(p.grad is not None and not p.grad.any() for c in (c1, c2) for p in c.parameters())
    assert empty.grad.shape == (0, 1)


def test_twin_critic_streamed_trace():
    env = make_env()
    c1, c2, twin = lstm_twin(env, H=256)
    src, pos = descriptors()
    actions = torch.randn((B, 1))

    def q_and_backward():
        q1, q2 = twin.q(src, pos, actions)
        (q1.sum() + q2.sum()).backward()
        return q1, q2

    weights = "env lr32 &FeCriticWeights &FeCriticWeights 256"
    trace, _ = traced(env, q_and_backward, lambda out: dict(src=src, pos=pos, actions=actions, q1=out[0], q2=out[1]))
    assert trace == [f"fe_twin_q_forward_streamed: {weights} src pos actions 5 q1 q2 None",
                     "fe_twin_q_streamed_grad_workspace_floats: 256 4 5",
                     f"fe_twin_q_backward_streamed: {weights} src pos actions 5 p p p &FeCriticGrads &FeCriticGrads None None"]
    assert c1.last_layer[0].weight.grad.shape == (1, 256) and c2.lstm.weight_hh_l0.grad.shape == (1024, 256)


@pytest.mark.parametrize("family", ["lstm", "mlp"])
def test_twin_critic_q_refusals_in_order(family):
    f = TWIN[family]
    env = make_env()
    c1, c2, twin = f["make"](env)
    src, pos = descriptors()
    a = types.SimpleNamespace(src=[0, 1], pos=pos.float(), actions=torch.zeros((B - 1, 1)))
    c2.double()
    for method in ("q", "forward"):
        call = lambda: getattr(twin, method)(a.src, a.pos, a.actions)  # noqa: E731
        a.src, a.pos, a.actions = [0, 1], pos.float(), torch.zeros((B - 1, 1))
        steps = [
            ("obs_src must be a torch.int64 tensor of -1 elements ((B,) or (B, 1)) on cpu, got <class 'list'> () on None",
             lambda: setattr(a, "src", src)),
            ("obs_pos must be a torch.float64 tensor of 5 elements ((B,) or (B, 1)) on cpu, got torch.float32 (5, 1) on cpu",
             lambda: setattr(a, "pos", pos)),
            ("actions must be a torch.float32 tensor of 5 elements ((B,) or (B, 1)) on cpu, got torch.float32 (4, 1) on cpu",
             lambda: setattr(a, "actions", torch.zeros((B, 1)))),
        ]
        if method == "q":
            steps.append((f["dtype"], lambda: c2.float()))
        else:  # the no-grad forward has no such rule: the pack converts
            c2.float()
        refusals(call, steps)
        c2.double()


# ---------------------------------------------------------------- heads
def lstm_head(env, H=H):
    from finenvs_amd.lstm_head import FusedLSTMHead, LSTMHead

    torch.manual_seed(0)
    module = LSTMHead(H, W)
    return module, FusedLSTMHead(env, module, streamed=H > 128)


def mlp_head(env):
    from finenvs_amd.mlp_head import FusedMLPHead, MLPHead

    torch.manual_seed(0)
    module = MLPHead(H, W)
    return module, FusedMLPHead(env, module)


def mlp2_head(env):
    from finenvs_amd.mlp2_head import FusedMLP2Head, MLP2Head

    torch.manual_seed(0)
    module = MLP2Head(H, W)
    return module, FusedMLP2Head(env, module)


HEAD = {
    "lstm": dict(make=lstm_head, made=["fe_env_describe: env obs_src obs_pos None"],
                 trace=["fe_lstm_forward: env lr32 p p p bout 32 0 src pos 5 values None",
                        "fe_lstm_grad_workspace_floats: 32 4 5",
                        "fe_lstm_backward: env lr32 p p p 32 0 src pos 5 values p p &FeLstmGrads None"],
                 dtype="the fused LSTM head's gradient needs float32 parameters"),
    "mlp": dict(make=mlp_head, made=["fe_env_describe: env obs_src obs_pos None", "fe_mlp_pack: p 32 4 p p None"],
                trace=["fe_mlp_pack: p 32 4 p p None",
                       "fe_mlp_forward: env lr32 &FeMlpWeights 32 0 0 src pos 5 values None",
                       "fe_mlp_grad_workspace_floats: 32 4 5",
                       "fe_mlp_backward: env lr32 &FeMlpWeights 32 0 0 src pos 5 values p p &FeMlpGrads None"],
                dtype="the fused MLP head's gradient needs float32 parameters"),
    "mlp2": dict(make=mlp2_head, made=["fe_env_describe: env obs_src obs_pos None", "fe_mlp_pack: p 32 4 p p None"],
                 trace=["fe_mlp_pack: p 32 4 p p None",
                        "fe_mlp2_forward: env lr32 &FeMlp2Weights 32 0 0 src pos 5 values None",
                        "fe_mlp2_grad_workspace_floats: 32 4 5",
                        "fe_mlp2_backward: env lr32 &FeMlp2Weights 32 0 0 src pos 5 values p p &FeMlp2Grads None"],
                 dtype="the fused MLP head's gradient needs float32 parameters"),
}


@pytest.mark.parametrize("family", ["lstm", "mlp", "mlp2"])
def test_head_traces_and_refusals(family):
    f = HEAD[family]
    env = make_env()
    module, head = f["make"](env)
    roll = head.rollout
    assert normalise(env._lib.calls, dict(obs_src=roll.obs_src, obs_pos=roll.obs_pos)) == f["made"]
    src, pos = descriptors()

    def call_and_backward(s, p):
        values = head(s, p)
        values.sum().backward()
        return values

    last = module.last_layer[0] if family == "lstm" else module.network[-2]
    trace, values = traced(env, lambda: call_and_backward(src, pos.reshape(B)),
                           lambda out: dict(src=src, pos=pos, values=out, bout=float(last.bias.detach())))
    assert trace == f["trace"]
    assert values.shape == (B, 1) and all(p.grad is not None for p in module.parameters())

    # B = 0: nothing is packed and nothing launches, in either direction; the gradients are zeros
    module.zero_grad(set_to_none=True)
    empty_src, empty_pos = descriptors(0)
    trace, values = traced(env, lambda: call_and_backward(empty_src, empty_pos), skip_sizing=True)
    assert trace == [] and values.shape == (0, 1)
    assert all(p.grad is not None and not p.grad.any() for p in module.parameters())

    a = types.SimpleNamespace(src=None, pos=pos)
    module.double()
    refusals(lambda: head(a.src, a.pos), [
        ("obs_src / obs_pos must be tensors of observation descriptors", lambda: setattr(a, "src", src[:4])),
        ("obs_pos must hold one position per descriptor (4), got (5, 1)", lambda: setattr(a, "src", src)),
        (f["dtype"], lambda: module.float()),
    ])
    module.double()
    module.to("meta")
    with pytest.raises(ValueError) as info:
        head(src, pos)
    assert str(info.value) == f["dtype"]  # the dtype is checked first
    module.float()
    with pytest.raises(ValueError) as info:
        head(src, pos)
    assert str(info.value) == "the head's parameters must live on the env's device cpu"


def test_lstm_head_streamed_trace():
    env = make_env()
    module, head = lstm_head(env, H=256)
    src, pos = descriptors()

    def call_and_backward():
        values = head(src, pos)
        values.sum().backward()
        return values

    trace, _ = traced(env, call_and_backward,
                      lambda out: dict(src=src, pos=pos, values=out, bout=float(module.last_layer[0].bias.detach())))
    assert trace == ["fe_lstm_forward: env lr32 p p p bout 256 0 src pos 5 values None",
                     "fe_lstm_streamed_grad_workspace_floats: 256 4 5",
                     "fe_lstm_backward_streamed: env lr32 p p p 256 0 src pos 5 values p p &FeLstmGrads None"]
