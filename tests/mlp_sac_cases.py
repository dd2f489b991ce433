"""What the CPU and the GPU tests of the SAC MLP actor share (tests/test_mlp_sac_host.py, tests/test_mlp_sac_gpu.py): the
shapes, the module builders, the three losses, and ``conditioned`` -- the gradient cases' batches with their conditions
decided on the CPU from the f64 copy alone, computed once per shape and cached.  No kernel runs in this file."""
import copy
import functools

import numpy as np
import torch

from tests.helpers import cpu_states, crafted_descriptors, modules_on_cpu

F32, F64 = torch.float32, torch.float64
NAMES = ("w1", "b1", "w2", "b2", "w_mu", "b_mu", "w_std", "b_std")
KINDS = ("chained", "log_probs", "actions")
WMAX = 72  # FE_MLP_SAC_MAX_WINDOW_H128
# (H, W, B, activation): a ragged last block; an odd window and a crossed 512-pair split; the largest image; several
# splits; the grid-stride path (2 188 blocks for at most 1 024 wavefronts)
SHAPES = [(32, 4, 33, "relu"), (64, 7, 513, "tanh"), (128, WMAX, 33, "elu"), (128, 4, 4097, "elu"), (32, 4, 70001, "relu")]
DAYS, TABLE_SEED = 12, 3  # tests/test_mlp_head_gpu.py::_env


def bars(W):
    return max(60, W + 40)  # tests/test_mlp_head_gpu.py::_env


def critic_width(H, W):
    return H if W <= 40 else 64  # the twin MLP critics admit W <= 40 at H = 128 and W <= 128 at H = 64


def actor(H, W, seed, activation="elu"):
    """SACActorMLP as torch draws it, with a moderate input scale (log-returns of ~5e-2 move z1 by O(1) at every W) and a
    lowered std bias, as tests/test_sac_grad_gpu.py::_actor: scaled far up, the first layer drives s to 0 and |u| into the
    hundreds."""
    from finenvs_amd.mlp_sac import SACActorMLP

    torch.manual_seed(seed)
    a = SACActorMLP(H=H, W=W, activation=activation, starting_alpha=0.7)
    with torch.no_grad():
        a.network[0].weight.view(H, W, 5)[:, :, :4].mul_(6.0 * np.sqrt(5 * W) / np.sqrt(W / 4.0))
        a.std_layer.bias.add_(-0.5)
    return a.cuda()


def critics(H, W, seed):
    from tests import test_mlp_critic_gpu as tq

    return tq._critic(critic_width(H, W), W, seed + 1), tq._critic(critic_width(H, W), W, seed + 2)


def loss(kind, actions, log_probs, q_fn, alpha, c, keep):
    """The three scalar functions of (actions, log_probs) every case differentiates; ``keep`` (B, 1) is 0 on the samples
    that get no upstream gradient."""
    if kind == "chained":  # Actor.compute_losses (SAC/actor.py:63-81)
        mean_lp = log_probs.mean(dim=1, keepdim=True)
        return -((torch.min(*q_fn(actions)) + -alpha * mean_lp) * keep).mean()
    if kind == "log_probs":
        return (log_probs * c * keep).sum()
    return (actions * keep).sum()


def torch_grads(kind, a, c1, c2, states, eps, c, keep, dtype):
    """Loss and the eight actor gradients of copies of the modules in ``dtype`` on rendered ``states``."""
    from finenvs_amd.mlp_sac import mlp_sac_parameters

    a, d1, d2 = copy.deepcopy(a).to(dtype), copy.deepcopy(c1).to(dtype), copy.deepcopy(c2).to(dtype)
    for m in (a, d1, d2):
        for p in m.parameters():
            p.grad = None
    s = states.to(dtype)
    actions, log_probs = a.get_actions_and_log_probs(s, eps.to(dtype))
    value = loss(kind, actions, log_probs, lambda x: (d1(s, x), d2(s, x)), a.log_alpha.detach().exp().to(dtype), c.to(dtype),
                 keep.to(dtype))
    value.backward()
    return value.detach(), [p.grad for p in mlp_sac_parameters(a)]


def _conditions(a, c1, c2, states, eps):
    """The batch conditions, decided from the f64 copies alone; returns (kink (B, 1), tie (B, 1)) or raises."""
    B = states.shape[0]
    a64, d1, d2 = copy.deepcopy(a).double(), copy.deepcopy(c1).double(), copy.deepcopy(c2).double()
    with torch.no_grad():
        s = states.double()
        z1 = a64.network[0](s.reshape(B, -1))
        dist = a64.get_distribution(s)
        u = dist.loc + eps.double() * dist.scale
        q1, q2 = d1(s, torch.tanh(u)), d2(s, torch.tanh(u))
    assert float(u.abs().max()) < 4.0, f"max|u| = {float(u.abs().max())}"
    assert float(dist.scale.min()) > 0.05, f"min s = {float(dist.scale.min())}"
    neg = float((z1 < 0).double().mean())
    assert 0.2 <= neg <= 0.8, f"share of negative z1 = {neg}"
    kink = (z1.abs() < 1e-5).any(dim=1, keepdim=True)
    assert int(kink.sum()) <= 0.02 * B, f"{int(kink.sum())} of {B} samples within 1e-5 of a kink"
    tie = (q1 - q2).abs() < 1e-4
    assert int((kink | tie).sum()) <= 0.02 * B, f"{int((kink | tie).sum())} of {B} samples at a kink or a tie of the critics"
    return kink, tie


@functools.lru_cache(maxsize=None)
def conditioned(H, W, B, activation, seed=40):
    """The gradient case of a shape, everything on the CPU: the modules of the first seed among ``seed``, ``seed + 1000``,
    ... that meets ``_conditions`` with no f64 gradient identically zero; crafted descriptors of the table of
    tests/test_mlp_head_gpu.py::_env, their rendered states (f64), the noise, the multiplier of the log_probs loss, the
    ``keep`` masks and the f64 gradients of the three losses.  The result is shared: leave it unchanged."""
    D, L = DAYS - 1, bars(W) + W
    src, pos = crafted_descriptors(D, L, W, B, seed + B)
    states, shape = cpu_states(DAYS, bars(W), W, TABLE_SEED, src, pos)
    assert shape == (D, L), (shape, D, L)
    gen = torch.Generator().manual_seed(seed + 7 * B)
    eps = torch.randn((B, 1), generator=gen)
    c = torch.rand((B, 1), generator=gen) + 0.5
    for s in range(seed, seed + 8000, 1000):
        with modules_on_cpu():
            a = actor(H, W, s, activation)
            c1, c2 = critics(H, W, s)
        try:
            kink, tie = _conditions(a, c1, c2, states, eps)
            keep = {"chained": (~(kink | tie)).float(), "log_probs": (~kink).float(), "actions": (~kink).float()}
            g64 = {k: torch_grads(k, a, c1, c2, states, eps, c, keep[k], F64) for k in KINDS}
            for k in KINDS:
                for name, g in zip(NAMES, g64[k][1]):
                    assert float(g.abs().max()) > 0, f"{k}: the f64 gradient of {name} is identically zero"
        except AssertionError as exc:
            print(f"seed {s} misses the batch conditions ({exc}); trying {s + 1000}")
            continue
        return {"seed": s, "actor": a, "critics": (c1, c2), "src": src, "pos": pos, "states": states, "eps": eps, "c": c,
                "keep": keep, "g64": g64}
    raise AssertionError("no seed meets the batch conditions")
