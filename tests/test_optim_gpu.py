"""GPU: ``FusedAdam`` (fe_net_update) and the front ends that read its resident weights.

* three ``step()``s on random parameters and gradients for the head (with a target head, TD3's pair), two critics with
  two targets in one optimizer, and the SAC actor with ``log_alpha`` beside it, at H = 32 / 64 / 128 (the head also at
  256): after every step the parameters, both moments, the targets and the step state equal ``reference_update`` run on
  the CPU from the same inputs bit for bit, every packed buffer equals the Python packer applied to the updated module
  and to the updated target bit for bit, and the gradients are zero;
* the same three steps against ``torch.optim.Adam`` and the examples' ``soft_update`` on cloned modules:
  ``max|p - p64| <= 4 max|p_torch32 - p64|`` over a network's parameters, and the same over its targets.  Measured on
  an MI355X, (fused distance) / (torch-f32 distance) after the third step, parameters / targets:
  head H = 64: 1.000 / 1.000; head H = 256: 1.000 / 1.000; critic H = 128: 1.000 / 1.000; actor H = 32: 1.000 (it has
  no target).  The distances themselves are 1.1e-8 to 1.2e-6, and the same elements decide both.  MEASURED_RATIOS
  below holds the same figures;
* ``soft_update=False`` leaves targets and their packed forms alone; ``repack()`` after an in-place edit; ``zero_grad()``
  zeroes the gradients and nothing else; a missing gradient is a ValueError at ``step()``; ``state_dict`` resumes;
* resident front ends: after a step, ``FusedLSTMHead`` / ``FusedTwinCritic`` / ``FusedSACRollout`` with ``weights=opt``
  return the bits of fresh front ends built without it from the same modules, gradients included (8 to 64 envs, W = 4,
  B = 33 and 257), and those calls and ``step()`` pass under ``torch.cuda.set_sync_debug_mode("error")``;
* a ``step()`` or ``repack()`` between a resident forward and its ``backward()`` is a RuntimeError, and
  ``rollout.set_weights`` takes a resident rollout off the optimizer's output bias;
* the SAC, TD3 and PPO examples with ``--fused-optim`` beside the same seed without it.
"""
import copy

import pytest
import torch

from tests import test_sac_grad_gpu as tsac

pytestmark = pytest.mark.gpu

# kind / H -> (parameters, targets): max|fused - f64| / max|torch f32 - f64| after three steps, measured on an MI355X
MEASURED_RATIOS = {("head", 64): (1.000, 1.000), ("head", 256): (1.000, 1.000), ("critic", 128): (1.000, 1.000),
                   ("actor", 32): (1.000, None)}  # the distances themselves: 1.1e-8 to 1.2e-6, the same elements decide both

LR, BETAS, EPS, RHO = 3e-3, (0.9, 0.999), 1e-8, 0.005
W = 4


def _bits(t):
    t = t.detach().reshape(-1)
    return t.view(torch.int32 if t.element_size() == 4 else torch.int64)


def _same_bits(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    return a.numel() == b.numel() and a.dtype is b.dtype and torch.equal(_bits(a), _bits(b))


def _head(H, seed):
    from finenvs_amd.lstm_head import LSTMHead

    torch.manual_seed(seed)
    return LSTMHead(H, W, "tanh").cuda()


def _pack_head(m):
    from finenvs_amd.rollout import lstm_fragment_major, lstm_pack

    H = m.lstm.hidden_size
    whh, wx = lstm_pack(m.lstm.weight_ih_l0, m.lstm.weight_hh_l0, m.lstm.bias_ih_l0, m.lstm.bias_hh_l0, H)
    if H > 128:
        whh = lstm_fragment_major(whh, H)
    last = m.last_layer[0]
    return {"whh": whh, "wx": wx, "wout": last.weight.detach().reshape(H), "bout": last.bias.detach().reshape(1)}


def _packer(kind):
    from finenvs_amd.critic import pack_critic_weights
    from finenvs_amd.sac import pack_sac_weights

    return {"head": _pack_head, "critic": pack_critic_weights, "actor": pack_sac_weights}[kind]


def _setup(kind, H):
    """(optimizer, [(module, target or None)], plain tensors) for a network kind."""
    from finenvs_amd.optim import FusedAdam

    opt = FusedAdam(lr=LR, betas=BETAS, eps=EPS)
    plain = []
    if kind == "head":
        m = _head(H, 1)
        t = copy.deepcopy(m)
        with torch.no_grad():
            for p in t.parameters():
                p.add_(0.01)
        nets = [(m, t)]
    elif kind == "critic":
        nets = []
        for seed in (10, 11):
            c = tsac._critic(H, W, seed)
            t = copy.deepcopy(c)
            with torch.no_grad():
                for p in t.parameters():
                    p.mul_(0.9)
            nets.append((c, t))
    else:
        a = tsac._actor(H, W, 20)
        nets = [(a, None)]
        plain = [a.log_alpha]
    for m, t in nets:
        opt.add(m, target=t, rho=RHO)
    for p in plain:
        opt.add_tensor(p)
    return opt, nets, plain


def _set_grads(opt, gen, step):
    """Random gradients, their scale running from 1e-3 to 10 over the tensors and the steps."""
    scales = (1e-3, 1e-2, 0.1, 1.0, 10.0)
    for i, p in enumerate(opt.parameters()):
        g = torch.randn(p.shape, generator=gen, device="cuda") * scales[(i + step) % len(scales)]
        if p.grad is None:
            p.grad = g
        else:
            p.grad.copy_(g)


def _cpu(ts):
    return [None if t is None else t.detach().cpu().clone() for t in ts]


KINDS = [("head", H) for H in (32, 64, 128, 256)] + [(k, H) for k in ("critic", "actor") for H in (32, 64, 128)]


@pytest.mark.parametrize("kind,H", KINDS)
def test_three_steps_equal_the_reference_update_and_the_packers_bit_for_bit(kind, H):
    from finenvs_amd.optim import initial_state, reference_update

    opt, nets, plain = _setup(kind, H)
    gen = torch.Generator(device="cuda").manual_seed(7)
    params, targets = opt.parameters(), opt.targets()
    assert len(params) == sum(6 if kind != "actor" else 10 for _ in nets) + len(plain)
    ref_p, ref_t = _cpu(params), _cpu(targets)
    ref_m = [torch.zeros_like(p) for p in ref_p]
    ref_v = [torch.zeros_like(p) for p in ref_p]
    state = initial_state()
    pack = _packer(kind)
    for step in range(3):
        _set_grads(opt, gen, step)
        grads = _cpu([p.grad for p in params])
        opt.step()
        state = reference_update(ref_p, grads, ref_m, ref_v, state, LR, BETAS, EPS, targets=ref_t, rho=opt.rhos())
        exp_avgs, exp_avg_sqs = opt.moments()
        for i, p in enumerate(params):
            assert _same_bits(p, ref_p[i]), (step, i, "param")
            assert _same_bits(exp_avgs[i], ref_m[i]), (step, i, "exp_avg")
            assert _same_bits(exp_avg_sqs[i], ref_v[i]), (step, i, "exp_avg_sq")
            if targets[i] is not None:
                assert _same_bits(targets[i], ref_t[i]), (step, i, "target")
            assert not bool(p.grad.any()), (step, i, "grad not zeroed")
        st = opt.state.cpu()
        assert float(st[0]) == state["beta1_pow"] and float(st[1]) == state["beta2_pow"], (st, state)
        assert int(st[2:3].view(torch.int64)) == step + 1 == opt.step_count() and float(st[3]) == 0.0
        for m, t in nets:
            for module in (m, t):
                if module is None:
                    continue
                want, got = pack(module), opt.packed(module)
                assert set(want) == set(got)
                for k in want:
                    assert tuple(got[k].shape) == tuple(want[k].shape), k
                    assert _same_bits(got[k], want[k]), (step, k, "target" if module is t else "network")


def _soft_update(target, source, rho):  # examples/sac_time_series.py
    with torch.no_grad():
        for t, s in zip(target.parameters(), source.parameters()):
            t.mul_(1.0 - rho).add_(s, alpha=rho)


@pytest.mark.parametrize("kind,H", [("head", 64), ("head", 256), ("critic", 128), ("actor", 32)])
def test_three_steps_against_torch_adam_within_the_f32_margin(kind, H):
    opt, nets, plain = _setup(kind, H)
    gen = torch.Generator(device="cuda").manual_seed(8)
    n32 = [(copy.deepcopy(m), copy.deepcopy(t)) for m, t in nets]
    n64 = [(copy.deepcopy(m).double(), None if t is None else copy.deepcopy(t).double()) for m, t in nets]
    pl32 = [p.detach().clone().requires_grad_(True) for p in plain]
    pl64 = [p.detach().double().clone().requires_grad_(True) for p in plain]

    def listed(ns, pl):
        # opt.parameters() order: per network its parameters() (the modules' registration order is the table's), then plain
        return [p for m, _ in ns for p in m.parameters()] + pl

    def torch_adam(ns, pl):
        return torch.optim.Adam(listed(ns, pl), lr=LR, betas=BETAS, eps=EPS, foreach=False)

    a32, a64 = torch_adam(n32, pl32), torch_adam(n64, pl64)
    fused = [p for m, _ in nets for p in m.parameters()] + plain
    assert [id(p) for p in fused] == [id(p) for p in opt.parameters()]
    for step in range(3):
        _set_grads(opt, gen, step)
        for p, q, r in zip(fused, listed(n32, pl32), listed(n64, pl64)):
            q.grad, r.grad = p.grad.clone(), p.grad.double()
        opt.step()
        a32.step()
        a64.step()
        for ns in (n32, n64):
            for m, t in ns:
                if t is not None:
                    _soft_update(t, m, RHO)
    dist = lambda xs, ys: max(float((x.detach().double() - y.detach()).abs().max()) for x, y in zip(xs, ys))  # noqa: E731
    e_f, e_t = dist(fused, listed(n64, pl64)), dist(listed(n32, pl32), listed(n64, pl64))
    print(f"{kind} H={H}: parameters |fused - f64| {e_f:.3e} |torch32 - f64| {e_t:.3e} ratio {e_f / e_t:.3f}")
    assert e_t > 0 and e_f <= 4 * e_t, (e_f, e_t)
    tf = [p for _, t in nets if t is not None for p in t.parameters()]
    if tf:
        t32 = [p for _, t in n32 if t is not None for p in t.parameters()]
        t64 = [p for _, t in n64 if t is not None for p in t.parameters()]
        e_f, e_t = dist(tf, t64), dist(t32, t64)
        print(f"{kind} H={H}: targets    |fused - f64| {e_f:.3e} |torch32 - f64| {e_t:.3e} ratio {e_f / e_t:.3f}")
        assert e_t > 0 and e_f <= 4 * e_t, (e_f, e_t)


def test_soft_update_off_repack_zero_grad_and_a_missing_gradient():
    from finenvs_amd.critic import pack_critic_weights

    opt, nets, _ = _setup("critic", 64)
    gen = torch.Generator(device="cuda").manual_seed(9)
    with pytest.raises(ValueError, match="no gradient"):
        opt.step()
    opt.zero_grad()  # nothing to zero yet: as torch's zero_grad, not an error
    assert all(p.grad is None for p in opt.parameters())
    _set_grads(opt, gen, 0)
    opt.step()
    # TD3's delayed update: the targets and their packed forms stay, the networks move
    t_before = _cpu(opt.targets())
    p_before = _cpu(opt.parameters())
    packed_t = [{k: v.clone() for k, v in opt.packed(t).items()} for _, t in nets]
    _set_grads(opt, gen, 1)
    opt.step(soft_update=False)
    assert all(_same_bits(a, b) for a, b in zip(opt.targets(), t_before))
    assert not any(_same_bits(a, b) for a, b in zip(opt.parameters(), p_before))
    for (m, t), before in zip(nets, packed_t):
        assert all(_same_bits(opt.packed(t)[k], before[k]) for k in before)
        assert all(_same_bits(opt.packed(m)[k], v) for k, v in pack_critic_weights(m).items())
    # zero_grad=False keeps the gradients; zero_grad() then zeroes them and nothing else
    _set_grads(opt, gen, 2)
    kept = _cpu([p.grad for p in opt.parameters()])
    opt.step(zero_grad=False)
    assert all(_same_bits(p.grad, g) for p, g in zip(opt.parameters(), kept))
    snap = _cpu(opt.parameters()) + _cpu(opt.targets()) + _cpu(opt.moments()[0]) + _cpu(opt.moments()[1]) + [opt.state.cpu()]
    packed = [{k: v.clone() for k, v in opt.packed(x).items()} for pair in nets for x in pair]
    opt.zero_grad()
    assert not any(bool(p.grad.any()) for p in opt.parameters())
    now = _cpu(opt.parameters()) + _cpu(opt.targets()) + _cpu(opt.moments()[0]) + _cpu(opt.moments()[1]) + [opt.state.cpu()]
    assert all(_same_bits(a, b) for a, b in zip(snap, now))
    for x, before in zip([x for pair in nets for x in pair], packed):
        assert all(_same_bits(opt.packed(x)[k], before[k]) for k in before)
    # an in-place edit outside step(): repack() reproduces the packers, for the network and the target
    with torch.no_grad():
        nets[0][0].lstm.weight_ih_l0.mul_(1.5)
        nets[1][1].last_layer[0].bias.add_(0.25)
        nets[1][1].lstm.bias_hh_l0.add_(0.125)
    opt.repack()
    for pair in nets:
        for x in pair:
            assert all(_same_bits(opt.packed(x)[k], v) for k, v in pack_critic_weights(x).items())
    assert opt.step_count() == 3
    # a module the optimizer does not know
    with pytest.raises(ValueError, match="not registered"):
        opt.packed(tsac._critic(64, W, 12))


def test_state_dict_resumes_the_run():
    opt_a, nets_a, _ = _setup("actor", 32)
    gen = torch.Generator(device="cuda").manual_seed(10)
    _set_grads(opt_a, gen, 0)
    opt_a.step()
    opt_b, nets_b, _ = _setup("actor", 32)
    nets_b[0][0].load_state_dict(nets_a[0][0].state_dict())
    with torch.no_grad():
        nets_b[0][0].log_alpha.copy_(nets_a[0][0].log_alpha)
    opt_b.load_state_dict(copy.deepcopy(opt_a.state_dict()))
    _set_grads(opt_a, gen, 1)
    for p, q in zip(opt_a.parameters(), opt_b.parameters()):
        q.grad = p.grad.clone()
    opt_a.step()
    opt_b.step()
    assert opt_b.step_count() == 2
    assert all(_same_bits(p, q) for p, q in zip(opt_a.parameters(), opt_b.parameters()))
    pa, pb = opt_a.packed(nets_a[0][0]), opt_b.packed(nets_b[0][0])
    assert all(_same_bits(pa[k], pb[k]) for k in pa)


# ---------------------------------------------------------------- resident front ends
class _no_sync:
    """``torch.cuda.set_sync_debug_mode("error")`` around the new path, where the installed torch offers it."""

    def __enter__(self):
        self.have = hasattr(torch.cuda, "set_sync_debug_mode")
        if self.have:
            self.before = torch.cuda.get_sync_debug_mode()
            torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        if self.have:
            torch.cuda.set_sync_debug_mode(self.before)
        return False


def _grads(modules):
    return [p.grad.clone() for m in modules for p in m.parameters()]


def _clear(modules):
    for m in modules:
        for p in m.parameters():
            p.grad = None


def _stepped(kind, H, gen):
    """An optimizer of `kind` after one step from random gradients (so every packed buffer was written by a step)."""
    opt, nets, plain = _setup(kind, H)
    _set_grads(opt, gen, 0)
    opt.step()
    return opt, nets


@pytest.mark.parametrize("H,N", [(32, 8), (128, 64), (256, 8)])
def test_resident_lstm_head_equals_a_fresh_front_end(H, N):
    from finenvs_amd.lstm_head import FusedLSTMHead

    gen = torch.Generator(device="cuda").manual_seed(11)
    opt, nets = _stepped("head", H, gen)
    module, target = nets[0]
    env_a, env_b = tsac._env(N, W), tsac._env(N, W)
    src, pos, _ = tsac._descriptors(tsac._env(64, W), 257)
    streamed = H > 128
    resident = FusedLSTMHead(env_a, module, streamed=streamed, weights=opt)
    resident_t = FusedLSTMHead(env_a, target, streamed=streamed, weights=opt)
    ups = {B: torch.randn((B, 1), generator=gen, device="cuda") for B in (33, 257)}
    noise = torch.randn((2, N, 1), generator=gen, device="cuda")
    torch.cuda.synchronize()
    out, grads = {}, {}
    with _no_sync():
        for B in (33, 257):
            y = resident(src[:B], pos[:B])
            (y * ups[B]).sum().backward()
            out[B] = y.detach()
            grads[B] = _grads([module])
            opt.zero_grad()
        yt = resident_t(src[:33], pos[:33]).detach()
        resident.refresh()  # a no-op
        run = resident.rollout.run(2, noise=noise, std=0.3)
    fresh = FusedLSTMHead(env_b, module, streamed=streamed)
    for B in (33, 257):
        _clear([module])
        y = fresh(src[:B], pos[:B])
        (y * ups[B]).sum().backward()
        assert _same_bits(out[B], y), B
        assert all(_same_bits(a, b) for a, b in zip(grads[B], _grads([module]))), B
    assert _same_bits(yt, FusedLSTMHead(env_b, target, streamed=streamed)(src[:33], pos[:33]))
    want = fresh.rollout.run(2, noise=noise, std=0.3)
    assert all(_same_bits(a, b) for a, b in zip(run, want))
    # the next step is seen without a refresh
    with _no_sync():
        (resident(src[:33], pos[:33]) * ups[33]).sum().backward()
        opt.step()
        y2 = resident(src[:33], pos[:33]).detach()
    assert _same_bits(y2, FusedLSTMHead(env_b, module, streamed=streamed)(src[:33], pos[:33]))
    assert not _same_bits(y2, out[33])
    with pytest.raises(ValueError, match="not registered"):
        FusedLSTMHead(env_b, _head(H, 5), streamed=streamed, weights=opt)


@pytest.mark.parametrize("H", [32, 128])
def test_resident_twin_critic_equals_a_fresh_front_end(H):
    from finenvs_amd.critic import FusedTwinCritic
    from finenvs_amd.replay import ReplayBuffer

    gen = torch.Generator(device="cuda").manual_seed(12)
    opt, nets = _stepped("critic", H, gen)
    (c1, t1), (c2, t2) = nets
    env = tsac._env(64, W)
    src, pos, traj = tsac._descriptors(env, 64 * 6)
    buffer = ReplayBuffer(env, max_size=64 * 5)
    buffer.extend(traj)
    resident = FusedTwinCritic(env, c1, c2, weights=opt)
    resident_t = FusedTwinCritic(env, t1, t2, weights=opt)
    fresh, fresh_t = FusedTwinCritic(env, c1, c2), FusedTwinCritic(env, t1, t2)
    for B in (33, 257):
        actions = torch.rand((B, 1), generator=gen, device="cuda") * 2 - 1
        a_req = actions.clone().requires_grad_(True)
        y = torch.randn((B, 1), generator=gen, device="cuda")
        idx = torch.randint(0, buffer.size(), (B,), generator=gen, device="cuda")
        torch.cuda.synchronize()
        with _no_sync():
            f = resident.forward(src[:B], pos[:B], actions)
            ft = resident_t.forward(src[:B], pos[:B], actions)
            q1, q2 = resident.q(src[:B], pos[:B], a_req)
            (q1 * y).sum().add((q2 * q2).sum()).backward()
            g_q, g_a = _grads([c1, c2]), a_req.grad.clone()
            opt.zero_grad()
            loss = resident.critic_loss(buffer, idx, y)
            loss.backward()
            g_l = _grads([c1, c2])
            opt.zero_grad()
        for a, b in zip(f + ft, fresh.forward(src[:B], pos[:B], actions) + fresh_t.forward(src[:B], pos[:B], actions)):
            assert _same_bits(a, b), B
        _clear([c1, c2])
        b_req = actions.clone().requires_grad_(True)
        w1, w2 = fresh.q(src[:B], pos[:B], b_req)
        (w1 * y).sum().add((w2 * w2).sum()).backward()
        assert _same_bits(q1, w1) and _same_bits(q2, w2) and _same_bits(g_a, b_req.grad), B
        assert all(_same_bits(a, b) for a, b in zip(g_q, _grads([c1, c2]))), B
        _clear([c1, c2])
        want = fresh.critic_loss(buffer, idx, y)
        want.backward()
        assert _same_bits(loss, want), B
        assert all(_same_bits(a, b) for a, b in zip(g_l, _grads([c1, c2]))), B
        opt.zero_grad()
    with pytest.raises(ValueError, match="not registered"):
        FusedTwinCritic(env, c1, tsac._critic(H, W, 13), weights=opt)


@pytest.mark.parametrize("H,N", [(32, 8), (64, 64), (128, 33)])
def test_resident_sac_rollout_equals_a_fresh_front_end(H, N):
    from finenvs_amd.sac import FusedSACRollout

    gen = torch.Generator(device="cuda").manual_seed(13)
    opt, nets = _stepped("actor", H, gen)
    actor = nets[0][0]
    env_a, env_b = tsac._env(N, W), tsac._env(N, W)
    src, pos, _ = tsac._descriptors(tsac._env(64, W), 257)
    resident = FusedSACRollout(env_a, actor, weights=opt)
    fresh = FusedSACRollout(env_b, actor)
    noise = torch.randn((2, N, 1), generator=gen, device="cuda")
    for B in (33, 257):
        eps = torch.randn((B, 1), generator=gen, device="cuda")
        c = torch.randn((B, 1), generator=gen, device="cuda")
        torch.cuda.synchronize()
        with _no_sync():
            fwd = resident.forward(src[:B], pos[:B], noise=eps)
            a, lp = resident.sample(src[:B], pos[:B], eps)
            (a.sum() + (lp * c).sum()).backward()
            g = _grads([actor])
            opt.zero_grad()
        for x, y in zip(fwd, fresh.forward(src[:B], pos[:B], noise=eps)):
            assert _same_bits(x, y), B
        _clear([actor])
        a2, lp2 = fresh.sample(src[:B], pos[:B], eps)
        (a2.sum() + (lp2 * c).sum()).backward()
        assert _same_bits(a, a2) and _same_bits(lp, lp2), B
        assert all(_same_bits(x, y) for x, y in zip(g, _grads([actor]))), B
        opt.zero_grad()
    with _no_sync():
        run = resident.run(2, noise=noise, record_means=True, record_stds=True)
    want = fresh.run(2, noise=noise, record_means=True, record_stds=True)
    assert all(_same_bits(x, y) for x, y in zip(run, want))
    assert _same_bits(resident.means, fresh.means) and _same_bits(resident.stds, fresh.stds)
    with pytest.raises(ValueError, match="not registered"):
        FusedSACRollout(env_b, tsac._actor(H, W, 21), weights=opt)


def test_an_optimizer_step_between_forward_and_backward_is_an_error():
    from finenvs_amd.critic import FusedTwinCritic
    from finenvs_amd.lstm_head import FusedLSTMHead
    from finenvs_amd.sac import FusedSACRollout

    gen = torch.Generator(device="cuda").manual_seed(17)
    src, pos, _ = tsac._descriptors(tsac._env(64, W), 33)
    act = torch.rand((33, 1), generator=gen, device="cuda") * 2 - 1
    eps = torch.randn((33, 1), generator=gen, device="cuda")

    opt, nets = _stepped("head", 32, gen)
    out = FusedLSTMHead(tsac._env(8, W), nets[0][0], weights=opt)(src, pos)
    opt.repack()
    with pytest.raises(RuntimeError, match="between this forward"):
        out.sum().backward()

    opt, nets = _stepped("critic", 32, gen)
    q1, q2 = FusedTwinCritic(tsac._env(8, W), nets[0][0], nets[1][0], weights=opt).q(src, pos, act)
    opt.repack()
    with pytest.raises(RuntimeError, match="between this forward"):
        (q1.sum() + q2.sum()).backward()

    opt, nets = _stepped("actor", 32, gen)
    a, lp = FusedSACRollout(tsac._env(8, W), nets[0][0], weights=opt).sample(src, pos, eps)
    opt.repack()
    with pytest.raises(RuntimeError, match="between this forward"):
        (a.sum() + lp.sum()).backward()
    a, lp = FusedSACRollout(tsac._env(8, W), nets[0][0], weights=opt).sample(src, pos, eps)
    opt.zero_grad()  # rewrites no weight
    (a.sum() + lp.sum()).backward()


def test_set_weights_takes_a_resident_rollout_off_the_optimizers_bias():
    from finenvs_amd.lstm_head import FusedLSTMHead
    from finenvs_amd.rollout import FusedLSTMRollout

    gen = torch.Generator(device="cuda").manual_seed(19)
    opt, nets = _stepped("head", 32, gen)
    other = _head(32, 23)
    src, pos, _ = tsac._descriptors(tsac._env(64, W), 33)
    roll = FusedLSTMHead(tsac._env(8, W), nets[0][0], weights=opt).rollout
    args = (other.lstm.weight_ih_l0, other.lstm.weight_hh_l0, other.lstm.bias_ih_l0, other.lstm.bias_hh_l0,
            other.last_layer[0].weight, float(other.last_layer[0].bias.detach()))
    roll.set_weights(*args)
    want = FusedLSTMRollout(tsac._env(8, W), *args, "tanh").forward(src, pos)
    assert _same_bits(roll.forward(src, pos), want)


def _examples():
    import os
    import sys

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    if path not in sys.path:
        sys.path.insert(0, path)


def _close(a, b, what):
    print(what, a, b)
    assert abs(a - b) <= 1e-3 * max(abs(a), abs(b)), (what, a, b)


def test_sac_example_with_fused_optim_follows_the_torch_optimizers():
    """Both runs draw the same numbers, so what the first iteration computes before any update -- the critic loss --
    is the same bits.  (Its actor and temperature losses follow ``critic_opt.step()`` and the actor's, so they are held
    to the tolerance.)  After an update the two differ by what separates ``reference_update`` from torch's fused
    multiply-adds: a few ulps per parameter and step (relative 1e-7 per step at lr = 3e-4).  Four iterations of an O(1)
    loss whose sensitivity to a relative parameter change is far below 1e3 stay within 1e-3 of each other."""
    _examples()
    import sac_time_series

    kw = dict(num_envs=64, hidden=32, iterations=4, chunk=4, batch=64, days=12, bars=60, quiet=True, fused_targets=True,
              fused_critics=True, fused_actor=True)
    plain = sac_time_series.main(**kw)
    fused = sac_time_series.main(fused_optim=True, **kw)
    assert len(plain) == len(fused) == 4
    assert plain[0]["critic_loss"] == fused[0]["critic_loss"]
    for k in ("critic_loss", "actor_loss", "alpha_loss"):
        for a, b in zip(plain, fused):
            _close(a[k], b[k], k)
    assert plain[-1]["alpha"] != plain[0]["alpha"]  # the temperature did train


def test_td3_example_with_fused_optim_follows_the_torch_optimizers():
    """As the SAC example's test: the first critic loss precedes every update and is the same bits; the later losses
    (six iterations, so three delayed actor and target updates) are O(1e-2 .. 1) quantities a few ulps of every
    parameter away from each other, held to the same 1e-3."""
    _examples()
    import td3_time_series

    kw = dict(num_envs=64, window=4, hidden=(32, 32), iterations=6, batch=64, days=12, bars=60, quiet=True)
    plain, _ = td3_time_series.main(**kw)
    fused, _ = td3_time_series.main(fused_optim=True, **kw)
    assert len(plain) == len(fused) == 6
    assert plain[0]["critic_loss"] == fused[0]["critic_loss"]
    for a, b in zip(plain, fused):
        assert ("actor_loss" in a) == ("actor_loss" in b) == (a["iteration"] % 2 == 0)
        _close(a["critic_loss"], b["critic_loss"], "critic_loss")
        if "actor_loss" in a:
            _close(a["actor_loss"], b["actor_loss"], "actor_loss")


def test_ppo_example_with_fused_optim_follows_the_torch_optimizers():
    """``--fused-update`` with and without ``--fused-optim``: the first rollout precedes every update, so its mean
    reward is the same bits.  The critic loss an iteration reports is its last minibatch's, eight updates of each head
    in; the second rollout runs the updated actor.  Both stay within the 1e-3 of the other examples' tests."""
    _examples()
    import ppo_lstm_fused

    kw = dict(envs=64, steps=4, iters=2, hidden=32, window=4, quiet=True, fused_update=True)
    plain = ppo_lstm_fused.main(**kw)
    fused = ppo_lstm_fused.main(fused_optim=True, **kw)
    assert len(plain) == len(fused) == 2
    assert plain[0][1] == fused[0][1]
    for (loss_a, reward_a, _), (loss_b, reward_b, _) in zip(plain, fused):
        _close(loss_a, loss_b, "critic loss")
        _close(reward_a, reward_b, "mean step reward")
