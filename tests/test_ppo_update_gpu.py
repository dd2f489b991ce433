"""GPU: the capturable PPO update (include/finenvs_amd_ppo.h, finenvs_amd/ppo.py, lstm_head.ppo_*_loss(fused=True)).

Shapes are the smallest at which these paths can still go wrong: H = 32, W = 4, one asset; N = 7 x T = 5 in M = 4
mini-batches drops three samples, N = 24 x T = 5 gives B = 30 (no multiple of a wavefront) from a chunk of capacity
32 > N (the row stride), n = 1 is the smallest permutation; the losses run at B = 61 (odd, one workgroup), B = 4 096
(16 workgroups: the partials, the ticket and the last workgroup's sum) and B = 70 001 (above 65 536 the grid is capped
at 256 workgroups and strides); the heads' backward at B = 30 runs a partial tile; N = 70 x T = 8 in M = 2 gives
B = 280: two loss workgroups (the ticket, inside a captured graph too) and more than one tile of the heads' backward.
The draw beyond one asset and one workgroup is tests/test_ppo_draw_gpu.py, the losses' edges under a derived bound
tests/test_ppo_loss_edges_gpu.py; both import this file's helpers.

* ``fe_ppo_minibatch`` against the host mirror bit for bit, its memory contract, the epoch counter;
* the two loss kernels against torch autograd in float64, with the float32 torch expression's own error as the bound;
* ``PPOUpdate(fused_loss=False).train()`` against a loop of today's public pieces, bit for bit;
* a graphed ``train`` against an eager twin, bit for bit;
* the example runs with ``graph_update=True``."""
import ctypes as ct
import math
import os
import sys

import pytest
import torch

from tests.helpers import assert_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 4, 32
GAMMA, CLIP, ENT = 0.99, 0.2, 0.01


@pytest.fixture(scope="module")
def fe():
    import finenvs_amd

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return finenvs_amd


# ------------------------------------------------------------------ 1. the draw and gather
def _random_chunk(T, N, C, seed):
    """A trajectory chunk of capacity C filled with seeded values (the launch only copies them)."""
    from finenvs_amd.trajectory import TrajectoryBuffer

    gen = torch.Generator(device="cuda").manual_seed(seed)
    traj = TrajectoryBuffer(T, N, 1, capacity=C, states=True)
    traj.obs_src.copy_(torch.randint(1, 1 << 40, (T + 1, N), generator=gen, device="cuda"))
    traj.obs_pos.copy_(torch.randn((T + 1, N, 1), generator=gen, device="cuda", dtype=torch.float64))
    traj.actions.copy_(torch.randn((T, N, 1), generator=gen, device="cuda"))
    traj.mark_filled(T)
    columns = [torch.randn((T, N), generator=gen, device="cuda") for _ in range(4)]
    return traj, columns


FIELDS = ("indices", "obs_src", "obs_pos", "actions", "col0", "col1", "col2", "col3")
GUARD = 512


def _window(k, B, A):
    return B * A if k in ("obs_pos", "actions") else B  # the two per-asset outputs are (B, A)


def _banded(B, A=1):
    dtypes = {"indices": torch.int64, "obs_src": torch.int64, "obs_pos": torch.float64}
    big = {k: torch.full((GUARD + _window(k, B, A) + GUARD,), -7, dtype=dtypes.get(k, torch.float32), device="cuda")
           for k in FIELDS}
    return big, {k: v[GUARD:GUARD + _window(k, B, A)] for k, v in big.items()}


def _bands_intact(big, B, skip=(), A=1):
    for k, v in big.items():
        n = _window(k, B, A)
        lo, hi = (GUARD, GUARD + n) if k not in skip else (GUARD + n, GUARD + n)  # a skipped output is untouched as a whole
        assert bool((v[:lo] == -7).all()) and bool((v[hi:] == -7).all()), f"{k}: written outside its window"


def _draw(lib, traj, columns, cursor, seed, offset, M, m, win, skip=(), A=1, num_columns=4, columns_out=True):
    """``skip``: outputs passed as null.  ``num_columns`` < 4 leaves the tail of both pointer arrays as it is (the launch
    must not look at it); ``columns_out=False`` passes the array itself as null."""
    from finenvs_amd import _lib

    ptr = lambda k: None if k in skip else win[k].data_ptr()  # noqa: E731
    cols = (ct.c_void_p * 4)(*(c.data_ptr() for c in columns))
    outs = (ct.c_void_p * 4)(*(ptr(f"col{i}") for i in range(4))) if columns_out else None
    _lib.check(lib.fe_ppo_minibatch(
        traj.obs_src.data_ptr(), traj.obs_pos.data_ptr(), traj.actions.data_ptr(), traj.T, traj.N, traj.C, A, cols, outs,
        num_columns, cursor.data_ptr(), seed, offset, M, m, win["indices"].data_ptr(), ptr("obs_src"), ptr("obs_pos"),
        ptr("actions"), torch.cuda.current_stream().cuda_stream), lib)


def _expected(traj, columns, seed, epoch, M, m):
    from finenvs_amd.ppo import minibatch_indices

    T, N = traj.T, traj.N
    idx = torch.tensor(minibatch_indices(seed, epoch, T * N, M, m), dtype=torch.int64, device="cuda")
    env, step = idx // T, idx % T
    src, pos = traj.minibatch_descriptors(idx)  # the numbering the learner's loop uses today
    assert_bits(src.cpu().numpy(), traj.obs_src[step, env].cpu().numpy(), "minibatch_descriptors")
    want = {"indices": idx, "obs_src": src, "obs_pos": pos.reshape(-1), "actions": traj.actions[step, env].reshape(-1)}
    for i, c in enumerate(columns):
        want[f"col{i}"] = c[step, env]
    return want


@pytest.mark.parametrize("N,T,C,M", [(7, 5, 7, 4), (24, 5, 32, 4), (1, 1, 1, 1)])
def test_minibatch_equals_the_host_mirror(fe, N, T, C, M):
    from finenvs_amd import _lib

    lib, seed = _lib.load(), 1234567
    traj, columns = _random_chunk(T, N, C, seed=N)
    B = (N * T) // M
    assert B == {7: 8, 24: 30, 1: 1}[N]
    cursor = torch.zeros((2,), dtype=torch.int64, device="cuda")
    first = {}
    for offset in (0, 1):
        for m in range(M):
            big, win = _banded(B)
            _draw(lib, traj, columns, cursor, seed, offset, M, m, win)
            _bands_intact(big, B)
            want = _expected(traj, columns, seed, offset, M, m)
            for k in FIELDS:
                assert_bits(win[k].cpu().numpy(), want[k].cpu().numpy(), f"{k} (epoch {offset}, mini-batch {m})")
            first[offset, m] = {k: v.clone() for k, v in win.items()}
    if N * T >= 16:
        assert not torch.equal(first[0, 0]["indices"], first[1, 0]["indices"])
    # null optional outputs are skipped, the others unchanged by that
    skip = ("obs_pos", "col1", "col3", "obs_src")
    big, win = _banded(B)
    _draw(lib, traj, columns, cursor, seed, 1, M, M - 1, win, skip)
    _bands_intact(big, B, skip)
    for k in FIELDS:
        if k not in skip:
            assert_bits(win[k].cpu().numpy(), first[1, M - 1][k].cpu().numpy(), f"{k} next to null outputs")
    assert cursor.tolist() == [0, 0]  # a draw moves nothing
    # the counter on the device: after two more epochs, offset 0 is epoch 2
    _lib.check(lib.fe_ppo_epochs_advance(cursor.data_ptr(), 2, torch.cuda.current_stream().cuda_stream), lib)
    big, win = _banded(B)
    _draw(lib, traj, columns, cursor, seed, 0, M, 0, win)
    _bands_intact(big, B)
    want = _expected(traj, columns, seed, 2, M, 0)
    for k in FIELDS:
        assert_bits(win[k].cpu().numpy(), want[k].cpu().numpy(), f"{k} (epoch 2 from the counter)")
    assert cursor.tolist() == [2, 0]


# ------------------------------------------------------------------ 2. the losses
RATIOS = (0.5, 0.7, 0.9, 1.0, 1.1, 1.3, 2.0)


LOSS_SIZES = (61, 4096, 70001)  # one workgroup; 16 workgroups; above 65 536, where the capped grid of 256 strides


def _loss_case(B):
    """B samples whose probability ratios are the seven of RATIOS, advantages of both signs under each."""
    from torch.distributions import Normal

    gen = torch.Generator(device="cuda").manual_seed(99)
    means = torch.tanh(torch.randn((B, 1), generator=gen, device="cuda"))
    actions = (means + 0.5 * torch.randn((B, 1), generator=gen, device="cuda")).clamp(-1, 1)
    log_std = torch.full((1,), math.log(0.5), device="cuda")
    new_lp = Normal(means.double(), log_std.double().exp()).log_prob(actions.double())
    b = torch.arange(B, device="cuda")
    target = torch.tensor(RATIOS, dtype=torch.float64, device="cuda")[b % 7].reshape(B, 1)
    old_lp = (new_lp - target.log()).float()
    sign = torch.where((b // 7) % 2 == 0, 1.0, -1.0).float().reshape(B, 1)
    advantages = sign * (0.1 + torch.rand((B, 1), generator=gen, device="cuda"))
    values = torch.randn((B, 1), generator=gen, device="cuda")
    returns = values + torch.randn((B, 1), generator=gen, device="cuda")
    return dict(B=B, means=means, actions=actions, log_std=log_std, old_lp=old_lp, advantages=advantages, values=values,
                returns=returns)


@pytest.fixture(scope="module")
def loss_cases():
    """The inputs and the float64 / float32 torch results of every size, computed once."""
    out = {}
    for B in LOSS_SIZES:
        c = _loss_case(B)
        c["actor64"], c["actor32"] = _torch_actor(c, torch.float64), _torch_actor(c, torch.float32)
        c["critic64"], c["critic32"] = _torch_critic(c, torch.float64), _torch_critic(c, torch.float32)
        out[B] = c
    return out


def _torch_actor(c, dtype):
    from finenvs_amd.lstm_head import torch_ppo_actor_loss

    means = c["means"].detach().to(dtype).clone().requires_grad_(True)  # (a clone: .to() of the same dtype is the fixture)
    log_std = c["log_std"].detach().to(dtype).clone().requires_grad_(True)
    loss = torch_ppo_actor_loss(means, log_std, c["actions"].to(dtype), c["old_lp"].to(dtype), c["advantages"].to(dtype),
                                CLIP, ENT)
    loss.backward()
    return loss.detach().double(), means.grad.double(), log_std.grad.double()


def _torch_critic(c, dtype):
    from finenvs_amd.lstm_head import torch_ppo_critic_loss

    values = c["values"].detach().to(dtype).clone().requires_grad_(True)
    loss = torch_ppo_critic_loss(values, c["returns"].to(dtype))
    loss.backward()
    return loss.detach().double(), values.grad.double()


def _fused_actor(c, workspace):
    from finenvs_amd.lstm_head import fused_ppo_actor_loss

    means, log_std = c["means"].detach().clone().requires_grad_(True), c["log_std"].detach().clone().requires_grad_(True)
    loss = fused_ppo_actor_loss(means, log_std, c["actions"], c["old_lp"], c["advantages"], CLIP, ENT, workspace=workspace)
    loss.backward()
    return loss.detach(), means.grad, log_std.grad


def _fused_critic(c, workspace):
    from finenvs_amd.lstm_head import fused_ppo_critic_loss

    values = c["values"].detach().clone().requires_grad_(True)
    loss = fused_ppo_critic_loss(values, c["returns"], workspace=workspace)
    loss.backward()
    return loss.detach(), values.grad


def _errors(got, want):
    return [float((g.double().reshape(-1) - w.reshape(-1)).abs().max()) for g, w in zip(got, want)]


def _kept_workspace(B):
    """One workspace for both launches of a test, between guard words: the second launch finds the ticket as the first
    left it, and the partials of ``grid`` workgroups stay inside ``fe_ppo_loss_workspace_doubles(B)`` doubles."""
    from finenvs_amd import _lib

    n = int(_lib.load().fe_ppo_loss_workspace_doubles(B))
    assert n == 1 + 2 * min(-(-B // 256), 256)
    big = torch.full((8 + n + 8,), -7.0, dtype=torch.float64, device="cuda")
    big[8:8 + n] = 0
    return big, big[8:8 + n]


def _workspace_left_clean(big, ws):
    assert int(ws[:1].view(torch.int64).item()) == 0, "the ticket is not back at zero"
    assert bool((big[:8] == -7).all()) and bool((big[-8:] == -7).all()), "written outside the workspace"


@pytest.mark.parametrize("B", LOSS_SIZES)
def test_actor_loss_kernel_against_float64(fe, loss_cases, B):
    """Measured on an MI355X (profiles/ppo_loss_check.txt): the kernel's errors are those of one f32 rounding of the
    f64 result, at or below the float32 torch expression's in all three outputs."""
    from torch.distributions import Normal

    c = loss_cases[B]
    # every clip branch occurs, and none within 1e-3 of a clip boundary: f32 and f64 choose alike for every sample
    ratio = (Normal(c["means"].double(), c["log_std"].double().exp()).log_prob(c["actions"].double()) - c["old_lp"].double()).exp()
    assert float(torch.minimum((ratio - (1 - CLIP)).abs(), (ratio - (1 + CLIP)).abs()).min()) > 1e-3
    adv = c["advantages"].double()
    for low, high, positive in ((0, 1 - CLIP, True), (0, 1 - CLIP, False), (1 + CLIP, 9, True), (1 + CLIP, 9, False),
                                (1 - CLIP, 1 + CLIP, True), (1 - CLIP, 1 + CLIP, False)):
        assert bool(((ratio > low) & (ratio < high) & ((adv > 0) == positive)).any()), (low, high, positive)
    want = c["actor64"]
    err32 = _errors(c["actor32"], want)
    big, ws = _kept_workspace(B)
    got = _fused_actor(c, ws)
    _workspace_left_clean(big, ws)
    err = _errors(got, want)
    print(f"B = {B}: actor loss / g_means / g_log_std: kernel errors", err, "float32 torch errors", err32)
    for name, e, e32 in zip(("loss", "g_means", "g_log_std"), err, err32):
        assert e <= 4.0 * e32, f"{name}: kernel error {e:.3e} against f64, the f32 torch expression's {e32:.3e}"
    again = _fused_actor(c, ws)  # the same workspace: the ticket the first launch reset
    _workspace_left_clean(big, ws)
    for name, a, b in zip(("loss", "g_means", "g_log_std"), got, again):
        assert_bits(a.cpu().numpy(), b.cpu().numpy(), f"{name}: two launches")


@pytest.mark.parametrize("B", LOSS_SIZES)
def test_value_loss_kernel_against_float64(fe, loss_cases, B):
    c = loss_cases[B]
    want = c["critic64"]
    err32 = _errors(c["critic32"], want)
    big, ws = _kept_workspace(B)
    got = _fused_critic(c, ws)
    _workspace_left_clean(big, ws)
    err = _errors(got, want)
    print(f"B = {B}: value loss / g_values: kernel errors", err, "float32 torch errors", err32)
    for name, e, e32 in zip(("loss", "g_values"), err, err32):
        assert e <= 4.0 * e32, f"{name}: kernel error {e:.3e} against f64, the f32 torch expression's {e32:.3e}"
    again = _fused_critic(c, ws)
    _workspace_left_clean(big, ws)
    for name, a, b in zip(("loss", "g_values"), got, again):
        assert_bits(a.cpu().numpy(), b.cpu().numpy(), f"{name}: two launches")


def test_loss_workspace_is_checked(fe, loss_cases):
    """A workspace that cannot hold the launch's partials is refused before anything is launched."""
    from finenvs_amd.lstm_head import fused_ppo_critic_loss, ppo_loss_workspace

    c = loss_cases[4096]
    for bad in (ppo_loss_workspace(61, "cuda"),                                   # sized for one workgroup
                torch.zeros((64,), dtype=torch.float32, device="cuda"),           # not float64
                torch.zeros((64,), dtype=torch.float64),                          # not on the device
                torch.zeros((128,), dtype=torch.float64, device="cuda")[::2]):    # not contiguous
        with pytest.raises(ValueError, match="workspace"):
            fused_ppo_critic_loss(c["values"], c["returns"], workspace=bad)


# ------------------------------------------------------------------ 3. - 5. the update
class Arm:
    """Env, heads, optimizers and a trajectory chunk, all from one seed: two arms of one seed hold identical bits.
    ``rollout()`` refills the chunk with the actor's rollout under seeded noise."""

    def __init__(self, fe, N=24, T=5, seed=5, capacity=None, **update):
        from finenvs_amd.data import synthetic
        from finenvs_amd.lstm_head import FusedLSTMHead, LSTMHead
        from finenvs_amd.optim import FusedAdam
        from finenvs_amd.ppo import PPOUpdate
        from finenvs_amd.trajectory import TrajectoryBuffer

        prices, day_id, _ = synthetic.synthetic_series(6, 1, 40, 1234 + seed)
        self.env = fe.TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=W, num_envs=N, redraw="device", seed=seed,
                                    obs_dtype=torch.float32)
        torch.manual_seed(seed)
        self.actor, self.critic = LSTMHead(H, W, "tanh", device="cuda"), LSTMHead(H, W, "none", device="cuda")
        self.log_std = torch.nn.Parameter(torch.full((1,), math.log(0.5), device="cuda"))
        self.opt_a, self.opt_c = FusedAdam(lr=3e-3), FusedAdam(lr=3e-3)
        self.opt_a.add(self.actor)
        self.opt_a.add_tensor(self.log_std)
        self.opt_c.add(self.critic)
        self.actor_head = FusedLSTMHead(self.env, self.actor, weights=self.opt_a)
        self.critic_head = FusedLSTMHead(self.env, self.critic, weights=self.opt_c)
        self.traj = TrajectoryBuffer(T, N, 1, capacity=capacity, states=True)
        self.T, self.N = T, N
        self.padded = capacity is not None and capacity != N  # the fused rollout writes chunks without padding only
        self.begun = False
        self.gen = torch.Generator(device="cuda").manual_seed(seed)
        self.update = PPOUpdate(self.env, self.traj, self.actor_head, self.critic_head, self.log_std, self.opt_a, self.opt_c,
                                clip_epsilon=CLIP, entropy_coefficient=ENT, gamma=GAMMA, seed=seed, **update)

    def rollout(self):
        self.traj.clear()
        noise = torch.randn((self.T, self.N, 1), generator=self.gen, device="cuda")
        roll = self.actor_head.rollout
        if self.padded:
            return self.rollout_by_steps(noise)
        roll.run(self.T, noise=noise, std=float(self.log_std.detach().exp()), record_means=True, trajectory=self.traj)
        self.update.load_means(roll.means)
        return roll.means

    def rollout_by_steps(self, noise):
        """The same chunk through ``env.step``, into a trajectory whose rows are ``capacity`` apart."""
        traj, roll, std = self.traj, self.actor_head.rollout, self.log_std.detach().exp()
        if not self.begun:  # (a later chunk's row 0 is carried over by clear())
            self.env.reset()
            traj.begin(self.env)
            self.begun = True
        means = torch.empty((self.T, self.N, 1), device="cuda")
        for t in range(self.T):
            roll.forward(traj.obs_src[t], traj.obs_pos[t], out=means[t])
            a_slot, r_slot, d_slot = traj.next_slot()
            self.env.step((means[t] + std * noise[t]).clamp(-1, 1), rewards_out=r_slot, dones_out=d_slot, actions_out=a_slot,
                          descriptors_out=traj.state_slot())
        self.update.load_means(means)
        return means

    def state(self):
        out = {"log_std": self.log_std.detach(), "cursor": self.update.cursor}
        for k, net, opt, head in (("actor", self.actor, self.opt_a, self.actor_head),
                                  ("critic", self.critic, self.opt_c, self.critic_head)):
            for name, p in net.named_parameters():
                out[f"{k}.{name}"] = p.detach()
            m, v = opt.moments()
            for i, (a, b) in enumerate(zip(m, v)):
                out[f"{k}.exp_avg[{i}]"], out[f"{k}.exp_avg_sq[{i}]"] = a, b
            for name, t in opt.packed(net).items():
                out[f"{k}.packed.{name}"] = t
            out[f"{k}.opt_state"] = opt.state
        return {k: v.clone() for k, v in out.items()}


def _assert_same(a, b):
    assert list(a) == list(b)
    for k in a:
        assert bool(torch.isfinite(a[k].double()).all()), k
        assert_bits(a[k].cpu().numpy(), b[k].cpu().numpy(), k)


def test_fused_loss_backward_accumulates(fe):
    """``ppo_actor_loss(fused=True).backward()`` adds to gradients that exist, in the head and in ``log_std``."""
    from finenvs_amd.lstm_head import head_parameters, ppo_actor_loss, ppo_critic_loss

    arm = Arm(fe)
    arm.rollout()
    u = arm.update
    u.prepare()
    u.draw(0, 0)
    params = list(head_parameters(arm.actor)) + [arm.log_std]

    def actor_backward():
        ppo_actor_loss(arm.actor_head, arm.log_std, u.mb_src, u.mb_pos, u.mb_actions, u.mb_old_log_probs, u.mb_advantages,
                       CLIP, ENT, fused=True).backward()

    actor_backward()
    single = [p.grad.clone() for p in params]
    assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in single)
    base = [torch.full_like(g, 0.25) for g in single]
    for p, b in zip(params, base):
        p.grad = b.clone()
    actor_backward()
    for p, b, g in zip(params, base, single):
        assert_bits(p.grad.cpu().numpy(), (b + g).cpu().numpy(), "accumulated actor gradient")
    cparams = list(head_parameters(arm.critic))
    ppo_critic_loss(arm.critic_head, u.mb_src, u.mb_pos, u.mb_returns, fused=True).backward()
    single = [p.grad.clone() for p in cparams]
    ppo_critic_loss(arm.critic_head, u.mb_src, u.mb_pos, u.mb_returns, fused=True).backward()
    for p, g in zip(cparams, single):
        assert_bits(p.grad.cpu().numpy(), (g + g).cpu().numpy(), "accumulated critic gradient")


# (N, T, M): B = 30 is one loss workgroup and a partial first tile of the heads' backward; N = 70, T = 8, M = 2 gives
# n = 560, B = 280: two loss workgroups (the ticket publishes a partial, inside a captured graph too) and more than one
# tile in the heads' backward
UPDATE_SHAPES = [(24, 5, 4), (70, 8, 2)]


@pytest.mark.parametrize("N,T,M,capacity", [(24, 5, 4, None), (24, 5, 4, 32), (70, 8, 2, None)], ids=["None", "32", "70-8-2"])
def test_eager_train_equals_the_hand_written_loop(fe, N, T, M, capacity):
    """``PPOUpdate(fused_loss=False).train()`` against the example's loop on ``minibatch_descriptors`` /
    ``ppo_actor_loss`` / ``ppo_critic_loss`` / ``FusedAdam.step``, driven by the host mirror's indices.  With capacity
    32 > N = 24 the chunk's rows are strided: ``prepare()`` then takes its dense copies of rewards and dones."""
    from torch.distributions import Normal

    from finenvs_amd.lstm_head import ppo_actor_loss, ppo_critic_loss
    from finenvs_amd.ppo import minibatch_indices

    E = 2
    a, b = (Arm(fe, N=N, T=T, capacity=capacity, epochs=E, minibatches=M, fused_loss=False) for _ in range(2))
    assert a.update.B == {24: 30, 70: 280}[N]
    means_a, means_b = a.rollout(), b.rollout()
    assert_bits(means_a.cpu().numpy(), means_b.cpu().numpy(), "the two arms' rollouts")
    loss_a, loss_c = a.update.train()
    assert a.update.cursor.tolist() == [E, 0] and a.update.epochs_drawn == E
    # the loop of examples/ppo_lstm_fused.py on the second arm
    traj = b.traj
    total = T * N
    with torch.no_grad():
        old_logp = Normal(means_b, b.log_std.exp()).log_prob(traj.actions)
        values = b.critic_head.rollout.forward(traj.obs_src, traj.obs_pos).reshape(T + 1, N)
        returns, advantages = traj.returns_and_advantages(values[:T], values[T], GAMMA)
    flat = lambda x: x.reshape(T, N).t().reshape(total)  # noqa: E731
    f_act, f_logp, f_adv, f_ret = flat(traj.actions), flat(old_logp), flat(advantages), flat(returns)
    for e in range(E):
        for m in range(M):
            mb = torch.tensor(minibatch_indices(5, e, total, M, m), dtype=torch.int64, device="cuda")
            assert torch.equal(mb, b.update.minibatch_indices(e, m))
            src, pos = traj.minibatch_descriptors(mb)
            la = ppo_actor_loss(b.actor_head, b.log_std, src, pos, f_act[mb], f_logp[mb], f_adv[mb], CLIP, ENT)
            la.backward()
            b.opt_a.step()
            lc = ppo_critic_loss(b.critic_head, src, pos, f_ret[mb])
            lc.backward()
            b.opt_c.step()
    assert_bits(a.update.indices.cpu().numpy(), mb.cpu().numpy(), "the last mini-batch drawn")
    assert_bits(loss_a.cpu().numpy(), la.detach().cpu().numpy(), "actor loss")
    assert_bits(loss_c.cpu().numpy(), lc.detach().cpu().numpy(), "critic loss")
    sa, sb = a.state(), b.state()
    sb["cursor"] = sa["cursor"]  # the loop has no counter
    _assert_same(sa, sb)
    assert a.opt_a.step_count() == E * M


def _three_updates(fe, graphed, fused_loss, N=24, T=5, M=4):
    from finenvs_amd.graphed import GraphedUpdate

    arm = Arm(fe, N=N, T=T, epochs=2, minibatches=M, fused_loss=fused_loss)
    drawn = []
    arm.rollout()
    if graphed:
        g = GraphedUpdate(arm.update.train, warmup=1)
        for _ in range(2):
            arm.rollout()
            losses = g.replay()
            drawn.append(arm.update.indices.clone())
    else:
        arm.update.train()
        for _ in range(2):
            arm.rollout()
            losses = arm.update.train()
            drawn.append(arm.update.indices.clone())
    state = arm.state()
    state["actor_loss"], state["critic_loss"] = losses[0].clone(), losses[1].clone()
    return state, drawn


@pytest.mark.parametrize("fused_loss,N,T,M", [(f, *shape) for shape in UPDATE_SHAPES for f in (True, False)],
                         ids=["True", "False", "True-70-8-2", "False-70-8-2"])  # (the first two: the ids they always had)
def test_graphed_train_equals_the_eager_one(fe, fused_loss, N, T, M):
    eager, drawn_eager = _three_updates(fe, False, fused_loss, N, T, M)
    graphed, drawn = _three_updates(fe, True, fused_loss, N, T, M)
    assert drawn[0].numel() == (N * T) // M
    if fused_loss:  # the loss launches of this shape: one workgroup, or two with the ticket between them
        from finenvs_amd import _lib

        assert int(_lib.load().fe_ppo_loss_workspace_doubles(drawn[0].numel())) == {24: 3, 70: 5}[N]
    assert eager["cursor"].tolist() == [6, 0]  # three train() of two epochs each, no walk without an end
    print({k: float(eager[k]) for k in ("actor_loss", "critic_loss")})
    _assert_same(eager, graphed)
    assert not torch.equal(drawn[0], drawn[1]), "two replays drew the same mini-batch: the counter did not move"
    for x, y in zip(drawn, drawn_eager):
        assert torch.equal(x, y)


def test_example_runs_with_graph_update(fe):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import ppo_lstm_fused

    history = ppo_lstm_fused.main(envs=64, steps=8, iters=2, hidden=32, window=4, epochs=2, minibatches=4, quiet=True,
                                  graph_update=True)
    assert len(history) == 2
    for critic_loss, reward, _ in history:
        assert math.isfinite(critic_loss) and math.isfinite(reward) and abs(critic_loss) < 1e6
