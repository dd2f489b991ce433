"""GPU: the replay ring's device cursor (include/finenvs_amd_replay_cursor.h, finenvs_amd/replay.py) and the captured
update it exists for (finenvs_amd/graphed.py).

Shapes are the smallest at which these paths can still go wrong: N = 8 envs, W = 4, H = 32 and a ring of C = 40
transitions stored in 2-step chunks of 16, so the third store wraps and the ring is full from then on; B = 37 is odd,
B = 300 needs two 256-thread workgroups (the draw counter's ticket with more than one holder).

* ``draw`` against the host: the indices against ``draw_indices``, every gathered field against the ring's tensors at
  ``physical_index`` of the host's integers, the device counter;
* the ``_c`` siblings against the by-value entries on a buffer object that shares the storage, bit for bit;
* the draw's memory contract (guard bands, null outputs, ring and cursor's head / size untouched);
* a captured ``draw + sac_targets`` follows the ring while it wraps between replays;
* a whole graphed SAC / TD3 iteration equals the eager fused one bit for bit;
* both examples run with ``--graph-update``."""
import copy
import os
import sys

import pytest
import torch

from tests.helpers import assert_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, W, H, C, T = 8, 4, 32, 40, 2
GAMMA = 0.97
FIELDS = ("state_src", "state_pos", "next_src", "next_pos", "actions", "rewards", "dones")


@pytest.fixture(scope="module")
def fe():
    import finenvs_amd

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return finenvs_amd


class Feed:
    """A seeded env stepped with seeded actions into 2-step trajectory chunks: two feeds of one seed give two rings of
    identical contents."""

    def __init__(self, fe, A=1, seed=3):
        from finenvs_amd.data import synthetic
        from finenvs_amd.trajectory import TrajectoryBuffer

        prices, day_id, _ = synthetic.synthetic_series(6, A, 40, 1234 + seed)
        self.env = fe.TimeSeriesEnv(prices=prices, day_id=day_id, num_intervals=W, num_envs=N, redraw="device", seed=seed)
        self.A = A
        self.env.reset()
        self.traj = TrajectoryBuffer(T, N, A, device=self.env.device, states=True)
        self.traj.begin(self.env)
        self.gen = torch.Generator(device="cuda").manual_seed(seed)

    def chunk(self):
        traj = self.traj
        traj.clear()  # (a full chunk's last state row becomes row 0)
        for _ in range(T):
            a_slot, r_slot, d_slot = traj.next_slot()
            a = torch.rand((N, self.A), generator=self.gen, device="cuda") * 2 - 1
            self.env.step(a, rewards_out=r_slot, dones_out=d_slot, actions_out=a_slot, descriptors_out=traj.state_slot())
        return traj

    def store(self, *buffers):
        traj = self.chunk()
        for b in buffers:
            b.extend(traj)


def _cursor(buffer):
    return [int(x) for x in buffer.cursor.cpu()]


def _by_value_twin(buffer):
    """A buffer object without a cursor on the same storage and ring state."""
    from finenvs_amd.replay import ReplayBuffer

    t = ReplayBuffer(buffer.env, max_size=buffer.max_size)
    for k in FIELDS + ("errors",):
        setattr(t, k, getattr(buffer, k))
    t._desc = buffer._desc
    t._ring.head, t._ring.size = buffer.head, buffer.size()
    return t


def _check_draw(buffer, draw, draws_before, B, what):
    from finenvs_amd.replay import draw_indices, physical_index

    A = buffer.A
    want = torch.tensor(draw_indices(buffer.seed, draws_before, buffer.size(), B), dtype=torch.int64)
    assert_bits(draw.indices.cpu().numpy(), want.numpy(), f"{what} indices")
    slots = physical_index(want, buffer.head, buffer.size(), buffer.max_size).cuda()
    for k in FIELDS:
        got, ring = getattr(draw, k), getattr(buffer, k)
        assert got.dtype == ring.dtype and tuple(got.shape) == (B,) + tuple(ring.shape[1:]), f"{what} {k}"
        assert_bits(got.cpu().numpy(), ring[slots].cpu().numpy(), f"{what} {k}")
    cur = _cursor(buffer)
    assert cur == [buffer.head, buffer.size(), draws_before + B, 0], f"{what} cursor {cur}"
    assert buffer.draws == draws_before + B


@pytest.mark.parametrize("A", [1, 2])
def test_draw_equals_the_host_rule_and_the_ring(fe, A):
    from finenvs_amd.replay import ReplayBuffer

    feed = Feed(fe, A=A)
    buffer = ReplayBuffer(feed.env, max_size=C, cursor=True, seed=0xC0FFEE12345)
    assert _cursor(buffer) == [0, 0, 0, 0]
    with pytest.raises(ValueError, match="empty"):
        buffer.draw(4)
    draws, states, reuse = 0, [], None
    for stores in range(1, 6):
        feed.store(buffer)
        if stores not in (1, 3, 5):
            continue
        states.append((buffer.head, buffer.size()))
        for B in ((1, 37, 300) if A == 1 else (37,)):
            draw = buffer.draw(B)
            _check_draw(buffer, draw, draws, B, f"A {A} stores {stores} B {B}")
            draws += B
        reuse = buffer.draw(37, out=reuse)  # the same tensors from the second time on
        _check_draw(buffer, reuse, draws, 37, f"A {A} stores {stores} out=")
        draws += 37
    assert states == [(16, 16), (8, 40), (0, 40)]  # partly filled, wrapped, full
    buffer.clear()  # head and size on the device too; the counter goes on
    assert _cursor(buffer) == [0, 0, draws, 0]
    feed.store(buffer)
    with pytest.raises(ValueError, match="ReplayDraw of 5"):
        buffer.draw(5, out=reuse)
    assert _cursor(buffer) == [16, 16, draws, 0]


def _sac_nets(env, seed, opt=True):
    from finenvs_amd.critic import CriticLSTM, FusedTwinCritic
    from finenvs_amd.optim import FusedAdam
    from finenvs_amd.sac import FusedSACRollout, SACActorLSTM

    torch.manual_seed(seed)
    dev = env.device
    actor = SACActorLSTM(H=H, W=W).to(dev)
    c1, c2 = CriticLSTM(H, W).to(dev), CriticLSTM(H, W).to(dev)
    t1, t2 = copy.deepcopy(c1), copy.deepcopy(c2)
    actor_opt, critic_opt = FusedAdam(lr=3e-3), FusedAdam(lr=3e-3)
    actor_opt.add(actor)
    actor_opt.add_tensor(actor.log_alpha)
    critic_opt.add(c1, target=t1, rho=0.05)
    critic_opt.add(c2, target=t2, rho=0.05)
    return dict(actor=actor, c1=c1, c2=c2, t1=t1, t2=t2, actor_opt=actor_opt, critic_opt=critic_opt,
                roll=FusedSACRollout(env, actor, weights=actor_opt),
                twin=FusedTwinCritic(env, c1, c2, weights=critic_opt),
                twin_t=FusedTwinCritic(env, t1, t2, weights=critic_opt))


def _td3_actor(env, seed):
    from finenvs_amd.lstm_head import FusedLSTMHead, LSTMHead
    from finenvs_amd.optim import FusedAdam

    torch.manual_seed(seed)
    actor = LSTMHead(H, W, "tanh").to(env.device)
    actor_t = copy.deepcopy(actor)
    opt = FusedAdam(lr=3e-3)
    opt.add(actor, target=actor_t, rho=0.05)
    return dict(td3_actor=actor, td3_actor_t=actor_t, td3_opt=opt, head=FusedLSTMHead(env, actor, weights=opt),
                target_roll=FusedLSTMHead(env, actor_t, weights=opt).rollout)


def test_cursor_siblings_equal_the_by_value_entries(fe):
    from finenvs_amd.replay import KEYS, ReplayBuffer

    feed = Feed(fe)
    buffer = ReplayBuffer(feed.env, max_size=C, cursor=True, seed=5)
    for _ in range(3):
        feed.store(buffer)  # wrapped: head 8, size 40
    plain = _by_value_twin(buffer)
    assert plain.cursor is None and (plain.head, plain.size()) == (8, 40)
    nets = {**_sac_nets(feed.env, 21), **_td3_actor(feed.env, 22)}
    B = 37
    draw = buffer.draw(B)
    eps = torch.randn((B, 1), device="cuda")
    twin = nets["twin_t"]
    for what, call in (
            ("sac", lambda buf, idx: twin.sac_targets(buf, idx, nets["roll"], eps, GAMMA, nets["actor"].log_alpha, 0.5)),
            ("td3", lambda buf, idx: twin.td3_targets(buf, idx, nets["target_roll"], eps, GAMMA, 0.2, 0.5, 0.5))):
        got = {"y": call(buffer, draw), "q1": twin.last["q1"], "q2": twin.last["q2"]}
        want = {"y": call(plain, draw.indices), "q1": twin.last["q1"], "q2": twin.last["q2"]}
        for k in ("y", "q1", "q2"):
            assert bool(torch.isfinite(got[k]).all()) and float(got[k].abs().max()) > 0
            assert_bits(got[k].cpu().numpy(), want[k].cpu().numpy(), f"{what} {k}")
    got, want = buffer.get_mini_batch(B, indices=draw), plain.get_mini_batch(B, indices=draw.indices)
    for k in KEYS:
        assert_bits(got[k].cpu().numpy(), want[k].cpu().numpy(), f"get_mini_batch {k}")
    assert int(buffer.errors.item()) == 0


def test_draw_memory_contract(fe):
    """The launch writes its outputs' B (x A) elements and the cursor's counter, nothing else: guard bands around every
    output, the ring and the cursor's head / size unchanged, null outputs skipped."""
    import ctypes as ct

    from finenvs_amd import _lib
    from finenvs_amd.replay import ReplayBuffer, draw_indices, physical_index

    A, B, G = 2, 37, 4096
    feed = Feed(fe, A=A)
    buffer = ReplayBuffer(feed.env, max_size=C, cursor=True, seed=77)
    for _ in range(3):
        feed.store(buffer)
    ring_before = {k: getattr(buffer, k).clone() for k in FIELDS}
    lib = _lib.load()
    shapes = {"indices": (B, torch.int64), "state_src": (B, torch.int64), "state_pos": (B * A, torch.float64),
              "next_src": (B, torch.int64), "next_pos": (B * A, torch.float64), "actions": (B * A, torch.float32),
              "rewards": (B, torch.float32), "dones": (B, torch.float32)}

    def banded():
        big = {k: torch.full((G + n + G,), -7, dtype=dt, device="cuda") for k, (n, dt) in shapes.items()}
        return big, {k: v[G:G + shapes[k][0]] for k, v in big.items()}

    def launch(win, skip=()):
        ptr = lambda k: None if k in skip else win[k].data_ptr()  # noqa: E731
        _lib.check(lib.fe_ring_draw(ct.byref(buffer._desc), buffer.cursor.data_ptr(), buffer.seed, B, win["indices"].data_ptr(),
                                    *(ptr(k) for k in FIELDS), buffer._stream()), lib)

    def bands_intact(big, skip=()):
        for k, v in big.items():
            n = shapes[k][0]
            lo, hi = (G, G + n) if k not in skip else (G + n, G + n)  # a skipped output is untouched as a whole
            assert bool((v[:lo] == -7).all()) and bool((v[hi:] == -7).all()), f"{k}: written outside its window"

    want = torch.tensor(draw_indices(buffer.seed, 0, buffer.size(), B), dtype=torch.int64)
    slots = physical_index(want, buffer.head, buffer.size(), C).cuda()
    big, win = banded()
    launch(win)
    bands_intact(big)
    assert_bits(win["indices"].cpu().numpy(), want.numpy(), "indices")
    for k in FIELDS:
        assert_bits(win[k].cpu().numpy(), getattr(buffer, k)[slots].reshape(-1).cpu().numpy(), k)
    # the same draw again (counter set back) with every second optional output null
    skip = ("state_pos", "next_src", "rewards")
    buffer.cursor[_lib.CURSOR_DRAWS] = 0
    big2, win2 = banded()
    launch(win2, skip)
    bands_intact(big2, skip)
    for k in shapes:
        if k not in skip:
            assert_bits(win2[k].cpu().numpy(), win[k].cpu().numpy(), f"{k} next to null outputs")
    assert _cursor(buffer) == [buffer.head, buffer.size(), B, 0]
    for k in FIELDS:
        assert_bits(getattr(buffer, k).cpu().numpy(), ring_before[k].cpu().numpy(), f"ring {k}")
    assert int(buffer.errors.item()) == 0
    # argument errors launch nothing
    for bad in (lambda: lib.fe_ring_draw(None, buffer.cursor.data_ptr(), 0, B, win["indices"].data_ptr(), *([None] * 7), None),
                lambda: lib.fe_ring_draw(ct.byref(buffer._desc), None, 0, B, win["indices"].data_ptr(), *([None] * 7), None),
                lambda: lib.fe_ring_draw(ct.byref(buffer._desc), buffer.cursor.data_ptr(), 0, B, None, *([None] * 7), None),
                lambda: lib.fe_ring_draw(ct.byref(buffer._desc), buffer.cursor.data_ptr(), 0, -1, win["indices"].data_ptr(),
                                         *([None] * 7), None)):
        assert bad() == _lib.FE_ERR_ARG
    assert _cursor(buffer) == [buffer.head, buffer.size(), B, 0]


def test_a_captured_graph_follows_the_ring(fe):
    """``draw + sac_targets`` captured after 2 stores, replayed, then replayed again after 2 more stores (the ring wraps
    and fills).  Each replay must equal an eager call on a second buffer at the same ring state and draw counter.  An
    implementation whose captured launches carry head / size by value (a stale cursor) passes the first comparison
    and fails the second: it would still sample the 32 transitions of the capture-time ring."""
    from finenvs_amd.graphed import GraphedUpdate
    from finenvs_amd.replay import ReplayBuffer

    feed = Feed(fe)
    graphed_buf = ReplayBuffer(feed.env, max_size=C, cursor=True, seed=13)
    eager_buf = ReplayBuffer(feed.env, max_size=C, cursor=True, seed=13)
    nets = _sac_nets(feed.env, 31)
    B = 37
    eps = torch.randn((B, 1), device="cuda")
    log_alpha = nets["actor"].log_alpha

    def targets(buffer, draw):
        buffer.draw(B, out=draw)
        y = nets["twin_t"].sac_targets(buffer, draw, nets["roll"], eps, GAMMA, log_alpha, 0.5)
        return y, nets["twin_t"].last["q1"], nets["twin_t"].last["q2"], draw.indices

    for _ in range(2):
        feed.store(graphed_buf, eager_buf)
    static = graphed_buf.new_draw(B)
    graph = GraphedUpdate(lambda: targets(graphed_buf, static), warmup=3)
    counter = 3 * B  # the warm-up calls drew; the capture executed nothing
    assert _cursor(graphed_buf)[2] == counter and graphed_buf.draws == 4 * B  # the host's mirror counts the capture's call too
    seen = []
    for phase in range(2):
        out = graph.replay()
        eager_buf.cursor[2] = counter
        want = targets(eager_buf, eager_buf.new_draw(B))
        for k, g, w in zip(("y", "q1", "q2", "indices"), out, want):
            assert_bits(g.cpu().numpy(), w.cpu().numpy(), f"replay {phase} {k}")
        assert bool(torch.isfinite(out[0]).all())
        counter += B
        assert _cursor(graphed_buf) == [graphed_buf.head, graphed_buf.size(), counter, 0]
        seen.append((graphed_buf.size(), int(out[3].max())))
        if phase == 0:
            for _ in range(2):
                feed.store(graphed_buf, eager_buf)
    assert [s for s, _ in seen] == [32, 40] and seen[0][1] < 32
    assert seen[1][1] >= 32, "37 draws from 40 transitions that never leave the first 32: the test would not see a stale size"


def _state(nets, keys, opts):
    out = {}
    for k in keys:
        for name, p in nets[k].named_parameters():
            out[f"{k}.{name}"] = p.detach()
    for k in opts:
        m, v = nets[k].moments()
        for i, (a, b) in enumerate(zip(m, v)):
            out[f"{k}.exp_avg[{i}]"], out[f"{k}.exp_avg_sq[{i}]"] = a, b
    return {k: v.clone() for k, v in out.items()}


def _assert_same(a, b):
    assert list(a) == list(b)
    for k in a:
        assert bool(torch.isfinite(a[k]).all()), k
        assert_bits(a[k].cpu().numpy(), b[k].cpu().numpy(), k)


def _sac_arm(fe, graphed):
    """Six SAC iterations at B = 37 with a 16-transition store between them: eager, or three warm-up iterations inside
    ``GraphedUpdate`` and three replays."""
    from finenvs_amd.graphed import GraphedUpdate
    from finenvs_amd.replay import ReplayBuffer

    feed = Feed(fe)
    env = feed.env
    nets = _sac_nets(env, 41)
    buffer = ReplayBuffer(env, max_size=C, cursor=True, seed=17)
    feed.store(buffer)
    B = 37
    draw = buffer.new_draw(B)
    gen = torch.Generator(device="cuda").manual_seed(5)
    eps_t, eps_a = torch.empty((B, 1), device="cuda"), torch.empty((B, 1), device="cuda")
    actor, roll, twin, twin_t = nets["actor"], nets["roll"], nets["twin"], nets["twin_t"]

    def refill():
        eps_t.copy_(torch.randn((B, 1), generator=gen, device="cuda"))
        eps_a.copy_(torch.randn((B, 1), generator=gen, device="cuda"))

    def fn():
        buffer.draw(B, out=draw)
        y = twin_t.sac_targets(buffer, draw, roll, eps_t, GAMMA, actor.log_alpha, 0.5)
        critic_loss = twin.critic_loss(buffer, draw, y)
        nets["critic_opt"].zero_grad()
        critic_loss.backward()
        nets["critic_opt"].step()
        actor_loss, alpha_loss = roll.actor_losses(buffer, draw, twin, eps_a)
        actor_loss.backward()
        alpha_loss.backward()
        nets["actor_opt"].step()
        return critic_loss.detach(), actor_loss.detach(), alpha_loss.detach()

    def between():
        feed.store(buffer)
        refill()

    refill()
    if graphed:
        g = GraphedUpdate(fn, warmup=3, between=between)
        for _ in range(3):
            losses = g.replay()
            between()
    else:
        for _ in range(6):
            losses = fn()
            between()
    state = _state(nets, ("actor", "c1", "c2", "t1", "t2"), ("actor_opt", "critic_opt"))
    state["log_alpha"] = actor.log_alpha.detach().clone()
    for k, x in zip(("critic_loss", "actor_loss", "alpha_loss"), losses):
        state[k] = x.clone()
    state["cursor"] = buffer.cursor.clone()
    return state


def test_graphed_sac_iteration_equals_the_eager_one(fe):
    eager, graphed = _sac_arm(fe, False), _sac_arm(fe, True)
    assert [int(x) for x in eager["cursor"].cpu()] == [32, 40, 6 * 37, 0]
    print({k: float(eager[k]) for k in ("critic_loss", "actor_loss", "alpha_loss")})
    _assert_same(eager, graphed)


def _td3_arm(fe, graphed):
    """Four TD3 iterations at B = 37, the actor and the targets updated every second one: eager, or one warm-up
    iteration in each of two ``GraphedUpdate`` (with / without the actor step) and one replay of each."""
    from finenvs_amd.graphed import GraphedUpdate
    from finenvs_amd.lstm_head import td3_actor_loss
    from finenvs_amd.replay import ReplayBuffer

    feed = Feed(fe)
    env = feed.env
    nets = {**_sac_nets(env, 51), **_td3_actor(env, 52)}
    buffer = ReplayBuffer(env, max_size=C, cursor=True, seed=19)
    feed.store(buffer)
    B = 37
    draw = buffer.new_draw(B)
    gen = torch.Generator(device="cuda").manual_seed(6)
    eps = torch.empty((B, 1), device="cuda")
    twin, twin_t, head = nets["twin"], nets["twin_t"], nets["head"]

    def fn(delayed):
        buffer.draw(B, out=draw)
        y = twin_t.td3_targets(buffer, draw, nets["target_roll"], eps, GAMMA, 0.2, 0.5, 0.5)
        critic_loss = twin.critic_loss(buffer, draw, y)
        nets["critic_opt"].zero_grad()  # (the actor loss's backward left values in the first critic's gradients)
        critic_loss.backward()
        nets["critic_opt"].step(soft_update=delayed)
        if not delayed:
            return (critic_loss.detach(),)
        actor_loss = td3_actor_loss(head, buffer, draw, twin)
        actor_loss.backward()
        nets["td3_opt"].step()
        return critic_loss.detach(), actor_loss.detach()

    def between():
        feed.store(buffer)
        eps.copy_(torch.randn((B, 1), generator=gen, device="cuda"))

    eps.copy_(torch.randn((B, 1), generator=gen, device="cuda"))
    losses = {}
    if graphed:
        graphs = {d: GraphedUpdate(lambda d=d: fn(d), warmup=1, between=between) for d in (True, False)}  # iterations 0, 1
        for d in (True, False):  # iterations 2, 3
            losses[d] = graphs[d].replay()
            between()
    else:
        for it in range(4):
            losses[it % 2 == 0] = fn(it % 2 == 0)
            between()
    state = _state(nets, ("td3_actor", "td3_actor_t", "c1", "c2", "t1", "t2"), ("td3_opt", "critic_opt"))
    state["critic_loss"], state["actor_loss"] = losses[False][0].clone(), losses[True][1].clone()
    state["critic_loss_delayed"] = losses[True][0].clone()
    state["cursor"] = buffer.cursor.clone()
    return state


def test_graphed_td3_iteration_equals_the_eager_one(fe):
    eager, graphed = _td3_arm(fe, False), _td3_arm(fe, True)
    assert [int(x) for x in eager["cursor"].cpu()] == [0, 40, 4 * 37, 0]
    _assert_same(eager, graphed)


def test_examples_run_with_graph_update(fe):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import sac_time_series
    import td3_time_series

    history = sac_time_series.main(num_envs=64, hidden=32, iterations=6, chunk=4, batch=100, max_size=1024, quiet=True,
                                   graph_update=True, log_every=1)
    assert [e["iteration"] for e in history] == list(range(6))  # 256 transitions per chunk: trains from the first
    for e in history:
        assert all(e[k] == e[k] and abs(e[k]) < 1e6 for k in ("critic_loss", "actor_loss", "alpha_loss", "alpha")), e
    assert history[-1]["buffer_size"] == 1024
    history, _ = td3_time_series.main(num_envs=64, window=4, hidden=(32, 32), iterations=8, batch=100, max_size=256,
                                      quiet=True, graph_update=True, log_every=1)
    assert [e["iteration"] for e in history] == list(range(1, 8))  # 64 transitions per step: trains from the second
    for e in history:
        assert e["critic_loss"] == e["critic_loss"] and abs(e["critic_loss"]) < 1e6, e
        assert ("actor_loss" in e) == (e["iteration"] % 2 == 0)
