"""OpenAI-ES on the device: the reference's EvoAgent + ParallelMLP (finenvs/agents/ES/evo_agent.py,
finenvs/agents/networks/parallel_mlp.py) with the per-env networks never materialised.

``FusedPopulationMLPRollout`` runs K env steps of the whole population per launch (C ABI ``fe_evo_rollout``,
include/finenvs_amd_evo.h; ``FusedPopulationMLP2Rollout`` is the same with the reference's default two hidden layers,
``fe_evo2_rollout``, include/finenvs_amd_evo2.h, or with ``streamed=True`` ``fe_evo2_rollout_streamed``,
include/finenvs_amd_evo2_streamed.h, which reads theta through L2 and runs the reference's H = 256): every training env acts with ``theta + s * sigma * z`` of its mirrored
pair, the noise ``z`` generated inside the kernel; finished episodes land in per-env slots on the device, so ``agent.store``'s per-step
``nonzero()`` / ``.item()`` host syncs are gone.  ``FusedEvoAgent`` is the EvoAgent loop on top of it.  The rank transform,
fitness, gradient and Adam step are small torch functions below (pinned against the reference by
tests/test_evo_host.py)."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .rollout import _FusedEvaluation, log_return_f32


# ---------------------------------------------------------------- the update (evo_agent.py:154-191, parallel_mlp.py:176-275)
def centered_ranks(returns: torch.Tensor) -> torch.Tensor:
    """Ranks of the finished episodes' returns scaled to [-0.5, 0.5] (evo_agent.py:177-186), f32.  Ties break by a stable
    sort over the order given (the population's order is (env, episode))."""
    r = returns.reshape(-1)
    order = torch.argsort(r, stable=True)
    ranks = torch.empty(r.shape, dtype=torch.float32, device=r.device)
    ranks[order] = torch.arange(r.numel(), dtype=torch.float32, device=r.device)
    return ranks / (r.numel() - 1) - 0.5


def final_ranks(episode_returns: torch.Tensor, episode_counts: torch.Tensor) -> torch.Tensor:
    """Centred ranks of all finished episodes summed per env (evo_agent.py:188-191's index_add, each env's episodes in
    finishing order).  ``episode_returns`` (N, M) f32 slots, ``episode_counts`` (N,)."""
    N, M = episode_returns.shape
    mask = torch.arange(M, device=episode_returns.device).unsqueeze(0) < episode_counts.to(torch.int64).unsqueeze(1)
    table = torch.zeros((N, M), dtype=torch.float32, device=episode_returns.device)
    table[mask] = centered_ranks(episode_returns[mask])
    out = torch.zeros((N,), dtype=torch.float32, device=episode_returns.device)
    for k in range(M):  # sequential per env, slot order = finishing order (an empty slot adds +0)
        out = out + table[:, k]
    return out


def fitness(ranks: torch.Tensor, num_training_envs: int) -> torch.Tensor:
    """diffed_p = rank[p] - rank[p + n_train / 2] (parallel_mlp.py:178-186)."""
    half = num_training_envs // 2
    return ranks[:half] - ranks[half:num_training_envs]


def es_gradient(noise_sum: torch.Tensor, num_pairs: int, theta: torch.Tensor, l2_coefficient: float) -> torch.Tensor:
    """grad = mean_p(diffed_p * z_p) - l2 * theta (parallel_mlp.py:216-220 with epsilon = sigma * z); ``noise_sum`` is
    sum_p diffed_p * z_p in f64 (``FusedPopulationMLPRollout.gradient``)."""
    return (noise_sum.to(torch.float64) / num_pairs).to(torch.float32) - l2_coefficient * theta


def adam_step(theta: torch.Tensor, grad: torch.Tensor, m: torch.Tensor, v: torch.Tensor, t: int, learning_rate: float,
              beta_1: float = 0.9, beta_2: float = 0.999) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The reference's ascent step (parallel_mlp.py:239-275), t >= 1: returns (theta, m, v) after it."""
    m = beta_1 * m + (1 - beta_1) * grad
    v = beta_2 * v + (1 - beta_2) * torch.square(grad)
    alpha_t = np.sqrt(1 - beta_2 ** t) / (1 - beta_1 ** t) * learning_rate
    return theta + alpha_t * torch.div(m, torch.sqrt(v) + 10 ** -8), m, v


def init_parameters(num_observations: int, hidden_dim: int, generator: torch.Generator,
                    hidden_layers: int = 1) -> Tuple[List[torch.Tensor], List[torch.Tensor]]:
    """ParallelMLP's initialisation (parallel_mlp.py:45-65) for (5W, H, 1), or (5W, H, H, 1) with ``hidden_layers=2``: every
    layer's weight (in, out) and bias (1, out) ~ N(0, sqrt(2 / in)), drawn in the order W1, b1, W2, b2[, W3, b3]."""
    if hidden_layers not in (1, 2):
        raise ValueError("hidden_layers must be 1 or 2")
    dims = (num_observations,) + (hidden_dim,) * hidden_layers + (1,)
    weights, biases = [], []
    for fan_in, fan_out in zip(dims[:-1], dims[1:]):
        std = float(np.sqrt(2 / fan_in))
        weights.append(torch.normal(0.0, std, (fan_in, fan_out), generator=generator))
        biases.append(torch.normal(0.0, std, (1, fan_out), generator=generator))
    return weights, biases


# ---------------------------------------------------------------- theta's layout
def evo_layout(num_observations: int, H: int, hidden_layers: int) -> Dict[str, Tuple[int, Tuple[int, int]]]:
    """The flat layout of theta with one or two hidden layers (include/finenvs_amd_evo.h, finenvs_amd_evo2.h): name ->
    (offset, ParallelMLP shape), W1, b1, W2, b2[, W3, b3] in the reference's layer order.  Every offset is a multiple of 4
    (H is), so the noise stream's definition is the same at either depth."""
    dims = (int(num_observations),) + (H,) * hidden_layers + (1,)
    out, off = {}, 0
    for i, (fan_in, fan_out) in enumerate(zip(dims[:-1], dims[1:]), start=1):
        for name, shape in ((f"W{i}", (fan_in, fan_out)), (f"b{i}", (1, fan_out))):
            out[name] = (off, shape)
            off += shape[0] * shape[1]
    return out


_LAYER_LISTS = {1: "expected one hidden layer: two weight and two bias layers",
                2: "expected two hidden layers: three weight and three bias layers"}


def evo_flatten(weight_layers: Sequence[torch.Tensor], bias_layers: Sequence[torch.Tensor], num_observations: int, H: int,
                hidden_layers: int, device=None) -> torch.Tensor:
    """ParallelMLP's lists of weight and bias layers as one f32 theta in ``evo_layout``'s order (each layer moved to
    ``device`` first, if one is given); refuses wrong shapes and non-finite entries."""
    if len(weight_layers) != hidden_layers + 1 or len(bias_layers) != hidden_layers + 1:
        raise ValueError(_LAYER_LISTS[hidden_layers])
    flat = [t for pair in zip(weight_layers, bias_layers) for t in pair]
    for t, (_, shp) in zip(flat, evo_layout(num_observations, H, hidden_layers).values()):
        if tuple(t.shape) != shp:
            raise ValueError(f"layer of shape {tuple(t.shape)}, expected {shp}")
    theta = torch.cat([t.detach().reshape(-1).to(device=device, dtype=torch.float32) for t in flat])
    if not bool(torch.isfinite(theta).all()):
        raise ValueError("parameters have non-finite entries")
    return theta.contiguous()


def evo_views(theta: torch.Tensor, num_observations: int, H: int, hidden_layers: int) -> Tuple[List[torch.Tensor], List[torch.Tensor]]:
    """(weight_layers, bias_layers) in ParallelMLP's shapes, views of ``theta``."""
    v = {k: theta[off:off + s[0] * s[1]].view(*s) for k, (off, s) in evo_layout(num_observations, H, hidden_layers).items()}
    return [v[f"W{i}"] for i in range(1, hidden_layers + 2)], [v[f"b{i}"] for i in range(1, hidden_layers + 2)]


def evo2_layout(num_observations: int, H: int) -> Dict[str, Tuple[int, Tuple[int, int]]]:
    """``evo_layout`` of the two-hidden-layer theta."""
    return evo_layout(num_observations, H, 2)


def evo2_flatten(weight_layers: Sequence[torch.Tensor], bias_layers: Sequence[torch.Tensor], num_observations: int,
                 H: int) -> torch.Tensor:
    """``evo_flatten`` of three weight and three bias layers, on the device they are on."""
    return evo_flatten(weight_layers, bias_layers, num_observations, H, 2)


def evo2_views(theta: torch.Tensor, num_observations: int, H: int) -> Tuple[List[torch.Tensor], List[torch.Tensor]]:
    """``evo_views`` of the two-hidden-layer theta."""
    return evo_views(theta, num_observations, H, 2)


# ---------------------------------------------------------------- the population rollout
class FusedPopulationMLPRollout(_FusedEvaluation):
    """K steps of an ES population per launch.  Env ``i < n_train/2`` acts with ``theta + sigma z_p`` (p = i), ``n_train/2 <= i
    < n_train`` with ``theta - sigma z_p`` (p = i - n_train/2), the last ``num_eval_envs`` envs with ``theta`` and no action
    noise; the network is ``tanh(W2^T tanh(W1^T x + b1) + b2)`` on the flattened window of every asset (include/finenvs_amd_evo.h).
    Needs a training-mode env with ``redraw="device"``."""

    HIDDEN = (32, 64)
    LAYERS = 1  # hidden layers
    _ENTRY = "fe_evo_rollout"  # the C ABI's rollout of this network shape

    @classmethod
    def _count_params(cls, num_observations: int, H: int) -> int:
        return sum(rows * cols for _, (rows, cols) in evo_layout(num_observations, H, cls.LAYERS).values())

    def _hidden_message(self) -> str:
        return f"hidden_dim must be one of {self.HIDDEN} (two hidden layers are out of scope)"

    def __init__(self, env, num_eval_envs: int, hidden_dim: int, noise_std_dev: float, seed: int,
                 action_noise_std: float = 0.01, max_episodes: int = 8):
        from . import _lib

        if env.evaluate:
            raise ValueError("the ES population needs a training-mode env (evaluate=False): its eval members are the last "
                             "num_eval_envs envs")
        if env.redraw != "device":
            raise ValueError('the ES population needs redraw="device": no host in the loop')
        if int(hidden_dim) not in self.HIDDEN:
            raise ValueError(self._hidden_message())
        N = env.num_envs
        n_train = N - int(num_eval_envs)
        if num_eval_envs < 0 or n_train <= 0 or n_train % 2:
            raise ValueError(f"the number of training envs ({N} - {num_eval_envs}) must be positive and even for mirrored sampling")
        if max_episodes < 1:
            raise ValueError("max_episodes must be >= 1")
        self.env, self.H = env, int(hidden_dim)
        self.num_eval_envs, self.num_training_envs, self.num_pairs = int(num_eval_envs), n_train, n_train // 2
        self.noise_std_dev, self.action_noise_std, self.seed = float(noise_std_dev), float(action_noise_std), int(seed)
        self.max_episodes = int(max_episodes)
        W, A, dev = env.num_intervals, env.num_assets, env._dev
        self.num_observations = 5 * W
        self.num_params = self._count_params(5 * W, self.H)
        self.obs_src = torch.empty((N,), dtype=torch.int64, device=dev)
        self.obs_pos = torch.empty((N, A), dtype=torch.float64, device=dev)
        self._lr32 = log_return_f32(env)
        self.theta = torch.zeros((self.num_params,), dtype=torch.float32, device=dev)
        self.returns = torch.zeros((N,), dtype=torch.float32, device=dev)
        self.timesteps = torch.zeros((N,), dtype=torch.float32, device=dev)
        self.episode_returns = torch.zeros((N, self.max_episodes), dtype=torch.float32, device=dev)
        self.episode_counts = torch.zeros((N,), dtype=torch.int32, device=dev)
        self.counters = torch.zeros((2,), dtype=torch.int64, device=dev)  # [0] finished timesteps, [1] overflow flag
        self._scratch_rew = torch.empty((N,), dtype=torch.float64, device=dev)
        self._scratch_done = torch.empty((N,), dtype=torch.int32, device=dev)
        self._workspace = None
        self.generation, self.step = 0, 0
        self.means = None
        self._pop = _lib.FeEvoPopulation()
        self.sync_from_env()

    # -- parameters
    def set_parameters(self, weight_layers: Sequence[torch.Tensor], bias_layers: Sequence[torch.Tensor]) -> None:
        """ParallelMLP's lists: ``weight_layers = [W1 (5W, H), W2 (H, 1)]``, ``bias_layers = [b1 (1, H), b2 (1, 1)]``; with two
        hidden layers ``[W1 (5W, H), W2 (H, H), W3 (H, 1)]`` and ``[b1 (1, H), b2 (1, H), b3 (1, 1)]``."""
        self.theta = evo_flatten(weight_layers, bias_layers, self.num_observations, self.H, self.LAYERS, device=self.env._dev)

    def parameters(self) -> Tuple[List[torch.Tensor], List[torch.Tensor]]:
        """(weight_layers, bias_layers) in ParallelMLP's shapes, views of ``theta``."""
        return evo_views(self.theta, self.num_observations, self.H, self.LAYERS)

    # -- rollout
    def run(self, num_steps: int, record: bool = False):
        """K steps of generation ``self.generation``.  ``record``: returns (actions (K, N, A) f32, rewards (K, N) f64, dones
        (K, N) int32) and keeps the network outputs before the action noise in ``self.means``; else returns None."""
        from . import _lib

        env, K = self.env, int(num_steps)
        if K < 1:
            raise ValueError("num_steps must be >= 1")
        N, A, dev = env.num_envs, env.num_assets, env._dev
        self._begin_run()
        actions = means = rewards = dones = None
        if record:
            actions = torch.empty((K, N, A), dtype=torch.float32, device=dev)
            means = torch.empty((K, N, A), dtype=torch.float32, device=dev)
            rewards = torch.empty((K, N), dtype=torch.float64, device=dev)
            dones = torch.empty((K, N), dtype=torch.int32, device=dev)
        pop = self._pop
        pop.num_train, pop.hidden, pop.max_episodes = self.num_training_envs, self.H, self.max_episodes
        pop.noise_std, pop.action_noise_std, pop.seed = self.noise_std_dev, self.action_noise_std, self.seed & (2 ** 64 - 1)
        pop.generation, pop.step = self.generation, self.step
        for name, t in (("logret_f32", self._lr32), ("theta", self.theta), ("obs_src", self.obs_src), ("obs_pos", self.obs_pos),
                        ("returns", self.returns), ("timesteps", self.timesteps), ("episode_returns", self.episode_returns),
                        ("episode_counts", self.episode_counts), ("counters", self.counters),
                        ("scratch_rewards", self._scratch_rew), ("scratch_dones", self._scratch_done)):
            setattr(pop, name, t.data_ptr())
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        _lib.check(getattr(env._lib, self._ENTRY)(env._handle, C.byref(pop), K, ptr(actions), ptr(means), ptr(rewards),
                                                  ptr(dones), env._stream()))
        self._end_run()
        self.step += K
        self.means = means
        return (actions, rewards, dones) if record else None

    # -- episode state
    def episodes(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(episode_returns (N, max_episodes) f32, episode_counts (N,) int32): per env, the finished episodes' returns
        in finishing order."""
        return self.episode_returns, self.episode_counts

    def num_finished(self) -> int:
        """Finished episodes of this generation, eval envs included (EvoAgent.store's first value): one host read."""
        return int(self.episode_counts.sum().item())

    def total_timesteps(self) -> int:
        return int(self.counters[0].item())

    def overflowed(self) -> bool:
        """True if an env finished more than max_episodes episodes this generation (the extra ones were not recorded)."""
        return bool(self.counters[1].item())

    def next_generation(self) -> None:
        """g += 1 and the episode state cleared (EvoAgent.log_progress, evo_agent.py:145-150); the envs carry on."""
        self.generation += 1
        self.step = 0
        for t in (self.returns, self.timesteps, self.episode_returns, self.episode_counts, self.counters):
            t.zero_()

    # -- noise and gradient
    def noise(self, pairs, generation: Optional[int] = None) -> torch.Tensor:
        """z_{g,p,.} for the given pairs: (len(pairs), num_params) f32 (fe_evo_noise)."""
        from . import _lib

        dev = self.env._dev
        p = torch.as_tensor(pairs, dtype=torch.int64).reshape(-1).to(dev).contiguous()
        if p.numel() == 0:
            return torch.empty((0, self.num_params), dtype=torch.float32, device=dev)
        if bool(((p < 0) | (p >= self.num_pairs)).any()):
            raise ValueError(f"pairs must be in [0, {self.num_pairs})")
        out = torch.empty((p.numel(), self.num_params), dtype=torch.float32, device=dev)
        g = self.generation if generation is None else int(generation)
        _lib.check(self.env._lib.fe_evo_noise(self.seed & (2 ** 64 - 1), g, p.data_ptr(), p.numel(), self.num_params,
                                              out.data_ptr(), self.env._stream()))
        return out

    def gradient(self, diffed: torch.Tensor) -> torch.Tensor:
        """sum_p diffed[p] * z_{g,p,j} for every j: (num_params,) f64, in a fixed order (fe_evo_gradient)."""
        from . import _lib

        env = self.env
        d = diffed.detach().to(device=env._dev, dtype=torch.float32).reshape(-1).contiguous()
        if d.numel() != self.num_pairs:
            raise ValueError(f"diffed must have {self.num_pairs} entries (one per mirrored pair)")
        if self._workspace is None:
            n = int(env._lib.fe_evo_gradient_workspace_doubles(self.num_pairs, self.num_params))
            self._workspace = torch.empty((n,), dtype=torch.float64, device=env._dev)
        out = torch.empty((self.num_params,), dtype=torch.float64, device=env._dev)
        _lib.check(env._lib.fe_evo_gradient(self.seed & (2 ** 64 - 1), self.generation, self.num_pairs, self.num_params,
                                            d.data_ptr(), self._workspace.data_ptr(), out.data_ptr(), env._stream()))
        return out


class FusedPopulationMLP2Rollout(FusedPopulationMLPRollout):
    """``FusedPopulationMLPRollout`` with the reference's default two hidden layers (H, H): the network is
    ``tanh(W3^T tanh(W2^T tanh(W1^T x + b1) + b2) + b3)`` (include/finenvs_amd_evo2.h, ``fe_evo2_rollout``); members, noise
    streams, episode state, ``noise`` and ``gradient`` are the one-layer class's, at ``num_params = 5WH + H^2 + 3H + 1``.
    theta lives in the LDS: H <= 128, and a window that cannot fit is refused here, before any launch.

    ``streamed=True`` reads theta through L2 instead (``fe_evo2_rollout_streamed``, include/finenvs_amd_evo2_streamed.h):
    the reference's H = 256 and any window run, and wherever both forms take the shape they give the same bits."""

    HIDDEN = (32, 64, 128)
    STREAMED_HIDDEN = (32, 64, 128, 256)
    LAYERS = 2
    LDS_BYTES = 160 * 1024
    _ENTRY = "fe_evo2_rollout"

    def _hidden_message(self) -> str:
        if self.streamed:
            return f"hidden_dim must be one of {self.HIDDEN} (the streamed two-hidden-layer kernels)"
        return (f"hidden_dim must be one of {self.HIDDEN} (theta lives in the 160 KiB LDS: the middle layer of the reference's "
                "256 alone is 256 KiB)")

    def __init__(self, env, num_eval_envs: int, hidden_dim: int, noise_std_dev: float, seed: int,
                 action_noise_std: float = 0.01, max_episodes: int = 8, streamed: bool = False):
        self.streamed = bool(streamed)
        if self.streamed:
            self.HIDDEN, self._ENTRY = self.STREAMED_HIDDEN, "fe_evo2_rollout_streamed"
        super().__init__(env, num_eval_envs, hidden_dim, noise_std_dev, seed, action_noise_std=action_noise_std,
                         max_episodes=max_episodes)
        W, A = env.num_intervals, env.num_assets
        if A > 128:
            raise ValueError(f"the ES population runs at most 128 assets per env (got {A})")
        if self.streamed:
            assert self.num_params == int(env._lib.fe_evo2_streamed_num_params(W, self.H))
            return
        need = int(env._lib.fe_evo2_lds_bytes(W, A, self.H))
        assert self.num_params == int(env._lib.fe_evo2_num_params(W, self.H))
        if need > self.LDS_BYTES:
            raise ValueError(f"theta ({self.num_params} floats at window {W}, H = {self.H}) does not fit the 160 KiB LDS "
                             f"({need} bytes needed with {A} asset(s))")


# ---------------------------------------------------------------- the agent
class FusedEvoAgent:
    """EvoAgent (evo_agent.py) on a TimeSeriesEnv with the fused population: ``collect`` replaces the loop
    agent.step -> env.step -> agent.store, ``train`` the update, ``log_progress`` the progress record."""

    def __init__(self, env, hidden_dim: int = 64, hidden_layers: int = 1, learning_rate: float = 0.01, noise_std_dev: float = 0.02,
                 l2_coefficient: float = 0.005, num_eval_envs: Optional[int] = None, seed: int = 0,
                 action_noise_std: float = 0.01, max_episodes: int = 8, streamed: Optional[bool] = None):
        """``streamed`` (two hidden layers only): None takes the streamed population where the LDS-resident one cannot take
        the shape (H = 256, or a window ``fe_evo2_lds_bytes`` puts above 160 KiB); True / False force the choice."""
        if num_eval_envs is None:
            num_eval_envs = 2 if env.num_envs % 2 == 0 else 1
        self.env = env
        self.learning_rate, self.l2_coefficient = float(learning_rate), float(l2_coefficient)
        if hidden_layers not in (1, 2):
            raise ValueError("hidden_layers must be 1 or 2")
        self.hidden_layers = int(hidden_layers)
        if hidden_layers == 1:
            if streamed:
                raise ValueError("streamed=True needs hidden_layers=2 (there is no one-layer streamed population)")
            self.population = FusedPopulationMLPRollout(env, num_eval_envs, hidden_dim, noise_std_dev, seed,
                                                        action_noise_std=action_noise_std, max_episodes=max_episodes)
        else:
            if streamed is None:
                need = int(env._lib.fe_evo2_lds_bytes(env.num_intervals, min(env.num_assets, 128), int(hidden_dim)))
                streamed = (int(hidden_dim) == 256 or need > FusedPopulationMLP2Rollout.LDS_BYTES)
            self.population = FusedPopulationMLP2Rollout(env, num_eval_envs, hidden_dim, noise_std_dev, seed,
                                                         action_noise_std=action_noise_std, max_episodes=max_episodes,
                                                         streamed=bool(streamed))
        pop = self.population
        w, b = init_parameters(pop.num_observations, pop.H, torch.Generator().manual_seed(int(seed)), self.hidden_layers)
        pop.set_parameters(w, b)
        self.first_moment = torch.zeros_like(pop.theta)
        self.second_moment = torch.zeros_like(pop.theta)
        self.adam_timestep = 0
        self.progress: Dict[str, float] = {}

    def collect(self, episodes_per_batch: int, chunk: int = 32, max_steps: int = 10_000_000) -> int:
        """Run the population until at least ``episodes_per_batch`` episodes have finished (one host read per launch);
        returns how many have."""
        pop, steps = self.population, 0
        done = pop.num_finished()
        while done < episodes_per_batch:
            if steps >= max_steps:
                raise RuntimeError(f"only {done} episodes finished within {max_steps} steps")
            pop.run(chunk)
            steps += chunk
            done = pop.num_finished()
        return done

    def train(self) -> float:
        """The ES update of this generation's episodes (evo_agent.py:159-175): ranks, fitness, gradient, Adam; then the
        next generation.  Returns the mean eval return."""
        pop = self.population
        if pop.overflowed():
            raise RuntimeError(f"an env finished more than max_episodes = {pop.max_episodes} episodes this generation: "
                               "its extra episodes were not recorded.  Raise max_episodes or collect fewer episodes")
        ep, cnt = pop.episodes()
        num_episodes = pop.num_finished()
        if num_episodes < 2:
            raise RuntimeError("train() needs at least two finished episodes (collect first)")
        ranks = final_ranks(ep, cnt)
        diffed = fitness(ranks, pop.num_training_envs)
        grad = es_gradient(pop.gradient(diffed), pop.num_pairs, pop.theta, self.l2_coefficient)
        self.adam_timestep += 1
        theta, self.first_moment, self.second_moment = adam_step(pop.theta, grad, self.first_moment, self.second_moment,
                                                                 self.adam_timestep, self.learning_rate)
        pop.theta = theta.contiguous()
        self.progress = self._progress(ep, cnt, num_episodes, pop.total_timesteps())
        pop.next_generation()
        return self.progress["mean_eval_return"]

    def _progress(self, ep: torch.Tensor, cnt: torch.Tensor, num_episodes: int, timesteps: int) -> Dict[str, float]:
        pop = self.population
        mask = torch.arange(pop.max_episodes, device=ep.device).unsqueeze(0) < cnt.to(torch.int64).unsqueeze(1)
        num = torch.where(mask, ep, torch.zeros_like(ep)).sum(dim=1)
        den = cnt.float()
        den[cnt == 0] = 1.0
        mean = num / den  # evo_agent.py:151-157
        train, evl = mean[:pop.num_training_envs], mean[pop.num_training_envs:]
        return {
            "num_episodes": num_episodes,
            "timesteps": timesteps,
            "mean_eval_return": evl.mean().item(),
            "std_dev_eval_return": evl.std().item() if evl.numel() > 1 else math.nan,
            "mean_training_return": train.mean().item(),
            "std_dev_training_return": train.std().item(),
            "L2_norm": pop.theta.square().sum().sqrt().item(),
        }

    def log_progress(self, print_line: bool = False) -> Dict[str, float]:
        """The fields EvoAgent.log_progress records (evo_agent.py:115-157) for the last train()."""
        p = self.progress
        if print_line and p:
            print(f"num eps: {p['num_episodes']} | steps: {p['timesteps']} | eval mean: {p['mean_eval_return']:.2f} | "
                  f"eval std: {p['std_dev_eval_return']:.2f} | train mean: {p['mean_training_return']:.2f} | "
                  f"train std: {p['std_dev_training_return']:.2f} | L2 norm: {p['L2_norm']:.2f}")
        return dict(p)
