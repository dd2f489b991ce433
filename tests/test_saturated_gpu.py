"""GPU: the fused forward and backward passes where activations SATURATE.

Every gradient suite of the fused heads asserts ``max|p| < 4`` ("not saturated") and scales its weights so that gate
pre-activations are O(1).  A trained policy lives elsewhere: actions at +-1, gates shut or open.  Here every family's
module is made "hot" (``tests/helpers.py::heat``: the recurrent / first layer times a gate scale, the output layer times an
output scale) until its f64 copy meets, on the crafted batch the case runs (``crafted_descriptors_for``), the conditions
of ``tests/helpers.py::hot_shares`` -- at least 10 % of the gate (hidden) pre-activations beyond 17, where the f32 sigmoid
is exactly 1.0, at least 1 % beyond 60 (LSTM: the clamp of ``lstm_exp_nonpos2``), at least 3 % below 2; of the output
pre-activation of a tanh-output head at least 20 % below 2, 20 % in (4, 9) and 5 % beyond 9.1, where the f32 tanh is exactly
+-1 -- and the two conditions ``reference`` asserts: no f64 gradient is identically zero (``w_hh`` at W = 1 aside), and
for every tensor ``max|g_torch32 - g64| <= 1e-3 max|g64|`` (the sharpness cap: a hot LSTM is chaotic in f32, and without
the cap the yardstick ``2e-5 max|g64| + 4 max|g_torch32 - g64|`` goes slack).  Gate scale, output scale and module seed are
the only things chosen per case (``HOT``); the shares are checked on the CPU too (tests/test_saturated_host.py).

Per case: the yardstick per gradient tensor, on the position column alone, on the loss and on every forward value; all
finite; upstream ``(y * c).sum()``, ``c ~ N(0, 1)``, and the chained losses (the TD3 actor loss and SAC's ``chained`` kind: at
(64, 7, 257) through the ordinary twin critics, at (32, 1, 33) through the hot ones -- ``CHAINED`` says why).  ReLU and the kink: a pair with a hidden pre-activation of the f64 copy within
``1e-5 max(1, mean|z|)`` of zero gets upstream gradient 0 (the siblings' rule, 1e-5 at their O(1) pre-activations, scaled
with the pre-activations; decided by the f64 copy alone).

Two exact checks the f64 reference cannot give:

* rows whose returned f32 output (SAC: action) is exactly +-1.0 contribute nothing: the backward with the upstream
  gradient zeroed on those rows gives the same bits (SAC: both upstream gradients zeroed, the ``mu_layer`` tensors
  compared -- the std path keeps ``-gl / s``);
* a batch on which EVERY output is exactly +-1.0 (output bias raised) gives gradients that are exactly 0.0, as torch f32
  does.

Then the SAC head alone against its stated contract through the C ABI (``fe_sac_forward`` / ``fe_sac_backward`` and their
``_streamed`` namesakes) with the std pre-activation q spanning [-15, 100] and crafted ``actions`` / ``stds`` up to
a = +-1, and the rollouts that share ``fe_activations.h`` in lock-step with the oracle at hot weights, bit for bit.

A third condition, ``one_element_response``: every ONE-ELEMENT gradient tensor must be resolvable -- one f32 rounding of the
weights, propagated through the f64 copy, moves it by no more than the yardstick's floor 2e-5 -- because four times torch
f32's single draw is no bound for a tensor whose maximum does not concentrate.  The LSTM head (tanh) and the SAC actor cannot
meet it at W = 7 and run (64, 5, 257) instead (``SHORTENED``).

MEASURED: worst err / tol per case on an MI355X and the shares each case reached.
"""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import test_critic_grad_gpu as tc
from tests import test_grad_descriptors_gpu as tg
from tests import test_lstm_grad_gpu as tl
from tests import test_mlp2_head_gpu as t2
from tests import test_mlp_critic_gpu as tq
from tests import test_mlp_head_gpu as th
from tests import test_sac_grad_gpu as tsac
from tests.helpers import cpu_states, crafted_descriptors, heat, hot_preactivations, hot_shares

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
DAYS, BARS, TABLE_SEED = 12, 60, 3  # the one-asset table of every family's ``_env``
CAP = 1e-3  # the sharpness cap
# The SAC actor's log-probability under the yardstick: 1 - tanh(u)^2 is 4 exp(-2|u|), and an f32 evaluation -- torch's as
# much as the kernel's -- holds it on a grid of 2^-24, so d log(1 - a^2 + 1e-7) / du = 2 a om / (om + 1e-7) is off by
# O(1) from |u| ~ 7.3 on (om ~ 2e-6) until f64 itself reaches 0 near |u| = 12.5; at |u| > 9.02 f32 gives exactly 0 where f64
# gives 0.67.  No batch that meets the output shares can meet the sharpness cap through those rows, so a pair whose f64
# |u| exceeds 6 (om = 2.5e-5: the grid moves the factor by 1e-5) gets upstream gradient 0 on its LOG-PROBABILITY; its action
# keeps its upstream gradient.  Decided by the f64 copy alone, like ReLU's kink.  That range of the log-probability's
# gradient is checked against the kernel's own contract instead: test_sac_head_contract below.
SAC_GUARD_U = 6.0

SHAPES = [(32, 4, 33), (64, 7, 257), (128, 4, 33), (32, 1, 33)]
STREAMED = (256, 4, 33)
ACTIVATIONS = ("elu", "relu", "tanh")


# ------------------------------------------------------------------------------------------------------- the families
class _Family:
    """What a case needs of a family: its modules, its fused front end, its outputs in torch and fused, its parameters."""
    lstm, tanh_output, leaves = True, False, ()
    position = staticmethod(lambda w: w[:, 4])  # of the first tensor of each module's parameters

    @staticmethod
    def aux(B, gen):
        return {}

    @staticmethod
    def fused_kwargs(H):
        return {"streamed": True} if H > 128 else {}


class Head(_Family):
    names = tl.NAMES

    def __init__(self, variant):
        self.variant, self.tanh_output = variant, variant == "tanh"

    def build(self, H, W, seed):
        return [tl._module(H, W, seed, self.variant)]

    params = staticmethod(tl._params)

    def fused(self, env, mods):
        from finenvs_amd.lstm_head import FusedLSTMHead

        return FusedLSTMHead(env, mods[0], **self.fused_kwargs(mods[0].hidden_size))

    def torch_out(self, mods, states, aux):
        return (mods[0](states),)

    def fused_out(self, fused, src, pos, aux):
        return (fused(src, pos),)

    def preacts(self, mods, states, aux):
        return [hot_preactivations(mods[0], states)]


class Critics(_Family):
    names = tuple(f"c{c}.{n}" for c in (1, 2) for n in tl.NAMES)
    leaves = ("actions",)

    def __init__(self, variant=None):
        self.variant = variant

    def build(self, H, W, seed):
        return [tc._critic(H, W, seed), tc._critic(H, W, seed + 1)]

    params = staticmethod(tc._params)

    aux = staticmethod(lambda B, gen: {"actions": torch.rand((B, 1), generator=gen) * 2 - 1})

    def fused(self, env, mods):
        from finenvs_amd.critic import FusedTwinCritic

        return FusedTwinCritic(env, *mods, **self.fused_kwargs(mods[0].hidden_size))

    def torch_out(self, mods, states, aux):
        return tuple(m(states, aux["actions"]) for m in mods)

    def fused_out(self, fused, src, pos, aux):
        return tuple(fused.q(src, pos, aux["actions"]))

    def preacts(self, mods, states, aux):
        return [hot_preactivations(m, states, actions=aux["actions"]) for m in mods]


class Sac(_Family):
    names, tanh_output = tsac.NAMES, True

    def __init__(self, variant=None):
        self.variant = variant

    def build(self, H, W, seed):
        return [tsac._actor(H, W, seed)]

    params = staticmethod(tsac._params)

    @staticmethod
    def aux(B, gen):
        return {"eps": torch.randn((B, 1), generator=gen)}

    def fused(self, env, mods):
        from finenvs_amd.sac import FusedSACRollout

        return FusedSACRollout(env, mods[0], **self.fused_kwargs(mods[0].hidden_size))

    def torch_out(self, mods, states, aux):
        return tuple(mods[0].get_actions_and_log_probs(states, aux["eps"]))

    def fused_out(self, fused, src, pos, aux):
        return tuple(fused.sample(src, pos, aux["eps"]))

    def preacts(self, mods, states, aux):
        return [hot_preactivations(mods[0], states, eps=aux["eps"])]


class Mlp(_Family):
    lstm, tanh_output = False, True
    position = staticmethod(lambda w: w[:, 4:5 * ((w.shape[1]) // 5):5])

    def __init__(self, variant, t=th):
        self.variant, self.t, self.names = variant, t, t.NAMES

    def build(self, H, W, seed):
        return [self.t._module(H, W, seed, self.variant, "tanh")]

    def params(self, m):
        return self.t._params(m)

    def fused(self, env, mods):
        from finenvs_amd.mlp2_head import FusedMLP2Head
        from finenvs_amd.mlp_head import FusedMLPHead

        return (FusedMLPHead if self.t is th else FusedMLP2Head)(env, mods[0])

    def torch_out(self, mods, states, aux):
        return (mods[0](states),)

    def fused_out(self, fused, src, pos, aux):
        return (fused(src, pos),)

    def preacts(self, mods, states, aux):
        return [hot_preactivations(mods[0], states)]


class MlpCritics(_Family):
    lstm = False
    names = tuple(f"c{c}.{n}" for c in (1, 2) for n in tq.NAMES)
    leaves = ("actions",)
    position = staticmethod(lambda w: w[:, 4:5 * ((w.shape[1]) // 5):5])
    aux = staticmethod(lambda B, gen: {"actions": torch.rand((B, 1), generator=gen) * 2 - 1})

    def __init__(self, variant):
        self.variant = variant

    def build(self, H, W, seed):
        return [tq._critic(H, W, seed, self.variant), tq._critic(H, W, seed + 1, self.variant)]

    params = staticmethod(tq._params)

    def fused(self, env, mods):
        from finenvs_amd.mlp_critic import FusedTwinMLPCritic

        return FusedTwinMLPCritic(env, *mods)

    def torch_out(self, mods, states, aux):
        return tuple(m(states, aux["actions"]) for m in mods)

    def fused_out(self, fused, src, pos, aux):
        return tuple(fused.q(src, pos, aux["actions"]))

    def preacts(self, mods, states, aux):
        return [hot_preactivations(m, states, actions=aux["actions"]) for m in mods]


FAMILIES = {"head": Head, "critics": Critics, "sac": Sac, "mlp": Mlp, "mlp2": lambda v: Mlp(v, t2), "mlp critics": MlpCritics}

# (family, variant, H, W, B) -> (gate scale, output scale, module seed): chosen on the f64 copy alone
HOT = {
    ('head', 'tanh', 32, 4, 33): (100, 30, 22),
    ('head', 'tanh', 64, 5, 257): (60, 30, 29),  # W = 5: SHORTENED below
    ('head', 'tanh', 128, 4, 33): (100, 20, 47),
    ('head', 'tanh', 32, 1, 33): (100, 50, 20),
    ('head', 'tanh', 256, 4, 33): (100, 20, 33),
    ('head', 'none', 32, 4, 33): (100, 1, 20),
    ('head', 'none', 128, 4, 33): (100, 1, 20),
    ('head', 'none', 32, 1, 33): (100, 1, 20),
    ('head', 'none', 256, 4, 33): (100, 1, 20),
    ('critics', None, 32, 4, 33): (60, 1, 20),
    ('critics', None, 64, 7, 257): (60, 1, 22),
    ('critics', None, 128, 4, 33): (100, 1, 20),
    ('critics', None, 32, 1, 33): (100, 1, 20),
    ('critics', None, 256, 4, 33): (100, 1, 20),
    ('sac', None, 32, 4, 33): (100, 50, 20),
    ('sac', None, 128, 4, 33): (100, 50, 20),
    ('sac', None, 32, 1, 33): (100, 80, 20),
    ('sac', None, 256, 4, 33): (60, 30, 20),
    ('mlp', 'elu', 32, 4, 33): (40, 0.3, 22),
    ('mlp', 'elu', 64, 7, 257): (30, 0.3, 20),
    ('mlp', 'elu', 128, 4, 33): (40, 0.2, 21),
    ('mlp', 'elu', 32, 1, 33): (20, 0.5, 20),
    ('mlp', 'relu', 32, 4, 33): (40, 0.3, 22),
    ('mlp', 'relu', 64, 7, 257): (30, 0.3, 20),
    ('mlp', 'relu', 128, 4, 33): (40, 0.2, 21),
    ('mlp', 'relu', 32, 1, 33): (20, 0.5, 20),
    ('mlp', 'tanh', 32, 4, 33): (40, 5, 20),
    ('mlp', 'tanh', 64, 7, 257): (30, 8, 21),
    ('mlp', 'tanh', 128, 4, 33): (40, 8, 21),
    ('mlp', 'tanh', 32, 1, 33): (20, 20, 20),
    ('mlp2', 'elu', 32, 4, 33): (40, 0.12, 20),
    ('mlp2', 'elu', 64, 7, 257): (30, 0.3, 20),
    ('mlp2', 'elu', 128, 4, 33): (40, 0.2, 20),
    ('mlp2', 'elu', 32, 1, 33): (30, 0.3, 21),
    ('mlp2', 'relu', 32, 4, 33): (40, 0.12, 20),
    ('mlp2', 'relu', 64, 7, 257): (30, 0.3, 20),
    ('mlp2', 'relu', 128, 4, 33): (40, 0.2, 20),
    ('mlp2', 'relu', 32, 1, 33): (30, 0.3, 21),
    ('mlp2', 'tanh', 32, 4, 33): (40, 8, 20),
    ('mlp2', 'tanh', 64, 7, 257): (30, 8, 20),
    ('mlp2', 'tanh', 128, 4, 33): (40, 8, 20),
    ('mlp2', 'tanh', 32, 1, 33): (30, 12, 21),
    ('mlp critics', 'elu', 32, 4, 33): (30, 1, 20),
    ('mlp critics', 'elu', 64, 7, 257): (30, 1, 20),
    ('mlp critics', 'elu', 128, 4, 33): (30, 1, 20),
    ('mlp critics', 'elu', 32, 1, 33): (30, 1, 20),
    ('mlp critics', 'relu', 32, 4, 33): (30, 1, 20),
    ('mlp critics', 'relu', 64, 7, 257): (30, 1, 20),
    ('mlp critics', 'relu', 128, 4, 33): (30, 1, 20),
    ('mlp critics', 'relu', 32, 1, 33): (30, 1, 20),
    ('mlp critics', 'tanh', 32, 4, 33): (30, 1, 20),
    ('mlp critics', 'tanh', 64, 7, 257): (30, 1, 20),
    ('mlp critics', 'tanh', 128, 4, 33): (30, 1, 20),
    ('mlp critics', 'tanh', 32, 1, 33): (30, 1, 20),
    ('head', 'none', 64, 7, 257): (60, 1, 20),
    ('sac', None, 64, 5, 257): (60, 30, 21),  # W = 5: SHORTENED below
}


# (family, variant, H, W, B) -> worst err / tol (values, gradients, position column), measured on an MI355X; then the
# sharpness gap max|g_torch32 - g64| / max|g64| of GPU torch, the rows whose returned output is exactly +-1.0 and the shares the
# case reached in per cent: |z| > 17, > 60, < 2 (per module) and, after the bar, |p| < 2, in (4, 9), > 9.1.  No case has a kink pair.
MEASURED = {
    ('head', 'tanh', 32, 4, 33): (0.112, 0.179, 0.168),  # gap 8.2e-06; rows at +-1.0: 7; shares % 66 15 4 | 24 36 21
    ('head', 'tanh', 64, 5, 257): (0.261, 0.239, 0.173),  # gap 1.7e-04; rows at +-1.0: 39; shares % 48 2 7 | 27 34 14
    ('head', 'tanh', 128, 4, 33): (0.432, 0.223, 0.129),  # gap 1.0e-04; rows at +-1.0: 2; shares % 66 14 4 | 27 36 6
    ('head', 'tanh', 32, 1, 33): (0.063, 0.104, 0.104),  # gap 1.6e-05; rows at +-1.0: 7; shares % 69 17 4 | 27 30 21
    ('head', 'tanh', 256, 4, 33): (0.279, 0.222, 0.135),  # gap 6.9e-05; rows at +-1.0: 4; shares % 66 14 4 | 39 21 9
    ('head', 'none', 32, 4, 33): (0.221, 0.490, 0.490),  # gap 3.0e-05; rows at +-1.0: 0; shares % 69 18 4
    ('head', 'none', 128, 4, 33): (0.133, 0.582, 0.570),  # gap 3.4e-05; rows at +-1.0: 0; shares % 65 14 4
    ('head', 'none', 32, 1, 33): (0.008, 0.024, 0.013),  # gap 1.1e-06; rows at +-1.0: 0; shares % 69 17 4
    ('head', 'none', 256, 4, 33): (0.264, 0.446, 0.286),  # gap 5.7e-04; rows at +-1.0: 0; shares % 66 14 4
    ('head', 'none', 64, 7, 257): (0.078, 0.310, 0.154),  # gap 5.5e-04; rows at +-1.0: 0; shares % 50 3 6
    ('critics', None, 32, 4, 33): (0.205, 0.311, 0.277),  # gap 5.7e-05; rows at +-1.0: 0; shares % 53 4 6 / 55 5 6
    ('critics', None, 64, 7, 257): (0.309, 0.450, 0.261),  # gap 7.4e-04; rows at +-1.0: 0; shares % 51 3 6 / 50 3 6
    ('critics', None, 128, 4, 33): (0.380, 0.476, 0.460),  # gap 9.5e-05; rows at +-1.0: 0; shares % 66 15 4 / 67 15 4
    ('critics', None, 32, 1, 33): (0.053, 0.183, 0.165),  # gap 1.6e-06; rows at +-1.0: 0; shares % 69 17 3 / 70 18 3
    ('critics', None, 256, 4, 33): (0.418, 0.954, 0.895),  # gap 1.3e-04; rows at +-1.0: 0; shares % 66 14 4 / 66 14 4
    ('sac', None, 32, 4, 33): (0.464, 0.558, 0.558),  # gap 6.2e-05; rows at +-1.0: 5; shares % 69 18 4 | 21 48 12
    ('sac', None, 128, 4, 33): (0.988, 0.284, 0.125),  # gap 7.1e-05; rows at +-1.0: 4; shares % 65 14 4 | 30 39 9
    ('sac', None, 32, 1, 33): (0.163, 0.015, 0.008),  # gap 5.3e-05; rows at +-1.0: 4; shares % 69 17 4 | 39 24 12
    ('sac', None, 256, 4, 33): (0.494, 0.458, 0.445),  # gap 6.8e-05; rows at +-1.0: 5; shares % 46 2 7 | 21 52 15
    ('sac', None, 64, 5, 257): (0.274, 0.501, 0.495),  # gap 1.5e-04; rows at +-1.0: 50; shares % 49 3 6 | 23 38 17
    ('mlp', 'elu', 32, 4, 33): (0.020, 0.072, 0.034),  # gap 2.6e-07; rows at +-1.0: 2; shares % 71 22 3 | 30 30 6
    ('mlp', 'elu', 64, 7, 257): (0.067, 0.064, 0.054),  # gap 9.0e-07; rows at +-1.0: 14; shares % 67 15 4 | 29 34 5
    ('mlp', 'elu', 128, 4, 33): (0.035, 0.025, 0.025),  # gap 8.8e-07; rows at +-1.0: 5; shares % 74 24 4 | 24 48 15
    ('mlp', 'elu', 32, 1, 33): (0.020, 0.040, 0.011),  # gap 2.5e-06; rows at +-1.0: 6; shares % 60 10 5 | 42 24 18
    ('mlp', 'relu', 32, 4, 33): (0.020, 0.145, 0.045),  # gap 9.0e-07; rows at +-1.0: 2; shares % 71 22 3 | 30 36 6
    ('mlp', 'relu', 64, 7, 257): (0.063, 0.060, 0.023),  # gap 6.3e-07; rows at +-1.0: 15; shares % 67 15 4 | 30 34 5
    ('mlp', 'relu', 128, 4, 33): (0.016, 0.010, 0.007),  # gap 1.6e-06; rows at +-1.0: 5; shares % 74 24 4 | 24 48 15
    ('mlp', 'relu', 32, 1, 33): (0.027, 0.156, 0.007),  # gap 1.7e-06; rows at +-1.0: 6; shares % 60 10 5 | 46 24 18
    ('mlp', 'tanh', 32, 4, 33): (0.120, 0.148, 0.072),  # gap 5.9e-06; rows at +-1.0: 2; shares % 76 24 4 | 42 24 6
    ('mlp', 'tanh', 64, 7, 257): (0.143, 0.079, 0.057),  # gap 5.8e-06; rows at +-1.0: 45; shares % 67 12 4 | 27 35 15
    ('mlp', 'tanh', 128, 4, 33): (0.073, 0.171, 0.092),  # gap 1.3e-05; rows at +-1.0: 8; shares % 74 24 4 | 30 30 21
    ('mlp', 'tanh', 32, 1, 33): (0.035, 0.248, 0.248),  # gap 3.7e-06; rows at +-1.0: 10; shares % 60 10 5 | 30 24 30
    ('mlp2', 'elu', 32, 4, 33): (0.026, 0.101, 0.050),  # gap 1.0e-06; rows at +-1.0: 9; shares % 76 24 4 | 27 36 27
    ('mlp2', 'elu', 64, 7, 257): (0.122, 0.076, 0.076),  # gap 2.3e-06; rows at +-1.0: 47; shares % 67 15 4 | 26 34 17
    ('mlp2', 'elu', 128, 4, 33): (0.164, 0.069, 0.042),  # gap 2.1e-06; rows at +-1.0: 3; shares % 74 26 3 | 27 33 9
    ('mlp2', 'elu', 32, 1, 33): (0.003, 0.055, 0.025),  # gap 5.4e-07; rows at +-1.0: 3; shares % 67 14 4 | 21 55 9
    ('mlp2', 'relu', 32, 4, 33): (0.050, 0.023, 0.012),  # gap 3.1e-07; rows at +-1.0: 9; shares % 76 24 4 | 27 36 27
    ('mlp2', 'relu', 64, 7, 257): (0.058, 0.058, 0.058),  # gap 1.4e-06; rows at +-1.0: 45; shares % 67 15 4 | 27 34 16
    ('mlp2', 'relu', 128, 4, 33): (0.043, 0.064, 0.057),  # gap 6.8e-07; rows at +-1.0: 3; shares % 74 26 3 | 30 33 6
    ('mlp2', 'relu', 32, 1, 33): (0.045, 0.026, 0.021),  # gap 7.2e-07; rows at +-1.0: 4; shares % 67 14 4 | 21 48 9
    ('mlp2', 'tanh', 32, 4, 33): (0.086, 0.097, 0.096),  # gap 1.2e-05; rows at +-1.0: 4; shares % 76 24 4 | 24 39 12
    ('mlp2', 'tanh', 64, 7, 257): (0.148, 0.102, 0.102),  # gap 7.6e-06; rows at +-1.0: 18; shares % 67 15 4 | 32 33 6
    ('mlp2', 'tanh', 128, 4, 33): (0.064, 0.221, 0.162),  # gap 2.4e-06; rows at +-1.0: 3; shares % 74 26 3 | 33 39 9
    ('mlp2', 'tanh', 32, 1, 33): (0.049, 0.171, 0.083),  # gap 4.5e-06; rows at +-1.0: 4; shares % 67 14 4 | 21 42 12
    ('mlp critics', 'elu', 32, 4, 33): (0.011, 0.047, 0.021),  # gap 6.0e-07; rows at +-1.0: 0; shares % 66 15 3 / 70 19 4
    ('mlp critics', 'elu', 64, 7, 257): (0.015, 0.089, 0.054),  # gap 1.8e-06; rows at +-1.0: 0; shares % 68 16 4 / 68 14 4
    ('mlp critics', 'elu', 128, 4, 33): (0.018, 0.069, 0.031),  # gap 3.8e-06; rows at +-1.0: 0; shares % 68 15 4 / 67 13 4
    ('mlp critics', 'elu', 32, 1, 33): (0.014, 0.053, 0.044),  # gap 1.2e-06; rows at +-1.0: 0; shares % 74 26 3 / 69 15 4
    ('mlp critics', 'relu', 32, 4, 33): (0.011, 0.017, 0.013),  # gap 3.0e-07; rows at +-1.0: 0; shares % 66 15 3 / 70 19 4
    ('mlp critics', 'relu', 64, 7, 257): (0.012, 0.022, 0.018),  # gap 5.7e-07; rows at +-1.0: 0; shares % 68 16 4 / 68 14 4
    ('mlp critics', 'relu', 128, 4, 33): (0.011, 0.017, 0.014),  # gap 4.0e-07; rows at +-1.0: 0; shares % 68 15 4 / 67 13 4
    ('mlp critics', 'relu', 32, 1, 33): (0.015, 0.008, 0.006),  # gap 2.7e-07; rows at +-1.0: 0; shares % 74 26 3 / 69 15 4
    ('mlp critics', 'tanh', 32, 4, 33): (0.024, 0.334, 0.086),  # gap 2.8e-06; rows at +-1.0: 0; shares % 66 15 3 / 70 19 4
    ('mlp critics', 'tanh', 64, 7, 257): (0.042, 0.073, 0.106),  # gap 7.3e-06; rows at +-1.0: 0; shares % 68 16 4 / 68 14 4
    ('mlp critics', 'tanh', 128, 4, 33): (0.020, 0.077, 0.050),  # gap 2.4e-06; rows at +-1.0: 0; shares % 68 15 4 / 67 13 4
    ('mlp critics', 'tanh', 32, 1, 33): (0.018, 0.136, 0.049),  # gap 2.4e-06; rows at +-1.0: 0; shares % 74 26 3 / 69 15 4
}
# the chained losses, the SAC head against its contract (err / tol per group) and the hot rollouts' shares:
#   td3 chained (64, 7, 257): 0.225 (module seed 20)
#   td3 chained (32, 1, 33): 0.171 (module seed 20)
#   sac chained (64, 7, 257): 0.321 (module seed 20, output scale halved 1 times)
#   sac chained (32, 1, 33): 0.096 (module seed 20, output scale halved 2 times)
#   rollout H = 32: shares 64 15 4 %
#   rollout H = 128: shares 65 16 4 %
#   rollout H = 256: shares 45 2 8 %
#   mlp rollout: shares 42 0 6 %
#   sac forward H = 32: {'means': 0.017, 'stds': 0.178, 'actions |u| <= 4': 0.004, 'log_probs |u| <= 4': 0.243, 'actions |u| > 4': 0.003, 'log_probs |u| > 4': 0.0} rows at +-1.0: 69
#   sac forward H = 128: {'means': 0.04, 'stds': 0.282, 'actions |u| <= 4': 0.003, 'log_probs |u| <= 4': 0.246, 'actions |u| > 4': 0.003, 'log_probs |u| > 4': 0.0} rows at +-1.0: 64
#   sac forward H = 256: {'means': 0.025, 'stds': 0.312, 'actions |u| <= 4': 0.004, 'log_probs |u| <= 4': 0.247, 'actions |u| > 4': 0.003, 'log_probs |u| > 4': 0.0} rows at +-1.0: 61
#   sac backward H = 32: {'both': 0.048, 'd_actions only': 0.027, 'd_log_probs only': 0.045}
#   sac backward H = 128: {'both': 0.047, 'd_actions only': 0.18, 'd_log_probs only': 0.04}
#   sac backward H = 256: {'both': 0.044, 'd_actions only': 0.07, 'd_log_probs only': 0.042}


def cases(family):
    return [k for k in HOT if k[0] == family]


# ------------------------------------------------------------------------------------------ a hot case and its reference
def descriptors(H, W, B):
    return crafted_descriptors(DAYS - 1, BARS + W, W, B, seed=1100 + H + W)  # (D, L) of the env's table: see cpu_states


def hot_case(case, states, dev, seed=None):
    """The family, its hot modules and the case's other inputs (drawn on the CPU, so that a CPU test sees the same)."""
    family, variant, H, W, B = case
    gate, out, seed0 = HOT[case] if case in HOT else CHAINED_SCALES[case]
    seed = seed0 if seed is None else seed
    fam = FAMILIES[family](variant)
    mods = [heat(m, gate, out).to(dev) for m in fam.build(H, W, seed)]
    gen = torch.Generator().manual_seed(7000 + H + W)
    aux = {k: v.to(dev) for k, v in fam.aux(B, gen).items()}
    n_out = 2 if family in ("critics", "sac", "mlp critics") else 1
    cs = [torch.randn((B, 1), generator=gen).to(dev) for _ in range(n_out)]
    return fam, mods, aux, cs


def shares(fam, mods, states, aux):
    """``hot_shares`` of every module of the case (asserted), and the kink mask of an MLP family."""
    out, kink = [], torch.zeros((states.shape[0], 1), dtype=torch.bool, device=states.device)
    for m, (z, p) in zip(mods, fam.preacts(mods, states, aux)):
        out.append(hot_shares(z, p, fam.lstm, fam.tanh_output))
        if not fam.lstm:
            zs = [z]
            if len([x for x in m.network if isinstance(x, torch.nn.Linear)]) == 3:  # the second hidden layer
                m64 = copy.deepcopy(m).double()
                with torch.no_grad():
                    zs.append(m64.network[2](m64.network[1](z)))
            for x in zs:
                kink |= (x.abs() < 1e-5 * max(1.0, float(x.abs().mean()))).any(dim=1, keepdim=True)
            if m.activation == "elu":  # both ends of __expf: inf above 88.7 (behind a select), 0 below -104
                assert bool((z > 88.7).any()) and bool((z < -104).any())
    assert int(kink.sum()) <= 0.02 * states.shape[0], int(kink.sum())
    return out, kink


def _loss(outs, cs, keep):
    return sum((torch.where(keep, o, o.detach()) * c.to(o.dtype)).sum() for o, c in zip(outs, cs))


def torch_eval(fam, mods, states, aux, cs, keep, dtype):
    ms = [copy.deepcopy(m).to(dtype) for m in mods]
    tl._zero(*ms)
    a = {k: v.detach().to(dtype).clone().requires_grad_(k in fam.leaves) for k, v in aux.items()}
    outs = fam.torch_out(ms, states.to(dtype), a)
    loss = _loss(outs, cs, keep)
    loss.backward()
    grads = [p.grad for m in ms for p in fam.params(m)] + [a[k].grad for k in fam.leaves]
    return [o.detach() for o in outs], loss.detach(), grads


def fused_eval(fam, fused, mods, src, pos, aux, cs, keep):
    tl._zero(*mods)
    a = {k: v.detach().clone().requires_grad_(k in fam.leaves) for k, v in aux.items()}
    outs = fam.fused_out(fused, src, pos, a)
    loss = _loss(outs, cs, keep)
    loss.backward()
    grads = [p.grad.clone() for m in mods for p in fam.params(m)] + [a[k].grad.clone() for k in fam.leaves]
    return [o.detach() for o in outs], loss.detach(), grads


RESOLVE = 2e-5  # the yardstick's floor, relative
# SHORTENED: the two tanh-output LSTM families run (64, 5, 257) in place of (64, 7, 257).  At W = 7 no module seed from 20 to 119
# at gate scale 60 (output scales 20 and 30; at gate scale 40 the share beyond 60 is 0.3 %) gives the head a b_out whose
# ``one_element_response`` is below 2.9e-5 (typically 1e-4 to 1e-3), and none from 20 to 59 gives the SAC actor a resolvable
# b_mu and b_std: a case that cannot meet a condition is not a case, and W is shortened until one does (W = 6: the SAC actor
# only; W = 5: both).  The chained losses below keep (64, 7, 257) and their own conditions, with these scales:
CHAINED_SCALES = {("head", "tanh", 64, 7, 257): (60, 20, 20), ("sac", None, 64, 7, 257): (60, 20, 20)}


def one_element_response(fam, mods, states, aux, cs, keep, g64, names):
    """``{name: r}`` for every ONE-ELEMENT gradient tensor: the rms over four draws of ``|g64(theta (1 + 2^-24 xi)) - g64(theta)|
    / |g64(theta)|``, ``xi ~ N(0, 1)`` per weight -- what one f32 rounding of the weights does to that gradient, measured on
    the f64 copy alone.  The maximum over a many-element tensor concentrates, so four times torch f32's realised error is a
    bound there even where rounding noise dominates; a one-element tensor's tolerance is four times ONE draw of that noise,
    which can be arbitrarily small, so only the floor ``2e-5 |g64|`` can be relied on and it has to cover the noise: the rule
    of tests/test_mlp2_head_gpu.py::_output_bias_gradient_is_resolvable with the ulp of p replaced by the response the hot
    recurrence gives it.  Met at b_out of (head, tanh, 64, 7, 257): err / tol 2.507 and 1.006 at two seeds where the other
    five tensors show 0.13 to 0.70; its response is 1e-4 to 1e-3 there."""
    gen = torch.Generator().manual_seed(24)  # on the CPU: the same draws on every device
    acc = [0.0] * len(g64)
    for _ in range(4):
        pm = [copy.deepcopy(m).double() for m in mods]
        with torch.no_grad():
            for m in pm:
                for p in m.parameters():
                    p.mul_(1 + 2.0 ** -24 * torch.randn(p.shape, generator=gen, dtype=F64).to(p.device))
        for i, (a, b) in enumerate(zip(torch_eval(fam, pm, states, aux, cs, keep, F64)[2], g64)):
            if b.numel() == 1:
                acc[i] += float((a - b).abs().max()) ** 2 / 4
    return {n: acc[i] ** 0.5 / float(b.abs().max()) for i, (n, b) in enumerate(zip(names, g64)) if b.numel() == 1}


def conditioned(case, states, dev):
    """``reference`` of the first module seed from the case's own up that meets every condition (the siblings'
    ``_conditioned_module``); ``HOT`` holds the seeds that do, so that nothing is re-drawn and the CPU test of the shares
    sees the modules the GPU runs.  The FIRST such seed from 20 up, never the one with the smallest torch gap among several: the
    gap is one draw of f32 noise, and picking its minimum picks torch's lucky draws and makes four times that draw too tight
    (met: SAC chained at seed 35, picked that way, w_ih err / tol 1.603 with torch's gap 6.0e-5 where seeds 36, 37 and 29 show
    5.8e-4, 1.6e-4 and 2.2e-4 and the kernel's error is 3.9e-4 against 3.1e-4, 1.6e-4 and 7.3e-4; NOTES.md)."""
    seed0 = HOT[case][2]
    for seed in range(seed0, seed0 + 16):
        try:
            return reference(case, states, dev, seed) + (seed,)
        except AssertionError as exc:
            print(f"REDRAW {case!r}: module seed {seed} misses a condition ({str(exc)[:160]}); trying {seed + 1}")
    raise AssertionError(f"no module seed meets the conditions of {case!r}")


def reference(case, states, dev, seed=None):
    """The case's conditions on its reference, asserted: the shares, no degenerate f64 gradient, the sharpness cap.
    Returns what the comparison needs."""
    fam, mods, aux, cs = hot_case(case, states, dev, seed)
    sh, kink = shares(fam, mods, states, aux)
    if case[0] == "sac":
        cs = [cs[0], torch.where(fam.preacts(mods, states, aux)[0][1].abs() <= SAC_GUARD_U, cs[1], torch.zeros_like(cs[1]))]
    r32 = torch_eval(fam, mods, states, aux, cs, ~kink, F32)
    r64 = torch_eval(fam, mods, states, aux, cs, ~kink, F64)
    names = list(fam.names) + list(fam.leaves)
    W = case[3]
    gap = 0.0
    for name, gt, gd in zip(names, r32[2], r64[2]):
        top = float(gd.abs().max())
        assert (top > 0) != (name.endswith("w_hh") and W == 1), (case, name)  # not degenerate
        if top:
            gap = max(gap, float((gt.double() - gd).abs().max()) / top)
    assert gap <= CAP, (case, gap)
    response = one_element_response(fam, mods, states, aux, cs, ~kink, r64[2], names)
    assert all(r <= RESOLVE for r in response.values()), (case, "a one-element tensor is not resolvable", response)
    return fam, mods, aux, cs, kink, r32, r64, names, sh, gap


# ------------------------------------------------------------------------------------------------------------ on the GPU
@functools.lru_cache(maxsize=None)
def _env(B, W):
    env = tl._env(B, W)
    assert tuple(int(x) for x in env.geometry()) == (DAYS - 1, BARS + W, W, 1)
    return env


def _batch(H, W, B):
    env = _env(B, W)
    src, pos = descriptors(H, W, B)
    env.check_descriptors(src.cuda())
    states = env.render(src.cuda(), pos.cuda())
    ref, _ = cpu_states(DAYS, BARS, W, TABLE_SEED, src, pos)
    assert float((states.cpu() - ref).abs().max()) <= 1e-12  # the batch the CPU test of the shares sees
    return env, src.cuda(), pos.cuda(), states


def _yardstick(label, tally, names, g, g32, g64, zero=()):
    for name, gf, gt, gd in zip(names, g, g32, g64):
        assert gf.shape == gd.shape and gf.dtype is F32, (label, name)
        assert bool(torch.isfinite(gf).all()), (label, name)
        err, tol = tg._ratio(gf, gt, gd)
        print(f"{label} {name:10s} err {err:.3e} tol {tol:.3e} ratio {err / tol if tol else err:.3f}")
        assert err <= tol, (label, name, err, tol)
        tally[0] = max(tally[0], err / tol if tol else err)


OUT_NAMES = {"head": ("y",), "critics": ("q1", "q2"), "sac": ("actions", "log_probs"), "mlp": ("y",), "mlp2": ("y",),
             "mlp critics": ("q1", "q2")}


def _same_on_saturated_rows(case, seed, fam, fused, mods, src, pos, aux, keep, y):
    """Rows whose returned output is exactly +-1.0 contribute nothing: zeroing their upstream gradient changes no bit."""
    S = y.abs() == 1.0
    n = int(S.sum())
    assert 0 < n < S.numel(), (case, n)
    _, _, _, cs = hot_case(case, None, "cuda", seed)  # as drawn (SAC: the log-probability's too)
    _, _, g_all = fused_eval(fam, fused, mods, src, pos, aux, cs, keep)
    _, _, g_cut = fused_eval(fam, fused, mods, src, pos, aux, [torch.where(S, torch.zeros_like(c), c) for c in cs], keep)
    names = list(fam.names) + list(fam.leaves)
    which = ("w_mu", "b_mu") if case[0] == "sac" else names  # S contributes du = 0; the std path keeps -gl / s
    for name, a, b in zip(names, g_all, g_cut):
        if name in which:
            assert torch.equal(a, b), (case, name, float((a - b).abs().max()))
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), (case, name)
    return n


def _check(case):
    family, variant, H, W, B = case
    env, src, pos, states = _batch(H, W, B)
    fam, mods, aux, cs, kink, r32, r64, names, sh, gap, seed = conditioned(case, states, "cuda")
    fused = fam.fused(env, mods)
    outs, loss, g = fused_eval(fam, fused, mods, src, pos, aux, cs, ~kink)
    values, grads, position = [0.0], [0.0], [0.0]
    u64 = fam.preacts(mods, states, aux)[0][1] if family == "sac" else None
    for name, o, o32, o64 in zip(OUT_NAMES[family], outs, r32[0], r64[0]):
        assert bool(torch.isfinite(o).all()), (case, name)
        if name == "log_probs":  # the bound of the family's forward test: compared where |u| <= 4, finite beyond
            rows = u64.abs() <= 4
            assert 0 < int(rows.sum()) < B
            o, o32, o64 = o[rows], o32[rows], o64[rows]
        _yardstick(str(case), values, [name], [o], [o32], [o64])
    _yardstick(str(case), grads, names, g, r32[2], r64[2])
    per = len(fam.names) // len(mods)
    for k in range(len(mods)):
        w, w32, w64 = (fam.position(x[k * per]) for x in (g, r32[2], r64[2]))
        assert float(w64.abs().max()) > 0
        _yardstick(str(case), position, [f"position {k}"], [w], [w32], [w64])
    err, tol = abs(float(loss) - float(r64[1])), 2e-5 * abs(float(r64[1])) + 4 * abs(float(r32[1]) - float(r64[1])) + 1e-7
    assert err <= tol, (case, "loss", err, tol)
    n = _same_on_saturated_rows(case, seed, fam, fused, mods, src, pos, aux, ~kink, outs[0]) if fam.tanh_output else 0
    print(f"MEASURED {case!r}: ({values[0]:.3f}, {grads[0]:.3f}, {position[0]:.3f}),  # seed {seed} gap {gap:.1e} rows at +-1.0: {n} "
          f"kink {int(kink.sum())} shares {[{k: round(v, 3) for k, v in s.items()} for s in sh]}")


@pytest.mark.parametrize("case", cases("head"), ids=str)
def test_lstm_head(case):
    _check(case)


@pytest.mark.parametrize("case", cases("critics"), ids=str)
def test_twin_critics(case):
    _check(case)


@pytest.mark.parametrize("case", cases("sac"), ids=str)
def test_sac_actor(case):
    _check(case)


@pytest.mark.parametrize("case", cases("mlp"), ids=str)
def test_mlp_head(case):
    _check(case)


@pytest.mark.parametrize("case", cases("mlp2"), ids=str)
def test_mlp2_head(case):
    _check(case)


@pytest.mark.parametrize("case", cases("mlp critics"), ids=str)
def test_twin_mlp_critics(case):
    _check(case)


# ------------------------------------------------------------------------------------------------- the chained losses
# (H, W, B, the critics are hot).  At (64, 7, 257) the critics the hot actor is chained through are the family's ORDINARY
# ones: a hot critic's d q / d a reaches 700 with a curvature of 1e6, the hot actor's f32 output (torch's) is off by up to
# 3e-4 from its f64 copy's, and torch f32 then misses the f64 gradient by 0.35 max|g64| (TD3) and 0.15 (SAC) at the critics'
# gate scale 60, by 0.02 to 0.3 at 30, and still by 1e-2 at 10, where no gate of the critic is beyond 17 any more; the cap of
# 1e-3 holds from 5 down (CPU torch, NOTES.md).  A case that cannot meet the cap is not a case.  At W = 1 both are hot.
CHAINED = [(64, 7, 257, False), (32, 1, 33, True)]


def _capped(label, names, g32, g64, W):
    for name, gt, gd in zip(names, g32, g64):
        top = float(gd.abs().max())
        assert (top > 0) != (name == "w_hh" and W == 1), (label, name)
        assert float((gt.double() - gd).abs().max()) <= CAP * top, (label, name)


def _twin(env, states, shape, hot):
    from finenvs_amd.critic import FusedTwinCritic

    H, W, B = shape
    if not hot:
        return FusedTwinCritic(env, tc._critic(H, W, 10), tc._critic(H, W, 11))
    fam, mods, aux, _ = hot_case(("critics", None) + shape, states, "cuda")
    shares(fam, mods, states, aux)
    return FusedTwinCritic(env, *mods)


def _chained(label, names, W, g, g32, g64, loss, l32, l64):
    _capped(label, names, g32, g64, W)
    worst = [0.0]
    _yardstick(label, worst, names, g, g32, g64)
    _yardstick(label, worst, ["w_ih[:, 4]"], [g[0][:, 4]], [g32[0][:, 4]], [g64[0][:, 4]])
    err, tol = abs(float(loss) - float(l64)), 2e-5 * abs(float(l64)) + 4 * abs(float(l32) - float(l64)) + 1e-7
    assert err <= tol, (label, "loss", err, tol)
    return worst[0]


@pytest.mark.parametrize("H,W,B,hot", CHAINED)
def test_td3_actor_loss_of_the_hot_head(H, W, B, hot):
    """``-q1(s, y(s)).mean()`` (TD3/actor.py:50-56) of the hot tanh head through the twin critics."""
    from finenvs_amd.lstm_head import FusedLSTMHead

    env, src, pos, states = _batch(H, W, B)
    twin = _twin(env, states, (H, W, B), hot)
    seed0 = 20
    for seed in range(seed0, seed0 + 16):  # the first module seed whose references meet the conditions of this loss
        fam, mods, aux, _ = hot_case(("head", "tanh", H, W, B), states, "cuda", seed)
        l32, g32, _ = tl._torch_grads("td3", mods[0], twin.critic_1, states.float(), None, F32)
        l64, g64, _ = tl._torch_grads("td3", mods[0], twin.critic_1, states.double(), None, F64)
        try:
            shares(fam, mods, states, aux)
            _capped("td3", tl.NAMES, g32, g64, W)
            break
        except AssertionError as exc:
            print(f"REDRAW td3 chained: module seed {seed} misses a condition ({str(exc)[:120]})")
    head = FusedLSTMHead(env, mods[0])
    loss, g = tl._fused_grads("td3", head, twin, src, pos, None)
    worst = _chained("td3", tl.NAMES, W, g, g32, g64, loss, l32, l64)
    print(f"MEASURED td3 chained ({H}, {W}, {B}): {worst:.3f} (module seed {seed})")


@pytest.mark.parametrize("H,W,B,hot", CHAINED)
def test_sac_chained_loss_of_the_hot_actor(H, W, B, hot):
    """``Actor.compute_losses`` (SAC/actor.py:63-81; the ``chained`` kind of tests/test_sac_grad_gpu.py).  Its
    log-probability term reaches every pair with the same weight, so (``SAC_GUARD_U`` above) the actor keeps its gate
    scale and its OUTPUT scale is halved until the f64 copy has ``max|u| <= 6`` on the batch."""
    from finenvs_amd.sac import FusedSACRollout

    env, src, pos, states = _batch(H, W, B)
    twin = _twin(env, states, (H, W, B), hot)
    seed0 = 20
    for seed in range(seed0, seed0 + 16):  # the first module seed whose references meet the conditions of this loss
        fam, mods, aux, cs = hot_case(("sac", None, H, W, B), states, "cuda", seed)
        halvings = 0
        while float(fam.preacts(mods, states, aux)[0][1].abs().max()) > SAC_GUARD_U:
            heat(mods[0], 1.0, 0.5)
            halvings += 1
            assert halvings < 12
        eps, c = aux["eps"], cs[0]
        l32, g32, _ = tsac._torch_grads("chained", mods[0], twin.critic_1, twin.critic_2, states.float(), eps, c, F32)
        l64, g64, _ = tsac._torch_grads("chained", mods[0], twin.critic_1, twin.critic_2, states.double(), eps, c, F64)
        try:
            hot_shares(fam.preacts(mods, states, aux)[0][0], None, True, False)  # the gates stay hot
            _capped("sac chained", tsac.NAMES, g32, g64, W)
            break
        except AssertionError as exc:
            print(f"REDRAW sac chained: module seed {seed} misses a condition ({str(exc)[:120]})")
    roll = FusedSACRollout(env, mods[0])
    loss, g, _ = tsac._fused_grads("chained", roll, twin, src, pos, eps, c)
    worst = _chained("sac chained", tsac.NAMES, W, g, g32, g64, loss, l32, l64)
    print(f"MEASURED sac chained ({H}, {W}, {B}): {worst:.3f} (module seed {seed}, output scale halved {halvings} times)")


# ------------------------------------------------------------------------------------------ an all-saturated batch: zero
@pytest.mark.parametrize("case", [("head", "tanh", 32, 4, 33)] + [("mlp", a, 32, 4, 33) for a in ACTIVATIONS], ids=str)
def test_an_all_saturated_batch_gives_exactly_zero(case):
    """The output bias raised until every returned ``y`` is exactly +-1.0: ``dp = c (1 - y y)`` is exactly 0 for every
    pair, and so is every gradient -- in torch f32 on the same batch too."""
    family, variant, H, W, B = case
    env, src, pos, states = _batch(H, W, B)
    fam, mods, aux, cs = hot_case(case, states, "cuda")
    (_, p), = fam.preacts(mods, states, aux)
    out = mods[0].last_layer[0] if family == "head" else mods[0].network[2]
    with torch.no_grad():
        out.bias.add_(float(p.abs().max()) + 20.0)
    keep = torch.ones((B, 1), dtype=torch.bool, device="cuda")
    outs, _, g = fused_eval(fam, fam.fused(env, mods), mods, src, pos, aux, cs, keep)
    o32, _, g32 = torch_eval(fam, mods, states, aux, cs, keep, F32)
    assert bool((outs[0] == 1.0).all()) and bool((o32[0] == 1.0).all())
    for name, a, b in zip(fam.names, g, g32):
        assert bool((a == 0).all()), (case, name, float(a.abs().max()))
        assert bool((b == 0).all()), (case, name, "torch f32")


# ------------------------------------------------------------------- forward bit parity with the oracle at hot weights
class _Bare(torch.nn.Module):
    """``lstm`` and ``last_layer`` under the names ``heat`` and ``hot_preactivations`` read."""

    def __init__(self, lstm, lin):
        super().__init__()
        self.lstm, self.last_layer = lstm, torch.nn.Sequential(lin, torch.nn.Tanh())


@pytest.mark.parametrize("H,gate", [(32, 100.0), (128, 100.0), (256, 100.0)])
def test_hot_lstm_rollout_equals_the_oracle_bit_for_bit(H, gate):
    """N = 35, K = 3, W = 4 in lock-step with ``fo.policy_lstm``: the oracle's header promises the bits of the
    exact-operation sigmoid / tanh; the clamp at -60 and the division without range handling are the two places where
    that could break, and only gates beyond 60 reach them.  H = 256: the fused streamed kernel."""
    import finenvs_amd as fe
    from finenvs_amd.rollout import FusedLSTMRollout
    from oracle import fe_oracle as fo
    from tests import test_lstm_rollout_gpu as tr

    fo.build()
    N, K, W = 35, 3, 4
    ref, env = tr._make(fe, fo, N, 1, W, 6, 40, 0.0, False, seed=3 * N + W)
    lstm, lin = tr._modules(H, seed=W + H, gain=6.0 if H <= 128 else 2.0)
    heat(_Bare(lstm, lin), gate, 4.0)
    whh, wx, wout, bout = tr._packed(fo, lstm, lin)
    roll = FusedLSTMRollout.from_modules(env, lstm, lin)
    if H > 128:
        roll.split = False  # the fused large-H kernel (so few pairs would otherwise take the per-time-step path)
    obs = ref.reset().copy()
    z, p = hot_preactivations(_Bare(lstm, lin), torch.from_numpy(obs))
    s = hot_shares(z, p, True, False)
    acts, rews, dones = roll.run(K)
    seen = set()
    for k in range(K):
        a_ref = fo.policy_lstm(obs, whh, wx, wout, bout)
        seen.update(np.unique(a_ref).tolist())
        obs, r_ref, d_ref, _ = ref.step(a_ref)
        obs = obs.copy()
        tr.assert_bits(tr.t2n(acts[k]), a_ref, f"H = {H} step {k} actions")
        tr.assert_bits(tr.t2n(rews[k]), r_ref, f"H = {H} step {k} rewards")
    tr.assert_bits(tr.t2n(roll.observation()), obs, "observation()")
    assert len(seen) > 5, sorted(seen)[:8]
    print(f"MEASURED rollout H = {H}: shares {s}")


def test_hot_mlp_rollout_with_tanh_hidden_equals_the_oracle_bit_for_bit():
    """The MLP rollout's tanh hidden activation is the same ``lstm_tanh``: N = 35, K = 3, W = 4, first layer times 20."""
    import finenvs_amd as fe
    from finenvs_amd.rollout import FusedMLPRollout
    from oracle import fe_oracle as fo
    from tests import test_mlp_rollout_gpu as tm

    fo.build()
    N, K, W, H, gate = 35, 3, 4, 64, 20.0
    ref, env = tm._make(fe, fo, N, 1, W, 6, 40, 0.0, False, seed=3 * N + W)
    W1, b1, W2, b2 = tm._weights(W, H, seed=W + H)
    W1, b1 = (W1 * np.float32(gate)).astype(np.float32), (b1 * np.float32(gate)).astype(np.float32)
    w1t, wpos = fo.mlp_pack(W1, W)
    roll = FusedMLPRollout(env, torch.from_numpy(W1), torch.from_numpy(b1), torch.from_numpy(W2), float(b2), activation="tanh")
    obs = ref.reset().copy()
    z = torch.from_numpy(obs.reshape(N, -1).astype(np.float64)) @ torch.from_numpy(W1.astype(np.float64)) + torch.from_numpy(b1.astype(np.float64))
    s = hot_shares(z, None, False, False)
    acts, rews, dones = roll.run(K)
    seen = set()
    for k in range(K):
        a_ref = fo.policy_mlp(obs, w1t, wpos, b1, W2, b2, act=2)
        seen.update(np.unique(a_ref).tolist())
        obs, r_ref, d_ref, _ = ref.step(a_ref)
        obs = obs.copy()
        tm.assert_bits(tm.t2n(acts[k]), a_ref, f"step {k} actions")
        tm.assert_bits(tm.t2n(rews[k]), r_ref, f"step {k} rewards")
    assert len(seen) >= 3, sorted(seen)[:8]
    print(f"MEASURED mlp rollout: shares {s}")


# ------------------------------------------------------------------ the SAC head against its own contract, head-locally
SAC_COUNT = 97  # three full tiles and one pair
EPS7 = float(np.float32(1e-7))  # the guard, the f32 constant
SPECIAL_NOISE = (0.0, 4.0, -4.0, 8.0, -8.0)


POOL = 3000


def _sac_bands(q):
    """Above the threshold of F.softplus where ``expf`` overflows; above it; just below and just above it; far below."""
    return [q > 89, (q > 20) & (q < 30), (q > 19) & (q < 20), (q > 20) & (q < 21), q < -10]


def _sac_q(actor, states):
    a64 = copy.deepcopy(actor).double()
    with torch.no_grad():
        return a64.std_layer(a64(states.double())).reshape(-1)


def _sac_select(actor, pstates, gen):
    """Shifts and scales ``actor.std_layer`` (in place) so that the f64 q of the pool's 10 % and 90 % quantiles are -15 and
    100 -- what lies outside is not drawn from, so the ends of the span are as densely populated as its middle -- and
    returns 97 rows of the pool: both ends, six of every band of ``_sac_bands`` and a random rest, shuffled."""
    ranked = _sac_q(actor, pstates).sort().values
    lo, hi = float(ranked[POOL // 10]), float(ranked[POOL - 1 - POOL // 10])
    k = 115.0 / (hi - lo)
    with torch.no_grad():
        actor.std_layer.bias.copy_(k * (actor.std_layer.bias.double() - lo) - 15.0)
        actor.std_layer.weight.mul_(k)
    q = _sac_q(actor, pstates).cpu()
    inside = (q >= -15.001) & (q <= 100.001)
    chosen = [int(torch.where(inside, q, torch.full_like(q, 1e9)).argmin()), int(torch.where(inside, q, torch.full_like(q, -1e9)).argmax())]
    for b in _sac_bands(q):
        chosen += [i for i in torch.nonzero(b & inside).reshape(-1).tolist() if i not in chosen][:6]
    rest = [i for i in torch.randperm(POOL, generator=gen).tolist() if bool(inside[i]) and i not in chosen]
    return torch.tensor(chosen + rest[:SAC_COUNT - len(chosen)])[torch.randperm(SAC_COUNT, generator=gen)]


def _sac_setup(H, W=4):
    """An ordinary ``_actor`` whose ``std_layer`` is shifted and scaled so that, on the f64 copy, q spans [-15, 100] over a
    pool of crafted descriptors; of the pool, 97 pairs with at least five in each band the head's code distinguishes."""
    from finenvs_amd.sac import FusedSACRollout

    env = _env(SAC_COUNT, W)
    psrc, ppos = crafted_descriptors(DAYS - 1, BARS + W, W, POOL, seed=1300 + H)  # every window several times, positions anew
    env.check_descriptors(psrc.cuda())
    actor = tsac._actor(H, W, 20)
    gen = torch.Generator().manual_seed(H)
    chosen = _sac_select(actor, env.render(psrc.cuda(), ppos.cuda()), gen)
    src, pos = psrc[chosen].cuda(), ppos[chosen].cuda()
    states = env.render(src, pos)
    q = _sac_q(actor, states)
    assert -15.01 < float(q.min()) < -14.5 and 99.5 < float(q.max()) < 100.01, (float(q.min()), float(q.max()))
    assert all(int(b.sum()) >= 5 for b in _sac_bands(q)), [int(b.sum()) for b in _sac_bands(q)]
    noise = torch.randn((SAC_COUNT, 1), generator=gen)
    noise[:3 * len(SPECIAL_NOISE), 0] = torch.tensor(SPECIAL_NOISE * 3)
    roll = FusedSACRollout(env, actor, streamed=H > 128)
    assert roll.streamed == (H > 128)
    return env, roll, actor, src, pos, states, noise.cuda(), gen


def _bound(label, got, t32, r64, rows=None):
    if rows is not None:
        got, t32, r64 = got[rows], t32[rows], r64[rows]
    assert bool(torch.isfinite(got).all()), label
    err = float((got.double() - r64).abs().max())
    tol = 2e-5 * float(r64.abs().max()) + 4 * float((t32.double() - r64).abs().max())
    print(f"{label:32s} err {err:.3e} tol {tol:.3e} ratio {err / tol:.3f}")
    assert err <= tol, (label, err, tol)
    return err / tol


def _sac_forward_contract(roll, actor, src, pos, states, noise, title):
    """The forward contract of a SAC head (the LSTM actor's or, tests/test_mlp_sac_contract_gpu.py, the MLP actor's): means
    and stds (relative) against the f64 copy within the yardstick, then actions and log_probs head-locally, from the
    kernel's own f32 means and stds.  Returns what ``roll.forward`` returned."""
    from torch.distributions import Normal

    actions, log_probs, means, stds = roll.forward(src, pos, noise)
    ref = {}
    for dtype in (F32, F64):
        a = copy.deepcopy(actor).to(dtype)
        with torch.no_grad():
            dist = a.get_distribution(states.to(dtype))
        ref[dtype] = (dist.loc, dist.scale)
    worst = {"means": _bound("means", means, ref[F32][0], ref[F64][0])}
    s64 = ref[F64][1]
    assert float(s64.min()) < 4e-7 and float(s64.max()) > 99  # they span 3e-7 to 100: in relative terms
    worst["stds"] = _bound("stds (relative)", stds.double() / s64, ref[F32][1].double() / s64, torch.ones_like(s64))
    assert bool(torch.isfinite(stds).all()) and bool((stds > 0).all())
    # head-local: from the kernel's own f32 means and stds and the given noise
    u64 = means.double() + noise.double() * stds.double()
    a64 = torch.tanh(u64)
    lp64 = Normal(means.double(), stds.double()).log_prob(u64) - torch.log(1 - actions.double().pow(2) + EPS7)
    u32 = means + noise * stds  # as SACActorLSTM.get_actions_and_log_probs writes it
    a32 = torch.tanh(u32)
    lp32 = Normal(means, stds).log_prob(u32) - torch.log(1 - torch.tanh(u32).pow(2) + 1e-7)
    inner = u64.abs() <= 4
    assert int(inner.sum()) >= 10 and int((~inner).sum()) >= 10
    for label, rows in (("|u| <= 4", inner), ("|u| > 4", ~inner)):
        worst[f"actions {label}"] = _bound(f"actions {label}", actions, a32, a64, rows)
        worst[f"log_probs {label}"] = _bound(f"log_probs {label}", log_probs, lp32, lp64, rows)
    # where the action is exactly +-1.0 the squash term is -log(1e-7f), to within 4 ulp of 16.1 (plus the yardstick's
    # allowance for the Gaussian term, which the kernel returns only inside the sum)
    S = actions.abs() == 1.0
    assert 5 <= int(S.sum()) < SAC_COUNT
    n64 = Normal(means.double(), stds.double()).log_prob(u64)[S]
    n32 = Normal(means, stds).log_prob(u32)[S].double()
    squash = log_probs.double()[S] - n64
    allow = 4 * 2.0 ** -20 + 2e-5 * float(n64.abs().max()) + 4 * float((n32 - n64).abs().max())
    assert float((squash + np.log(EPS7)).abs().max()) <= allow, (float((squash + np.log(EPS7)).abs().max()), allow)
    print(f"MEASURED {title}: {({k: round(v, 3) for k, v in worst.items()})} rows at +-1.0: {int(S.sum())}")
    return actions, log_probs, means, stds


@pytest.mark.parametrize("H", [32, 128, 256])
def test_sac_head_forward_contract(H):
    env, roll, actor, src, pos, states, noise, _ = _sac_setup(H)
    _sac_forward_contract(roll, actor, src, pos, states, noise, f"sac forward H = {H}")


GRID_ACTIONS = [0.0] + [s * v for v in (0.5, 0.999, 1 - 2.0 ** -12, 1 - 2.0 ** -23, 1 - 2.0 ** -24, 1.0) for s in (1, -1)]
GRID_STDS = [1e-6, 1e-3, 0.3, 5.0, 25.0]


def _surrogate_grads(actor, states, du, ds, dtype, params=tsac._params):
    a = copy.deepcopy(actor).to(dtype)
    tl._zero(a)
    hid = a(states.to(dtype))
    (du.detach() * a.mu_layer(hid) + ds.detach() * torch.nn.functional.softplus(a.std_layer(hid))).sum().backward()
    return [p.grad for p in params(a)]


def _sac_grid(gen, count=SAC_COUNT):
    """Crafted ``actions`` x ``stds`` (``GRID_ACTIONS`` x ``GRID_STDS``, the rest drawn from the grid) and the upstream
    gradients ``ga``, ``gl`` with zeros sprinkled in, each (count, 1) f32 on the device."""
    grid = [(a, s) for a in GRID_ACTIONS for s in GRID_STDS]
    grid += [grid[i] for i in torch.randint(0, len(grid), (count - len(grid),), generator=gen).tolist()]
    actions = torch.tensor([g[0] for g in grid], dtype=F64).float().reshape(-1, 1).cuda()
    stds = torch.tensor([g[1] for g in grid], dtype=F64).float().reshape(-1, 1).cuda()
    assert int((actions.abs() == 1.0).sum()) >= 10 and float(actions.abs().max()) == 1.0
    ga, gl = (torch.randn((count, 1), generator=gen) for _ in range(2))
    ga[5::11] = 0.0
    gl[7::13] = 0.0
    return actions, stds, ga.cuda(), gl.cuda()


def _sac_contract_grads(actor, states, noise, actions, stds, da, dl, params=tsac._params):
    """``{dtype: gradients}`` of the surrogate ``sum(du mu(theta) + ds softplus(q(theta)))`` with the contract's ``du``, ``ds``
    (include/finenvs_amd_sac_grad.h, include/finenvs_amd_mlp_sac.h) in f32 and f64; ``da`` / ``dl`` None: no upstream."""
    per = {}
    for dtype in (F32, F64):
        a, s, e = actions.to(dtype), stds.to(dtype), noise.to(dtype)
        xa = torch.zeros_like(a) if da is None else da.to(dtype)
        xl = torch.zeros_like(a) if dl is None else dl.to(dtype)
        om = 1 - a * a
        du = xa * om + xl * (2 * a * om / (om + (EPS7 if dtype is F64 else 1e-7)))
        ds = du * e - xl / s
        per[dtype] = _surrogate_grads(actor, states, du, ds, dtype, params)
    return per


UPSTREAMS = ("both", "d_actions only", "d_log_probs only")


@pytest.mark.parametrize("H", [32, 128, 256])
def test_sac_head_backward_contract_on_crafted_forward_outputs(H):
    """``fe_sac_backward(_streamed)`` takes ``actions`` and ``stds`` as inputs: a grid up to a = +-1 and s = 1e-6, against
    the contract of include/finenvs_amd_sac_grad.h in f64 -- ``om = 1 - a^2``, ``du = ga om + gl 2 a om / (om + 1e-7f)``,
    ``ds = du eps - gl / s`` per pair, the parameter gradients the backward of ``sum(du mu(theta) + ds softplus(q(theta)))``."""
    from finenvs_amd import _lib
    from finenvs_amd.sac import SAC_GRAD_KEYS

    W = 4
    env, roll, actor, src, pos, states, noise, gen = _sac_setup(H, W)
    roll.forward(src, pos, noise)  # packs the weights the backward reads
    actions, stds, ga, gl = _sac_grid(gen)
    params = tsac._params(actor)
    lib = env._lib
    floats = lib.fe_sac_streamed_grad_workspace_floats if roll.streamed else lib.fe_sac_grad_workspace_floats
    backward = lib.fe_sac_backward_streamed if roll.streamed else lib.fe_sac_backward
    w, (bmu, bstd) = roll._packed, roll._biases
    worst = {}
    for label, da, dl in zip(UPSTREAMS, (ga, ga, None), (gl, None, gl)):
        ws = torch.full((int(floats(H, W, SAC_COUNT)),), float("nan"), dtype=F32, device="cuda")
        g = [torch.full(p.shape, float("nan"), dtype=F32, device="cuda") for p in params]
        sg = _lib.FeSacGrads(*(x.data_ptr() for x in g))
        _lib.check(backward(
            env._handle, roll._lr32.data_ptr(), w["whh"].data_ptr(), w["wx"].data_ptr(), w["wl"].data_ptr(),
            w["bl"].data_ptr(), w["wmu"].data_ptr(), bmu, w["wstd"].data_ptr(), bstd, H, src.data_ptr(), pos.data_ptr(),
            SAC_COUNT, noise.data_ptr(), actions.data_ptr(), stds.data_ptr(), None if da is None else da.data_ptr(),
            None if dl is None else dl.data_ptr(), ws.data_ptr(), C.byref(sg), env._stream()), lib)
        torch.cuda.synchronize()
        per = _sac_contract_grads(actor, states, noise, actions, stds, da, dl)
        tally = [0.0]
        for name, gf, gd in zip(SAC_GRAD_KEYS, g, per[F64]):
            assert bool(torch.isfinite(gf).all()), (label, name)
            assert float(gd.abs().max()) > 0, (label, name)
        _yardstick(f"H = {H} {label}", tally, SAC_GRAD_KEYS, g, per[F32], per[F64])
        worst[label] = round(tally[0], 3)
    print(f"MEASURED sac backward H = {H}: {worst}")
