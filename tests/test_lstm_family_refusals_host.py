"""CPU: what the LSTM-family entries refuse before they touch the env, and in which order.

The one-output head, the SAC actor and the twin critics each exist register-resident (H = 32 / 64 / 128) and streamed
(H = 256 / 512 / 1024), some with *_p siblings (output biases in device memory) and *_c siblings (the ring's cursor in
device memory); an entry and its siblings share one host implementation in csrc/fe_env.hip.  Every argument set below is
refused before `env` is dereferenced, so made-up non-null pointers do: no device is needed.  Return code and whole message
stand here as the library gave them before the host paths were shared; sets in which two refusals apply at once pin the
order of each entry's checks, which differs between siblings in places (the two SAC rollouts).  Refusals that need the
env (A = 1, the LDS fit, the ring's size / head / assets, an unbound state) are the GPU suites'."""
import ctypes as C

import pytest

P = 16  # a made-up non-null pointer, never dereferenced
NAN = float("nan")


def _structs():
    from finenvs_amd import _lib

    return {"cw": _lib.FeCriticWeights, "cg": _lib.FeCriticGrads, "lg": _lib.FeLstmGrads, "sg": _lib.FeSacGrads,
            "ring": _lib.FeReplayRing}


# "name" a pointer (default P), "name=value" a scalar, "name:kind" a pointer to a struct whose pointers default to P
_HEAD_ROLLOUT = "env lr32 whh wx wout bout=0.25 H=32 out_act=0 K=2 src pos noise std=0.5 actions means rewards dones ssrc spos"
_HEAD_FORWARD = "env lr32 whh wx wout bout=0.25 H=32 out_act=0 src pos count=4 out"
_HEAD_BACKWARD = "env lr32 whh wx wout H=%d out_act=2 src pos count=4 outputs d_outputs workspace grads:lg"
_SAC_ROLLOUT = "env lr32 whh wx wl bl wmu bmu=0.5 wstd bstd=0.5 H=%d K=2 src pos noise actions means stds rewards dones ssrc spos"
_SAC_FORWARD = "env lr32 whh wx wl bl wmu bmu=0.5 wstd bstd=0.5 H=%d src pos count=4 noise actions log_probs means stds"
_SAC_BACKWARD = ("env lr32 whh wx wl bl wmu bmu=0.5 wstd bstd=0.5 H=%d src pos count=4 noise actions stds d_actions d_log_probs "
                 "workspace grads:sg")
_Q_FORWARD = "env lr32 c1:cw c2:cw H=%d src pos actions count=4 q1 q2"
_Q_TARGET = ("env lr32 c1:cw c2:cw H=%d ring:ring head=0 size=4 indices count=4 next_actions smooth_noise=None smooth_std=0.25 "
             "smooth_clip=0.5 log_probs=None alpha=None gamma=0.5 reward_scale=1.0 targets q1 q2")
_Q_BACKWARD = "env lr32 c1:cw c2:cw H=%d src pos actions count=4 dq1 dq2 workspace grads1:cg grads2:cg d_actions"


def _by_pointer(spec):
    return spec.replace("bout=0.25", "bout").replace("bmu=0.5", "bmu").replace("bstd=0.5", "bstd")


_SPECS = {
    "fe_env_rollout_lstm": _HEAD_ROLLOUT, "fe_env_rollout_lstm_p": _by_pointer(_HEAD_ROLLOUT),
    "fe_lstm_forward": _HEAD_FORWARD, "fe_lstm_forward_p": _by_pointer(_HEAD_FORWARD),
    "fe_lstm_backward": _HEAD_BACKWARD % 32, "fe_lstm_backward_streamed": _HEAD_BACKWARD % 256,
    "fe_env_rollout_sac": _SAC_ROLLOUT % 32, "fe_env_rollout_sac_p": _by_pointer(_SAC_ROLLOUT % 32),
    "fe_env_rollout_sac_streamed": _by_pointer(_SAC_ROLLOUT % 256),
    "fe_sac_forward": _SAC_FORWARD % 32, "fe_sac_forward_p": _by_pointer(_SAC_FORWARD % 32),
    "fe_sac_forward_streamed": _by_pointer(_SAC_FORWARD % 256),
    "fe_sac_backward": _SAC_BACKWARD % 32, "fe_sac_backward_p": _by_pointer(_SAC_BACKWARD % 32),
    "fe_sac_backward_streamed": _by_pointer(_SAC_BACKWARD % 256),
    "fe_twin_q_forward": _Q_FORWARD % 32, "fe_twin_q_forward_streamed": _Q_FORWARD % 256,
    "fe_twin_q_target": _Q_TARGET % 32, "fe_twin_q_target_streamed": _Q_TARGET % 256,
    "fe_twin_q_target_c": (_Q_TARGET % 32).replace("head=0 size=4", "cursor"),
    "fe_twin_q_target_streamed_c": (_Q_TARGET % 256).replace("head=0 size=4", "cursor"),
    "fe_twin_q_backward": _Q_BACKWARD % 32, "fe_twin_q_backward_streamed": _Q_BACKWARD % 256,
}


def _call(lib, name, overrides):
    """Calls entry `name` with its spec's defaults and `overrides`: {"src": None}, {"H": 48}, a whole struct
    {"grads": None} or one of its fields {"grads.w_ih": None}, {"ring.capacity": 0}.  The stream is null."""
    structs, args, keep, used = _structs(), [], [], set()
    for token in _SPECS[name].split():
        key, kind, value = token, None, P
        if "=" in token:
            key, text = token.split("=")
            value = None if text == "None" else (float(text) if "." in text else int(text))
        elif ":" in token:
            key, kind = token.split(":")
        if key in overrides:
            value = overrides[key]
            used.add(key)
        if kind and value is not None:
            fields = {f: (8 if f == "capacity" else 1 if f == "num_assets" else 0 if f == "reserved" else P)
                      for f, _ in structs[kind]._fields_}
            for k, v in overrides.items():
                if k.startswith(key + "."):
                    assert k[len(key) + 1:] in fields, k
                    fields[k[len(key) + 1:]] = v
                    used.add(k)
            keep.append(structs[kind](*(fields[f] for f, _ in structs[kind]._fields_)))
            value = C.byref(keep[-1])
        args.append(value)
    assert used == set(overrides), (name, set(overrides) - used)  # a misspelt override would test nothing
    return getattr(lib, name)(*args, None)


def _nulls(names):
    return [{n: None} for n in names.split()]


_H_BAD = (16, 48, 129, 2048)
_CW = "c1 c1.whh c1.wx c1.wout c1.bout c2 c2.whh c2.wx c2.wout c2.bout"
_RING = "ring ring.state_src ring.state_pos ring.next_src ring.next_pos ring.actions ring.rewards ring.dones ring.errors"
_LG = "grads grads.w_ih grads.w_hh grads.b_ih grads.b_hh grads.w_out grads.b_out"
_SG = _LG.replace(" grads.w_out grads.b_out", "") + " grads.w_l grads.b_l grads.w_mu grads.b_mu grads.w_std grads.b_std"
_SAC_W = "whh wx wl bl wmu wstd"

# entry -> [(message, [argument sets that get it])]; the return code is FE_ERR_ARG throughout
_REFUSED = {}


def _head_rollout(name, first):
    who = "fe_env_rollout_lstm"  # the _p sibling reports under this name once its own pointer is there
    _REFUSED[name] = first + [
        (who + ": states_src_out and states_pos_out go together",
         [{"ssrc": None}, {"spos": None}, {"ssrc": None, "env": None}, {"spos": None, "std": -0.5}, {"ssrc": None, "out_act": 3}]),
        (who + ": std must be >= 0 when noise is given", [{"std": -0.5}, {"std": NAN}, {"std": -0.5, "whh": None}, {"std": -1.0, "K": 0}]),
        (who + ": bad argument",
         _nulls("env lr32 whh wx wout src pos rewards dones") + [{"K": 0}, {"K": -1}, {"K": 0, "out_act": 3}, {"dones": None, "out_act": -1}]),
        (who + ": out_activation must be 0 (tanh) or 1 (clamp)", [{"out_act": -1}, {"out_act": 2}, {"out_act": 3}]),
    ]


_head_rollout("fe_env_rollout_lstm", [])
_head_rollout("fe_env_rollout_lstm_p", [("fe_env_rollout_lstm_p: bad argument",
                                         [{"bout": None}, {"bout": None, "ssrc": None}, {"bout": None, "std": -0.5}])])


def _head_forward(name, first):
    who = "fe_lstm_forward"
    _REFUSED[name] = first + [
        (who + ": bad argument",
         _nulls("env lr32 whh wx wout src pos out") + [{"count": -1}, {"out": None, "out_act": 3}, {"count": -1, "H": 48}]),
        (who + ": out_activation must be 0 (tanh), 1 (clamp) or 2 (none)", [{"out_act": -1}, {"out_act": 3}, {"out_act": 3, "H": 16}]),
    ] + [(who + ": H must be 32, 64, 128, 256, 512 or 1024 (got %d)" % H, [{"H": H}, {"H": H, "out_act": 1}]) for H in _H_BAD]


_head_forward("fe_lstm_forward", [])
_head_forward("fe_lstm_forward_p", [("fe_lstm_forward_p: bad argument", [{"bout": None}, {"bout": None, "out_act": 3}, {"bout": None, "H": 16}])])


def _head_backward(who, other, h_message):
    _REFUSED[who] = [
        (who + ": bad argument",
         _nulls("env lr32 whh wx wout src pos d_outputs workspace " + _LG) +
         [{"count": -1}, {"src": None, "out_act": 1}, {"grads.b_out": None, "H": 48}, {"workspace": None, "out_act": 0, "outputs": None}]),
    ] + [(who + ": out_activation must be 0 (tanh) or 2 (none); 1 (clamp) has no gradient to train on (got %d)" % a,
          [{"out_act": a}, {"out_act": a, "H": 16}, {"out_act": a, "outputs": None}]) for a in (-1, 1, 3)] + [
        (who + ": out_activation 0 (tanh) needs outputs, the values fe_lstm_forward returned",
         [{"out_act": 0, "outputs": None}, {"out_act": 0, "outputs": None, "H": 48}]),
    ] + [(who + h_message % H, [{"H": H}, {"H": H, "out_act": 0}, {"H": H, "outputs": None}]) for H in _H_BAD + (other,)]


_head_backward("fe_lstm_backward", 256, ": H must be 32, 64 or 128 (got %d): the streamed-weight forward of H >= 256 has no "
               "register-resident recurrence to mirror")
_head_backward("fe_lstm_backward_streamed", 64, ": H must be 256, 512 or 1024 (got %d); fe_lstm_backward runs H = 32, 64 and 128")

_SAC_H = ": H must be 256, 512 or 1024 (got %d); %s runs H = 32, 64 and 128"


def _sac_rollout_resident(name, first):
    who = "fe_env_rollout_sac"  # H is refused after the state is known to be bound: the GPU suites' case
    _REFUSED[name] = first + [
        (who + ": states_src_out and states_pos_out go together",
         [{"ssrc": None}, {"spos": None}, {"ssrc": None, "whh": None}, {"spos": None, "env": None}, {"ssrc": None, "K": 0},
          {"spos": None, "dones": None}]),
        (who + ": bad argument", _nulls("env lr32 src pos rewards dones " + _SAC_W) + [{"K": 0}, {"K": -1}, {"K": 0, "wl": None}]),
    ]


_sac_rollout_resident("fe_env_rollout_sac", [])
_sac_rollout_resident("fe_env_rollout_sac_p", [("fe_env_rollout_sac_p: bad argument",
                                                [{"bmu": None}, {"bstd": None}, {"bmu": None, "ssrc": None}, {"bstd": None, "K": 0}])])
_REFUSED["fe_env_rollout_sac_streamed"] = [
    ("fe_env_rollout_sac_streamed: bad argument",
     _nulls("env lr32 src pos rewards dones bmu bstd " + _SAC_W) +
     [{"K": 0}, {"K": -1}, {"ssrc": None, "whh": None}, {"spos": None, "env": None}, {"ssrc": None, "K": 0}, {"spos": None, "dones": None},
      {"ssrc": None, "bmu": None}, {"wl": None, "H": 16}]),
    ("fe_env_rollout_sac_streamed: states_src_out and states_pos_out go together",
     [{"ssrc": None}, {"spos": None}, {"ssrc": None, "H": 16}, {"spos": None, "H": 64}]),
] + [("fe_env_rollout_sac_streamed" + _SAC_H % (H, "fe_env_rollout_sac"), [{"H": H}, {"H": H, "noise": None}]) for H in _H_BAD + (64,)]


def _sac_forward(name, who, first, other, h_message):
    _REFUSED[name] = first + [
        (who + ": bad argument",
         _nulls("env lr32 src pos " + _SAC_W) + [{"count": -1}, {"pos": None, "noise": None}, {"count": -1, "H": 16}]),
        (who + ": actions_out and log_probs_out need noise",
         [{"noise": None}, {"noise": None, "actions": None}, {"noise": None, "log_probs": None}, {"noise": None, "H": 16}]),
    ] + [(who + h_message(H), [{"H": H}, {"H": H, "actions": None, "log_probs": None, "noise": None}]) for H in _H_BAD + (other,)]


def _sac_h_resident(H):
    return ": H must be 32, 64 or 128 (got %d): the SAC head has no streamed or split kernel" % H


_sac_forward("fe_sac_forward", "fe_sac_forward", [], 256, _sac_h_resident)
_sac_forward("fe_sac_forward_p", "fe_sac_forward",
             [("fe_sac_forward_p: bad argument", [{"bmu": None}, {"bstd": None}, {"bmu": None, "noise": None}, {"bstd": None, "H": 16}])],
             256, _sac_h_resident)
_sac_forward("fe_sac_forward_streamed", "fe_sac_forward_streamed", [], 64, lambda H: _SAC_H % (H, "fe_sac_forward"))
_REFUSED["fe_sac_forward_streamed"][0][1].extend([{"bmu": None}, {"bstd": None}, {"bmu": None, "noise": None}, {"bstd": None, "H": 16}])


def _sac_backward(name, who, first, other, h_message):
    _REFUSED[name] = first + [
        (who + ": bad argument",
         _nulls("env lr32 src pos noise actions stds workspace " + _SAC_W + " " + _SG) +
         [{"count": -1}, {"d_actions": None, "d_log_probs": None}, {"stds": None, "H": 16}, {"grads.w_l": None, "H": 2048},
          {"d_actions": None, "d_log_probs": None, "H": 48}]),
    ] + [(who + h_message(H), [{"H": H}, {"H": H, "d_actions": None}, {"H": H, "d_log_probs": None}]) for H in _H_BAD + (other,)]


_sac_backward("fe_sac_backward", "fe_sac_backward", [], 256, lambda H: ": H must be 32, 64 or 128 (got %d)" % H)
_sac_backward("fe_sac_backward_p", "fe_sac_backward",
              [("fe_sac_backward_p: bad argument", [{"bmu": None}, {"bstd": None}, {"bmu": None, "H": 16}, {"bstd": None, "stds": None}])],
              256, lambda H: ": H must be 32, 64 or 128 (got %d)" % H)
_sac_backward("fe_sac_backward_streamed", "fe_sac_backward_streamed", [], 64, lambda H: _SAC_H % (H, "fe_sac_backward"))
_REFUSED["fe_sac_backward_streamed"][0][1].extend([{"bmu": None}, {"bstd": None}, {"bmu": None, "H": 16}])


def _critic_h(who, streamed):
    if streamed:
        return (who + ": H must be 256, 512 or 1024 (got %d); H = 32, 64 and 128 run the register-resident entries of "
                "finenvs_amd_critic.h / finenvs_amd_critic_grad.h")
    return who + ": H must be 32, 64 or 128 (got %d): the twin critic has no streamed or split kernel"


for _who, _streamed in (("fe_twin_q_forward", False), ("fe_twin_q_forward_streamed", True)):
    _REFUSED[_who] = [
        (_who + ": bad argument",
         _nulls("env lr32 src pos actions q1 q2 " + _CW) + [{"count": -1}, {"q2": None, "H": 16}, {"c2.bout": None, "H": 48}, {"count": -1, "H": 129}]),
    ] + [(_critic_h(_who, _streamed) % H, [{"H": H}]) for H in _H_BAD + (64 if _streamed else 256,)]

for _name, _who, _streamed in (("fe_twin_q_target", "fe_twin_q_target", False), ("fe_twin_q_target_c", "fe_twin_q_target", False),
                               ("fe_twin_q_target_streamed", "fe_twin_q_target_streamed", True),
                               ("fe_twin_q_target_streamed_c", "fe_twin_q_target_streamed", True)):
    _first = []
    if _name.endswith("_c"):
        _first = [(_name + ": null cursor", [{"cursor": None}, {"cursor": None, "env": None}, {"cursor": None, "log_probs": P}, {"cursor": None, "H": 16}])]
    _REFUSED[_name] = _first + [
        (_who + ": bad argument",
         _nulls("env lr32 indices next_actions targets q1 q2 " + _CW + " " + _RING) +
         [{"count": -1}, {"ring.capacity": 0}, {"ring.num_assets": 0}, {"indices": None, "log_probs": P}, {"targets": None, "H": 16},
          {"c1.wx": None, "smooth_noise": P, "log_probs": P, "alpha": P}]),
        (_who + ": log_probs (SAC) need alpha", [{"log_probs": P}, {"log_probs": P, "H": 16}, {"log_probs": P, "smooth_noise": P}]),
        (_who + ": smooth_noise (TD3) and log_probs (SAC) are exclusive",
         [{"smooth_noise": P, "log_probs": P, "alpha": P}, {"smooth_noise": P, "log_probs": P, "alpha": P, "H": 16}]),
    ] + [(_critic_h(_who, _streamed) % H, [{"H": H}, {"H": H, "smooth_noise": P}, {"H": H, "log_probs": P, "alpha": P}])
         for H in _H_BAD + (64 if _streamed else 256,)]

for _who, _streamed in (("fe_twin_q_backward", False), ("fe_twin_q_backward_streamed", True)):
    _h = _critic_h(_who, True) if _streamed else _who + ": H must be 32, 64 or 128 (got %d)"
    _REFUSED[_who] = [
        (_who + ": bad argument",
         _nulls("env lr32 src pos actions workspace " + _CW + " " + _LG.replace("grads", "grads1")[7:] + " " + _LG.replace("grads", "grads2")[7:]) +
         [{"count": -1}, {"grads1": None, "d_actions": None}, {"grads2": None, "d_actions": None}, {"workspace": None, "H": 16},
          {"grads2.w_out": None, "H": 48}, {"grads2": None, "d_actions": None, "H": 129}, {"dq1": None, "c2": None}]),
    ] + [(_h % H, [{"H": H}, {"H": H, "dq1": None, "c1": None}, {"H": H, "dq2": None, "c2": None, "grads2": None}, {"H": H, "grads1": None},
                   {"H": H, "d_actions": None}, {"H": H, "dq1": None, "dq2": None, "c1": None, "c2": None}])
         for H in _H_BAD + (64 if _streamed else 256,)]


def test_every_entry_of_the_family_has_a_table():
    assert sorted(_REFUSED) == sorted(_SPECS) and len(_SPECS) == 23
    for name, table in _REFUSED.items():
        pairs = [kw for _, sets in table for kw in sets if len({k.split(".")[0] for k in kw}) >= 2]
        assert len(pairs) >= 3, name  # sets in which two refusals apply (or one applies beside a legal variation)


@pytest.mark.parametrize("name", sorted(_SPECS))
def test_refusals_need_no_device_and_keep_their_order(name):
    from finenvs_amd import _lib

    lib = _lib.load()
    for message, sets in _REFUSED[name]:
        for kw in sets:
            rc = _call(lib, name, kw)
            assert rc == _lib.FE_ERR_ARG == -1, (name, kw, rc)
            assert lib.fe_last_error() == message.encode(), (name, kw, lib.fe_last_error())
