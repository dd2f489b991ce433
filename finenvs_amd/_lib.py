"""ctypes binding of include/finenvs_amd.h (the C ABI of the HIP hot path).

This is the only place the package touches the native library.  There is no
fallback: if the library cannot be loaded, or no HIP device is visible, the
environment refuses to construct.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libfinenvs_amd.so")

FE_ABI_VERSION = 5
FE_OK, FE_ERR_ARG, FE_ERR_HIP, FE_ERR_STATE = 0, -1, -2, -3
FE_MAX_ASSETS = 256


class FeConfig(C.Structure):
    """struct fe_config of include/finenvs_amd.h."""

    _fields_ = [
        ("N", C.c_int64), ("D", C.c_int64), ("L", C.c_int64),
        ("W", C.c_int32), ("A", C.c_int32),
        ("max_shares", C.c_int32), ("evaluate", C.c_int32),
        ("starting_balance", C.c_double), ("commission", C.c_double),
        ("init_margin", C.c_double), ("maint_margin", C.c_double),
        ("obs_is_f32", C.c_int32), ("redraw_mode", C.c_int32),
        ("seed", C.c_uint64), ("eval_env", C.c_int64),
    ]


# name -> (restype, argtypes); every symbol include/finenvs_amd.h (the frozen surface) declares
_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32
SIGNATURES = {
    "fe_version": (C.c_int, []),
    "fe_last_error": (C.c_char_p, []),
    "fe_device_count": (C.c_int, []),
    "fe_env_create": (C.c_int, [C.POINTER(FeConfig), _vp, _vp, C.POINTER(_vp)]),
    "fe_env_bind_state": (C.c_int, [_vp] * 10),
    "fe_env_bind_f32_table": (C.c_int, [_vp, _vp]),
    "fe_env_bind_stats": (C.c_int, [_vp, _vp, _vp, _vp]),
    "fe_env_stats_reduce": (C.c_int, [_vp, _vp, _vp]),
    "fe_env_reset_obs": (C.c_int, [_vp, _vp, _vp]),
    "fe_env_step": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "fe_env_describe": (C.c_int, [_vp, _vp, _vp, _vp]),
    "fe_env_render": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "fe_env_step_notify": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_uint64, _vp]),
    "fe_env_step_traj_notify": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_uint64, _vp]),
    "fe_env_step_promoted": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_uint64, _vp]),
    "fe_host_flag_create": (C.c_int, [C.POINTER(_vp)]),
    "fe_host_flag_destroy": (C.c_int, [_vp]),
    "fe_env_render_n": (C.c_int, [_vp, _vp, _vp, _i64, _vp, _vp]),
    "fe_env_check_descriptors": (C.c_int, [_vp, _vp, _i64, C.POINTER(_i64), _vp]),
    "fe_env_step_traj": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "fe_env_rollout_linear": (C.c_int, [_vp, _vp, C.c_double, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "fe_env_set_day": (C.c_int, [_vp, _i64, _i64, _vp]),
    "fe_env_launch_info": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "fe_env_destroy": (C.c_int, [_vp]),
    "fe_build_tag": (C.c_char_p, []),
    "fe_env_device": (C.c_int, [_vp]),
    "fe_env_logret": (_vp, [_vp]),
    "fe_build_logret": (C.c_int, [_vp, _vp, _i64, _i32, _vp]),
    "fe_build_logret_tables": (C.c_int, [_vp, _vp, _i64, _i64, _i32, _vp]),
    "fe_build_tables": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _i32, _vp, _vp]),
    "fe_traj_store": (C.c_int, [_i64, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "fe_traj_returns": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i64, C.c_double, _vp, _vp, _vp]),
    "fe_csv_count_lines": (_i64, [C.c_char_p]),
    "fe_csv_read": (_i64, [C.c_char_p, _i64, _i32, _vp, _vp, _vp, _vp]),
}
# include/finenvs_amd_ext.h: the experimental in-kernel policy heads and the tuning hook (same library)
EXT_SIGNATURES = {
    "fe_policy_table": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "fe_env_rollout_table": (C.c_int, [_vp, _vp, _vp, C.c_double, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "fe_env_rollout_mlp": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_float, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "fe_env_rollout_lstm": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_float, _i32, _i32, _i32, _vp, _vp, _vp, C.c_float, _vp, _vp, _vp,
                                      _vp, _vp, _vp, _vp]),
    "fe_lstm_activations": (C.c_int, [_vp, _vp, _vp, _i64, _vp]),
    "fe_lstm_split_workspace_floats": (_i64, [_i32, _i64]),
    "fe_env_rollout_lstm_split": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_float, _i32, _i32, _i32, _vp, _vp, _vp, C.c_float, _vp, _vp,
                                            _vp, _vp, _vp, _vp, _vp, _vp]),
    "fe_lstm_forward": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_float, _i32, _i32, _vp, _vp, _i64, _vp, _vp]),
    "fe_env_set_launch": (C.c_int, [_vp, _i32, _i32, _i32]),
}

# include/finenvs_amd_evo.h: the evolution-strategies population (finenvs_amd/evo.py; same library)
class FeEvoPopulation(C.Structure):
    """struct fe_evo_population of include/finenvs_amd_evo.h."""

    _fields_ = [
        ("num_train", C.c_int64), ("hidden", C.c_int32), ("max_episodes", C.c_int32),
        ("noise_std", C.c_float), ("action_noise_std", C.c_float), ("seed", C.c_uint64),
        ("generation", C.c_uint32), ("step", C.c_uint32),
        ("logret_f32", _vp), ("theta", _vp), ("obs_src", _vp), ("obs_pos", _vp), ("returns", _vp), ("timesteps", _vp),
        ("episode_returns", _vp), ("episode_counts", _vp), ("counters", _vp), ("scratch_rewards", _vp),
        ("scratch_dones", _vp),
    ]


EVO_SIGNATURES = {
    "fe_evo_rollout": (C.c_int, [_vp, C.POINTER(FeEvoPopulation), _i32, _vp, _vp, _vp, _vp, _vp]),
    "fe_evo_gradient_workspace_doubles": (_i64, [_i64, _i64]),
    "fe_evo_gradient": (C.c_int, [C.c_uint64, C.c_uint32, _i64, _i64, _vp, _vp, _vp, _vp]),
    "fe_evo_noise": (C.c_int, [C.c_uint64, C.c_uint32, _vp, _i64, _i64, _vp, _vp]),
}

# include/finenvs_amd_evo2.h: the same population with two hidden layers (FeEvoPopulation again)
EVO2_SIGNATURES = {
    "fe_evo2_rollout": EVO_SIGNATURES["fe_evo_rollout"],
    "fe_evo2_num_params": (_i64, [_i32, _i32]),
    "fe_evo2_lds_bytes": (_i64, [_i32, _i32, _i32]),
}

# include/finenvs_amd_evo2_streamed.h: the two-hidden-layer population with theta read through L2 (H up to 256)
EVO2_STREAMED_SIGNATURES = {
    "fe_evo2_rollout_streamed": EVO_SIGNATURES["fe_evo_rollout"],
    "fe_evo2_streamed_num_params": (_i64, [_i32, _i32]),
    "fe_evo2_streamed_lds_bytes": (_i64, [_i32, _i32, _i32]),
}


# include/finenvs_amd_replay.h: the off-policy replay ring (finenvs_amd/replay.py; same library)
class FeReplayRing(C.Structure):
    """struct fe_replay_ring of include/finenvs_amd_replay.h."""

    _fields_ = [
        ("capacity", C.c_int64), ("num_assets", C.c_int32), ("reserved", C.c_int32),
        ("state_src", _vp), ("state_pos", _vp), ("next_src", _vp), ("next_pos", _vp), ("actions", _vp),
        ("rewards", _vp), ("dones", _vp), ("errors", _vp),
    ]


REPLAY_SIGNATURES = {
    "fe_replay_append": (C.c_int, [C.POINTER(FeReplayRing), _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp,
                                   _i32, _vp, _vp, _vp]),
    "fe_replay_sample": (C.c_int, [_vp, C.POINTER(FeReplayRing), _i64, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
}

# include/finenvs_amd_sac.h: the SAC actor's head on the fused LSTM rollout (finenvs_amd/sac.py; same library)
SAC_SIGNATURES = {
    "fe_env_rollout_sac": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_float, _vp, C.c_float, _i32, _i32, _vp, _vp, _vp,
                                     _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "fe_sac_forward": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_float, _vp, C.c_float, _i32, _vp, _vp, _i64, _vp,
                                 _vp, _vp, _vp, _vp, _vp]),
}


# include/finenvs_amd_critic.h: the twin LSTM critics and their Bellman targets (finenvs_amd/critic.py; same library)
class FeCriticWeights(C.Structure):
    """struct fe_critic_weights of include/finenvs_amd_critic.h."""

    _fields_ = [("whh", _vp), ("wx", _vp), ("wout", _vp), ("bout", _vp)]


_cw = C.POINTER(FeCriticWeights)
CRITIC_SIGNATURES = {
    "fe_twin_q_forward": (C.c_int, [_vp, _vp, _cw, _cw, _i32, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "fe_twin_q_target": (C.c_int, [_vp, _vp, _cw, _cw, _i32, C.POINTER(FeReplayRing), _i64, _i64, _vp, _i64, _vp, _vp,
                                   C.c_float, C.c_float, _vp, _vp, C.c_float, C.c_float, _vp, _vp, _vp, _vp]),
}


# include/finenvs_amd_critic_grad.h: the twin critics' backward pass (finenvs_amd/critic.py; same library)
class FeCriticGrads(C.Structure):
    """struct fe_critic_grads of include/finenvs_amd_critic_grad.h."""

    _fields_ = [("w_ih", _vp), ("w_hh", _vp), ("b_ih", _vp), ("b_hh", _vp), ("w_out", _vp), ("b_out", _vp)]


_cg = C.POINTER(FeCriticGrads)
CRITIC_GRAD_SIGNATURES = {
    "fe_twin_q_grad_workspace_floats": (_i64, [_i32, _i32, _i64]),
    "fe_twin_q_backward": (C.c_int, [_vp, _vp, _cw, _cw, _i32, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _cg, _cg, _vp, _vp]),
}


# include/finenvs_amd_critic_streamed.h: the twin critics at H = 256 / 512 / 1024 (FeCriticWeights / FeCriticGrads again);
# each entry takes the argument list of its register-resident namesake
CRITIC_STREAMED_SIGNATURES = {
    "fe_twin_q_forward_streamed": CRITIC_SIGNATURES["fe_twin_q_forward"],
    "fe_twin_q_target_streamed": CRITIC_SIGNATURES["fe_twin_q_target"],
    "fe_twin_q_target_streamed_c": (C.c_int, [_vp, _vp, _cw, _cw, _i32, C.POINTER(FeReplayRing), _vp, _vp, _i64, _vp, _vp,
                                              C.c_float, C.c_float, _vp, _vp, C.c_float, C.c_float, _vp, _vp, _vp, _vp]),
    "fe_twin_q_streamed_grad_workspace_floats": (_i64, [_i32, _i32, _i64]),
    "fe_twin_q_backward_streamed": CRITIC_GRAD_SIGNATURES["fe_twin_q_backward"],
}

# include/finenvs_amd_sac_grad.h: the SAC actor's backward pass (finenvs_amd/sac.py; same library)
class FeSacGrads(C.Structure):
    """struct fe_sac_grads of include/finenvs_amd_sac_grad.h."""

    _fields_ = [("w_ih", _vp), ("w_hh", _vp), ("b_ih", _vp), ("b_hh", _vp), ("w_l", _vp), ("b_l", _vp), ("w_mu", _vp),
                ("b_mu", _vp), ("w_std", _vp), ("b_std", _vp)]


SAC_GRAD_SIGNATURES = {
    "fe_sac_grad_workspace_floats": (_i64, [_i32, _i32, _i64]),
    "fe_sac_backward": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_float, _vp, C.c_float, _i32, _vp, _vp, _i64, _vp,
                                  _vp, _vp, _vp, _vp, _vp, C.POINTER(FeSacGrads), _vp]),
}


# include/finenvs_amd_lstm_grad.h: the one-output LSTM head's backward pass (finenvs_amd/lstm_head.py; same library)
class FeLstmGrads(C.Structure):
    """struct fe_lstm_grads of include/finenvs_amd_lstm_grad.h."""

    _fields_ = [("w_ih", _vp), ("w_hh", _vp), ("b_ih", _vp), ("b_hh", _vp), ("w_out", _vp), ("b_out", _vp)]


LSTM_GRAD_SIGNATURES = {
    "fe_lstm_grad_workspace_floats": (_i64, [_i32, _i32, _i64]),
    "fe_lstm_backward": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _vp,
                                   C.POINTER(FeLstmGrads), _vp]),
}

# include/finenvs_amd_lstm_grad_streamed.h: the same head's backward pass at H = 256 / 512 / 1024 (FeLstmGrads again)
LSTM_STREAMED_GRAD_SIGNATURES = {
    "fe_lstm_streamed_grad_chunk_pairs": (_i64, [_i32, _i32]),
    "fe_lstm_streamed_grad_workspace_floats": (_i64, [_i32, _i32, _i64]),
    "fe_lstm_backward_streamed": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _vp,
                                            C.POINTER(FeLstmGrads), _vp]),
}


# include/finenvs_amd_optim.h: Adam, soft update and packing in one launch; the device-bias siblings (finenvs_amd/optim.py)
class FeOptimSegment(C.Structure):
    """struct fe_optim_segment of include/finenvs_amd_optim.h."""

    _fields_ = [("param", _vp), ("grad", _vp), ("exp_avg", _vp), ("exp_avg_sq", _vp), ("target", _vp),
                ("param2", _vp), ("grad2", _vp), ("exp_avg2", _vp), ("exp_avg_sq2", _vp), ("target2", _vp),
                ("packed", _vp), ("packed_target", _vp), ("numel", _i64), ("first_block", _i64),
                ("kind", _i32), ("H", _i32), ("cols", _i32), ("reserved", _i32),
                ("one_minus_rho", C.c_float), ("rho", C.c_float)]


class FeOptimDesc(C.Structure):
    """struct fe_optim_desc of include/finenvs_amd_optim.h."""

    _fields_ = [("segments", _vp), ("state", _vp), ("num_segments", _i32), ("mode", _i32), ("num_blocks", _i64),
                ("soft_update", _i32), ("zero_grad", _i32), ("beta1", C.c_double), ("beta2", C.c_double), ("lr", C.c_double),
                ("one_minus_beta1", C.c_float), ("beta2_f32", C.c_float), ("one_minus_beta2", C.c_float), ("eps", C.c_float)]


OPTIM_SIGNATURES = {
    "fe_net_update": (C.c_int, [C.POINTER(FeOptimDesc), _vp]),
    # the by-value entries' siblings: the same argument lists with every C.c_float bias a device pointer
    "fe_lstm_forward_p": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _i64, _vp, _vp]),
    "fe_env_rollout_lstm_p": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, C.c_float, _vp, _vp,
                                        _vp, _vp, _vp, _vp, _vp]),
    "fe_env_rollout_lstm_split_p": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, C.c_float, _vp,
                                              _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "fe_env_rollout_sac_p": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp,
                                       _vp, _vp, _vp, _vp, _vp, _vp]),
    "fe_sac_forward_p": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i64, _vp, _vp, _vp,
                                   _vp, _vp, _vp]),
    "fe_sac_backward_p": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i64, _vp, _vp, _vp,
                                    _vp, _vp, _vp, C.POINTER(FeSacGrads), _vp]),
}

# include/finenvs_amd_sac_streamed.h: the SAC actor at H = 256 / 512 / 1024 (FeSacGrads again); each entry takes the
# argument list of its register-resident namesake with the two output biases in device memory (the *_p form)
SAC_STREAMED_SIGNATURES = {
    "fe_env_rollout_sac_streamed": OPTIM_SIGNATURES["fe_env_rollout_sac_p"],
    "fe_sac_forward_streamed": OPTIM_SIGNATURES["fe_sac_forward_p"],
    "fe_sac_streamed_grad_workspace_floats": (_i64, [_i32, _i32, _i64]),
    "fe_sac_backward_streamed": OPTIM_SIGNATURES["fe_sac_backward_p"],
}

# include/finenvs_amd_replay_cursor.h: the ring's cursor in device memory and the draw from it (finenvs_amd/replay.py)
CURSOR_HEAD, CURSOR_SIZE, CURSOR_DRAWS, CURSOR_TICKET, CURSOR_WORDS = 0, 1, 2, 3, 4  # int64 words of fe_replay_cursor
REPLAY_CURSOR_SIGNATURES = {
    # fe_replay_append's list, then cursor, new_size, stream
    "fe_replay_append_c": (C.c_int, [C.POINTER(FeReplayRing), _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp,
                                     _i32, _vp, _vp, _vp, _i64, _vp]),
    "fe_ring_draw": (C.c_int, [C.POINTER(FeReplayRing), _vp, C.c_uint64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # the by-value entries' lists with `head, size` replaced by the cursor
    "fe_twin_q_target_c": (C.c_int, [_vp, _vp, _cw, _cw, _i32, C.POINTER(FeReplayRing), _vp, _vp, _i64, _vp, _vp,
                                     C.c_float, C.c_float, _vp, _vp, C.c_float, C.c_float, _vp, _vp, _vp, _vp]),
    "fe_replay_sample_c": (C.c_int, [_vp, C.POINTER(FeReplayRing), _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
}

# include/finenvs_amd_ppo.h: PPO's mini-batch from a keyed permutation, its epoch counter and losses (finenvs_amd/ppo.py)
PPO_PERM_SALT = 0x50504F5045524D31  # FE_PPO_PERM_SALT
PPO_CURSOR_EPOCH, PPO_CURSOR_ERRORS, PPO_CURSOR_WORDS = 0, 1, 2
PPO_MAX_COLUMNS = 4
_f64 = C.c_double
PPO_SIGNATURES = {
    "fe_ppo_minibatch": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i32, _vp, _vp, _i32, _vp, C.c_uint64, _i64, _i64, _i64,
                                   _vp, _vp, _vp, _vp, _vp]),
    "fe_ppo_epochs_advance": (C.c_int, [_vp, _i64, _vp]),
    "fe_ppo_loss_workspace_doubles": (_i64, [_i64]),
    "fe_ppo_actor_loss": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _f64, _f64, _vp, _vp, _vp, _vp, _vp]),
    "fe_ppo_value_loss": (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp]),
}


# include/finenvs_amd_mlp_head.h: the MLP head trained on descriptors (finenvs_amd/mlp_head.py, FusedMLPRollout)
MLP_GRAD_CHUNK_PAIRS = 512  # FE_MLP_GRAD_CHUNK_PAIRS


class FeMlpWeights(C.Structure):
    """struct fe_mlp_weights of include/finenvs_amd_mlp_head.h."""

    _fields_ = [("w1t", _vp), ("wpos", _vp), ("b1", _vp), ("w2", _vp), ("b2", _vp)]


class FeMlpGrads(C.Structure):
    """struct fe_mlp_grads of include/finenvs_amd_mlp_head.h."""

    _fields_ = [("w1", _vp), ("b1", _vp), ("w2", _vp), ("b2", _vp)]


_mw = C.POINTER(FeMlpWeights)
MLP_HEAD_SIGNATURES = {
    "fe_mlp_pack": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _vp]),
    "fe_env_rollout_mlp_sampled": (C.c_int, [_vp, _vp, _mw, _i32, _i32, _i32, _i32, _vp, _vp, _vp, C.c_float, _vp, _vp, _vp,
                                             _vp, _vp, _vp, _vp]),
    "fe_mlp_forward": (C.c_int, [_vp, _vp, _mw, _i32, _i32, _i32, _vp, _vp, _i64, _vp, _vp]),
    "fe_mlp_grad_workspace_floats": (_i64, [_i32, _i32, _i64]),
    "fe_mlp_backward": (C.c_int, [_vp, _vp, _mw, _i32, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _vp, C.POINTER(FeMlpGrads), _vp]),
}

# include/finenvs_amd_mlp2_head.h: the two-hidden-layer MLP head (finenvs_amd/mlp2_head.py, FusedMLP2Rollout)
MLP2_GRAD_CHUNK_PAIRS = 512  # FE_MLP2_GRAD_CHUNK_PAIRS
MLP2_MAX_WINDOW = {32: 296, 64: 128, 128: 40}  # FE_MLP2_MAX_WINDOW_H*: the largest window admitted with one asset


class FeMlp2Weights(C.Structure):
    """struct fe_mlp2_weights of include/finenvs_amd_mlp2_head.h."""

    _fields_ = [("w1t", _vp), ("wpos", _vp), ("b1", _vp), ("w2", _vp), ("b2", _vp), ("w3", _vp), ("b3", _vp)]


class FeMlp2Grads(C.Structure):
    """struct fe_mlp2_grads of include/finenvs_amd_mlp2_head.h."""

    _fields_ = [("w1", _vp), ("b1", _vp), ("w2", _vp), ("b2", _vp), ("w3", _vp), ("b3", _vp)]


_mw2 = C.POINTER(FeMlp2Weights)
MLP2_HEAD_SIGNATURES = {
    "fe_env_rollout_mlp2_sampled": (C.c_int, [_vp, _vp, _mw2, _i32, _i32, _i32, _i32, _vp, _vp, _vp, C.c_float, _vp, _vp, _vp,
                                              _vp, _vp, _vp, _vp]),
    "fe_mlp2_forward": (C.c_int, [_vp, _vp, _mw2, _i32, _i32, _i32, _vp, _vp, _i64, _vp, _vp]),
    "fe_mlp2_grad_workspace_floats": (_i64, [_i32, _i32, _i64]),
    "fe_mlp2_backward": (C.c_int, [_vp, _vp, _mw2, _i32, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _vp, C.POINTER(FeMlp2Grads), _vp]),
}

# include/finenvs_amd_mlp_critic.h: the twin MLP critics Q(s, a) (finenvs_amd/mlp_critic.py)
MLPQ_GRAD_CHUNK_PAIRS = 512  # FE_MLPQ_GRAD_CHUNK_PAIRS


class FeMlpqWeights(C.Structure):
    """struct fe_mlpq_weights of include/finenvs_amd_mlp_critic.h."""

    _fields_ = [("w1t", _vp), ("wpos", _vp), ("wact", _vp), ("b1", _vp), ("w2", _vp), ("b2", _vp), ("w3", _vp), ("b3", _vp)]


class FeMlpqGrads(C.Structure):
    """struct fe_mlpq_grads of include/finenvs_amd_mlp_critic.h."""

    _fields_ = [("w1", _vp), ("b1", _vp), ("w2", _vp), ("b2", _vp), ("w3", _vp), ("b3", _vp)]


_qw, _qg = C.POINTER(FeMlpqWeights), C.POINTER(FeMlpqGrads)
_mlpq_target_tail = [_vp, _i64, _vp, _vp, C.c_float, C.c_float, _vp, _vp, C.c_float, C.c_float, _vp, _vp, _vp, _vp]
MLP_CRITIC_SIGNATURES = {
    "fe_twin_mlpq_forward": (C.c_int, [_vp, _vp, _qw, _qw, _i32, _i32, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "fe_twin_mlpq_target": (C.c_int, [_vp, _vp, _qw, _qw, _i32, _i32, C.POINTER(FeReplayRing), _i64, _i64] + _mlpq_target_tail),
    "fe_twin_mlpq_target_c": (C.c_int, [_vp, _vp, _qw, _qw, _i32, _i32, C.POINTER(FeReplayRing), _vp] + _mlpq_target_tail),
    "fe_twin_mlpq_grad_workspace_floats": (_i64, [_i32, _i32, _i64]),
    "fe_twin_mlpq_backward": (C.c_int, [_vp, _vp, _qw, _qw, _i32, _i32, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _qg, _qg, _vp, _vp]),
}

# include/finenvs_amd_mlp_sac.h: the SAC MLP actor with the folded head (finenvs_amd/mlp_sac.py)
MLP_SAC_GRAD_CHUNK_PAIRS = 512  # FE_MLP_SAC_GRAD_CHUNK_PAIRS
MLP_SAC_GRAD_MAX_GROUPS = 256  # FE_MLP_SAC_GRAD_MAX_GROUPS
MLP_SAC_MAX_WINDOW = {32: 304, 64: 144, 128: 72}  # FE_MLP_SAC_MAX_WINDOW_H*: the largest window admitted with one asset


class FeMlpSacWeights(C.Structure):
    """struct fe_mlp_sac_weights of include/finenvs_amd_mlp_sac.h."""

    _fields_ = [("w1t", _vp), ("wpos", _vp), ("b1", _vp), ("w2", _vp), ("b2", _vp), ("wmu", _vp), ("bmu", _vp), ("wstd", _vp),
                ("bstd", _vp), ("vmu", _vp), ("vstd", _vp), ("cfold", _vp)]


class FeMlpSacGrads(C.Structure):
    """struct fe_mlp_sac_grads of include/finenvs_amd_mlp_sac.h."""

    _fields_ = [("w1", _vp), ("b1", _vp), ("w2", _vp), ("b2", _vp), ("w_mu", _vp), ("b_mu", _vp), ("w_std", _vp), ("b_std", _vp)]


_sw, _sg = C.POINTER(FeMlpSacWeights), C.POINTER(FeMlpSacGrads)
MLP_SAC_SIGNATURES = {
    "fe_mlp_sac_pack": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "fe_env_rollout_mlp_sac": (C.c_int, [_vp, _vp, _sw, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "fe_mlp_sac_forward": (C.c_int, [_vp, _vp, _sw, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "fe_mlp_sac_grad_workspace_floats": (_i64, [_i32, _i32, _i64]),
    "fe_mlp_sac_backward": (C.c_int, [_vp, _vp, _sw, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _sg, _vp]),
}

_lib: Optional[C.CDLL] = None


class FinEnvsNativeError(RuntimeError):
    pass


def load(path: Optional[str] = None) -> C.CDLL:
    """Load libfinenvs_amd.so (building it in-tree first if it is missing)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        try:
            from .csrc import build as _build

            _build.build()
        except Exception as exc:  # noqa: BLE001
            raise FinEnvsNativeError(
                f"native library {p} is missing and could not be built ({exc}); "
                "finenvs_amd has no CPU fallback"
            ) from exc
    lib = C.CDLL(p)
    for name, (res, args) in {**SIGNATURES, **EXT_SIGNATURES, **EVO_SIGNATURES, **REPLAY_SIGNATURES, **SAC_SIGNATURES,
                         **CRITIC_SIGNATURES, **CRITIC_GRAD_SIGNATURES, **SAC_GRAD_SIGNATURES,
                         **LSTM_GRAD_SIGNATURES, **LSTM_STREAMED_GRAD_SIGNATURES, **CRITIC_STREAMED_SIGNATURES,
                         **OPTIM_SIGNATURES, **SAC_STREAMED_SIGNATURES,
                         **REPLAY_CURSOR_SIGNATURES, **PPO_SIGNATURES, **MLP_HEAD_SIGNATURES, **MLP2_HEAD_SIGNATURES,
                         **MLP_CRITIC_SIGNATURES, **MLP_SAC_SIGNATURES, **EVO2_SIGNATURES, **EVO2_STREAMED_SIGNATURES}.items():
        fn = getattr(lib, name)  # AttributeError here means the .so is stale
        fn.restype = res
        fn.argtypes = args
    if lib.fe_version() != FE_ABI_VERSION:
        raise FinEnvsNativeError(f"ABI mismatch: library {lib.fe_version()} != binding {FE_ABI_VERSION}")
    tag = lib.fe_build_tag()
    if path is None and tag:
        raise FinEnvsNativeError(f"{p} is an experiment build ({tag.decode()}); rebuild the product library "
                                 "(python -m finenvs_amd.csrc.build --force) or load variants by explicit path")
    if path is None:
        _lib = lib
    return lib


def check(rc: int, lib: Optional[C.CDLL] = None) -> None:
    if rc != 0:
        msg = (lib or load()).fe_last_error()
        raise FinEnvsNativeError(f"finenvs_amd native call failed ({rc}): {msg.decode() if msg else ''}")
