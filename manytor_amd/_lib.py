"""ctypes binding of libmanytor_hip.so (C ABI: include/manytor_hip.h).

The library is the only compute path of this package: if it cannot be loaded the
import of anything that needs it raises -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# MT_LIB_OVERRIDE: load another build of the SAME library (tools/sanitize_host.sh points it at the ASan/UBSan build)
LIB_PATH = os.environ.get("MT_LIB_OVERRIDE") or os.path.join(PKG_DIR, "libmanytor_hip.so")

MT_MAX_DOF = 8
MT_MAX_TARGETS = 32
MT_MAX_RETURN_RING = 64
MT_UNIQUE_ID_BYTES = 128

# mt_status
MT_OK = 0
MT_ERR_INVALID_ARG = -1
MT_ERR_HIP = -2
MT_ERR_NO_DEVICE = -3
MT_ERR_ALLOC = -4
MT_ERR_STATE = -5
MT_ERR_UNSUPPORTED = -6

# mt_field
(F_ACTIONS, F_GOALS, F_POINTS, F_ALIVE, F_OBS, F_REWARD, F_DONE, F_DONE_BITS, F_EE, F_TOTAL_REWARD, F_JOINTS,
 F_EPISODES, F_LAST_RETURN, F_RETURN_RING, F_TRACE, F_ZMIN) = range(16)
# mt_dtype
DT_F32, DT_F64, DT_I32, DT_I64, DT_U8, DT_U32, DT_U64 = range(7)
# mt_layout
ENV_MAJOR, SOA = 0, 1
# flags
FLAG_TERMINATE_ON_GROUND = 0x1
FLAG_HW_TRIG = 0x2
FLAG_DH_IN_LDS = 0x4
FLAG_DIRECT_TRIG = 0x8
FLAG_NO_SPECIALIZE = 0x10
FLAG_TRACE = 0x20
FLAG_DEBUG_ZMIN = 0x40
FLAG_ABLATE_LOOP = 0x100
FLAG_ABLATE_OBS = 0x200


class ManytorError(RuntimeError):
    """A call into libmanytor_hip.so failed."""

    def __init__(self, status, message):
        super().__init__(f"libmanytor_hip: {message} (status {status})")
        self.status = status


class MtReturnStats(C.Structure):
    _fields_ = [("sum", C.c_double), ("min", C.c_double), ("max", C.c_double), ("count", C.c_int64), ("done", C.c_int64)]


class MtConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32),
        ("device", C.c_int32),
        ("n_envs", C.c_int64),
        ("env_id_base", C.c_int64),
        ("dof", C.c_int32),
        ("n_targets", C.c_int32),
        ("substeps", C.c_int32),
        ("flags", C.c_uint32),
        ("pickup_tol", C.c_float),
        ("radius", C.c_float),
        ("dh_table", C.c_float * (MT_MAX_DOF * 4)),
        ("return_ring", C.c_int32),
        ("obs_frame", C.c_int32),
        ("ee_frame", C.c_int32),
        ("reserved", C.c_int32),
    ]


class MtTape(C.Structure):
    """mt_tape of include/manytor_hip.h: the argument block of mt_rollout_tape."""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_steps", C.c_int32),
        ("actions", C.c_void_p),
        ("ld", C.c_int64),
        ("reward_log", C.c_void_p),
        ("done_log", C.c_void_p),
        ("log_ld", C.c_int64),
        ("return_out", C.c_void_p),
        ("seed", C.c_uint64),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


TAPE_AUTO_RESET = 0x1
TAPE_DRY_RUN = 0x2


class MtShoot(C.Structure):
    """mt_shoot of include/manytor_hip.h: the argument block of mt_shoot."""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_steps", C.c_int32),
        ("n_candidates", C.c_int32),
        ("commit_steps", C.c_int32),
        ("actions", C.c_void_p),
        ("ld", C.c_int64),
        ("cand_stride", C.c_int64),
        ("returns_out", C.c_void_p),
        ("ret_ld", C.c_int64),
        ("best_out", C.c_void_p),
        ("best_return_out", C.c_void_p),
        ("reward_log", C.c_void_p),
        ("done_log", C.c_void_p),
        ("log_ld", C.c_int64),
        ("return_out", C.c_void_p),
        ("seed", C.c_uint64),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


SHOOT_AUTO_RESET = 0x1



class MtCem(C.Structure):
    """struct mt_cem of include/manytor_hip.h: the argument block of mt_cem and mt_sample_plans."""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_steps", C.c_int32),
        ("n_candidates", C.c_int32),
        ("n_elites", C.c_int32),
        ("commit_steps", C.c_int32),
        ("draw", C.c_uint32),
        ("mean", C.c_void_p),
        ("sigma", C.c_void_p),
        ("ld", C.c_int64),
        ("mean_out", C.c_void_p),
        ("sigma_out", C.c_void_p),
        ("out_ld", C.c_int64),
        ("lo", C.c_float),
        ("hi", C.c_float),
        ("sigma_min", C.c_float),
        ("returns_out", C.c_void_p),
        ("ret_ld", C.c_int64),
        ("best_out", C.c_void_p),
        ("best_return_out", C.c_void_p),
        ("elite_mask_out", C.c_void_p),
        ("chosen_out", C.c_void_p),
        ("chosen_ld", C.c_int64),
        ("reward_log", C.c_void_p),
        ("done_log", C.c_void_p),
        ("log_ld", C.c_int64),
        ("return_out", C.c_void_p),
        ("seed", C.c_uint64),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


CEM_AUTO_RESET = 0x1
CEM_KEEP_MEAN = 0x2


class MtMppi(C.Structure):
    """struct mt_mppi of include/manytor_hip.h: the argument block of mt_mppi."""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_steps", C.c_int32),
        ("n_candidates", C.c_int32),
        ("commit_steps", C.c_int32),
        ("draw", C.c_uint32),
        ("decay", C.c_float),
        ("mean", C.c_void_p),
        ("sigma", C.c_void_p),
        ("ld", C.c_int64),
        ("mean_out", C.c_void_p),
        ("sigma_out", C.c_void_p),
        ("out_ld", C.c_int64),
        ("lo", C.c_float),
        ("hi", C.c_float),
        ("sigma_min", C.c_float),
        ("returns_out", C.c_void_p),
        ("ret_ld", C.c_int64),
        ("weights_out", C.c_void_p),
        ("w_ld", C.c_int64),
        ("weight_sum_out", C.c_void_p),
        ("best_out", C.c_void_p),
        ("best_return_out", C.c_void_p),
        ("chosen_out", C.c_void_p),
        ("chosen_ld", C.c_int64),
        ("reward_log", C.c_void_p),
        ("done_log", C.c_void_p),
        ("log_ld", C.c_int64),
        ("return_out", C.c_void_p),
        ("seed", C.c_uint64),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


MPPI_AUTO_RESET = 0x1
MPPI_KEEP_MEAN = 0x2
MPPI_MAX_STEPS = 127


class MtPolicy(C.Structure):
    """struct mt_policy of include/manytor_hip.h: the argument block of mt_rollout_policy."""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_steps", C.c_int32),
        ("n_layers", C.c_int32),
        ("width", C.c_int32 * 2),
        ("hidden_act", C.c_int32),
        ("out_act", C.c_int32),
        ("draw", C.c_uint32),
        ("weight", C.c_void_p * 3),
        ("bias", C.c_void_p * 3),
        ("out_scale", C.c_float),
        ("lo", C.c_float),
        ("hi", C.c_float),
        ("sigma", C.c_float * MT_MAX_DOF),
        ("flags", C.c_uint32),
        ("action_log", C.c_void_p),
        ("act_ld", C.c_int64),
        ("obs_log", C.c_void_p),
        ("obs_ld", C.c_int64),
        ("reward_log", C.c_void_p),
        ("done_log", C.c_void_p),
        ("log_ld", C.c_int64),
        ("return_out", C.c_void_p),
        ("seed", C.c_uint64),
        ("reserved", C.c_uint64),
    ]


POLICY_AUTO_RESET = 0x1
POLICY_DRY_RUN = 0x2
POLICY_SEE_POSE = 0x4
POLICY_MAX_LAYERS = 3
POLICY_MAX_WIDTH = 64
ACT_IDENTITY, ACT_TANH, ACT_RELU = 0, 1, 2


class MtActorCritic(C.Structure):
    """struct mt_actor_critic of include/manytor_hip.h: the argument block of mt_rollout_actor_critic."""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("critic_layers", C.c_int32),
        ("policy", MtPolicy),
        ("critic_width", C.c_int32 * 2),
        ("critic_hidden_act", C.c_int32),
        ("critic_out_act", C.c_int32),
        ("critic_weight", C.c_void_p * 3),
        ("critic_bias", C.c_void_p * 3),
        ("critic_out_scale", C.c_float),
        ("pad_", C.c_uint32),
        ("logp_log", C.c_void_p),
        ("logp_ld", C.c_int64),
        ("value_log", C.c_void_p),
        ("value_ld", C.c_int64),
        ("last_value_out", C.c_void_p),
        ("reserved", C.c_uint64),
    ]


ACTOR_CRITIC_MAX_LDS = 163840


class MtEsSample(C.Structure):
    """struct mt_es_sample of include/manytor_hip.h: the argument block of mt_es_sample."""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_members", C.c_int32),
        ("n_params", C.c_int64),
        ("theta", C.c_void_p),
        ("pop", C.c_void_p),
        ("pitch", C.c_int64),
        ("sigma", C.c_float),
        ("draw", C.c_uint32),
        ("seed", C.c_uint64),
        ("reserved", C.c_uint64),
    ]


class MtPopulation(C.Structure):
    """struct mt_population: the argument block of mt_rollout_population, and mt_es's scoring."""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_steps", C.c_int32),
        ("n_members", C.c_int32),
        ("n_layers", C.c_int32),
        ("width", C.c_int32 * 2),
        ("hidden_act", C.c_int32),
        ("out_act", C.c_int32),
        ("pop", C.c_void_p),
        ("pitch", C.c_int64),
        ("out_scale", C.c_float),
        ("lo", C.c_float),
        ("hi", C.c_float),
        ("flags", C.c_uint32),
        ("action_log", C.c_void_p),
        ("act_ld", C.c_int64),
        ("obs_log", C.c_void_p),
        ("obs_ld", C.c_int64),
        ("reward_log", C.c_void_p),
        ("done_log", C.c_void_p),
        ("log_ld", C.c_int64),
        ("return_out", C.c_void_p),
        ("fitness_out", C.c_void_p),
        ("seed", C.c_uint64),
        ("reserved", C.c_uint64),
    ]


class MtEs(C.Structure):
    """struct mt_es: the argument block of mt_es."""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("shaping", C.c_int32),
        ("sigma", C.c_float),
        ("lr", C.c_float),
        ("draw", C.c_uint32),
        ("flags", C.c_uint32),
        ("theta", C.c_void_p),
        ("grad_out", C.c_void_p),
        ("best_out", C.c_void_p),
        ("coeff_out", C.c_void_p),
        ("pop", MtPopulation),
        ("reserved", C.c_uint64),
    ]


ES_MAX_MEMBERS = 4096
ES_INPLACE = 0x1
ES_UPDATE_ONLY = 0x2
ES_SHAPE_RANK, ES_SHAPE_RAW = 0, 1


class MtPolicyGrad(C.Structure):
    """struct mt_policy_grad of include/manytor_hip.h: the argument block of mt_policy_grad."""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_steps", C.c_int32),
        ("n_layers", C.c_int32),
        ("width", C.c_int32 * 2),
        ("hidden_act", C.c_int32),
        ("out_act", C.c_int32),
        ("weight", C.c_void_p * 3),
        ("bias", C.c_void_p * 3),
        ("out_scale", C.c_float),
        ("sigma", C.c_float * MT_MAX_DOF),
        ("flags", C.c_uint32),
        ("obs", C.c_void_p),
        ("obs_ld", C.c_int64),
        ("action", C.c_void_p),
        ("act_ld", C.c_int64),
        ("coef", C.c_void_p),
        ("coef_ld", C.c_int64),
        ("scale", C.c_float),
        ("grad_out", C.c_void_p),
        ("loss_out", C.c_void_p),
        ("workspace", C.c_void_p),
        ("workspace_bytes", C.c_size_t),
        ("reserved", C.c_uint64),
    ]


class MtRewardToGo(C.Structure):
    """struct mt_reward_to_go of include/manytor_hip.h: the argument block of mt_reward_to_go."""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_steps", C.c_int32),
        ("reward_log", C.c_void_p),
        ("done_log", C.c_void_p),
        ("log_ld", C.c_int64),
        ("gamma", C.c_float),
        ("baseline", C.c_float),
        ("out", C.c_void_p),
        ("out_ld", C.c_int64),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


RTG_MASK_AFTER_DONE = 0x1


class MtPolicyEval(C.Structure):
    """struct mt_policy_eval of include/manytor_hip.h: the argument block of mt_policy_eval."""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_steps", C.c_int32),
        ("n_layers", C.c_int32),
        ("width", C.c_int32 * 2),
        ("hidden_act", C.c_int32),
        ("out_act", C.c_int32),
        ("weight", C.c_void_p * 3),
        ("bias", C.c_void_p * 3),
        ("out_scale", C.c_float),
        ("flags", C.c_uint32),
        ("obs", C.c_void_p),
        ("obs_ld", C.c_int64),
        ("n_out", C.c_int32),
        ("mean_out", C.c_void_p),
        ("mean_ld", C.c_int64),
        ("action", C.c_void_p),
        ("act_ld", C.c_int64),
        ("sigma", C.c_float * MT_MAX_DOF),
        ("logp_out", C.c_void_p),
        ("logp_ld", C.c_int64),
        ("reserved", C.c_uint64),
    ]


class MtGae(C.Structure):
    """struct mt_gae of include/manytor_hip.h: the argument block of mt_gae."""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_steps", C.c_int32),
        ("reward_log", C.c_void_p),
        ("done_log", C.c_void_p),
        ("log_ld", C.c_int64),
        ("value", C.c_void_p),
        ("value_ld", C.c_int64),
        ("last_value", C.c_void_p),
        ("gamma", C.c_float),
        ("lambda_", C.c_float),
        ("adv_out", C.c_void_p),
        ("adv_ld", C.c_int64),
        ("ret_out", C.c_void_p),
        ("ret_ld", C.c_int64),
        ("weight_out", C.c_void_p),
        ("weight_ld", C.c_int64),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class MtValueGrad(C.Structure):
    """struct mt_value_grad of include/manytor_hip.h: the argument block of mt_value_grad."""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_steps", C.c_int32),
        ("n_layers", C.c_int32),
        ("width", C.c_int32 * 2),
        ("hidden_act", C.c_int32),
        ("out_act", C.c_int32),
        ("weight", C.c_void_p * 3),
        ("bias", C.c_void_p * 3),
        ("out_scale", C.c_float),
        ("flags", C.c_uint32),
        ("obs", C.c_void_p),
        ("obs_ld", C.c_int64),
        ("target", C.c_void_p),
        ("target_ld", C.c_int64),
        ("coef", C.c_void_p),
        ("coef_ld", C.c_int64),
        ("scale", C.c_float),
        ("grad_out", C.c_void_p),
        ("loss_out", C.c_void_p),
        ("workspace", C.c_void_p),
        ("workspace_bytes", C.c_size_t),
        ("reserved", C.c_uint64),
    ]


GAE_MASK_AFTER_DONE = 0x1


class MtPpoGrad(C.Structure):
    """struct mt_ppo_grad of include/manytor_hip.h: the argument block of mt_ppo_grad."""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("n_steps", C.c_int32),
        ("n_layers", C.c_int32),
        ("width", C.c_int32 * 2),
        ("hidden_act", C.c_int32),
        ("out_act", C.c_int32),
        ("weight", C.c_void_p * 3),
        ("bias", C.c_void_p * 3),
        ("out_scale", C.c_float),
        ("sigma", C.c_float * MT_MAX_DOF),
        ("flags", C.c_uint32),
        ("obs", C.c_void_p),
        ("obs_ld", C.c_int64),
        ("action", C.c_void_p),
        ("act_ld", C.c_int64),
        ("adv", C.c_void_p),
        ("adv_ld", C.c_int64),
        ("old_logp", C.c_void_p),
        ("old_ld", C.c_int64),
        ("sample_weight", C.c_void_p),
        ("weight_ld", C.c_int64),
        ("clip", C.c_float),
        ("log_ratio_shift", C.c_float),
        ("scale", C.c_float),
        ("grad_out", C.c_void_p),
        ("loss_out", C.c_void_p),
        ("ratio_out", C.c_void_p),
        ("ratio_ld", C.c_int64),
        ("coef_out", C.c_void_p),
        ("coef_ld", C.c_int64),
        ("sigma_grad_out", C.c_void_p),
        ("kl_out", C.c_void_p),
        ("count_out", C.c_void_p),
        ("workspace", C.c_void_p),
        ("workspace_bytes", C.c_size_t),
        ("reserved", C.c_uint64),
    ]


PPO_MAX_LOG_RATIO = 20.0
PPO_EXTRA_WORDS = MT_MAX_DOF + 3


class MtIk(C.Structure):
    """struct mt_ik of include/manytor_hip.h: the argument block of mt_ik."""
    _fields_ = [
        ("struct_size", C.c_int32),
        ("iters", C.c_int32),
        ("damping", C.c_float),
        ("max_step_deg", C.c_float),
        ("tol", C.c_float),
        ("flags", C.c_uint32),
        ("target", C.c_void_p),
        ("target_ld", C.c_int64),
        ("start", C.c_void_p),
        ("start_ld", C.c_int64),
        ("angles_out", C.c_void_p),
        ("angles_ld", C.c_int64),
        ("residual_out", C.c_void_p),
        ("iters_out", C.c_void_p),
        ("index_out", C.c_void_p),
        ("reserved", C.c_uint64),
    ]


IK_STAGE = 0x1
IK_WRAP = 0x2
IK_MAX_ITERS = 255

_HANDLE = C.c_void_p

# name -> (restype, argtypes); exactly the prototypes of include/manytor_hip.h
PROTOTYPES = {
    "mt_version": (C.c_int, []),
    "mt_status_string": (C.c_char_p, [C.c_int]),
    "mt_last_error": (C.c_char_p, [_HANDLE]),
    "mt_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "mt_create": (C.c_int, [C.POINTER(_HANDLE), C.POINTER(MtConfig)]),
    "mt_destroy": (C.c_int, [_HANDLE]),
    "mt_step_kernel_name": (C.c_char_p, [_HANDLE]),
    "mt_describe_dispatch": (C.c_char_p, [_HANDLE]),
    "mt_set_stream": (C.c_int, [_HANDLE, C.c_void_p]),
    "mt_use_own_stream": (C.c_int, [_HANDLE]),
    "mt_sync": (C.c_int, [_HANDLE]),
    "mt_reset": (C.c_int, [_HANDLE, C.c_void_p, C.c_int, C.c_int]),
    "mt_reset_random": (C.c_int, [_HANDLE, C.c_uint64, C.c_uint32]),
    "mt_reset_done": (C.c_int, [_HANDLE, C.c_uint64]),
    "mt_env_reset": (C.c_int, [_HANDLE, C.c_int64, C.c_void_p, C.c_uint64, C.c_uint32]),
    "mt_set_actions": (C.c_int, [_HANDLE, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "mt_sample_actions": (C.c_int, [_HANDLE, C.c_uint64, C.c_uint32]),
    "mt_step": (C.c_int, [_HANDLE]),
    "mt_step_host": (C.c_int, [_HANDLE, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mt_env_step": (C.c_int, [_HANDLE, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mt_bad_action_count": (C.c_int, [_HANDLE, C.POINTER(C.c_uint64)]),
    "mt_step_random": (C.c_int, [_HANDLE, C.c_uint64, C.c_uint32]),
    "mt_rollout": (C.c_int, [_HANDLE, C.c_int, C.c_uint64, C.c_uint32]),
    "mt_rollout_fused": (C.c_int, [_HANDLE, C.c_int, C.c_uint64, C.c_uint32, C.c_int]),
    "mt_rollout_tape": (C.c_int, [_HANDLE, C.POINTER(MtTape)]),
    "mt_shoot": (C.c_int, [_HANDLE, C.POINTER(MtShoot)]),
    "mt_cem": (C.c_int, [_HANDLE, C.POINTER(MtCem)]),
    "mt_sample_plans": (C.c_int, [_HANDLE, C.POINTER(MtCem), C.c_void_p, C.c_int64, C.c_int64]),
    "mt_mppi": (C.c_int, [_HANDLE, C.POINTER(MtMppi)]),
    "mt_rollout_policy": (C.c_int, [_HANDLE, C.POINTER(MtPolicy)]),
    "mt_rollout_actor_critic": (C.c_int, [_HANDLE, C.POINTER(MtActorCritic)]),
    "mt_es_sample": (C.c_int, [_HANDLE, C.POINTER(MtEsSample)]),
    "mt_rollout_population": (C.c_int, [_HANDLE, C.POINTER(MtPopulation)]),
    "mt_es": (C.c_int, [_HANDLE, C.POINTER(MtEs)]),
    "mt_policy_grad": (C.c_int, [_HANDLE, C.POINTER(MtPolicyGrad)]),
    "mt_policy_grad_workspace": (C.c_size_t, [_HANDLE, C.c_int, C.POINTER(C.c_int32), C.c_uint32, C.c_int]),
    "mt_reward_to_go": (C.c_int, [_HANDLE, C.POINTER(MtRewardToGo)]),
    "mt_policy_eval": (C.c_int, [_HANDLE, C.POINTER(MtPolicyEval)]),
    "mt_gae": (C.c_int, [_HANDLE, C.POINTER(MtGae)]),
    "mt_value_grad": (C.c_int, [_HANDLE, C.POINTER(MtValueGrad)]),
    "mt_value_grad_workspace": (C.c_size_t, [_HANDLE, C.c_int, C.POINTER(C.c_int32), C.c_uint32, C.c_int]),
    "mt_ppo_grad": (C.c_int, [_HANDLE, C.POINTER(MtPpoGrad)]),
    "mt_ppo_grad_workspace": (C.c_size_t, [_HANDLE, C.c_int, C.POINTER(C.c_int32), C.c_uint32, C.c_int]),
    "mt_ik": (C.c_int, [_HANDLE, C.POINTER(MtIk)]),
    "mt_jacobian": (C.c_int, [_HANDLE, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]),
    "mt_observe": (C.c_int, [_HANDLE]),
    "mt_check_done": (C.c_int, [_HANDLE]),
    "mt_get": (C.c_int, [_HANDLE, C.c_int, C.c_void_p, C.c_int64, C.c_int]),
    "mt_set": (C.c_int, [_HANDLE, C.c_int, C.c_void_p, C.c_int64]),
    "mt_set_episode_base": (C.c_int, [_HANDLE, C.c_uint32]),
    "mt_device_ptr": (C.c_int, [_HANDLE, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                C.POINTER(C.c_int)]),
    "mt_comm_unique_id": (C.c_int, [C.c_void_p]),
    "mt_comm_init": (C.c_int, [_HANDLE, C.c_void_p, C.c_int, C.c_int]),
    "mt_comm_destroy": (C.c_int, [_HANDLE]),
    "mt_gather_returns": (C.c_int, [_HANDLE, C.c_int, C.c_int, C.c_void_p, C.c_int64]),
    "mt_gather_returns_begin": (C.c_int, [_HANDLE, C.c_int, C.c_int, C.c_void_p, C.c_int64]),
    "mt_gather_returns_wait": (C.c_int, [_HANDLE, C.c_int, C.POINTER(C.c_float)]),
    "mt_gather_returns_begin_inplace": (C.c_int, [_HANDLE, C.c_int, C.c_int, C.c_void_p, C.c_int64]),
    "mt_comm_total_envs": (C.c_int, [_HANDLE, C.POINTER(C.c_int64)]),
    "mt_reduce_returns": (C.c_int, [_HANDLE, C.c_int, C.c_int, C.c_void_p]),
    "mt_timer_start": (C.c_int, [_HANDLE]),
    "mt_timer_stop": (C.c_int, [_HANDLE, C.POINTER(C.c_float)]),
    "mt_timer_stop_async": (C.c_int, [_HANDLE]),
    "mt_timer_read": (C.c_int, [_HANDLE, C.POINTER(C.c_float)]),
    "mt_timer_lap_begin": (C.c_int, [_HANDLE]),
    "mt_timer_lap_end": (C.c_int, [_HANDLE]),
    "mt_timer_laps_total": (C.c_int, [_HANDLE, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "mt_timer_lap_times": (C.c_int, [_HANDLE, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int)]),
    "mt_fk_batch": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p]),
    "mt_route_trace": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "mt_r_theta_batch": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "mt_stream_probe": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int64)]),
}

_lib = None


def _share_torch_hip_runtime():
    """A torch-ROCm wheel bundles its own libamdhip64.so (soname libamdhip64.so.7) and librccl.so.  Two HIP runtimes
    in one process do not share streams, events or allocations, so if torch is installed its copy is loaded FIRST
    (without importing torch): this library's `libamdhip64.so.7` dependency then resolves to it, whatever the import
    order, and comm.hip is pointed at the RCCL that sits on the same runtime.  Without torch the system ROCm is used."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
    hip = os.path.join(libdir, "libamdhip64.so")
    if os.path.exists(hip):
        try:
            C.CDLL(hip, mode=C.RTLD_GLOBAL)
        except OSError:
            return
        rccl = os.path.join(libdir, "librccl.so")
        if os.path.exists(rccl):
            os.environ.setdefault("MT_RCCL_LIB", rccl)


def load():
    """Load (once) and return the ctypes library.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the HIP extension has not been built. "
            "Run `python -m manytor_amd.build` (needs hipcc); this package has no CPU fallback."
        )
    _share_torch_hip_runtime()
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)     # AttributeError if the .so does not export what the header declares
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status, handle=None):
    if status == MT_OK:
        return
    lib = load()
    msg = lib.mt_last_error(handle)
    msg = msg.decode() if msg else ""
    if not msg:
        msg = lib.mt_status_string(status).decode()
    if status == MT_ERR_INVALID_ARG:
        raise ValueError(f"libmanytor_hip: {msg}")
    raise ManytorError(status, msg)


def device_count() -> int:
    lib = load()
    n = C.c_int(0)
    rc = lib.mt_device_count(C.byref(n))
    return n.value if rc == MT_OK else 0
