"""ctypes mirror of include/pcgym_hip.h (structs + constants).

tests/test_abi.py parses the header and checks every #define / enum value and
struct field order against this file, so the two cannot drift silently.
"""
from __future__ import annotations

import ctypes as C

PCG_ABI_VERSION = 16
PCG_MAX_NX = 24
PCG_MAX_NA = 5
PCG_MAX_NDM = 4
PCG_MAX_NSP = 4
PCG_MAX_NCON = 8
PCG_MAX_NUNC = 8
PCG_MAX_PARAMS = 128
PCG_MAX_USER_PARAMS = 64
PCG_MAX_NOBS = PCG_MAX_NX + PCG_MAX_NSP + PCG_MAX_NDM + PCG_MAX_NUNC
PCG_MAX_NU = PCG_MAX_NA + PCG_MAX_NDM
PCG_MAX_N = 4096

PCG_OK = 0
PCG_ST_OK = 0
PCG_ST_MAX_STEPS = 1
PCG_ST_UNDERFLOW = 2
PCG_ST_NONFINITE = 3
PCG_E_NULL = -1
PCG_E_MODEL = -2
PCG_E_DIM = -3
PCG_E_VALUE = -4
PCG_E_PLAN = -5
PCG_E_UNSUPPORTED = -6
PCG_E_JIT = -7

PCG_OPT_ENV_OFFSET = 1
PCG_OPT_LDS_STAGES = 2
PCG_OPT_VARIANT = 3
PCG_OPT_STREAM_BLOCKS_PER_CU = 4
PCG_OPT_NT_STORES = 5

PCG_INT_RK4 = 0
PCG_INT_DOPRI5 = 1
PCG_INT_RODAS3 = 2
PCG_INT_RODAS4 = 3
PCG_INT_TSIT5 = 4
PCG_INT_RK4G = 5
PCG_INT_T5G = 6
PCG_INT_CV8 = 7
PCG_INT_RODAS5 = 8

PCG_F_NORMALISE_A = 0x0001
PCG_F_NORMALISE_O = 0x0002
PCG_F_A_DELTA = 0x0004
PCG_F_R_PENALTY = 0x0008
PCG_F_DONE_ON_CONS = 0x0010
PCG_F_NOISE = 0x0020
PCG_F_REWARD_BATCH = 0x0040
PCG_F_MAXIMISE = 0x0080
PCG_F_REF_COMPAT = 0x0100
PCG_F_GAUSS_DIST = 0x0200
PCG_F_X0_NORMAL = 0x0400
PCG_F_UNC_EMPIRICAL = 0x0800
PCG_F_REWARD_TRACK = 0x1000
PCG_F_REWARD_CRYST = 0x2000
PCG_MAX_RBOX = 4
PCG_MAX_EMP = 65536

PCG_ACT_TANH = 0
PCG_ACT_RELU = 1
PCG_POL_NONE = 0
PCG_POL_CLIP = 1
PCG_POL_TANH = 2
PCG_POL_MAX_WIDTH = 64
PCG_POL_F64 = 0
PCG_POL_F32 = 1
PCG_RNG_POLICY = 0x400
PCG_RNG_SEARCH = 0x500
PCG_POP_CHUNK = 64

_pd = C.POINTER(C.c_double)
_pi = C.POINTER(C.c_int32)
_pu8 = C.POINTER(C.c_uint8)


class pcg_env_cfg(C.Structure):
    _fields_ = [
        ("model_id", C.c_int32),
        ("integrator_id", C.c_int32),
        ("nx", C.c_int32),
        ("na", C.c_int32),
        ("ndm", C.c_int32),
        ("nd", C.c_int32),
        ("nsp", C.c_int32),
        ("nsp_obs", C.c_int32),
        ("ncon", C.c_int32),
        ("nrew", C.c_int32),
        ("nunc", C.c_int32),
        ("N", C.c_int32),
        ("substeps", C.c_int32),
        ("max_steps", C.c_int32),
        ("flags", C.c_uint32),
        ("n_params", C.c_int32),
        ("dt", C.c_double),
        ("rtol", C.c_double),
        ("atol", C.c_double),
        ("params", _pd),
        ("x0", _pd),
        ("x0_unc", _pd),
        ("a_low", _pd),
        ("a_high", _pd),
        ("a_act_low", _pd),
        ("a_act_high", _pd),
        ("a_0", _pd),
        ("o_low", _pd),
        ("o_high", _pd),
        ("obs_mask", _pu8),
        ("sp_index", _pi),
        ("sp", _pd),
        ("r_scale", _pd),
        ("rew_index", _pi),
        ("d_slot", _pi),
        ("d_sched", _pd),
        ("d_default", _pd),
        ("d_sigma", _pd),
        ("d_clip_lo", _pd),
        ("d_clip_hi", _pd),
        ("con_A", _pd),
        ("con_b", _pd),
        ("noise_pct", _pd),
        ("unc_index", _pi),
        ("unc_pct", _pd),
        ("unc_emp", _pd),
        ("unc_emp_off", _pi),
        ("rew_R_du", C.c_double),
        ("rew_R_u", C.c_double),
        ("rew_nbox", C.c_int32),
        ("rew_box_index", _pi),
        ("rew_box_lo", _pd),
        ("rew_box_hi", _pd),
        ("user_cons_src", C.c_char_p),
        ("user_reward_src", C.c_char_p),
        ("jit_include_dir", C.c_char_p),
        ("user_rhs_src", C.c_char_p),
        ("ep_frac", C.c_double),
        ("ep_kmax", C.c_int32),
        ("d_param_index", _pi),
        ("coop_thr", C.c_double),
    ]


class pcg_buffers(C.Structure):
    _fields_ = [
        ("B", C.c_int64),
        ("x", C.c_void_p),
        ("a", C.c_void_p),
        ("d", C.c_void_p),
        ("t", C.c_void_p),
        ("a_save", C.c_void_p),
        ("obs", C.c_void_p),
        ("rew", C.c_void_p),
        ("done", C.c_void_p),
        ("viol", C.c_void_p),
        ("g", C.c_void_p),
        ("g_pre", C.c_void_p),
        ("nsteps", C.c_void_p),
        ("u_prev", C.c_void_p),
        ("p_unc", C.c_void_p),
        ("status", C.c_void_p),
    ]


class pcg_policy_cfg(C.Structure):
    _fields_ = [
        ("n_in", C.c_int32),
        ("n_out", C.c_int32),
        ("n_hidden", C.c_int32),
        ("width", C.c_int32 * 2),
        ("activation", C.c_int32),
        ("out_map", C.c_int32),
        ("out_low", C.c_double),
        ("out_high", C.c_double),
        ("W", _pd * 3),
        ("b", _pd * 3),
    ]


# every extern "C" symbol the header declares (tests check the .so exports all)
EXPORTS = [
    "pcg_version",
    "pcg_build_id",
    "pcg_strerror",
    "pcg_model_info",
    "pcg_model_default_params",
    "pcg_plan_create",
    "pcg_plan_destroy",
    "pcg_plan_bytes_per_env_step",
    "pcg_step",
    "pcg_reset",
    "pcg_plan_set_env_offset",
    "pcg_plan_set_option",
    "pcg_cfg_validate",
    "pcg_rhs",
    "pcg_integrate",
    "pcg_rollout",
    "pcg_rollout_strided",
    "pcg_policy_validate",
    "pcg_policy_create",
    "pcg_policy_destroy",
    "pcg_policy_update",
    "pcg_policy_create_f32",
    "pcg_policy_dtype",
    "pcg_rollout_policy",
    "pcg_plan_prepare_closed_loop",
    "pcg_rollout_actor",
    "pcg_rollout_policy_cons",
    "pcg_rollout_actor_cons",
    "pcg_rollout_policy_unc",
    "pcg_rollout_actor_unc",
    "pcg_actor_logp_const",
    "pcg_policy_noise",
    "pcg_gae",
    "pcg_policy_pop_create",
    "pcg_policy_pop_create_f32",
    "pcg_policy_pop_dtype",
    "pcg_policy_pop_update",
    "pcg_policy_pop_destroy",
    "pcg_policy_pop_size",
    "pcg_rollout_policy_pop",
    "pcg_rollout_policy_pop_unc",
    "pcg_rollout_policy_pop_cons",
    "pcg_policy_pop_nparams",
    "pcg_policy_pop_sample",
    "pcg_policy_pop_noise_dot",
    "pcg_policy_pop_get_flat",
    "pcg_policy_pop_set_flat",
    "pcg_step_autoreset",
    "pcg_graph_create",
    "pcg_graph_launch",
    "pcg_graph_set_seed",
    "pcg_graph_destroy",
    "pcg_graph_held",
    "pcg_graph_chained",
    "pcg_last_jit_log",
    "pcg_philox4x32_10",
    "pcg_test_sort_tile",
    "pcg_coverage_names",
]


def declare(lib):
    """Attach argtypes/restype to a loaded libpcgym_hip.so."""
    vp = C.c_void_p
    lib.pcg_version.restype = C.c_int
    lib.pcg_version.argtypes = []
    lib.pcg_build_id.restype = C.c_char_p
    lib.pcg_build_id.argtypes = []
    lib.pcg_strerror.restype = C.c_char_p
    lib.pcg_strerror.argtypes = [C.c_int]
    lib.pcg_model_info.restype = C.c_int
    lib.pcg_model_info.argtypes = [C.c_int, _pi, _pi, _pi, _pi]
    lib.pcg_model_default_params.restype = C.c_int
    lib.pcg_model_default_params.argtypes = [C.c_int, _pd, C.c_int32]
    lib.pcg_plan_create.restype = C.c_int
    lib.pcg_plan_create.argtypes = [C.POINTER(vp), C.POINTER(pcg_env_cfg)]
    lib.pcg_plan_destroy.restype = C.c_int
    lib.pcg_plan_destroy.argtypes = [vp]
    lib.pcg_plan_bytes_per_env_step.restype = C.c_int64
    lib.pcg_plan_bytes_per_env_step.argtypes = [vp, C.POINTER(pcg_buffers)]
    lib.pcg_step.restype = C.c_int
    lib.pcg_step.argtypes = [vp, C.POINTER(pcg_buffers), C.c_int32, C.c_uint64, vp]
    lib.pcg_reset.restype = C.c_int
    lib.pcg_reset.argtypes = [vp, C.POINTER(pcg_buffers), vp, C.c_uint64, vp]
    lib.pcg_plan_set_env_offset.restype = C.c_int
    lib.pcg_plan_set_env_offset.argtypes = [vp, C.c_int64]
    lib.pcg_plan_set_option.restype = C.c_int
    lib.pcg_plan_set_option.argtypes = [vp, C.c_int, C.c_int64]
    lib.pcg_cfg_validate.restype = C.c_int
    lib.pcg_cfg_validate.argtypes = [C.POINTER(pcg_env_cfg)]
    lib.pcg_rhs.restype = C.c_int
    lib.pcg_rhs.argtypes = [vp, C.c_int64, vp, vp, vp, vp]
    lib.pcg_integrate.restype = C.c_int
    lib.pcg_integrate.argtypes = [vp, C.c_int64, vp, vp, vp, vp]
    lib.pcg_rollout.restype = C.c_int
    lib.pcg_rollout.argtypes = [vp, C.POINTER(pcg_buffers), C.c_int32, C.c_int32, vp, vp, vp,
                                C.c_uint64, vp]
    lib.pcg_rollout_strided.restype = C.c_int
    lib.pcg_rollout_strided.argtypes = [vp, C.POINTER(pcg_buffers), C.c_int32, C.c_int32, vp, C.c_int64, C.c_int64,
                                        vp, C.c_int64, C.c_int64, vp, C.c_int64, C.c_uint64, vp]
    lib.pcg_policy_validate.restype = C.c_int
    lib.pcg_policy_validate.argtypes = [C.POINTER(pcg_policy_cfg)]
    lib.pcg_policy_create.restype = C.c_int
    lib.pcg_policy_create.argtypes = [C.POINTER(vp), C.POINTER(pcg_policy_cfg)]
    lib.pcg_policy_create_f32.restype = C.c_int
    lib.pcg_policy_create_f32.argtypes = [C.POINTER(vp), C.POINTER(pcg_policy_cfg)]
    lib.pcg_policy_dtype.restype = C.c_int
    lib.pcg_policy_dtype.argtypes = [vp]
    lib.pcg_policy_destroy.restype = C.c_int
    lib.pcg_policy_destroy.argtypes = [vp]
    lib.pcg_rollout_policy.restype = C.c_int
    lib.pcg_rollout_policy.argtypes = [vp, C.POINTER(pcg_buffers), vp, C.c_int32, C.c_int32, vp, C.c_int64, C.c_int64,
                                       vp, C.c_int64, C.c_int64, vp, C.c_int64, C.c_int32, C.c_uint64, vp]
    lib.pcg_plan_prepare_closed_loop.restype = C.c_int
    lib.pcg_plan_prepare_closed_loop.argtypes = [vp]
    lib.pcg_policy_update.restype = C.c_int
    lib.pcg_policy_update.argtypes = [vp, C.POINTER(pcg_policy_cfg)]
    lib.pcg_rollout_actor.restype = C.c_int
    lib.pcg_rollout_actor.argtypes = [vp, C.POINTER(pcg_buffers), vp, vp, _pd, C.c_int32, C.c_int32,
                                      vp, C.c_int64, C.c_int64, vp, C.c_int64, C.c_int64, vp, C.c_int64, vp, C.c_int64,
                                      vp, C.c_int64, C.c_int64, vp, C.c_int64, C.c_int32, C.c_uint64, vp]
    # (the two on plans with constraint rows: the same lists with g_seq / strides / viol_seq / stride ahead of the seed)
    lib.pcg_rollout_policy_cons.restype = C.c_int
    lib.pcg_rollout_policy_cons.argtypes = (lib.pcg_rollout_policy.argtypes[:-2] + [vp, C.c_int64, C.c_int64, vp, C.c_int64]
                                            + lib.pcg_rollout_policy.argtypes[-2:])
    lib.pcg_rollout_actor_cons.restype = C.c_int
    lib.pcg_rollout_actor_cons.argtypes = (lib.pcg_rollout_actor.argtypes[:-2] + [vp, C.c_int64, C.c_int64, vp, C.c_int64]
                                           + lib.pcg_rollout_actor.argtypes[-2:])
    lib.pcg_rollout_policy_unc.restype = C.c_int
    lib.pcg_rollout_policy_unc.argtypes = list(lib.pcg_rollout_policy.argtypes)
    lib.pcg_rollout_actor_unc.restype = C.c_int
    lib.pcg_rollout_actor_unc.argtypes = list(lib.pcg_rollout_actor.argtypes)
    lib.pcg_actor_logp_const.restype = C.c_double
    lib.pcg_actor_logp_const.argtypes = [_pd, C.c_int32]
    lib.pcg_policy_noise.restype = C.c_int
    lib.pcg_policy_noise.argtypes = [vp, C.c_int64, C.c_int32, C.c_uint64, vp, vp]
    lib.pcg_gae.restype = C.c_int
    lib.pcg_gae.argtypes = [C.c_int64, C.c_int32, vp, C.c_int64, vp, C.c_int64, vp, C.c_int64, C.c_double, C.c_double, C.c_int32,
                            vp, C.c_int64, vp, C.c_int64, vp]
    lib.pcg_policy_pop_create.restype = C.c_int
    lib.pcg_policy_pop_create.argtypes = [C.POINTER(vp), C.POINTER(pcg_policy_cfg), C.c_int32]
    lib.pcg_policy_pop_create_f32.restype = C.c_int
    lib.pcg_policy_pop_create_f32.argtypes = [C.POINTER(vp), C.POINTER(pcg_policy_cfg), C.c_int32]
    lib.pcg_policy_pop_dtype.restype = C.c_int
    lib.pcg_policy_pop_dtype.argtypes = [vp]
    lib.pcg_policy_pop_update.restype = C.c_int
    lib.pcg_policy_pop_update.argtypes = [vp, C.POINTER(pcg_policy_cfg), C.c_int32, C.c_int32]
    lib.pcg_policy_pop_destroy.restype = C.c_int
    lib.pcg_policy_pop_destroy.argtypes = [vp]
    lib.pcg_policy_pop_size.restype = C.c_int
    lib.pcg_policy_pop_size.argtypes = [vp]
    # (pcg_rollout_policy's list with envs_per_policy after the handle and gamma / ret_out ahead of the seed)
    lib.pcg_rollout_policy_pop.restype = C.c_int
    lib.pcg_rollout_policy_pop.argtypes = (lib.pcg_rollout_policy.argtypes[:3] + [C.c_int64] + lib.pcg_rollout_policy.argtypes[3:-2]
                                           + [C.c_double, vp] + lib.pcg_rollout_policy.argtypes[-2:])
    lib.pcg_rollout_policy_pop_unc.restype = C.c_int
    lib.pcg_rollout_policy_pop_unc.argtypes = list(lib.pcg_rollout_policy_pop.argtypes)
    # (on plans with constraint rows: g_seq / strides / viol_seq / stride after record_next_action, nviol_out / gmax_out after ret_out)
    lib.pcg_rollout_policy_pop_cons.restype = C.c_int
    lib.pcg_rollout_policy_pop_cons.argtypes = (lib.pcg_rollout_policy_pop.argtypes[:-4] + [vp, C.c_int64, C.c_int64, vp, C.c_int64]
                                                + lib.pcg_rollout_policy_pop.argtypes[-4:-2] + [vp, vp]
                                                + lib.pcg_rollout_policy_pop.argtypes[-2:])
    # (the weights of a population on the device: sample, noise sum, flat vectors out and in)
    lib.pcg_policy_pop_nparams.restype = C.c_int
    lib.pcg_policy_pop_nparams.argtypes = [vp]
    lib.pcg_policy_pop_sample.restype = C.c_int
    lib.pcg_policy_pop_sample.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, C.c_int32, C.c_uint64, C.c_uint32, vp]
    lib.pcg_policy_pop_noise_dot.restype = C.c_int
    lib.pcg_policy_pop_noise_dot.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_uint32, vp, vp, vp, vp]
    lib.pcg_policy_pop_get_flat.restype = C.c_int
    lib.pcg_policy_pop_get_flat.argtypes = [vp, vp, C.c_int32, C.c_int32, vp, C.c_int64, vp]
    lib.pcg_policy_pop_set_flat.restype = C.c_int
    lib.pcg_policy_pop_set_flat.argtypes = [vp, C.c_int32, C.c_int32, vp, C.c_int64, vp]
    lib.pcg_step_autoreset.restype = C.c_int
    lib.pcg_step_autoreset.argtypes = [vp, C.POINTER(pcg_buffers), C.c_int32, C.c_uint64, C.c_uint64, vp]
    lib.pcg_graph_create.restype = C.c_int
    lib.pcg_graph_create.argtypes = [C.POINTER(vp), vp, C.POINTER(pcg_buffers), C.POINTER(vp), C.POINTER(vp),
                                     C.c_int32, C.c_int32, C.c_uint64, C.c_int]
    lib.pcg_graph_launch.restype = C.c_int
    lib.pcg_graph_launch.argtypes = [vp, vp]
    lib.pcg_graph_set_seed.restype = C.c_int
    lib.pcg_graph_set_seed.argtypes = [vp, C.c_uint64]
    lib.pcg_graph_destroy.restype = C.c_int
    lib.pcg_graph_destroy.argtypes = [vp]
    lib.pcg_graph_held.restype = C.c_int
    lib.pcg_graph_held.argtypes = [vp, _pi, _pi]
    lib.pcg_graph_chained.restype = C.c_int
    lib.pcg_graph_chained.argtypes = [vp, _pi, _pi]
    lib.pcg_last_jit_log.restype = C.c_char_p
    lib.pcg_last_jit_log.argtypes = []
    lib.pcg_test_sort_tile.restype = C.c_int
    lib.pcg_test_sort_tile.argtypes = [vp, C.c_int32, C.c_int32, C.c_int64, vp]
    lib.pcg_coverage_names.restype = C.c_int64
    lib.pcg_coverage_names.argtypes = [C.c_char_p, C.c_int64, C.c_int]
    lib.pcg_philox4x32_10.restype = None
    lib.pcg_philox4x32_10.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                      C.POINTER(C.c_uint32)]
    return lib
