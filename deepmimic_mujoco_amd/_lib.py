"""ctypes binding of libdeepmimic_hip.so (include/deepmimic_hip.h).

There is NO CPU fallback: if the HIP library is missing or no MI355X is visible
the constructor of :class:`HipEngine` raises.  PyTorch is used only as the owner
of device buffers (``tensor.data_ptr()``) and of the HIP stream.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .model import DmModel, NBODY, NQ, NV, NU, NOBS

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdeepmimic_hip.so")
DEBUG_STRIDE = 416

REASONS = {0: None, 1: "low_z", 2: "high_z", 3: "max_ep_len", 4: "acyclical_end",
           5: "sim_error", 6: "obs_out_of_bounds", 7: "fallen without amnesty"}
TASK_DPENV, TASK_COMBINED = 0, 1

EXPORTS = ["dm_default_config", "dm_create", "dm_destroy", "dm_last_error", "dm_num_envs",
           "dm_load_clip", "dm_set_env_clips", "dm_reset", "dm_step", "dm_step_forced", "dm_physics_step",
           "dm_set_state", "dm_get_state", "dm_get_counters", "dm_set_counters", "dm_set_debug",
           "dm_fill_random_actions", "dm_last_step_ms", "dm_enable_timing", "dm_get_work",
           "dm_set_clip_flags", "dm_obs_dim", "dm_terms_dim", "dm_get_env_clips", "dm_mean_step_ms", "dm_ppo_loss", "dm_forward", "dm_linear_wgrad", "dm_ppo_gather", "dm_flat_adam_step", "dm_policy_sample",
           "dm_rollout_store", "dm_policy_pack", "dm_policy_forward", "dm_policy_packed_floats", "dm_ppo_mlp_grad", "dm_ppo_mlp_workspace_floats", "dm_flat_adam_update", "dm_flat_adam_step_gather", "dm_colsum", "dm_set_seed",
           "dm_linear_tanh", "dm_tanh_linear_wgrad", "dm_tanh_bwd_colsum",
           "dm_ppo_wide_grad", "dm_ppo_wide_packed_elems", "dm_ppo_wide_dp", "dm_ppo_wide_supported",
           "dm_ppo_wide3_grad", "dm_ppo_wide3_packed_elems", "dm_ppo_wide3_supported",
           "dm_sac_act", "dm_sac_store", "dm_sac_gather", "dm_sac_head_fwd", "dm_sac_critic_loss", "dm_sac_actor_loss",
           "dm_sac_head_bwd", "dm_sac_linear_relu", "dm_sac_relu_bwd_colsum", "dm_sac_polyak",
           "dm_rollout_finish", "dm_rollout_finish_workspace_bytes",
           "dm_policy_forward_bf16", "dm_rollout_store_bf16", "dm_ppo_gather_bf16", "dm_flat_adam_step_gather_bf16",
           "dm_step_active", "dm_eval_advance"]
# include/deepmimic_render.h (csrc/dm_render.hip); EXPORTS above is the list of include/deepmimic_hip.h alone
RENDER_EXPORTS = ["dm_render_create", "dm_render_destroy", "dm_render_last_error", "dm_render_kinematics", "dm_render_cast", "dm_render"]
# include/deepmimic_trace.h (csrc/dm_trace.hip): the episode debug log, debug_log.FlightRecorder
TRACE_EXPORTS = ["dm_trace_record", "dm_trace_mark", "dm_trace_last_error"]
# include/deepmimic_vecnorm.h (csrc/dm_vecnorm.hip): SB3's VecNormalize, vec_normalize.HipVecNormalize
VECNORM_EXPORTS = ["dm_vecnorm_scratch_bytes", "dm_vecnorm_step", "dm_vecnorm_reset", "dm_vecnorm_apply", "dm_vecnorm_last_error",
                   "dm_vecnorm_step_sync", "dm_vecnorm_reset_sync", "dm_vecnorm_sync_pack", "dm_vecnorm_sync_merge"]
# include/deepmimic_sac_norm.h (csrc/dm_sac.hip): SAC's minibatch gather with VecNormalize applied at sample time, SAC(normalizer=)
SAC_NORM_EXPORTS = ["dm_sac_gather_norm"]
# include/deepmimic_sac_nstep.h (csrc/dm_sac.hip): SAC's minibatch gather with n-step returns, SAC(n_steps=)
SAC_NSTEP_EXPORTS = ["dm_sac_gather_nstep"]
SAC_NSTEP_MAX = 64                                       # DM_SAC_NSTEP_MAX: one lane of a wave per step of the chain


class DmVecNormSync(C.Structure):
    """include/deepmimic_vecnorm.h: DmVecNormSync"""
    _fields_ = [("world", C.c_int32), ("rank", C.c_int32), ("base", C.c_void_p), ("acc", C.c_void_p), ("gather", C.c_void_p)]


class DmConfig(C.Structure):
    _fields_ = [("num_envs", C.c_int32), ("max_ep_length", C.c_int32),
                ("vel_obs_scale", C.c_float), ("low_z", C.c_float), ("high_z", C.c_float),
                ("w_pose", C.c_float), ("w_vel", C.c_float), ("w_end_eff", C.c_float),
                ("w_com", C.c_float), ("w_joint_limit", C.c_float), ("obs_bound", C.c_float),
                ("seed", C.c_uint64), ("auto_reset", C.c_int32), ("device", C.c_int32),
                ("lpt_schedule", C.c_int32), ("task", C.c_int32),
                ("amnesty_steps", C.c_int32), ("to_getup_len", C.c_int32),
                ("integrator", C.c_int32), ("stale_contact_slots", C.c_int32)]


INTEGRATORS = {None: 0, "model": 0, "Euler": 1, "euler": 1, "RK4": 2, "rk4": 2}   # DM_CFG_INT_*


class DmPpoStepHead(C.Structure):
    """The fields DmPpoMlpStep and DmPpoWideStep (include/deepmimic_hip.h) share, B through g_log_std.  It ends on a pointer, so it
    has no tail padding and a derived struct's own fields follow at the offsets the header gives them."""
    _fields_ = [("B", C.c_int32), ("D", C.c_int32), ("H1", C.c_int32), ("H2", C.c_int32), ("A", C.c_int32),
                ("normalize_advantage", C.c_int32), ("clip_range", C.c_float), ("vf_coef", C.c_float), ("ent_coef", C.c_float),
                ("reserved", C.c_int32),
                ("obs", C.c_void_p), ("act", C.c_void_p), ("adv", C.c_void_p), ("ret", C.c_void_p), ("old_logp", C.c_void_p),
                ("log_std", C.c_void_p),
                ("W", (C.c_void_p * 3) * 2), ("b", (C.c_void_p * 3) * 2), ("gW", (C.c_void_p * 3) * 2), ("gb", (C.c_void_p * 3) * 2),
                ("g_log_std", C.c_void_p)]


class DmPpoMlpStep(DmPpoStepHead):
    """include/deepmimic_hip.h: DmPpoMlpStep"""
    _fields_ = [("out8", C.c_void_p), ("workspace", C.c_void_p), ("workspace_floats", C.c_longlong),
                ("zero_ptr", C.c_void_p), ("zero_floats", C.c_longlong), ("adam_state2", C.c_void_p), ("loss_acc", C.c_void_p)]


class DmGatherSpec(C.Structure):
    """include/deepmimic_hip.h: DmGatherSpec"""
    _fields_ = [("idx", C.c_void_p), ("B", C.c_int32), ("D", C.c_int32), ("A", C.c_int32), ("reserved", C.c_int32),
                ("obs", C.c_void_p), ("act", C.c_void_p), ("adv", C.c_void_p), ("ret", C.c_void_p), ("logp", C.c_void_p),
                ("o_obs", C.c_void_p), ("o_act", C.c_void_p), ("o_adv", C.c_void_p), ("o_ret", C.c_void_p), ("o_logp", C.c_void_p)]


class DmGatherSpecBf16(DmGatherSpec):
    """include/deepmimic_hip.h: DmGatherSpecBf16 — DmGatherSpec's layout; obs / act point at bf16 rows"""


class DmPpoWideStep(DmPpoStepHead):
    """include/deepmimic_hip.h: DmPpoWideStep"""
    _fields_ = [("wpk", C.c_void_p * 2), ("xbT", C.c_void_p), ("h1T", C.c_void_p * 2), ("dz1T", C.c_void_p * 2), ("h2T", C.c_void_p * 2),
                ("dz2T", C.c_void_p * 2), ("dz3T", C.c_void_p * 2), ("part", C.c_void_p), ("stats8", C.c_void_p), ("out8", C.c_void_p),
                ("zero_ptr", C.c_void_p), ("zero_floats", C.c_longlong), ("adam_state2", C.c_void_p), ("loss_acc", C.c_void_p)]


class DmPpoWide3Step(DmPpoWideStep):
    """include/deepmimic_hip.h: DmPpoWide3Step — DmPpoWideStep's layout; every bf16 scratch array holds two planes (hi, lo)"""


class DmTraceBufs(C.Structure):
    """include/deepmimic_trace.h: DmTraceBufs"""
    _fields_ = [("N", C.c_int32), ("K", C.c_int32), ("C", C.c_int32), ("nq", C.c_int32), ("nv", C.c_int32), ("na", C.c_int32),
                ("W", C.c_int32), ("device", C.c_int32),
                ("ring", C.c_void_p), ("head", C.c_void_p), ("cap", C.c_void_p), ("cap_meta", C.c_void_p), ("cap_count", C.c_void_p),
                ("trig", C.c_void_p)]


class DmVecNorm(C.Structure):
    """include/deepmimic_vecnorm.h: DmVecNorm"""
    _fields_ = [("N", C.c_int32), ("D", C.c_int32), ("device", C.c_int32), ("training", C.c_int32), ("norm_obs", C.c_int32),
                ("norm_reward", C.c_int32), ("gamma", C.c_double), ("epsilon", C.c_double), ("clip_obs", C.c_double),
                ("clip_reward", C.c_double), ("obs_mean", C.c_void_p), ("obs_var", C.c_void_p), ("obs_count", C.c_void_p),
                ("ret_stats", C.c_void_p), ("returns", C.c_void_p), ("scratch", C.c_void_p), ("scratch_bytes", C.c_int64)]


# floats of the state2 buffer of dm_flat_adam_*: {scratch, step count, DM_ADAM_PARTIALS partial sums} (include/deepmimic_hip.h)
ADAM_STATE_FLOATS = 2 + 1024

_LIB = None


def load_library():
    """dlopen the in-tree HIP library; raise loudly if it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libdeepmimic_hip.so is missing (%s). Build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C deepmimic_mujoco_amd/csrc`. There is no CPU fallback." % LIB_PATH)
    # PyTorch bundles its own libamdhip64.so.7; import it first so this library binds to the SAME
    # HIP runtime instance (two runtimes in one process cannot share a device context).
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    vp, i32 = C.c_void_p, C.c_int
    L.dm_default_config.argtypes = [C.POINTER(DmConfig)]
    L.dm_default_config.restype = None
    L.dm_create.argtypes = [C.POINTER(DmModel), C.POINTER(DmConfig), C.POINTER(vp)]
    L.dm_destroy.argtypes = [vp]
    L.dm_last_error.argtypes = [vp]
    L.dm_last_error.restype = C.c_char_p
    L.dm_num_envs.argtypes = [vp]
    L.dm_obs_dim.argtypes = [vp]
    L.dm_terms_dim.argtypes = [vp]
    L.dm_get_env_clips.argtypes = [vp, vp, vp]
    L.dm_load_clip.argtypes = [vp, i32, i32, vp, vp, vp, vp]
    L.dm_set_env_clips.argtypes = [vp, vp, vp]
    L.dm_reset.argtypes = [vp, vp, vp, vp, vp]
    L.dm_step.argtypes = [vp] * 9
    L.dm_step_forced.argtypes = [vp] * 9
    L.dm_step_active.argtypes = [vp, vp, vp, i32] + [vp] * 6
    L.dm_eval_advance.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp, i32] + [vp] * 8 + [i32, vp]
    L.dm_physics_step.argtypes = [vp] * 3
    L.dm_set_state.argtypes = [vp, vp, i32, vp, vp, vp, vp, i32, vp]
    L.dm_get_state.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp]
    L.dm_forward.argtypes = [vp, vp, i32, vp]
    L.dm_linear_wgrad.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp]
    L.dm_policy_sample.argtypes = [vp, vp, i32, i32, C.c_uint64, vp, vp, vp, vp, vp, vp, vp]
    L.dm_rollout_store.argtypes = [i32, i32, i32] + [vp] * 16
    L.dm_rollout_store_bf16.argtypes = L.dm_rollout_store.argtypes
    L.dm_policy_packed_floats.argtypes = [i32] * 4
    L.dm_ppo_mlp_workspace_floats.argtypes = [i32] * 5
    L.dm_ppo_mlp_grad.argtypes = [C.POINTER(DmPpoMlpStep), vp]
    L.dm_ppo_wide_grad.argtypes = [C.POINTER(DmPpoWideStep), vp]
    L.dm_ppo_wide_packed_elems.argtypes = [i32, i32, i32]
    L.dm_ppo_wide_dp.argtypes = [i32]
    L.dm_ppo_wide_supported.argtypes = [i32] * 5
    L.dm_ppo_wide3_grad.argtypes = [C.POINTER(DmPpoWide3Step), vp]
    L.dm_ppo_wide3_packed_elems.argtypes = [i32, i32, i32]
    L.dm_ppo_wide3_supported.argtypes = [i32] * 5
    L.dm_policy_pack.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp, vp]
    L.dm_policy_forward.argtypes = [vp] + [i32] * 5 + [vp] * 9 + [C.c_uint64, vp, C.c_uint32, i32] + [vp] * 9
    L.dm_policy_forward_bf16.argtypes = L.dm_policy_forward.argtypes
    L.dm_flat_adam_step.argtypes = [vp, vp, vp, vp, i32] + [C.c_float] * 6 + [vp, i32, vp]
    L.dm_colsum.argtypes = [vp, i32, i32, vp, vp]
    L.dm_linear_tanh.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp]
    L.dm_tanh_linear_wgrad.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp]
    L.dm_tanh_bwd_colsum.argtypes = [vp, vp, vp, vp, i32, i32, vp]
    L.dm_flat_adam_update.argtypes = [vp, vp, vp, vp, i32] + [C.c_float] * 6 + [vp, i32, vp]
    L.dm_flat_adam_step_gather.argtypes = [vp, vp, vp, vp, i32] + [C.c_float] * 6 + [vp, i32, i32, vp, vp]
    L.dm_flat_adam_step_gather.restype = i32
    L.dm_flat_adam_step_gather_bf16.argtypes = L.dm_flat_adam_step_gather.argtypes
    L.dm_ppo_gather.argtypes = [vp, i32, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.dm_ppo_gather_bf16.argtypes = L.dm_ppo_gather.argtypes
    L.dm_get_counters.argtypes = [vp, vp, vp, vp, vp]
    L.dm_set_counters.argtypes = [vp, vp, vp, vp]
    L.dm_set_debug.argtypes = [vp, vp]
    L.dm_set_seed.argtypes = [vp, C.c_uint64]
    L.dm_get_work.argtypes = [vp, vp, vp]
    L.dm_set_clip_flags.argtypes = [vp, i32, i32]
    L.dm_fill_random_actions.argtypes = [vp, vp, C.c_uint32, vp]
    L.dm_last_step_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.dm_enable_timing.argtypes = [vp, i32]
    L.dm_ppo_loss.argtypes = [vp] * 7 + [i32, i32, C.c_float, C.c_float, C.c_float, i32] + [vp] * 6
    L.dm_mean_step_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_int32)]
    u64, f32 = C.c_uint64, C.c_float
    L.dm_sac_act.argtypes = [vp, i32, i32, i32, u64, vp, i32, i32, vp, vp, vp, vp, vp]
    L.dm_sac_store.argtypes = [i32, i32, i32, i32] + [vp] * 17
    L.dm_sac_gather.argtypes = [i32, i32, i32, i32, u64] + [vp] * 15
    L.dm_sac_head_fwd.argtypes = [vp, i32, i32, i32, u64, vp, vp, vp, i32, vp, vp, i32, f32, f32, vp]
    L.dm_sac_critic_loss.argtypes = [vp] * 5 + [i32, f32] + [vp] * 4
    L.dm_sac_actor_loss.argtypes = [vp, vp, i32, vp, vp, vp]
    L.dm_sac_head_bwd.argtypes = [vp, i32, i32, u64, vp, vp, i32, i32, vp, vp, vp, vp]
    L.dm_sac_linear_relu.argtypes = [vp, i32, vp, vp, vp, i32, i32, i32, i32, vp]
    L.dm_sac_relu_bwd_colsum.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp]
    L.dm_sac_polyak.argtypes = [vp, vp, C.c_longlong, f32, vp, vp]
    L.dm_rollout_finish_workspace_bytes.argtypes = [i32, i32]
    L.dm_rollout_finish.argtypes = [i32, i32, vp, vp, i32, vp, vp, C.c_double, C.c_double] + [vp] * 7 + [C.c_longlong, vp]
    L.dm_render_create.argtypes = [vp, C.POINTER(vp)]
    L.dm_render_destroy.argtypes = [vp]
    L.dm_render_last_error.argtypes = [vp]
    L.dm_render_last_error.restype = C.c_char_p
    L.dm_render_kinematics.argtypes = [vp, vp, vp, i32, vp, vp, vp]
    L.dm_render_cast.argtypes = [vp, vp, vp, i32, vp, i32, i32, vp, vp, vp, vp]
    L.dm_render.argtypes = [vp, vp, vp, i32, vp, i32, i32, vp, vp, vp, vp, vp]
    L.dm_trace_record.argtypes = [C.POINTER(DmTraceBufs)] + [vp] * 8 + [i32, C.c_uint32, vp]
    L.dm_trace_mark.argtypes = [C.POINTER(DmTraceBufs)] + [vp] * 4 + [i32, vp]
    L.dm_trace_last_error.argtypes = []
    L.dm_trace_last_error.restype = C.c_char_p
    L.dm_vecnorm_scratch_bytes.argtypes = [i32, i32]
    L.dm_vecnorm_scratch_bytes.restype = C.c_longlong
    L.dm_vecnorm_step.argtypes = [C.POINTER(DmVecNorm)] + [vp] * 8
    L.dm_vecnorm_reset.argtypes = [C.POINTER(DmVecNorm)] + [vp] * 3
    L.dm_vecnorm_apply.argtypes = [C.POINTER(DmVecNorm), i32] + [vp] * 5
    L.dm_vecnorm_last_error.argtypes = []
    L.dm_vecnorm_step_sync.argtypes = [C.POINTER(DmVecNorm)] + [vp] * 7 + [C.POINTER(DmVecNormSync), vp]
    L.dm_vecnorm_reset_sync.argtypes = [C.POINTER(DmVecNorm)] + [vp] * 2 + [C.POINTER(DmVecNormSync), vp]
    L.dm_vecnorm_sync_pack.argtypes = [C.POINTER(DmVecNorm), C.POINTER(DmVecNormSync), vp]
    L.dm_vecnorm_sync_merge.argtypes = [C.POINTER(DmVecNorm), C.POINTER(DmVecNormSync), vp]
    L.dm_vecnorm_last_error.restype = C.c_char_p
    L.dm_sac_gather_norm.argtypes = L.dm_sac_gather.argtypes[:-1] + [C.POINTER(DmVecNorm), vp]
    L.dm_sac_gather_norm.restype = C.c_int
    # dm_sac_gather's arguments up to idx_out, then cap_steps, n_steps, gamma, k_out, the nullable DmVecNorm, the stream
    L.dm_sac_gather_nstep.argtypes = L.dm_sac_gather.argtypes[:-1] + [i32, i32, f32, vp, C.POINTER(DmVecNorm), vp]
    L.dm_sac_gather_nstep.restype = C.c_int
    for name in EXPORTS:
        if name not in ("dm_default_config", "dm_last_error"):
            getattr(L, name).restype = C.c_longlong if name in ("dm_policy_packed_floats", "dm_ppo_mlp_workspace_floats", "dm_ppo_wide_packed_elems", "dm_ppo_wide3_packed_elems", "dm_rollout_finish_workspace_bytes") else C.c_int
    _LIB = L
    return L


def call(name, *args, device):
    """Run the entry point ``name`` on ``device``'s current stream: a tensor argument becomes its ``data_ptr()``, anything else
    (ints, floats, ``None``, ``byref(...)``) goes through ``argtypes`` as it is, the stream is appended as the last argument.
    Raises ``RuntimeError("<name> failed (<rc>)")`` on a non-zero return."""
    import torch
    rc = getattr(load_library(), name)(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args],
                                       torch.cuda.current_stream(device).cuda_stream)
    if rc != 0:
        raise RuntimeError("%s failed (%d)" % (name, rc))


def default_config(**kw) -> DmConfig:
    cfg = DmConfig()
    load_library().dm_default_config(C.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class EngineBase:
    """Handle lifetime and the entry points that ``dm_*`` (humanoid3d) and ``dmg1_*`` (Unitree G1) mirror.  A subclass sets
    ``PREFIX``, the dimensions and, in its constructor, ``torch``, ``L``, ``h``, ``N``, ``device``, ``obs_dim``, ``terms_dim``,
    ``_debug = None``; all tensors are torch CUDA tensors owned by the caller."""

    PREFIX = None          # "dm_" / "dmg1_"
    DEBUG_STRIDE = None    # floats per env of the debug buffer
    NQ = NV = NBODY = None

    def close(self):
        if getattr(self, "h", None):
            getattr(self.L, self.PREFIX + "destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, name, *args, stream=True):
        """``<PREFIX><name>(handle, *args[, current stream])``: tensors go as their ``data_ptr()``; a non-zero return raises."""
        entry = self.PREFIX + name
        args = [_ptr(a) if isinstance(a, self.torch.Tensor) else a for a in args]
        if stream:
            args.append(C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream))
        rc = getattr(self.L, entry)(self.h, *args)
        if rc != 0:
            raise RuntimeError("%s failed (%d): %s" % (entry, rc, (getattr(self.L, self.PREFIX + "last_error")(self.h) or b"").decode()))

    def _zeros(self, *shape, dtype=None):
        return self.torch.zeros(self.N, *shape, dtype=dtype or self.torch.float32, device=self.device)

    def alloc_outputs(self):
        z, t = self._zeros, self.torch
        return dict(obs=z(self.obs_dim), rew=z(), done=z(dtype=t.uint8), terms=z(self.terms_dim), reason=z(dtype=t.int32),
                    terminal_obs=z(self.obs_dim))

    def enable_debug(self, on=True):
        self._debug = self._zeros(self.DEBUG_STRIDE) if on else None
        self._call("set_debug", self._debug, stream=False)
        return self._debug

    def body_xpos(self, env=0):
        """[nbody, 3] float64 world positions of ``env``'s bodies at its stored state.  The derived arrays are refreshed by a
        forward evaluation and the warm start is put back: looking at an env is not physics."""
        if self._debug is None:
            self.enable_debug()
        rec, self._recorder = self._recorder, None      # the refresh goes through set_state: not an event of the episode
        try:
            self._refresh_derived()
        finally:
            self._recorder = rec
        return self._debug[env, :3 * self.NBODY].double().cpu().numpy().reshape(self.NBODY, 3)

    # ---- hot path.  ``_recorder``: a debug_log.FlightRecorder attached to this engine, or None.  With one attached every step is
    # followed by ``record`` and every state set from outside by ``mark``; without one the calls below are the engine's alone.
    _recorder = None

    def _reason_of(self, out):
        """``out``'s reason tensor; the recorder's own when it needs one and the caller asked for none."""
        r = out.get("reason")
        return self._recorder.reason if (r is None and self._recorder is not None) else r

    def reset(self, obs, idx_init=None, mask=None):
        self._call("reset", mask, idx_init, obs)
        if self._recorder is not None:
            self._recorder.mark_reset(mask)

    def step(self, actions, out):
        reason = self._reason_of(out)
        self._call("step", actions, out["obs"], out["rew"], out["done"], out.get("terms"), reason, out.get("terminal_obs"))
        if self._recorder is not None:
            self._recorder.record(actions, out, reason=reason)

    def step_forced(self, qpos, qvel, out):
        self._call("step_forced", qpos, qvel, out["obs"], out["rew"], out["done"], out.get("terms"), out.get("reason"))
        if self._recorder is not None:
            self._recorder.mark()

    def step_active(self, actions, env_ids, nslots, out):
        """``dm_step_active`` / ``dmg1_step_active``: the envs listed in ``env_ids[:nslots]`` (int32 device tensor, entries < 0
        skipped) take one step without auto-reset; ``actions`` and the rows of ``out`` stay indexed by env."""
        reason = self._reason_of(out)
        self._call("step_active", actions, env_ids, int(nslots), out["obs"], out["rew"], out["done"], out.get("terms"), reason)
        if self._recorder is not None:
            self._recorder.record(actions, out, env_ids=env_ids, nslots=int(nslots), reason=reason)

    def get_counters(self):
        """(idx_curr int32[N], episode_length int32[N], episode_reward float32[N])"""
        t = self.torch
        idx, ln, rew = self._zeros(dtype=t.int32), self._zeros(dtype=t.int32), self._zeros()
        self._call("get_counters", idx, ln, rew)
        return idx, ln, rew

    def set_counters(self, idx_curr=None, episode_length=None):
        self._call("set_counters", idx_curr, episode_length)

    def set_seed(self, seed):
        """gym's env.seed(): re-key the reset / random-action generator."""
        self._call("set_seed", int(seed) & 0xFFFFFFFFFFFFFFFF, stream=False)

    def get_env_clips(self):
        """Per-env clip id (DPEnv task) or motion id 0 walk / 1 run / 2 getup / 3 to_getup (combined task)."""
        out = self._zeros(dtype=self.torch.int32)
        self._call("get_env_clips", out)
        return out


class HipEngine(EngineBase):
    """The humanoid3d engine: thin object wrapper over a DmHandle."""

    PREFIX, DEBUG_STRIDE, NQ, NV, NBODY = "dm_", DEBUG_STRIDE, NQ, NV, NBODY

    def __init__(self, model, num_envs, device=0, seed=1234, auto_reset=True, integrator=None, **cfg_kw):
        import torch
        cfg_kw["integrator"] = INTEGRATORS[integrator]
        if not torch.cuda.is_available():
            raise RuntimeError("no MI355X visible to HIP: the DeepMimic engine has no CPU fallback")
        self.torch = torch
        self.L = load_library()
        self.model = model
        self.N = int(num_envs)
        self.device = torch.device("cuda", device)
        self.auto_reset = bool(auto_reset)
        self.cfg = default_config(num_envs=self.N, device=device, seed=seed,
                                  auto_reset=1 if auto_reset else 0, **cfg_kw)
        h = C.c_void_p()
        rc = self.L.dm_create(C.byref(model.cstruct), C.byref(self.cfg), C.byref(h))
        if rc != 0:
            raise RuntimeError("dm_create failed with code %d" % rc)
        self.h = h
        self.obs_dim = self.L.dm_obs_dim(h)      # 67 (DPEnv) or 72 (DPCombinedEnv)
        self.terms_dim = self.L.dm_terms_dim(h)  # 5 or 8
        self.clip_len = {}
        self._debug = None

    # ---- clips
    def load_clip(self, clip_id, mocap, floor=False, acyclic=False):
        q, v, b, g = [np.ascontiguousarray(a, np.float64) for a in mocap.tables()]
        self._call("load_clip", clip_id, len(q), *[a.ctypes.data_as(C.c_void_p) for a in (q, v, b, g)], stream=False)
        self.clip_len[clip_id] = len(q)
        self._call("set_clip_flags", clip_id, (1 if floor else 0) | (2 if acyclic else 0), stream=False)

    def set_env_clips(self, clip_ids):
        t = None if clip_ids is None else clip_ids.to(self.device, self.torch.int32).contiguous()
        self._call("set_env_clips", t)
        self._keep = t

    # ---- state
    def physics_step(self, actions):
        """sim.step() alone (src/deepmimic_env.py:362): the state advances, nothing is observed (dm_physics_step)."""
        self._call("physics_step", actions)

    def set_state(self, qpos, qvel, warm=None, ctrl=None, env_ids=None, run_forward=False):
        self._call("set_state", env_ids, qpos.shape[0], qpos, qvel, warm, ctrl, 1 if run_forward else 0)
        if self._recorder is not None:
            self._recorder.mark(env_ids=env_ids, nslots=qpos.shape[0])

    def forward(self, env_ids=None, n=None):
        """sim.forward(): re-evaluate the derived quantities at the stored state."""
        self._call("forward", env_ids, self.N if n is None else n)

    def get_state(self, env_ids=None, n=None):
        t, d = self.torch, self.device
        n = self.N if n is None else n
        qpos, qvel = t.zeros(n, NQ, device=d), t.zeros(n, NV, device=d)
        warm, ctrl = t.zeros(n, NV, device=d), t.zeros(n, NU, device=d)
        self._call("get_state", env_ids, n, qpos, qvel, warm, ctrl)
        return qpos, qvel, warm, ctrl

    def _refresh_derived(self):
        q, v, w, c = self.get_state()
        self.forward()
        self.set_state(q, v, warm=w, ctrl=c, run_forward=False)     # the forward pass overwrote warm start and ctrl

    def fill_random_actions(self, actions, step_index):
        self._call("fill_random_actions", actions, int(step_index))

    def get_work(self):
        w = self._zeros(dtype=self.torch.int32)
        self._call("get_work", w)
        return w

    def enable_timing(self, on=True, stride=1):
        """HIP event pair around every ``stride``-th step-kernel launch (ring of 512 pairs, read by mean_step_ms)."""
        self._call("enable_timing", max(1, int(stride)) if on else 0, stream=False)

    def mean_step_ms(self):
        """(mean kernel ms, launches) over the steps since enable_timing(True); synchronises."""
        ms, n = C.c_float(0), C.c_int32(0)
        self._call("mean_step_ms", C.byref(ms), C.byref(n), stream=False)
        return ms.value, n.value

    def last_step_ms(self):
        ms = C.c_float(0)
        self._call("last_step_ms", C.byref(ms), stream=False)
        return ms.value
