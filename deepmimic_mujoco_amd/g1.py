"""Unitree G1 engine — ctypes binding of the dmg1_* entry points of libdeepmimic_hip.so (include/deepmimic_g1_hip.h).

Second robot of the reference: ``DPEnv(robot="unitree_g1")`` (src/deepmimic_env.py:272-484 with the unitree_g1 branches,
model ``deepmimic_unitree_g1.xml``).  The model is compiled by :mod:`mjcf` (general MJCF compiler + hull asset) into
``struct DmModel`` at the G1 dimensions (include/dm_model.h under ``-DDM_ROBOT_G1``), mirrored here as :class:`DmModelG1`.
No CPU fallback: :class:`G1HipEngine` raises if the HIP library or a GPU is missing.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import mjcf, model as _model
from ._lib import INTEGRATORS, EngineBase, load_library
from .vec_env import Box, HipBatchEnv, HipImitationEnv, HipSingleEnv, _LazyCombinedInfos, _action_space, _check_renderer, _combined_info
from .config import RobotConfig

NQ, NV, NU, NBODY, NGEOM, NJNT, NM, MAXPAIR, NOBS = 44, 43, 37, 39, 94, 38, 434, 1024, 85
NACT, NMESH, NMESHVERT, NREWJ, NEE = 23, 32, 40000, 23, 4
NOBS_COMBINED = 98
TASK_DPENV, TASK_COMBINED = 0, 1
MAXCON, MAXROW, DEBUG_STRIDE = 48, 256, 1024
# [mjmodel.get_joint_qpos_addr(n) ...] minus root and hand joints (src/deepmimic_env.py:206-207)
REW_QPOS = [7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 32, 33, 34, 35, 36]
REW_QVEL = [6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 31, 32, 33, 34, 35]
CLIP_FLOOR, CLIP_ACYCLIC, CLIP_RUN_RULE = 1, 2, 4
REASONS = {0: None, 1: "low_z", 2: "high_z", 3: "max_ep_len", 4: "acyclical_end", 5: "sim_error", 6: "obs_out_of_bounds",
           7: "fallen without amnesty", 8: "run roll/pitch limit"}
EXPORTS = ["dmg1_default_config", "dmg1_model_sizeof", "dmg1_create", "dmg1_destroy", "dmg1_last_error", "dmg1_load_clip",
           "dmg1_reset", "dmg1_step", "dmg1_step_forced", "dmg1_set_state", "dmg1_get_state", "dmg1_get_counters",
           "dmg1_set_counters", "dmg1_set_debug", "dmg1_last_kernel_ms", "dmg1_obs_dim", "dmg1_get_motion", "dmg1_set_motion",
           "dmg1_set_seed", "dmg1_set_env_clips", "dmg1_get_env_clips", "dmg1_queue_counters", "dmg1_step_active",
           "dmg1_set_active_schedule", "dmg1_set_null_cache", "dmg1_sep_cache_entries"]

_i32, _f64 = C.c_int32, C.c_double


class DmModelG1(C.Structure):
    """ctypes mirror of ``struct DmModel`` under -DDM_ROBOT_G1 (include/dm_model.h) — keep in sync (size is checked)."""

    _fields_ = [
        ("nq", _i32), ("nv", _i32), ("nu", _i32), ("nbody", _i32), ("ngeom", _i32), ("njnt", _i32), ("npair", _i32),
        ("nM", _i32), ("integrator", _i32), ("iterations", _i32), ("pad0", _i32), ("pad1", _i32),
        ("timestep", _f64), ("tolerance", _f64), ("gravity", _f64 * 3), ("meaninertia", _f64), ("solref", _f64 * 2),
        ("solimp", _f64 * 5), ("qpos0", _f64 * NQ),
        ("body_parent", _i32 * NBODY), ("body_jntadr", _i32 * NBODY), ("body_jntnum", _i32 * NBODY),
        ("body_dofadr", _i32 * NBODY), ("body_dofnum", _i32 * NBODY), ("body_depth", _i32 * NBODY),
        ("body_pos", _f64 * 3 * NBODY), ("body_quat", _f64 * 4 * NBODY), ("body_ipos", _f64 * 3 * NBODY),
        ("body_inertia", _f64 * 6 * NBODY), ("body_mass", _f64 * NBODY), ("body_invweight0", _f64 * 2 * NBODY),
        ("jnt_type", _i32 * NJNT), ("jnt_body", _i32 * NJNT), ("jnt_qposadr", _i32 * NJNT), ("jnt_dofadr", _i32 * NJNT),
        ("jnt_limited", _i32 * NJNT), ("jnt_pos", _f64 * 3 * NJNT), ("jnt_axis", _f64 * 3 * NJNT),
        ("jnt_range", _f64 * 2 * NJNT),
        ("dof_body", _i32 * NV), ("dof_jnt", _i32 * NV), ("dof_parent", _i32 * NV), ("dof_Madr", _i32 * NV),
        ("dof_armature", _f64 * NV), ("dof_damping", _f64 * NV), ("dof_invweight0", _f64 * NV),
        ("geom_type", _i32 * NGEOM), ("geom_body", _i32 * NGEOM), ("geom_condim", _i32 * NGEOM),
        ("geom_pos", _f64 * 3 * NGEOM), ("geom_quat", _f64 * 4 * NGEOM), ("geom_size", _f64 * 3 * NGEOM),
        ("geom_friction", _f64 * 3 * NGEOM), ("geom_margin", _f64 * NGEOM), ("geom_rbound", _f64 * NGEOM),
        ("act_dof", _i32 * NU), ("act_gear", _f64 * NU), ("act_ctrlrange", _f64 * 2 * NU),
        ("pair_geom1", _i32 * MAXPAIR), ("pair_geom2", _i32 * MAXPAIR),
        ("ee_geom", _i32 * NEE), ("torso_body", _i32), ("rfoot_geom", _i32), ("lfoot_geom", _i32), ("floor_geom", _i32),
        # trailing G1 fields
        ("dof_frictionloss", _f64 * NV), ("geom_mesh", _i32 * NGEOM), ("mesh_vertadr", _i32 * NMESH),
        ("mesh_vertnum", _i32 * NMESH), ("mesh_center", _f64 * 3 * NMESH), ("mesh_vert", _f64 * 3 * NMESHVERT),
        ("nconmax", _i32), ("n_policy_action", _i32), ("action_scale", _f64), ("low_z", _f64),
        ("rew_qposadr", _i32 * NREWJ), ("rew_dofadr", _i32 * NREWJ), ("rew_jnt", _i32 * NREWJ), ("extra_geom", _i32 * 8),
    ]


def to_cstruct(g) -> DmModelG1:
    """GModel (mjcf.compile_mjcf_general of the G1 asset, with hulls) -> DmModelG1."""
    rc = RobotConfig("unitree_g1")
    assert (g.nq, g.nv, g.nu, g.nbody, g.ngeom, g.njnt, g.nM) == (NQ, NV, NU, NBODY, NGEOM, NJNT, NM)
    if g.solver != "PGS" or g.npair > MAXPAIR:
        raise ValueError("unsupported G1 model options")
    s = DmModelG1()
    s.nq, s.nv, s.nu, s.nbody, s.ngeom, s.njnt, s.npair, s.nM = NQ, NV, NU, NBODY, NGEOM, NJNT, g.npair, NM
    s.integrator = {"Euler": 0, "RK4": 1}[g.integrator]
    s.iterations, s.timestep, s.tolerance, s.meaninertia = g.iterations, g.timestep, g.tolerance, g.meaninertia

    def put(name, arr):
        dst = np.ctypeslib.as_array(getattr(s, name))
        dst[...] = np.ascontiguousarray(arr).reshape(dst.shape)

    for name in ["gravity", "solref", "solimp", "qpos0", "body_parent", "body_jntadr", "body_jntnum", "body_dofadr",
                 "body_dofnum", "body_depth", "body_pos", "body_quat", "body_ipos", "body_inertia", "body_mass",
                 "body_invweight0", "jnt_type", "jnt_body", "jnt_qposadr", "jnt_dofadr", "jnt_limited", "jnt_pos",
                 "jnt_axis", "jnt_range", "dof_body", "dof_jnt", "dof_parent", "dof_Madr", "dof_armature", "dof_damping",
                 "dof_invweight0", "geom_type", "geom_body", "geom_condim", "geom_pos", "geom_quat", "geom_size",
                 "geom_friction", "geom_margin", "geom_rbound", "act_dof", "act_gear", "act_ctrlrange", "dof_frictionloss"]:
        put(name, getattr(g, name))
    p1, p2 = np.full(MAXPAIR, -1, np.int32), np.full(MAXPAIR, -1, np.int32)
    p1[:g.npair], p2[:g.npair] = g.pairs[:, 0], g.pairs[:, 1]
    put("pair_geom1", p1)
    put("pair_geom2", p2)
    put("ee_geom", [g.geom_id(n) for n in rc.endeffector_geom_names])
    s.torso_body = g.body_id(rc.torso_body_name)
    s.rfoot_geom, s.lfoot_geom, s.floor_geom = (g.geom_id(rc.rfoot_geom_name), g.geom_id(rc.lfoot_geom_name),
                                                g.geom_id(rc.floor_geom_name))
    put("geom_mesh", g.geom_meshid)
    adr, num, verts = np.zeros(NMESH, np.int32), np.zeros(NMESH, np.int32), np.zeros((NMESHVERT, 3))
    cen = np.zeros((NMESH, 3))
    a = 0
    if len(g.mesh_vert) > NMESH:
        raise ValueError("too many meshes")
    for i, v in enumerate(g.mesh_vert):
        adr[i], num[i] = a, len(v)
        verts[a:a + len(v)] = v
        cen[i] = g.mesh_center[i]
        a += len(v)
    if a > NMESHVERT:
        raise ValueError("too many hull vertices")
    put("mesh_vertadr", adr)
    put("mesh_vertnum", num)
    put("mesh_vert", verts)
    put("mesh_center", cen)
    s.nconmax, s.n_policy_action, s.action_scale, s.low_z = g.nconmax, NU - 14, 20.0, rc.low_z
    put("rew_qposadr", REW_QPOS)
    put("rew_dofadr", REW_QVEL)
    put("rew_jnt", np.array(REW_QPOS) - 7 + 1)
    put("extra_geom", [g.geom_id(n) for n in rc.extra_contact_geom_names])
    return s


_MODEL = []


def load_g1_model():
    """(GModel, DmModelG1) of the packaged ``deepmimic_unitree_g1.xml`` + hull asset, cached."""
    if not _MODEL:
        hulls = mjcf.load_g1_hulls()
        if hulls is None:
            raise RuntimeError("assets/unitree_g1_hulls.npz is missing (scripts/make_g1_hulls.py writes it)")
        g = mjcf.compile_mjcf_general(os.path.join(_model.ASSET_DIR, "deepmimic_unitree_g1.xml"), hulls=hulls)
        _MODEL.append((g, to_cstruct(g)))
    return _MODEL[0]


class DmG1Config(C.Structure):
    _fields_ = [("num_envs", C.c_int32), ("max_ep_length", C.c_int32), ("vel_obs_scale", C.c_float), ("high_z", C.c_float),
                ("obs_bound", C.c_float), ("seed", C.c_uint64), ("auto_reset", C.c_int32), ("device", C.c_int32),
                ("task", C.c_int32), ("amnesty_steps", C.c_int32), ("to_getup_len", C.c_int32), ("pipeline", C.c_int32),
                ("integrator", C.c_int32)]


_BOUND = []


def _lib():
    L = load_library()
    if not _BOUND:
        vp, i32 = C.c_void_p, C.c_int
        L.dmg1_default_config.argtypes = [C.POINTER(DmG1Config)]
        L.dmg1_default_config.restype = None
        L.dmg1_model_sizeof.restype = C.c_size_t
        L.dmg1_create.argtypes = [vp, C.c_size_t, C.POINTER(DmG1Config), C.POINTER(vp)]
        L.dmg1_destroy.argtypes = [vp]
        L.dmg1_last_error.argtypes = [vp]
        L.dmg1_last_error.restype = C.c_char_p
        L.dmg1_load_clip.argtypes = [vp, i32, i32, vp, vp, vp, vp, i32]
        L.dmg1_obs_dim.argtypes = [vp]
        L.dmg1_get_motion.argtypes = [vp, vp, vp]
        L.dmg1_set_motion.argtypes = [vp, vp, vp]
        L.dmg1_reset.argtypes = [vp] * 5
        L.dmg1_step.argtypes = [vp] * 9
        L.dmg1_step_forced.argtypes = [vp] * 9
        L.dmg1_step_active.argtypes = [vp, vp, vp, i32] + [vp] * 6
        L.dmg1_set_active_schedule.argtypes = [vp, i32]
        L.dmg1_set_state.argtypes = [vp, vp, vp, vp, i32, vp]
        L.dmg1_get_state.argtypes = [vp] * 5
        L.dmg1_get_counters.argtypes = [vp] * 5
        L.dmg1_set_counters.argtypes = [vp] * 4
        L.dmg1_set_debug.argtypes = [vp, vp]
        L.dmg1_set_null_cache.argtypes = [vp, i32]
        L.dmg1_sep_cache_entries.argtypes = [vp, vp]
        L.dmg1_set_seed.argtypes = [vp, C.c_uint64]
        L.dmg1_set_env_clips.argtypes = [vp, vp, vp]
        L.dmg1_get_env_clips.argtypes = [vp, vp, vp]
        L.dmg1_last_kernel_ms.argtypes = [vp]
        L.dmg1_last_kernel_ms.restype = C.c_float
        if L.dmg1_model_sizeof() != C.sizeof(DmModelG1):
            raise RuntimeError("DmModelG1 layout mismatch: C %d, ctypes %d" % (L.dmg1_model_sizeof(), C.sizeof(DmModelG1)))
        _BOUND.append(True)
    return L


class G1HipEngine(EngineBase):
    """Batch of N Unitree G1 DeepMimic environments resident on one MI355X (tensors in, tensors out)."""

    PREFIX, DEBUG_STRIDE, NQ, NV, NBODY = "dmg1_", DEBUG_STRIDE, NQ, NV, NBODY

    def __init__(self, num_envs, device=0, seed=0, auto_reset=True, max_ep_length=1000, task=TASK_DPENV, pipeline=0, integrator=None,
                 cmodel=None):
        """``integrator``: None / "model" (the model's: RK4 in the XML), "RK4" or "Euler" (MuJoCo's semi-implicit Euler with implicit
        joint damping: one forward evaluation per step instead of four), as :class:`_lib.HipEngine`.  ``cmodel``: a
        :class:`DmModelG1` to create the engine from instead of the packaged model's (an edited copy of it)."""
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("G1HipEngine needs an MI355X (torch.cuda.is_available() is False); there is no CPU fallback")
        self.torch = torch
        self.L = _lib()
        self.gmodel, self.cmodel = load_g1_model()
        if cmodel is not None:
            self.cmodel = cmodel
        self.N = int(num_envs)
        self.device = torch.device("cuda", device)
        cfg = DmG1Config()
        self.L.dmg1_default_config(C.byref(cfg))
        cfg.num_envs, cfg.seed, cfg.auto_reset, cfg.device, cfg.max_ep_length = self.N, seed, int(auto_reset), device, max_ep_length
        cfg.task = int(task)
        cfg.pipeline = int(pipeline)        # 0 auto (split pipeline from 512 envs up), 1 monolithic, 2 split
        cfg.integrator = INTEGRATORS[integrator]
        self.auto_reset = bool(auto_reset)
        self.split = int(pipeline) == 2 or (int(pipeline) == 0 and self.N >= 512)      # the rule of dmg1_create (csrc/dm_g1.hip)
        self.task = int(task)
        self.obs_dim = NOBS_COMBINED if task else NOBS
        self.terms_dim = 8 if task else 5
        self.h = C.c_void_p()
        rc = self.L.dmg1_create(C.byref(self.cmodel), C.sizeof(DmModelG1), C.byref(cfg), C.byref(self.h))
        if rc != 0:
            raise RuntimeError("dmg1_create failed (%d): %s" % (rc, (self.L.dmg1_last_error(None) or b"").decode()))
        self.clip_len = 0
        self._debug = None

    def load_clip(self, mocap, floor=False, acyclic=False, run_rule=False, clip_id=0):
        q, v, bx, gx = [np.ascontiguousarray(a, np.float64) for a in mocap.tables()]
        if clip_id == 0:
            self.clip_len = len(q)
        flags = (CLIP_FLOOR if floor else 0) | (CLIP_ACYCLIC if acyclic else 0) | (CLIP_RUN_RULE if run_rule else 0)
        self._call("load_clip", int(clip_id), len(q), q.ctypes.data, v.ctypes.data, bx.ctypes.data, gx.ctypes.data, flags, stream=False)

    def _rows(self, qpos, qvel):
        return qpos.shape == (self.N, NQ) and qvel.shape == (self.N, NV) and qpos.is_contiguous() and qvel.is_contiguous()

    def step(self, actions, out):
        assert actions.shape == (self.N, NACT) and actions.dtype == self.torch.float32 and actions.is_contiguous()
        super().step(actions, out)

    def set_active_schedule(self, on=True):
        """``step_active`` launches its slots longest-first (default, from 512 envs up) or in the list's order; same results."""
        self._call("set_active_schedule", 1 if on else 0, stream=False)

    def step_active(self, actions, env_ids, nslots, out):
        assert actions.shape == (self.N, NACT) and actions.dtype == self.torch.float32 and actions.is_contiguous()
        assert env_ids.dtype == self.torch.int32 and env_ids.is_contiguous() and env_ids.numel() >= int(nslots)
        super().step_active(actions, env_ids, nslots, out)

    def step_forced(self, qpos, qvel, out):
        assert self._rows(qpos, qvel)
        super().step_forced(qpos, qvel, out)

    def set_state(self, qpos, qvel, warm=None, run_forward=True):
        assert self._rows(qpos, qvel)
        self._call("set_state", qpos, qvel, warm, int(run_forward))
        if self._recorder is not None:
            self._recorder.mark()

    def get_state(self):
        q, v, w = self._zeros(NQ), self._zeros(NV), self._zeros(NV)
        self._call("get_state", q, v, w)
        return q, v, w

    def _refresh_derived(self):
        q, v, w = self.get_state()
        self.set_state(q, v, warm=w, run_forward=True)
        self.set_state(q, v, warm=w, run_forward=False)     # the forward pass overwrote the warm start

    def get_motion(self):
        m = self._zeros(dtype=self.torch.int32)
        self._call("get_motion", m)
        return m

    def set_motion(self, motion):
        self._call("set_motion", motion)

    def set_env_clips(self, clip_ids):
        """DPEnv task: per-env clip id (int32 device tensor [N]) among the loaded clip slots."""
        assert clip_ids.dtype == self.torch.int32 and clip_ids.numel() == self.N and clip_ids.is_contiguous()
        self._call("set_env_clips", clip_ids)

    def last_kernel_ms(self):
        return float(self.L.dmg1_last_kernel_ms(self.h))

    def set_null_cache(self, on=True):
        """Test hook: the monolithic kernel runs MPR without its separating-direction cache from the next launch on."""
        self._call("set_null_cache", 1 if on else 0, stream=False)

    def sep_cache_entries(self):
        """Test hook: live entries of the (monolithic kernel's, pair kernel's) separating-direction cache."""
        buf = (C.c_int32 * 2)()
        self._call("sep_cache_entries", buf, stream=False)
        return int(buf[0]), int(buf[1])

    def queue_counters(self):
        """split pipeline: per round of the last step (support-query pair tickets, analytic pair tickets, tickets pulled)."""
        buf = (C.c_int32 * 24)()
        self.L.dmg1_queue_counters.argtypes = [C.c_void_p, C.c_void_p]
        self._call("queue_counters", buf, stream=False)
        return [tuple(buf[4 * r:4 * r + 3]) for r in range(6)]


# ------------------------------------------------------------------------------------------ Gym / VecEnv surfaces
def _g1_mocap(motion):
    from .config import MotionConfig
    from .mocap import MocapDM
    mcfg = MotionConfig(motion, robot="unitree_g1")
    mc = MocapDM(robot="unitree_g1")
    mc.load_mocap(mcfg.mocap_path)
    return mcfg, mc


def _load(engine, mcfg, mc, clip_id=0):
    engine.load_clip(mc, floor=mcfg.motion in mcfg.floor_motions, acyclic=mcfg.motion in mcfg.acyclical_motions,
                     run_rule=mcfg.motion == "run", clip_id=clip_id)                 # src/deepmimic_env.py:426


class HipG1VecEnv(HipBatchEnv):
    """N ``DPEnv(robot="unitree_g1")`` instances as one HIP batch with SubprocVecEnv semantics (auto-reset,
    ``terminal_observation``): the G1 counterpart of :class:`deepmimic_env.HipDeepMimicVecEnv`, which constructs this class
    when asked for ``robot="unitree_g1"``.  Actions are the policy's 23 values (src/deepmimic_env.py:303-307).
    ``motion`` may be a list (per-env clip id = env index mod len(list), as BASELINE config 5 mixes clips)."""

    def __init__(self, num_envs, motion=None, device=0, seed=1234, auto_reset=True, sub_batches=1, integrator=None, renderer="stick"):
        from .deepmimic_env import DPEnvConfig
        motions = [motion] if (motion is None or isinstance(motion, str)) else list(motion)
        assert 1 <= len(motions) <= 8, "an engine holds up to 8 clips (DMG1_MAX_CLIPS)"
        pairs = [_g1_mocap(m) for m in motions]
        self.motion_config, self.mocap = pairs[0]
        self.motions = [mcfg.motion for mcfg, _ in pairs]
        self.mocaps = [mc for _, mc in pairs]
        self.robot_config = RobotConfig("unitree_g1")

        def make(nk, k):
            e = G1HipEngine(nk, device=device, seed=seed + 104729 * k, auto_reset=auto_reset, max_ep_length=DPEnvConfig().MAX_EP_LENGTH,
                            integrator=integrator)
            for cid, (mcfg, mc) in enumerate(pairs):
                _load(e, mcfg, mc, clip_id=cid)
            if len(pairs) > 1:
                ids = (e.torch.arange(nk, device=e.device) + k * nk) % len(pairs)
                e.set_env_clips(ids.to(e.torch.int32).contiguous())
            return e
        super().__init__(num_envs, sub_batches, make, load_g1_model()[0], NOBS, 5, NACT, renderer=renderer)

    def _step_engines(self, actions):
        """sub_batches > 1: every engine's launches go to its own HIP stream, forked from and joined back into the current one.
        While one engine's g1_env_kernel drains its heaviest envs, the CUs it has left idle run the other engines' kernels (the
        envs of a batch are independent; results do not depend on the overlap).  The humanoid step has no such tail."""
        t = self._torch
        cur = t.cuda.current_stream(self.device)
        if getattr(self, "_streams", None) is None:
            from .streams import concurrent_streams
            self._streams = concurrent_streams(self.device, len(self.engines))      # on distinct hardware queues (probed)
        fork = cur.record_event()
        for e, o, sl, s in zip(self.engines, self.sub_out, self.sub_slices, self._streams):
            s.wait_event(fork)
            with t.cuda.stream(s):
                e.step(actions[sl], o)
            cur.wait_event(s.record_event())


class G1DPEnv(HipImitationEnv):
    """``DPEnv(motion, robot="unitree_g1")`` (src/deepmimic_env.py:272-510): one environment of the batch engine behind the
    reference's Gym surface; ``deepmimic_env.DPEnv`` constructs this class for the G1 robot."""

    version = "v1.0"
    REASONS = REASONS      # the G1 table has reason 8, the run clip's roll / pitch limit

    def __init__(self, motion=None, load_mocap=True, robot="unitree_g1", _profile=False, device=0, integrator=None, renderer="stick"):
        import random
        import torch
        from .deepmimic_env import DPEnvConfig
        self.renderer = _check_renderer(renderer)
        if robot != "unitree_g1":
            raise ValueError("G1DPEnv is the unitree_g1 environment")
        if not load_mocap:
            raise NotImplementedError("the mocap-less probing instance (src/deepmimic_env.py:287-293) is only used by MocapDM's "
                                      "own kinematics pass, which mjcf.forward_kinematics_general replaces")
        self._torch, self._random = torch, random
        self.ENV_CFG = DPEnvConfig()
        self.robot_config = RobotConfig("unitree_g1")
        self.motion_config, self.mocap = _g1_mocap(motion)
        self._eng = G1HipEngine(1, device=device, auto_reset=False, max_ep_length=self.ENV_CFG.MAX_EP_LENGTH, integrator=integrator)
        _load(self._eng, self.motion_config, self.mocap)
        self.model = self._eng.gmodel
        self._out = self._eng.alloc_outputs()
        self.mocap_dt, self.mocap_data_len = self.mocap.dt, len(self.mocap.data_config)
        self.idx_curr, self.episode_reward, self.episode_length = -1, 0, 0
        self.action_space = _action_space(self.model, NACT)
        self.observation_space = Box(-np.inf, np.inf, (NOBS,), np.float64)
        self.reference_state_init()

    def reference_state_init(self, idx_init=None):
        self.idx_init = self._random.randint(0, self.mocap_data_len - 1) if idx_init is None else idx_init
        self.idx_curr = self.idx_init

    def step(self, action, force_state=None):
        action = np.asarray(action, np.float64)
        if action.shape == (NU,):          # the full action vector MujocoEnv.__init__ probes with (:349): hands are dropped
            action = action[:NACT]
        assert action.shape == (NACT,)
        return self._imitation_step(action, force_state)


# ------------------------------------------------------------------------------------------ DPCombinedEnv on the G1
COMBINED_CLIPS = ("walk", "run", "getup_facedown_towalk")      # src/combined_env.py:168-170
MOTION_WALK, MOTION_RUN, MOTION_GETUP, MOTION_TO_GETUP = 0, 1, 2, 3


def _combined_engine(num_envs, device, seed, auto_reset, integrator=None):
    from .combined_env import DPCombinedEnvConfig
    cfg = DPCombinedEnvConfig()
    eng = G1HipEngine(num_envs, device=device, seed=seed, auto_reset=auto_reset, max_ep_length=cfg.MAX_EP_LENGTH, task=TASK_COMBINED,
                      integrator=integrator)
    mocaps = []
    for cid, m in enumerate(COMBINED_CLIPS):
        mcfg, mc = _g1_mocap(m)
        eng.load_clip(mc, clip_id=cid)
        mocaps.append(mc)
    return eng, mocaps


class HipG1CombinedVecEnv(HipG1VecEnv):
    """N ``DPCombinedEnv()`` instances — the reference's training environment (src/sb3_ppo.py:277-278): Unitree G1, walk / run /
    getup / to_getup motion state machine, obs 98, 23 actions — as one HIP batch with SubprocVecEnv semantics."""

    def __init__(self, num_envs, device=0, seed=1234, auto_reset=True, sub_batches=1, integrator=None, renderer="stick"):
        self.mocaps = None
        self.robot_config = RobotConfig("unitree_g1")

        def make(nk, k):
            e, mocaps = _combined_engine(nk, device, seed + 104729 * k, auto_reset, integrator)
            self.mocaps = self.mocaps or mocaps
            return e
        # action space = ctrlrange / ACT_SCALE (src/combined_env.py:196-200)
        HipBatchEnv.__init__(self, num_envs, sub_batches, make, load_g1_model()[0], NOBS_COMBINED, 8, NACT, act_scale=1.0 / 20.0,
                             infos=_LazyCombinedInfos, renderer=renderer)
        self.mocap = self.mocaps[0]


class G1CombinedEnv(HipSingleEnv):
    """``DPCombinedEnv()`` of the reference (src/combined_env.py:102-533) — hard-wired to the Unitree G1 there — as one
    environment of the batch engine; ``combined_env.DPCombinedEnv(robot="unitree_g1")`` constructs this class."""

    version = "v0.2.up"

    def __init__(self, verbose=0, _profile=False, device=0, integrator=None, renderer="stick"):
        import random
        import torch
        from .combined_env import DPCombinedEnvConfig, MTToGetup, PAWalk
        self.renderer = _check_renderer(renderer)
        self._torch, self._random, self.verbose = torch, random, verbose
        self.ENV_CFG = DPCombinedEnvConfig()
        self.robot = "unitree_g1"
        self.robot_config = RobotConfig(self.robot)
        self._eng, mocaps = _combined_engine(1, device, 0, False, integrator)
        self.walk_mocap, self.run_mocap, self.getup_mocap = mocaps
        self.action_mocap = None
        self.to_getup_mocap = MTToGetup(self.getup_mocap)
        self._motions = [self.walk_mocap, self.run_mocap, self.getup_mocap, self.to_getup_mocap]
        self.model = self._eng.gmodel
        self._out = self._eng.alloc_outputs()
        self.episode_reward, self.episode_length, self.debug_n_bad_angles = 0, 0, 0
        self.current_motion_n_steps, self.current_motion_mocap, self.current_player_action = None, None, PAWalk()
        # divided, where the batch class multiplies by 1 / 20: the two bounds differ in the last bit and both stay as they were
        lo, hi = self.model.act_ctrlrange[:NACT, 0].astype(np.float32) / 20.0, self.model.act_ctrlrange[:NACT, 1].astype(np.float32) / 20.0
        self.action_space = Box(lo, hi, dtype=np.float32)
        self.observation_space = Box(-np.inf, np.inf, (NOBS_COMBINED,), np.float64)

    def _motion_id(self):
        return self._motions.index(self.current_motion_mocap)

    def get_current_motion_state(self):
        idx = self.current_motion_n_steps % self.current_motion_mocap.get_length()
        return self.current_motion_mocap.get_qpos(idx) * 1.0, self.current_motion_mocap.get_qvel(idx) * 1.0

    def change_to_motion(self, motion):
        self.current_motion_mocap = motion
        self.current_motion_n_steps = 0

    def reset(self, rsi=True):
        from .combined_env import PAWalk
        if rsi:   # :219-227
            if self._random.randint(0, 1) == 0:
                self.current_motion_mocap = self.walk_mocap
                self.current_motion_n_steps = self.ENV_CFG.AMNESTY_STEPS + 10 + self._random.randint(0, self.walk_mocap.get_length() - 1)
            else:
                self.current_motion_mocap = self.getup_mocap
                self.current_motion_n_steps = self._random.randint(0, self.getup_mocap.get_length() - 1)
        else:
            self.current_motion_mocap, self.current_motion_n_steps = self.getup_mocap, 0
        self.current_player_action = PAWalk()
        self.episode_reward, self.episode_length = 0, 0
        self._eng.set_motion(self._i32(self._motion_id()))
        obs = self._torch.zeros(1, NOBS_COMBINED, device=self._eng.device)
        self._eng.reset(obs, idx_init=self._i32(self.current_motion_n_steps))
        return obs[0].double().cpu().numpy()

    def step(self, action, force_state=None):
        action = np.asarray(action, np.float64)
        if action.shape == (NU,):
            action = action[:NACT]
        assert action.shape == (NACT,)
        self._eng.set_motion(self._i32(self._motion_id()))
        self._eng.set_counters(self._i32(self.current_motion_n_steps), self._i32(self.episode_length))
        obs, reason, done = self._drive(action, force_state)
        if reason == 5:
            return obs, 0, True, {}
        terms = self._out["terms"][0].cpu().numpy()
        self.current_motion_mocap = self._motions[int(self._eng.get_motion()[0].item())]
        self.current_motion_n_steps = int(self._eng.get_counters()[0][0].item())
        self.debug_n_bad_angles = int(terms[7])
        self.episode_length += 1                     # counted on the host; the engine's reward sum is read on reason 6 only
        if reason == 6:
            self.episode_reward = float(self._eng.get_counters()[2][0].item())
            return obs, 0, True, {}
        reward = float(self._out["rew"][0].item())
        self.episode_reward += reward
        return obs, reward, done, _combined_info(terms, reason, REASONS)
