"""DPEnv / HipDeepMimicVecEnv — host-side mirror of the reference's environment surfaces.

Surface 1 (gym.Env, per env):   ``DPEnv``            <- src/deepmimic_env.py:273-538
Surface 2 (SB3 VecEnv, batched): ``HipDeepMimicVecEnv`` <- what SubprocVecEnv([DPEnv]*N) gives
                                                          src/sb3_ppo.py:273-278, src/ppo.py:32

Both are thin: every number they return is produced by the HIP engine through the C-ABI
(deepmimic_mujoco_amd/_lib.py).  Neither gym nor stable-baselines3 is needed; if
stable_baselines3 is importable the VecEnv subclasses its ``VecEnv`` so it can be handed to
``PPO(MlpPolicy, envs, ...)`` unchanged.
"""
from __future__ import annotations

import random

import numpy as np

from . import _lib
from .config import MotionConfig, RobotConfig
from .mocap import MocapDM
from .model import NOBS, NU, NV, load_model
from .vec_env import Box, HipBatchEnv, HipImitationEnv, LazyInfos, _INFO_KEYS, _action_space, _check_renderer, _make_info  # noqa: F401 (re-exported)


class DPEnvConfig:
    """src/deepmimic_env.py:258-270 (the HIP kernels implement exactly this flag set)."""

    def __init__(self):
        self.MAX_EP_LENGTH = 1000
        self.VEL_OBS_SCALE = 0.1
        self.FRC_OBS_SCALE = 0.001
        self.ADD_FOOT_CONTACT_OBS = True
        self.ADD_EXTRA_CONTACT_OBS = False
        self.ADD_TORSO_OBS = True
        self.ADD_JOINT_FORCE_OBS = False
        self.ADD_ABSPOS_OBS = False
        self.ADD_PHASE_OBS = True
        self.ADD_PLAYER_ACTION_OBS = False
        self.MAX_PLAYER_ACTIONS = 3


class _SimView:
    """`env.sim.data.qpos / qvel` as read by the reference's tools (deepmimic_env.py:591-597)."""

    def __init__(self, env):
        self._env = env
        self.data = self

    @property
    def qpos(self):
        return self._env._state()[0]

    @property
    def qvel(self):
        return self._env._state()[1]

    @property
    def time(self):
        return self._env._time

    def forward(self):
        self._env._eng.forward()


class DPEnv(HipImitationEnv):
    """Single-clip imitation env with the reference's public surface (deepmimic_env.py:273)."""

    version = "v1.0"
    ENV_CFG = DPEnvConfig()
    metadata = {"render.modes": []}

    def __new__(cls, motion=None, load_mocap=True, robot="humanoid3d", _profile=False, device=0, renderer="stick"):
        if robot == "unitree_g1" and cls is DPEnv:   # the second robot has its own engine (g1.py, csrc/dm_g1.hip)
            from .g1 import G1DPEnv
            return G1DPEnv(motion=motion, load_mocap=load_mocap, robot=robot, _profile=_profile, device=device, renderer=renderer)
        return super().__new__(cls)

    def __init__(self, motion=None, load_mocap=True, robot="humanoid3d", _profile=False, device=0, renderer="stick"):
        import torch
        self.renderer = _check_renderer(renderer)
        self.PROFILE = _profile
        self.motion_config = MotionConfig(motion=motion, robot=robot)
        self.robot_config = RobotConfig(robot=robot)
        self.model = load_model(self.robot_config.xml_path)
        self.mocap = MocapDM(robot=robot, model=self.model)
        self._torch = torch
        self._eng = _lib.HipEngine(self.model, 1, device=device, auto_reset=False,
                                   max_ep_length=self.ENV_CFG.MAX_EP_LENGTH,
                                   vel_obs_scale=self.ENV_CFG.VEL_OBS_SCALE, low_z=self.robot_config.low_z)
        self._out = self._eng.alloc_outputs()
        self._time = 0.0
        if load_mocap:
            self.load_mocap(self.motion_config.mocap_path)
            self.reference_state_init()
            assert len(self.mocap.data_config) != 0
        else:  # deepmimic_env.py:287-293
            self.mocap.data_config = None
            self.mocap.data_vel = None
            self.mocap_data_len = 1
            self._load_rest_clip()
        self.idx_curr = -1
        self.episode_reward = 0
        self.episode_length = 0
        self.sim = _SimView(self)
        self.action_space = _action_space(self.model, NU)                     # from ctrlrange [EXT]
        self.observation_space = Box(-np.inf, np.inf, (NOBS,), np.float64)
        self.init_qpos = self.model.qpos0.copy()
        self.init_qvel = np.zeros(NV)

    # ---- reference helpers -------------------------------------------------------------
    def _load_rest_clip(self):
        class _Rest:
            def __init__(s, m):
                from .model import forward_kinematics
                kin = forward_kinematics(m, m.qpos0)
                s.t = (m.qpos0[None], np.zeros((1, NV)), kin["xpos"][None], kin["geom_xpos"][None])

            def tables(s):
                return s.t
        self._eng.load_clip(0, _Rest(self.model))

    def load_mocap(self, filepath):
        self.mocap.load_mocap(filepath)
        self.mocap_dt = self.mocap.dt
        self.mocap_data_len = len(self.mocap.data_config)
        mcfg = self.motion_config
        self._eng.load_clip(0, self.mocap, floor=mcfg.motion in mcfg.floor_motions,
                            acyclic=mcfg.motion in mcfg.acyclical_motions)

    def reference_state_init(self, idx_init=None):     # deepmimic_env.py:312-316
        self.idx_init = random.randint(0, self.mocap_data_len - 1)
        if idx_init is not None:
            self.idx_init = idx_init
        self.idx_curr = self.idx_init

    def _get_obs(self):
        raise NotImplementedError("observations are produced by dm_step/dm_reset; call step() or reset()")

    # ---- gym.Env surface ------------------------------------------------------------------
    def step(self, action, force_state=None):
        action = np.asarray(action, np.float64) * 1.0
        assert action.shape == (NU,)                                          # deepmimic_env.py:352
        if force_state is None:
            self._time += self.model.timestep
        return self._imitation_step(action, force_state)

    def get_time(self):                                                       # :493
        return self._time

    def seed(self, seed=None):
        random.seed(seed)
        if seed is not None:
            self._eng.set_seed(seed)
        return [seed]


class HipDeepMimicVecEnv(HipBatchEnv):
    """N DPEnv instances as one HIP batch with SubprocVecEnv semantics (auto-reset, terminal_observation).

    ``motion`` may be one clip name or a list (per-env clip id = env index mod len(list): BASELINE
    config 5).  ``step_tensor`` is the zero-copy path used by deepmimic_mujoco_amd.ppo.  ``integrator`` (None / "model", "RK4",
    "Euler") goes to whichever engine the robot has.
    """

    version, ENV_CFG = DPEnv.version, DPEnv.ENV_CFG

    def __new__(cls, num_envs, motion=None, robot="humanoid3d", device=0, seed=1234, auto_reset=True, sub_batches=1, integrator=None,
                renderer="stick"):
        if robot == "unitree_g1" and cls is HipDeepMimicVecEnv:
            from .g1 import HipG1VecEnv
            return HipG1VecEnv(num_envs, motion=motion, device=device, seed=seed, auto_reset=auto_reset, sub_batches=sub_batches,
                               integrator=integrator, renderer=renderer)
        return super().__new__(cls)

    def __init__(self, num_envs, motion=None, robot="humanoid3d", device=0, seed=1234, auto_reset=True, sub_batches=1, integrator=None,
                 renderer="stick"):
        import torch
        self.robot_config = RobotConfig(robot)
        model = load_model(self.robot_config.xml_path)
        motions = [motion] if (motion is None or isinstance(motion, str)) else list(motion)
        self.motions = [MotionConfig(m, robot).motion for m in motions]
        self.mocaps = []
        for m in self.motions:
            mc = MocapDM(robot=robot, model=model)
            mc.load_mocap(MotionConfig(m, robot).mocap_path)
            self.mocaps.append(mc)

        def make(nk, k):
            e = _lib.HipEngine(model, nk, device=device, seed=seed + 104729 * k, auto_reset=auto_reset, low_z=self.robot_config.low_z,
                               integrator=integrator)
            for cid, (m, mc) in enumerate(zip(self.motions, self.mocaps)):
                mcfg = MotionConfig(m, robot)
                e.load_clip(cid, mc, floor=m in mcfg.floor_motions, acyclic=m in mcfg.acyclical_motions)
            if len(self.motions) > 1:
                ids = (torch.arange(nk, device=e.device) + k * nk) % len(self.motions)
                e.set_env_clips(ids.to(torch.int32))
            return e
        super().__init__(num_envs, sub_batches, make, model, NOBS, 5, NU, renderer=renderer)
