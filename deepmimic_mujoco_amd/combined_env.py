"""Host-side mirror of the reference's `DPCombinedEnv` (src/combined_env.py:101-533) over the HIP engine.

The reference class is hard-wired to `unitree_g1` (:165); its walk / run / getup / to_getup motion state machine,
task reward, amnesty logic and player-action observation are model-independent, and this module runs them on the
`humanoid3d` model with the humanoid3d RobotConfig: no action scale (ACT_SCALE applies to G1 only,
:251), no extra-contact geoms (RobotConfig.extra_contact_geom_names is None), low_z 0.7, getup clip
`getup_facedown`.  All per-step arithmetic (physics, obs, both rewards, transitions, termination, RSI reset) runs in
`dm_step_combined_kernel` (DM_TASK_COMBINED); the classes below only keep the reference's public surface.
"""
from __future__ import annotations

import random

import numpy as np

from . import _lib
from .config import MotionConfig, RobotConfig
from .deepmimic_env import _SimView
from .mocap import MocapDM
from .model import load_model, NU
from .vec_env import Box, HipBatchEnv, HipSingleEnv, _LazyCombinedInfos, _action_space, _check_renderer, _combined_info  # noqa: F401 (re-exported)

NOBS_COMBINED = 72
MOTION_WALK, MOTION_RUN, MOTION_GETUP, MOTION_TO_GETUP = 0, 1, 2, 3
MOTION_NAMES = {0: "walk", 1: "run", 2: "getup", 3: "to_getup"}


class DPCombinedEnvConfig:
    """src/combined_env.py:20-34."""

    def __init__(self):
        self.MAX_EP_LENGTH = 2000
        self.VEL_OBS_SCALE = 0.1
        self.FRC_OBS_SCALE = 0.001
        self.ADD_FOOT_CONTACT_OBS = False
        self.ADD_EXTRA_CONTACT_OBS = True      # humanoid3d has no extra-contact geoms: contributes 0 entries
        self.ACT_SCALE = 20.                   # unitree_g1 only (:251)
        self.ADD_TORSO_OBS = True
        self.ADD_JOINT_FORCE_OBS = False
        self.ADD_ABSPOS_OBS = False
        self.ADD_PHASE_OBS = True
        self.ADD_PLAYER_ACTION_OBS = True
        self.MAX_PLAYER_ACTIONS = 3
        self.AMNESTY_STEPS = 150


class PlayerAction:
    """src/combined_env.py:37-56."""
    IDXS = {"walk": 0, "run": 1, "action": 2}

    def __init__(self, name, vx, vy):
        self.name, self.vx, self.vy = name, vx, vy
        assert name in PlayerAction.IDXS

    def onehot(self, n_max_actions):
        vec = np.zeros(n_max_actions)
        vec[PlayerAction.IDXS[self.name]] = 1.0
        return vec

    def heading_in_world(self):
        target_vel = np.linalg.norm([self.vx, self.vy])
        return np.array([self.vx, self.vy, 0]) / target_vel if target_vel != 0 else np.array([0, 0, 0])


class PAWalk(PlayerAction):
    def __init__(self):
        super().__init__("walk", 1.0, 0.0)


class PARun(PlayerAction):
    def __init__(self):
        super().__init__("run", 3.0, 0.0)


class MotionTransition:
    """Pseudo clip whose target is frame 1 of `target_mocap` for `length` steps (src/combined_env.py:67-99)."""
    motion_name = None
    length = None

    def __init__(self, target_mocap):
        self.target_mocap = target_mocap

    def get_qpos(self, index):
        return self.target_mocap.get_qpos(1)

    def get_qvel(self, index):
        return self.target_mocap.get_qvel(1)

    def get_body_xpos(self, index):
        return self.target_mocap.get_body_xpos(1)

    def get_geom_xpos(self, index):
        return self.target_mocap.get_geom_xpos(1)

    def get_length(self):
        return self.length


class MTToWalk(MotionTransition):
    motion_name, length = "to_walk", 120


class MTToRun(MotionTransition):
    motion_name, length = "to_run", 120


class MTToGetup(MotionTransition):
    motion_name, length = "to_getup", 180


class _Clip:
    """MocapDM plus the two attributes combined_env.py reads (`motion_name`, `get_length`)."""

    def __init__(self, model, robot, motion):
        self.mocap = MocapDM(robot=robot, model=model)
        self.mocap.load_mocap(MotionConfig(motion, robot).mocap_path)
        self.motion_name = motion

    def __getattr__(self, name):
        return getattr(self.mocap, name)

    def get_length(self):
        return len(self.mocap.data_config)


def _load_clips(engine, model, robot, getup_motion):
    clips = [_Clip(model, robot, "walk"), _Clip(model, robot, "run"), _Clip(model, robot, getup_motion)]
    for cid, c in enumerate(clips):
        mcfg = MotionConfig(c.motion_name, robot)
        engine.load_clip(cid, c.mocap, floor=c.motion_name in mcfg.floor_motions,
                         acyclic=c.motion_name in mcfg.acyclical_motions)
    return clips


class DPCombinedEnv(HipSingleEnv):
    """Single-env surface of src/combined_env.py:101 (ctor args, step/reset/get_current_motion_state/change_to_motion)."""

    version = "v0.2.up"
    ENV_CFG = DPCombinedEnvConfig()
    metadata = {"render.modes": []}

    def __new__(cls, verbose=0, _profile=False, robot="unitree_g1", getup_motion="getup_facedown", device=0, renderer="stick"):
        if robot == "unitree_g1" and cls is DPCombinedEnv:   # the reference's own configuration (:165): the G1 engine
            from .g1 import G1CombinedEnv
            return G1CombinedEnv(verbose=verbose, _profile=_profile, device=device, renderer=renderer)
        return super().__new__(cls)

    def __init__(self, verbose=0, _profile=False, robot="unitree_g1", getup_motion="getup_facedown", device=0, renderer="stick"):
        import torch
        self._torch = torch
        self.renderer = _check_renderer(renderer)
        self.PROFILE = _profile
        self.verbose = verbose
        self.robot = robot
        self.robot_config = RobotConfig(robot=robot)
        self.model = load_model(self.robot_config.xml_path)
        cfg = self.ENV_CFG
        self._eng = _lib.HipEngine(self.model, 1, device=device, auto_reset=False, task=_lib.TASK_COMBINED,
                                   max_ep_length=cfg.MAX_EP_LENGTH, vel_obs_scale=cfg.VEL_OBS_SCALE,
                                   low_z=self.robot_config.low_z, amnesty_steps=cfg.AMNESTY_STEPS,
                                   to_getup_len=MTToGetup.length)
        self.walk_mocap, self.run_mocap, self.getup_mocap = _load_clips(self._eng, self.model, robot, getup_motion)
        self.action_mocap = None
        self.to_getup_mocap = MTToGetup(self.getup_mocap)
        self._motions = [self.walk_mocap, self.run_mocap, self.getup_mocap, self.to_getup_mocap]
        self._out = self._eng.alloc_outputs()
        self.episode_reward = 0
        self.episode_length = 0
        self.debug_n_bad_angles = 0
        self.current_motion_n_steps = None
        self.current_motion_mocap = None
        self.current_player_action = None
        self._time = 0.0
        self.sim = _SimView(self)
        self.action_space = _action_space(self.model, NU)
        self.observation_space = Box(-np.inf, np.inf, (NOBS_COMBINED,), np.float64)

    # ---- helpers
    def _push(self):
        self._eng.set_env_clips(self._i32(self._motions.index(self.current_motion_mocap)))
        self._eng.set_counters(self._i32(self.current_motion_n_steps), self._i32(self.episode_length))

    def _pull(self):
        self.current_motion_mocap = self._motions[int(self._eng.get_env_clips()[0].item())]
        idx, ln, rew = self._eng.get_counters()
        self.current_motion_n_steps = int(idx[0].item())
        self.episode_length = int(ln[0].item())          # advanced in the kernel (:454-460)
        self.episode_reward = float(rew[0].item())

    def get_current_motion_state(self):                                        # :199-203
        idx = self.current_motion_n_steps % self.current_motion_mocap.get_length()
        return self.current_motion_mocap.get_qpos(idx) * 1.0, self.current_motion_mocap.get_qvel(idx) * 1.0

    def change_to_motion(self, motion):                                        # :529-533
        if self.verbose:
            print("Changing to motion: {}".format(motion.motion_name))
        self.current_motion_mocap = motion
        self.current_motion_n_steps = 0

    # ---- gym.Env surface
    def reset(self, rsi=True):                                                 # :205-241
        if rsi:
            if random.randint(0, 1) == 0:
                self.current_motion_mocap = self.walk_mocap
                self.current_motion_n_steps = self.ENV_CFG.AMNESTY_STEPS + 10 + \
                    random.randint(0, self.current_motion_mocap.get_length() - 1)
            else:
                self.current_motion_mocap = self.getup_mocap
                self.current_motion_n_steps = random.randint(0, self.current_motion_mocap.get_length() - 1)
        else:
            self.current_motion_mocap = self.getup_mocap
            self.current_motion_n_steps = 0
        self.current_player_action = PAWalk()
        self.episode_reward = 0
        self.episode_length = 0
        t = self._torch
        self._eng.set_env_clips(self._i32(self._motions.index(self.current_motion_mocap)))
        obs = t.zeros(1, NOBS_COMBINED, device=self._eng.device)
        self._eng.reset(obs, idx_init=self._i32(self.current_motion_n_steps))
        return obs[0].double().cpu().numpy()

    def step(self, action, force_state=None):                                  # :243-493
        action = np.asarray(action, np.float64) * 1.0
        assert action.shape == (NU,)
        self._push()
        if force_state is None:
            self._time += self.model.timestep
        obs, reason, done = self._drive(action, force_state)
        if reason == 5:                                                        # :271-284 (no counter moves)
            return obs, 0, True, {}
        self._pull()                                                           # episode_length / episode_reward come from the engine
        if reason == 6:                                                        # :472-484 (counters already advanced)
            return obs, 0, True, {}
        terms = self._out["terms"][0].cpu().numpy()
        self.debug_n_bad_angles = int(terms[7])
        return obs, float(self._out["rew"][0].item()), done, _combined_info(terms, reason)

    def seed(self, seed=None):
        random.seed(seed)
        return [seed]


class HipCombinedVecEnv(HipBatchEnv):
    """N DPCombinedEnv instances as one HIP batch with SubprocVecEnv semantics (auto-reset = reset(rsi=True))."""

    version, ENV_CFG = DPCombinedEnv.version, DPCombinedEnv.ENV_CFG

    def __new__(cls, num_envs, robot="unitree_g1", getup_motion="getup_facedown", device=0, seed=1234, auto_reset=True, **kw):
        if robot == "unitree_g1" and cls is HipCombinedVecEnv:
            from .g1 import HipG1CombinedVecEnv
            return HipG1CombinedVecEnv(num_envs, device=device, seed=seed, auto_reset=auto_reset, sub_batches=kw.get("sub_batches", 1),
                                       integrator=kw.get("integrator"), renderer=kw.get("renderer", "stick"))
        return super().__new__(cls)

    def __init__(self, num_envs, robot="unitree_g1", getup_motion="getup_facedown", device=0, seed=1234,
                 auto_reset=True, integrator=None, renderer="stick"):
        self.robot_config = RobotConfig(robot)
        model, cfg = load_model(self.robot_config.xml_path), self.ENV_CFG

        def make(nk, k):
            e = _lib.HipEngine(model, nk, device=device, seed=seed, auto_reset=auto_reset,
                               task=_lib.TASK_COMBINED, max_ep_length=cfg.MAX_EP_LENGTH,
                               vel_obs_scale=cfg.VEL_OBS_SCALE, low_z=self.robot_config.low_z,
                               amnesty_steps=cfg.AMNESTY_STEPS, to_getup_len=MTToGetup.length, integrator=integrator)
            self.clips = _load_clips(e, model, robot, getup_motion)
            return e
        super().__init__(num_envs, 1, make, model, NOBS_COMBINED, 8, NU, infos=_LazyCombinedInfos,
                         renderer=renderer)   # one engine: no sub_batches here

    def motion_state(self):
        """(motion id int32[N], n_steps int32[N]) — `current_motion_mocap` / `current_motion_n_steps` per env."""
        return self.engine.get_env_clips(), self.engine.get_counters()[0]
