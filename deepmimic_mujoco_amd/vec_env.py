"""What the environment classes of both robots and both tasks share.

``HipBatchEnv`` is the SB3 VecEnv surface over one or more engines (deepmimic_env.HipDeepMimicVecEnv, combined_env.HipCombinedVecEnv,
g1.HipG1VecEnv, g1.HipG1CombinedVecEnv); ``HipSingleEnv`` is the gym.Env plumbing of the four one-env classes.  The concrete
classes only say which engines to build (``make_engine``), the shapes, and what their ``step`` keeps on the host.  Neither gym
nor stable-baselines3 is needed; if stable_baselines3 is importable the batch classes subclass its ``VecEnv`` so they can be
handed to ``PPO(MlpPolicy, envs, ...)`` unchanged.
"""
from __future__ import annotations

import numpy as np

from . import _lib

try:  # optional: real SB3 base class when present (it is not in this image)
    from stable_baselines3.common.vec_env.base_vec_env import VecEnv as _SB3VecEnv
except Exception:  # pragma: no cover
    _SB3VecEnv = object


class Box:
    """Minimal stand-in for gym.spaces.Box (gym is not installed here)."""

    def __init__(self, low, high, shape=None, dtype=np.float32):
        self.dtype = np.dtype(dtype)
        if shape is None:
            shape = np.shape(low)
        self.shape = tuple(shape)
        self.low = np.broadcast_to(np.asarray(low, self.dtype), self.shape).copy()
        self.high = np.broadcast_to(np.asarray(high, self.dtype), self.shape).copy()
        self._rng = np.random.default_rng()

    def sample(self):
        lo = np.where(np.isfinite(self.low), self.low, -1.0)
        hi = np.where(np.isfinite(self.high), self.high, 1.0)
        return self._rng.uniform(lo, hi).astype(self.dtype)

    def contains(self, x):
        x = np.asarray(x)
        return x.shape == self.shape and bool(np.all(x >= self.low) and np.all(x <= self.high))

    def seed(self, seed=None):
        self._rng = np.random.default_rng(seed)

    def __repr__(self):
        return "Box(%s, %s, %s, %s)" % (self.low.min(), self.high.max(), self.shape, self.dtype)


def _action_space(model, n_actions, scale=1.0):
    """Box over the first ``n_actions`` actuators' ctrlrange [EXT], times ``scale``."""
    lo, hi = (model.act_ctrlrange[:n_actions, j].astype(np.float32) * scale for j in (0, 1))
    return Box(lo, hi, dtype=np.float32)


_INFO_KEYS = ["reward_config", "reward_qvel", "reward_end_eff", "reward_com", "reward_joint_limit"]


def _make_info(terms, reason, reasons=_lib.REASONS):
    """info dict of deepmimic_env.py:251-255,424,438 (empty on the two early-out paths :378,:476); ``reasons`` names ``reason``."""
    if reason in (5, 6):
        return {}
    info = {k: float(v) for k, v in zip(_INFO_KEYS, terms)}
    r = reasons.get(int(reason))
    if r is not None:
        info["done_reason"] = r
    return info


def _combined_info(terms, reason, reasons=_lib.REASONS):
    """info dict of combined_env.py:357-358,436,445 (+ the calc_imitation_reward keys); {} on the early-outs."""
    if reason in (5, 6):
        return {}
    info = _make_info(terms[:5], 0)
    info["imitation_reward"] = float(terms[5])
    info["task_reward"] = float(terms[6])
    r = reasons.get(int(reason))
    if r is not None:
        info["done_reason"] = r
    return info


RENDERERS = ("stick", "raycast")
FRAME_W, FRAME_H = 320, 240          # what render() returns, either renderer


def _check_renderer(renderer):
    if renderer not in RENDERERS:
        raise ValueError("renderer must be one of %s, got %r" % (RENDERERS, renderer))
    return renderer


class _RayCastSurface:
    """``renderer="raycast"`` of the environment classes: frames cast on the device (raycast.RayRenderer) from the state that
    ``get_state`` returns.  No forward evaluation runs and no warm start is touched, so the next step does not depend on whether a
    frame was rendered.  The owner sets ``renderer`` and provides ``_render_engines()``."""

    renderer = "stick"
    _ray = None

    def _ray_renderer(self):
        if self._ray is None:
            from .raycast import RayRenderer
            self._ray = RayRenderer(self.model, device=self._render_engines()[0].device.index or 0)
        return self._ray

    def _render_qpos(self):
        q = [e.get_state()[0] for e in self._render_engines()]
        return q[0] if len(q) == 1 else self._torch.cat(q)

    def render_batch(self, env_ids=None, width=FRAME_W, height=FRAME_H, camera=None, rgb=True, depth=False, segmentation=False):
        """Frames of the listed envs (all without a list) as device tensors: ``rgb`` uint8 [n, H, W, 3], ``depth`` float32
        [n, H, W] (metres along the view axis, inf = sky), ``segmentation`` int32 [n, H, W] (model geom id, -1 = sky)."""
        if self.renderer != "raycast":
            raise RuntimeError('render_batch needs renderer="raycast"')
        return self._ray_renderer().render(self._render_qpos(), camera, width, height, env_ids=env_ids, rgb=rgb, depth=depth,
                                           segmentation=segmentation)

    def _raycast_frame(self, mode):
        """``render(mode)`` of env 0: "rgb_array" (or None) -> uint8 [240, 320, 3]; "depth_array" -> float32 [240, 320]."""
        if mode not in (None, "rgb_array", "depth_array"):
            raise ValueError("render mode %r" % (mode,))
        key = "depth" if mode == "depth_array" else "rgb"
        return self.render_batch([0], rgb=key == "rgb", depth=key == "depth")[key][0].cpu().numpy()


class LazyInfos(list):
    """`infos` of a VecEnv step: a real ``list`` (SB3's wrappers slice it, assign into it and test it with
    ``isinstance(infos, (list, tuple))``) whose dicts are built on first access — 4096 dicts per step would dominate the
    numpy surface.  Unmaterialised slots hold ``None`` internally; every public access path materialises them."""

    _make = staticmethod(_make_info)

    def __init__(self, terms, reason, done, terminal_obs):
        super().__init__([None] * len(done))
        self._terms, self._reason, self._done, self._tobs = terms, reason, done, terminal_obs

    def _get(self, i):
        v = list.__getitem__(self, i)
        if v is None:
            if i < 0:
                i += len(self)
            v = self._make(self._terms[i], self._reason[i])
            if self._done[i]:
                v["terminal_observation"] = self._tobs[i].copy()
            list.__setitem__(self, i, v)
        return v

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self._get(j) for j in range(*i.indices(len(self)))]
        return self._get(i)

    def __iter__(self):
        return (self._get(i) for i in range(len(self)))

    def _all(self):
        return [self._get(i) for i in range(len(self))]

    def copy(self):
        return self._all()

    def __eq__(self, other):
        return self._all() == list(other)

    __hash__ = None

    # every list operation that would read the raw (unmaterialised) slots goes through _all()
    def __add__(self, other):
        return self._all() + list(other)

    def __radd__(self, other):
        return list(other) + self._all()

    def __mul__(self, k):
        return self._all() * k

    __rmul__ = __mul__

    def __reversed__(self):
        return reversed(self._all())

    def __contains__(self, item):
        return item in self._all()

    def count(self, item):
        return self._all().count(item)

    def index(self, item, *a):
        return self._all().index(item, *a)

    def __repr__(self):
        return repr(self._all())

    def __reduce__(self):          # pickles / deep-copies as the plain list it stands for
        return (list, (self._all(),))


class _LazyCombinedInfos(LazyInfos):
    """`infos` of a DPCombinedEnv batch step: this env's info dict (imitation terms, imitation_reward, task_reward, done_reason)."""

    _make = staticmethod(_combined_info)


class HipBatchEnv(_RayCastSurface, _SB3VecEnv):
    """N environments as one HIP batch with SubprocVecEnv semantics (auto-reset, ``terminal_observation``).

    ``sub_batches`` > 1: independent engines over contiguous env ranges, so a rollout can keep one range simulating while the
    policy runs on another (deepmimic_mujoco_amd.ppo; INTEGRATION.md "double-buffered halves").  There is one set of [N, ...]
    output tensors; every engine writes its contiguous block of rows (``sub_out[k]`` are views of ``out`` at ``sub_slices[k]``).
    ``step_tensor`` / ``reset_tensor`` / ``step_sub`` are the zero-copy paths used by deepmimic_mujoco_amd.ppo."""

    def __init__(self, num_envs, sub_batches, make_engine, model, obs_dim, terms_dim, n_actions, act_scale=1.0, infos=LazyInfos,
                 renderer="stick"):
        """``make_engine(nk, k)`` builds the engine of sub-batch ``k`` (``nk`` envs, clips loaded); ``infos`` is the LazyInfos class."""
        import torch
        self._torch = torch
        self.renderer = _check_renderer(renderer)
        self.num_envs, self.sub_batches = int(num_envs), int(sub_batches)
        assert self.sub_batches >= 1 and self.num_envs % self.sub_batches == 0
        nk = self.num_envs // self.sub_batches
        self.model, self._infos = model, infos
        self.engines = [make_engine(nk, k) for k in range(self.sub_batches)]
        self.engine = self.engines[0]
        self.device = self.engine.device
        assert (self.engine.obs_dim, self.engine.terms_dim) == (obs_dim, terms_dim)     # the engines write rows of exactly this width
        z = lambda *shape, dt=torch.float32: torch.zeros(*shape, device=self.device, dtype=dt)
        N = self.num_envs
        self.out = dict(obs=z(N, obs_dim), rew=z(N), done=z(N, dt=torch.uint8), terms=z(N, terms_dim), reason=z(N, dt=torch.int32),
                        terminal_obs=z(N, obs_dim))
        self.sub_slices = [slice(k * nk, (k + 1) * nk) for k in range(self.sub_batches)]
        self.sub_out = [self.out] if self.sub_batches == 1 else [{k_: v[sl] for k_, v in self.out.items()} for sl in self.sub_slices]
        self.action_space = _action_space(model, n_actions, act_scale)
        self.observation_space = Box(-np.inf, np.inf, (obs_dim,), np.float32)
        self._actions = torch.zeros(self.num_envs, n_actions, device=self.device)
        self.render_mode = None
        self.reset_infos = [{} for _ in range(self.num_envs)]
        if _SB3VecEnv is not object:  # pragma: no cover
            _SB3VecEnv.__init__(self, self.num_envs, self.observation_space, self.action_space)

    @property
    def auto_reset(self):
        """What the engines were built with: ``True`` = SubprocVecEnv worker semantics (reset inside the step of a done env)."""
        return bool(self.engine.auto_reset)

    # ---- zero-copy tensor API
    def reset_tensor(self, idx_init=None):
        for e, o, sl in zip(self.engines, self.sub_out, self.sub_slices):
            e.reset(o["obs"], idx_init=None if idx_init is None else idx_init[sl].contiguous())
        return self.out["obs"]

    def step_tensor(self, actions):
        """actions: float32 device tensor [N, A] -> dict of device tensors (obs, rew, done, terms, reason, terminal_obs)."""
        actions = actions.contiguous()
        if self.sub_batches == 1:
            self.engine.step(actions, self.out)
        else:
            self._step_engines(actions)
        return self.out

    def _step_engines(self, actions):
        """sub_batches > 1: the engines step one after the other on the current stream."""
        for e, o, sl in zip(self.engines, self.sub_out, self.sub_slices):
            e.step(actions[sl], o)

    def step_sub(self, k, actions_k):
        """Step sub-batch k only (on the current stream): actions_k [N / sub_batches, A] -> its slice of the outputs."""
        self.engines[k].step(actions_k.contiguous(), self.sub_out[k])
        return self.sub_out[k]

    # ---- SB3 VecEnv protocol (numpy in / numpy out)
    def reset(self):
        return self.reset_tensor().cpu().numpy()

    def step_async(self, actions):
        t = self._torch
        self._actions.copy_(t.as_tensor(np.ascontiguousarray(actions, dtype=np.float32)).reshape(self._actions.shape))

    def step_wait(self):
        """numpy surface: the six outputs are packed into one [N, 2 obs + terms + 3] float32 device tensor (one small
        kernel) and cross PCIe as ONE download + synchronisation (2.3 MB at 4 096 envs); CPU reads of ROCm's pinned
        staging memory are uncached, so the download targets ordinary pageable memory."""
        t = self._torch
        out = self.step_tensor(self._actions)
        packed = t.cat([out["obs"], out["terminal_obs"], out["terms"], out["rew"][:, None], out["done"][:, None].float(),
                        out["reason"][:, None].float()], dim=1).cpu().numpy()
        d, k = out["obs"].shape[1], out["terms"].shape[1]
        obs, tobs, terms = (np.ascontiguousarray(packed[:, 0:d]), np.ascontiguousarray(packed[:, d:2 * d]),
                            np.ascontiguousarray(packed[:, 2 * d:2 * d + k]))
        rew = packed[:, 2 * d + k].copy()
        done = packed[:, 2 * d + k + 1] != 0
        reason = packed[:, 2 * d + k + 2].astype(np.int32)
        return obs, rew, done, self._infos(terms, reason, done, tobs)

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def enable_debug_log(self, steps=64, captures=16, reasons=("sim_error", "obs_out_of_bounds")):
        """The reference's ``episode_debug_log`` for the batch (debug_log.py): from now on every engine keeps the last ``steps``
        steps of each of its envs on the device and freezes up to ``captures`` copies (per engine, between two dumps) of the rings
        of envs whose step ends with one of ``reasons``.  Returns the object whose ``dump(directory)`` writes them as
        ``deepmimic_episode_<time>_env<i>.json`` and whose ``counts()`` is (captures, triggers).  Switch it on before a rollout
        graph is captured."""
        from .debug_log import BatchDebugLog
        self.debug_log = BatchDebugLog(self, steps, captures, reasons)
        return self.debug_log

    def close(self):
        if self._ray is not None:
            self._ray.close()
        for e in getattr(self, "engines", []):
            e.close()

    def seed(self, seed=None):
        """SB3 VecEnv.seed: env i gets seed + i.  Here: re-keys the engines' counter-based reset generator (env index and
        reset count are part of the key already) and returns the per-env seeds SB3 expects."""
        if seed is None:
            return [None] * self.num_envs
        for k, e in enumerate(self.engines):
            e.set_seed(int(seed) + 104729 * k)
        return [int(seed) + i for i in range(self.num_envs)]

    # ---- the rest of SB3's surface: the envs of the batch are identical, so the batch object answers for every env
    def _n_indices(self, indices):
        return self.num_envs if indices is None else len(np.atleast_1d(indices))

    def get_attr(self, attr_name, indices=None):
        return [getattr(self, attr_name)] * self._n_indices(indices)

    def set_attr(self, attr_name, value, indices=None):
        setattr(self, attr_name, value)

    def env_method(self, method_name, *method_args, indices=None, **method_kwargs):
        """A method of the batch object answers for every env (what SB3 itself uses it for: ``seed``, ``get_wrapper_attr``-style
        queries); unknown names raise AttributeError as a missing method of a sub-env would."""
        return [getattr(self, method_name)(*method_args, **method_kwargs)] * self._n_indices(indices)

    def env_is_wrapped(self, wrapper_class, indices=None):
        return [False] * self._n_indices(indices)

    def getattr_depth_check(self, name, already_found):
        return None

    @property
    def unwrapped(self):
        return self

    def _render_engines(self):
        return self.engines

    def get_images(self):
        """One frame per env in SB3; a 4 096-tile mosaic is of no use: the frame of env 0 stands for the batch."""
        return [self.render(mode="rgb_array")]

    def render(self, mode=None):
        """Software stick figure (render.py) of env 0 of the batch, 240 x 320 x 3 uint8 (what VecVideoRecorder-style callers
        get).  ``body_xpos`` puts the warm start back: rendering is not physics.  With ``renderer="raycast"``: the ray-cast frame of
        env 0 (``mode="depth_array"``: its depth image)."""
        if self.renderer == "raycast":
            return self._raycast_frame(mode)
        from .render import stick_figure
        return stick_figure(self.engine.body_xpos(), self.model.body_parent)


class HipSingleEnv(_RayCastSurface):
    """gym.Env plumbing of one environment of a batch engine (``self._eng``, one env, outputs in ``self._out``); a subclass that
    takes the ``renderer`` keyword sets ``self.renderer``."""

    def _render_engines(self):
        return [self._eng]

    def _i32(self, v):
        t = self._torch
        return t.tensor([int(v)], dtype=t.int32, device=self._eng.device)

    def _row(self, x):
        """[1, n] float32 device tensor of a host vector."""
        t = self._torch
        return t.tensor(np.asarray(x)[None], dtype=t.float32, device=self._eng.device)

    def _drive(self, action, force_state):
        """One ``step`` (or ``step_forced`` to ``force_state = (qpos, qvel)``) into ``self._out`` -> (obs float64, reason, done).
        The caller has pushed its counters already."""
        if force_state is not None:
            qpos, qvel = force_state
            self._eng.step_forced(self._row(qpos), self._row(qvel), self._out)
        else:
            self._eng.step(self._row(action), self._out)
        obs = self._out["obs"][0].double().cpu().numpy()
        reason = int(self._out["reason"][0].item())
        if self._debug_log is not None:
            self._debug_log.on_step(reason)
        return obs, reason, bool(self._out["done"][0].item())

    # ---- src/deepmimic_env.py:299,457-476: episode_debug_log, off unless enable_debug_log() was called
    _debug_log = None

    def enable_debug_log(self):
        """Keep the reference's ``episode_debug_log`` (debug_log.py): every step of the running episode on the device, cleared on
        ``reset``; a step that ends with a sim error or an out-of-bounds observation writes ``/tmp/deepmimic_episode_<time>.json``
        and prints the reference's message."""
        from .debug_log import SingleDebugLog
        self._debug_log = SingleDebugLog(self)
        return self._debug_log

    @property
    def episode_debug_log(self):
        """The reference-shaped dict of the running episode ({} before the first step, and without ``enable_debug_log``)."""
        return {} if self._debug_log is None else self._debug_log.log()

    def _state(self):
        q, v = self._eng.get_state()[:2]
        return q[0].double().cpu().numpy(), v[0].double().cpu().numpy()

    def set_state(self, qpos, qvel):                                          # MujocoEnv.set_state + sim.forward
        assert np.shape(qpos) == (self._eng.NQ,) and np.shape(qvel) == (self._eng.NV,)
        self._eng.set_state(self._row(qpos), self._row(qvel), run_forward=True)

    def render(self, mode=None):
        """Software stick figure (render.py) of the current body poses: there is no MuJoCo viewer behind this env.  With
        ``renderer="raycast"``: the ray-cast frame (``mode="depth_array"``: the depth image)."""
        if self.renderer == "raycast":
            return self._raycast_frame(mode)
        from .render import stick_figure
        return stick_figure(self._eng.body_xpos(), self.model.body_parent)

    def close(self):
        if self._ray is not None:
            self._ray.close()
        self._eng.close()


class HipImitationEnv(HipSingleEnv):
    """``DPEnv`` of either robot (src/deepmimic_env.py:273-510): what follows the action checks of ``step``, and ``reset``."""

    REASONS = _lib.REASONS

    def _imitation_step(self, action, force_state):
        self._eng.set_counters(self._i32(max(self.idx_curr, 0)), self._i32(self.episode_length))
        obs, reason, done = self._drive(action, force_state)
        if self.mocap.data_config is None:                                    # deepmimic_env.py:394-395
            return obs, 0, False, {}
        if reason in (5, 6):                                                  # :366-378 / :465-476
            if reason == 6:
                # the reference advances idx_curr / episode_reward / episode_length (:452-455) BEFORE the observation
                # guard (:465-476) zeroes the returned reward: take the pre-guard sum from the engine's counter
                self.idx_curr = (self.idx_curr + 1) % self.mocap_data_len
                self.episode_reward = float(self._eng.get_counters()[2][0].item())
                self.episode_length += 1
            return obs, 0, True, {}
        reward = float(self._out["rew"][0].item())
        info = _make_info(self._out["terms"][0].cpu().numpy(), reason, self.REASONS)
        self.idx_curr = (self.idx_curr + 1) % self.mocap_data_len              # :452-455
        self.episode_reward += reward
        self.episode_length += 1
        return obs, reward, done, info

    def reset(self):                                                          # :496-500
        self.episode_reward = 0
        self.episode_length = 0
        return self.reset_model()

    def reset_model(self, idx_init=None):                                     # :502-510
        self.reference_state_init(idx_init=idx_init)
        obs = self._torch.zeros(1, self.observation_space.shape[0], device=self._eng.device)
        self._eng.reset(obs, idx_init=self._i32(self.idx_init))
        self._eng.set_counters(None, self._i32(self.episode_length))
        return obs[0].double().cpu().numpy()
