"""SB3's ``VecNormalize`` [EXT] for the batch envs, with the running statistics on the device.

``HipVecNormalize(venv)`` wraps any ``HipBatchEnv`` (both robots, both tasks).  The running mean / variance of the observation
columns and of the discounted returns are fp64 device tensors; a training step is ``dm_vecnorm_step`` (csrc/dm_vecnorm.hip, three
launches on the current stream, capturable, no host round trip), ``training=False`` stepping and ``normalize_obs`` /
``normalize_reward`` of device tensors are ``dm_vecnorm_apply`` (one launch, statistics untouched).  The wrapper writes into
tensors of its own: the inner env's ``out`` stays raw.  With ``sub_batches > 1`` the inner env is stepped as one batch — there is
no ``step_sub`` here, so ``rollout.route`` takes the serial driver and the statistics see all N envs at once, as in SB3.

On a CPU device the same arithmetic runs as torch fp64 ops (the wrapper's logic is testable without a GPU over any object that
offers ``reset_tensor`` / ``step_tensor`` / ``num_envs`` / ``device`` / the two spaces).  The semantics are restated in numpy in
tests/vecnorm_ref.py.  The flags ``training`` / ``norm_obs`` / ``norm_reward`` and the settings ``clip_obs`` / ``clip_reward`` /
``gamma`` / ``epsilon`` may be set between steps; a rollout graph captured earlier keeps the values it was captured with.

``sync_group=`` (a ``torch.distributed`` group, or ``"world"`` for the default group, looked up at the first use) keeps ONE set of
running statistics over the ranks of a data-parallel run: beside the running set a rank holds ``base``, what all
ranks agreed on at the last ``sync()``, and ``acc``, what it alone has seen since; every step folds its batch into ``acc`` and
normalises with merge(base, acc) (``dm_vecnorm_step_sync``, the same three launches), and ``sync()`` — two launches around one
all-reduce of a [world, 2 D + 4] fp64 buffer, once per rollout in ``PPO`` — merges every rank's ``acc`` into ``base`` in rank order,
after which the statistics are bit-identical on all ranks.  ``returns`` stays per rank.  Restated in tests/vecnorm_sync_ref.py.

``SAC(env, normalizer=HipVecNormalize(env))`` is the off-policy use (sac.py): the learner steps the inner env itself, feeds
``normalize_step_`` for the statistics and the actor's observation, stores raw transitions and normalises each sampled minibatch.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

COUNT0 = 1e-4           # RunningMeanStd's epsilon: the weight of the prior (mean 0, var 1)


class _RmsView:
    """``obs_rms`` / ``ret_rms``: read-only ``mean``, ``var``, ``count`` as numpy fp64 copies of the device state."""

    def __init__(self, mean, var, count):
        self._m, self._v, self._c = mean, var, count

    @property
    def mean(self):
        return self._m.detach().cpu().numpy().copy()

    @property
    def var(self):
        return self._v.detach().cpu().numpy().copy()

    @property
    def count(self):
        return float(self._c.detach().cpu().reshape(-1)[0])


class HipVecNormalize:
    """See the module docstring.  ``out`` after a step: ``obs`` / ``rew`` / ``terminal_obs`` normalised (terminal observations of
    done envs only, the other rows as the inner env left them), ``obs_raw`` / ``rew_raw`` the inner env's tensors, everything else
    (``done``, ``terms``, ``reason``) the inner env's."""

    _HIDDEN = ("step_sub", "sub_out")      # never forwarded: the wrapper steps all N envs at once

    def __init__(self, venv, training=True, norm_obs=True, norm_reward=True, clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8,
                 sync_group=None):
        import torch
        if isinstance(sync_group, str) and sync_group != "world":
            raise ValueError("HipVecNormalize: sync_group is None, a torch.distributed group or \"world\", not %r" % (sync_group,))
        self._torch = t = torch
        self.venv = venv
        self.num_envs = N = int(venv.num_envs)
        self.device = t.device(venv.device)
        self.observation_space, self.action_space = venv.observation_space, venv.action_space
        self.obs_dim = D = int(venv.observation_space.shape[0])
        self.clip_obs, self.clip_reward, self.gamma, self.epsilon = float(clip_obs), float(clip_reward), float(gamma), float(epsilon)
        if not (0.0 <= self.gamma <= 1.0 and self.epsilon >= 0.0 and self.clip_obs > 0.0 and self.clip_reward > 0.0):
            raise ValueError("HipVecNormalize: gamma in [0, 1], epsilon >= 0 and positive clips, not %r" % ((gamma, epsilon, clip_obs, clip_reward),))
        self.on_gpu = self.device.type == "cuda"
        # one fp64 arena: obs mean [D] | obs var [D] | obs count | ret mean, var, count
        self._state = t.zeros(2 * D + 4, dtype=t.float64, device=self.device)
        self._obs_mean, self._obs_var = self._state[:D], self._state[D:2 * D]
        self._obs_count, self._ret = self._state[2 * D:2 * D + 1], self._state[2 * D + 1:2 * D + 4]
        self.returns = t.zeros(N, dtype=t.float64, device=self.device)
        # several ranks, one set of statistics: base | acc laid out like _state; the descriptor and the all-reduce buffer wait for the group
        self._sync_group, self._sync, self._pg, self._gather, self.sync_calls = sync_group, None, None, None, 0
        self._base = self._acc = None
        if sync_group is not None:
            self._base, self._acc = t.zeros_like(self._state), t.zeros_like(self._state)
        self._init_state()
        z = lambda *shape: t.zeros(*shape, device=self.device)
        self._own = dict(obs=z(N, D), rew=z(N), terminal_obs=z(N, D))
        self.out = dict(self._own)
        self._actions = t.zeros(N, int(venv.action_space.shape[0]), device=self.device)
        self._desc = None
        if self.on_gpu:
            L = _lib.load_library()
            nbytes = int(L.dm_vecnorm_scratch_bytes(N, D))
            self._scratch = t.zeros(nbytes // 8, dtype=t.float64, device=self.device)
            self._desc = _lib.DmVecNorm(N=N, D=D, device=self.device.index or 0, gamma=self.gamma, epsilon=self.epsilon,
                                        clip_obs=self.clip_obs, clip_reward=self.clip_reward, obs_mean=self._obs_mean.data_ptr(),
                                        obs_var=self._obs_var.data_ptr(), obs_count=self._obs_count.data_ptr(), ret_stats=self._ret.data_ptr(),
                                        returns=self.returns.data_ptr(), scratch=self._scratch.data_ptr(), scratch_bytes=nbytes)
        self.training, self.norm_obs, self.norm_reward = training, norm_obs, norm_reward
        self.obs_rms = _RmsView(self._obs_mean, self._obs_var, self._obs_count)
        self.ret_rms = _RmsView(self._ret[0:1], self._ret[1:2], self._ret[2:3])

    def _init_state(self):
        self._state.zero_()
        self._obs_var.fill_(1.0)
        self._obs_count.fill_(COUNT0)
        self._ret[1] = 1.0
        self._ret[2] = COUNT0
        self.returns.zero_()
        self._rebase()

    def _rebase(self):
        """Synchronised object: the running statistics as they stand become ``base``, ``acc`` is emptied."""
        if self._base is not None:
            self._base.copy_(self._state)
            self._acc.zero_()

    @property
    def synced(self):
        return self._sync_group is not None

    def _sync_world(self):
        """(world, rank) of the sync group, resolved at the first use; ``"world"`` without an initialised process group is a world of
        one.  Makes the all-reduce buffer and, on the GPU, the DmVecNormSync descriptor."""
        if self._gather is None:
            import torch.distributed as dist
            g = self._sync_group
            if isinstance(g, str):
                g = dist.group.WORLD if dist.is_initialized() else None
            self._pg = g
            self._world, self._rank = (dist.get_world_size(g), dist.get_rank(g)) if g is not None else (1, 0)
            self._gather = self._torch.zeros(self._world, self._state.numel(), dtype=self._torch.float64, device=self.device)
            if self.on_gpu:
                self._sync = _lib.DmVecNormSync(world=self._world, rank=self._rank, base=self._base.data_ptr(), acc=self._acc.data_ptr(),
                                                gather=self._gather.data_ptr())
        return self._world, self._rank

    def _sets(self, flat):
        """The two (mean, var, count) triples of views of a flat [2 D + 4] moment set: observations, returns."""
        D = self.obs_dim
        return (flat[:D], flat[D:2 * D], flat[2 * D:2 * D + 1]), (flat[2 * D + 1:2 * D + 2], flat[2 * D + 2:2 * D + 3], flat[2 * D + 3:2 * D + 4])

    @staticmethod
    def _merge_into(a, b):
        """a <- merge(a, b) on (mean, var, count) views: ``update_from_moments`` with b as the batch (dm_vn_merge of
        include/deepmimic_vecnorm.h on the torch path); a set of count 0 is skipped exactly."""
        if float(b[2]) == 0.0:
            return
        if float(a[2]) == 0.0:
            for x, y in zip(a, b):
                x.copy_(y)
            return
        d, tot = b[0] - a[0], a[2] + b[2]
        new_var = (a[1] * a[2] + b[1] * b[2] + d * d * a[2] * b[2] / tot) / tot
        a[0].copy_(a[0] + d * b[2] / tot)
        a[1].copy_(new_var)
        a[2].copy_(tot)

    def _rms_update_sync(self, which, x):
        """The torch path of the synchronised update of set ``which`` (0 observations, 1 returns) with the rows x fp64 [n, ...]:
        acc = merge(acc, batch), running = merge(base, acc)."""
        t = self._torch
        batch = (x.mean(0), x.var(0, unbiased=False), t.full((1,), float(x.shape[0]), dtype=t.float64))
        acc, base, run = self._sets(self._acc)[which], self._sets(self._base)[which], self._sets(self._state)[which]
        self._merge_into(acc, batch)
        for r, b in zip(run, base):
            r.copy_(b)
        self._merge_into(run, acc)

    def sync(self):
        """Make the statistics of every rank of the sync group identical again: ``base`` = merge(base, every rank's ``acc`` in rank
        order), ``acc`` emptied, running = base.  Pack launch, ONE all-reduce (sum; every rank fills its own row of a zeroed
        [world, 2 D + 4] buffer, so the sum is a gather), merge launch: eager, on the current stream, never inside a captured graph."""
        if not self.synced:
            raise RuntimeError("HipVecNormalize.sync: built without a sync_group")
        world, rank = self._sync_world()
        if self.on_gpu:
            self._call("dm_vecnorm_sync_pack", C.byref(self._sync))
        else:
            self._gather.zero_()
            self._gather[rank].copy_(self._acc)
        if self._pg is not None and world > 1:
            import torch.distributed as dist
            dist.all_reduce(self._gather, op=dist.ReduceOp.SUM, group=self._pg)
        if self.on_gpu:
            self._call("dm_vecnorm_sync_merge", C.byref(self._sync))
        else:
            for r in range(world):
                for a, b in zip(self._sets(self._base), self._sets(self._gather[r])):
                    self._merge_into(a, b)
            self._acc.zero_()
            self._state.copy_(self._base)
        self.sync_calls += 1

    # ---- the three flags live in the descriptor the kernels read
    def _flag(name):
        def get(self):
            return self.__dict__["_" + name]

        def set_(self, v):
            self.__dict__["_" + name] = bool(v)
            if self._desc is not None:
                setattr(self._desc, name, int(bool(v)))
        return property(get, set_)

    training, norm_obs, norm_reward = _flag("training"), _flag("norm_obs"), _flag("norm_reward")
    del _flag

    # ---- so do the four settings: one changed between steps reaches the next launch (and SAC's sample-time transform)
    def _setting(name):
        def get(self):
            return self.__dict__["_" + name]

        def set_(self, v):
            self.__dict__["_" + name] = float(v)
            if self.__dict__.get("_desc") is not None:
                setattr(self._desc, name, float(v))
        return property(get, set_)

    clip_obs, clip_reward, gamma, epsilon = _setting("clip_obs"), _setting("clip_reward"), _setting("gamma"), _setting("epsilon")
    del _setting

    def __getattr__(self, name):
        """Everything else of the VecEnv surface (``seed``, ``get_attr``, ``render``, ``enable_debug_log``, ``sub_batches`` ...) is
        the inner env's.  ``engine`` / ``engines`` are forwarded for a one-engine env only: they are what sends ``PPO`` down the
        one-launch ``policy_forward`` route, which normalises in place after that engine's step."""
        if name.startswith("__") or name in ("venv", "_desc") or name in self._HIDDEN:
            raise AttributeError(name)
        venv = self.__dict__.get("venv")
        if venv is None:
            raise AttributeError(name)
        if name in ("engine", "engines") and int(getattr(venv, "sub_batches", 1)) != 1:
            raise AttributeError(name)
        return getattr(venv, name)

    @property
    def unwrapped(self):
        return getattr(self.venv, "unwrapped", self.venv)

    # ---- the arithmetic: HIP on the GPU, torch fp64 on the CPU
    def _call(self, entry, *args):
        t = self._torch
        L = _lib.load_library()
        ptrs = [C.c_void_p(a.data_ptr()) if isinstance(a, t.Tensor) else a for a in args]
        rc = getattr(L, entry)(C.byref(self._desc), *ptrs, C.c_void_p(t.cuda.current_stream(self.device).cuda_stream))
        if rc != 0:
            raise RuntimeError("%s failed (%d): %s" % (entry, rc, (L.dm_vecnorm_last_error() or b"").decode()))

    def _f32(self, x, what):
        if not (x.dtype == self._torch.float32 and x.is_contiguous()):
            raise ValueError("HipVecNormalize: %s must be a contiguous fp32 tensor" % what)
        return x

    def _rms_update(self, mean, var, count, x):
        """RunningMeanStd.update(x) on views of the state; x fp64 [n, ...]."""
        n = float(x.shape[0])
        bm, bv = x.mean(0), x.var(0, unbiased=False)
        d, tot = bm - mean, count + n
        new_var = (var * count + bv * n + d * d * count * n / tot) / tot
        mean += d * n / tot
        var.copy_(new_var)
        count.copy_(tot)

    def _norm_obs_t(self, x):
        t = self._torch
        if not self.norm_obs:
            return x.float()
        y = (x.double() - self._obs_mean) / t.sqrt(self._obs_var + self.epsilon)
        return t.clamp(y, -self.clip_obs, self.clip_obs).float()

    def _norm_rew_t(self, r):
        t = self._torch
        if not self.norm_reward:
            return r.float()
        return t.clamp(r.double() / t.sqrt(self._ret[1] + self.epsilon), -self.clip_reward, self.clip_reward).float()

    def normalize_step_(self, obs, rew, done, tobs, obs_out, rew_out, tobs_out):
        """Steps 2 to 7 of SB3's ``step_wait`` on device tensors; an output may be its input.  ``tobs`` / ``tobs_out`` may be None."""
        t = self._torch
        if self.on_gpu:
            for x, what in ((obs, "obs"), (rew, "rew"), (obs_out, "obs_out"), (rew_out, "rew_out")):
                self._f32(x, what)
            if not (done.dtype == t.uint8 and done.is_contiguous()):
                raise ValueError("HipVecNormalize: done flags must be a contiguous uint8 tensor")
            assert obs.shape == (self.num_envs, self.obs_dim) and rew.numel() == self.num_envs and done.numel() == self.num_envs
            if tobs is not None:
                self._f32(tobs, "terminal_obs"), self._f32(tobs_out, "terminal_obs out")
            if self.synced:
                self._sync_world()
                self._call("dm_vecnorm_step_sync", obs, rew, done, tobs, obs_out, rew_out, tobs_out, C.byref(self._sync))
            else:
                self._call("dm_vecnorm_step", obs, rew, done, tobs, obs_out, rew_out, tobs_out)
            return
        dn = done != 0
        if self.training and self.norm_obs:
            if self.synced:
                self._rms_update_sync(0, obs.double())
            else:
                self._rms_update(self._obs_mean, self._obs_var, self._obs_count, obs.double())
        new_obs = self._norm_obs_t(obs)
        if self.training:
            self.returns.mul_(self.gamma).add_(rew.double())
            if self.synced:
                self._rms_update_sync(1, self.returns)
            else:
                self._rms_update(self._ret[0:1], self._ret[1:2], self._ret[2:3], self.returns[:, None])
        new_rew = self._norm_rew_t(rew)
        if tobs is not None:
            new_tobs = t.where(dn[:, None], self._norm_obs_t(tobs), tobs)
            tobs_out.copy_(new_tobs)
        obs_out.copy_(new_obs)
        rew_out.copy_(new_rew)
        self.returns[dn] = 0.0

    def step_inplace(self, obs, rew_raw, done, rew_out):
        """The ``policy_forward`` rollout route: ``obs`` [N, D] (what the engine just wrote) is normalised in place, ``rew_raw`` is
        read and its normalised value written to ``rew_out``.  No terminal observations on that route."""
        self.normalize_step_(obs, rew_raw, done, None, obs, rew_out, None)

    # ---- zero-copy tensor API
    def reset_tensor(self, idx_init=None):
        obs = self.venv.reset_tensor() if idx_init is None else self.venv.reset_tensor(idx_init)
        self.out = dict(self._own, obs_raw=obs)
        if self.on_gpu and self.synced:
            self._sync_world()
            self._call("dm_vecnorm_reset_sync", self._f32(obs, "obs"), self._own["obs"], C.byref(self._sync))
        elif self.on_gpu:
            self._call("dm_vecnorm_reset", self._f32(obs, "obs"), self._own["obs"])
        else:
            self.returns.zero_()
            if self.training and self.norm_obs:
                if self.synced:
                    self._rms_update_sync(0, obs.double())
                else:
                    self._rms_update(self._obs_mean, self._obs_var, self._obs_count, obs.double())
            self._own["obs"].copy_(self._norm_obs_t(obs))
        return self._own["obs"]

    def step_tensor(self, actions):
        """actions: float32 device tensor [N, A] -> dict of device tensors, see the class docstring."""
        inner = self.venv.step_tensor(actions)
        own = self._own
        self.normalize_step_(inner["obs"], inner["rew"], inner["done"], inner.get("terminal_obs"), own["obs"], own["rew"],
                             own["terminal_obs"] if inner.get("terminal_obs") is not None else None)
        self.out = dict(inner, obs=own["obs"], rew=own["rew"], obs_raw=inner["obs"], rew_raw=inner["rew"])
        if inner.get("terminal_obs") is not None:
            self.out["terminal_obs"] = own["terminal_obs"]
        return self.out

    # ---- SB3 VecEnv protocol (numpy in / numpy out)
    def reset(self):
        return self.reset_tensor().cpu().numpy()

    def step_async(self, actions):
        t = self._torch
        self._actions.copy_(t.as_tensor(np.ascontiguousarray(actions, dtype=np.float32)).reshape(self._actions.shape))

    def step_wait(self):
        out = self.step_tensor(self._actions)
        obs, rew, done = out["obs"].cpu().numpy(), out["rew"].cpu().numpy(), out["done"].cpu().numpy() != 0
        if "terms" not in out:
            return obs, rew, done, [{} for _ in range(self.num_envs)]
        from .vec_env import LazyInfos
        infos = getattr(self.venv, "_infos", LazyInfos)
        return obs, rew, done, infos(out["terms"].cpu().numpy(), out["reason"].cpu().numpy().astype(np.int32), done,
                                     out["terminal_obs"].cpu().numpy())

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def close(self):
        self.venv.close()

    # ---- SB3's own methods.  A device tensor goes through dm_vecnorm_apply and comes back as a new device tensor; anything else
    # is numpy in, numpy out, with the arithmetic of the formulas in fp64 on a host copy of the statistics.
    def _apply(self, obs=None, rew=None):
        t = self._torch
        x = obs if obs is not None else rew
        if not (x.is_cuda and self.on_gpu):
            return self._norm_obs_t(x.to(self.device)) if obs is not None else self._norm_rew_t(x.to(self.device))
        x = x.contiguous() if x.dtype == t.float32 else x.float().contiguous()
        y = t.empty_like(x)
        if obs is not None:
            if x.dim() < 1 or x.shape[-1] != self.obs_dim:
                raise ValueError("normalize_obs: rows of %d columns, not %r" % (self.obs_dim, tuple(x.shape)))
            n = x.numel() // self.obs_dim
            if n:
                self._call("dm_vecnorm_apply", n, x, y, None, None)
        elif x.numel():
            self._call("dm_vecnorm_apply", x.numel(), None, None, x, y)
        return y

    def _host_stats(self):
        s = self._state.detach().cpu().numpy()
        D = self.obs_dim
        return s[:D], s[D:2 * D], s[2 * D + 2]

    def normalize_obs(self, obs):
        if isinstance(obs, self._torch.Tensor):
            return self._apply(obs=obs)
        x = np.asarray(obs)
        if not self.norm_obs:
            return x
        mean, var, _ = self._host_stats()
        return np.clip((x.astype(np.float64) - mean) / np.sqrt(var + self.epsilon), -self.clip_obs, self.clip_obs).astype(np.float32)

    def normalize_reward(self, reward):
        if isinstance(reward, self._torch.Tensor):
            return self._apply(rew=reward)
        r = np.asarray(reward)
        if not self.norm_reward:
            return r
        return np.clip(r.astype(np.float64) / np.sqrt(self._host_stats()[2] + self.epsilon), -self.clip_reward, self.clip_reward).astype(np.float32)

    def unnormalize_obs(self, obs):
        is_t = isinstance(obs, self._torch.Tensor)
        x = obs.detach().cpu().numpy() if is_t else np.asarray(obs)
        if self.norm_obs:
            mean, var, _ = self._host_stats()
            x = (x.astype(np.float64) * np.sqrt(var + self.epsilon) + mean).astype(np.float32)
        return self._torch.as_tensor(x, device=obs.device) if is_t else x

    def unnormalize_reward(self, reward):
        is_t = isinstance(reward, self._torch.Tensor)
        r = reward.detach().cpu().numpy() if is_t else np.asarray(reward)
        if self.norm_reward:
            r = (r.astype(np.float64) * np.sqrt(self._host_stats()[2] + self.epsilon)).astype(np.float32)
        return self._torch.as_tensor(r, device=reward.device) if is_t else r

    def get_original_obs(self):
        """The unnormalised observations of the last ``reset`` / ``step`` (a numpy copy, as in SB3).  Not kept on PPO's
        ``policy_forward`` route, which normalises the engine's output in place."""
        raw = self.out.get("obs_raw")
        if raw is None:
            raise RuntimeError("get_original_obs before the first reset")
        return raw.detach().cpu().numpy().copy()

    def get_original_reward(self):
        raw = self.out.get("rew_raw")
        if raw is None:
            raise RuntimeError("get_original_reward before the first step")
        return raw.detach().cpu().numpy().copy()

    # ---- persistence
    def state_dict(self):
        """numpy copies of the running statistics and the settings (``returns`` included, so a resumed run continues bit for bit).
        The same keys with or without a sync group: a file of either kind of object loads into the other."""
        s = self._state.detach().cpu().numpy().copy()
        D = self.obs_dim
        return dict(obs_mean=s[:D], obs_var=s[D:2 * D], obs_count=s[2 * D:2 * D + 1], ret_mean=s[2 * D + 1:2 * D + 2],
                    ret_var=s[2 * D + 2:2 * D + 3], ret_count=s[2 * D + 3:2 * D + 4], returns=self.returns.detach().cpu().numpy().copy(),
                    settings=np.array([self.clip_obs, self.clip_reward, self.gamma, self.epsilon]),
                    flags=np.array([self.training, self.norm_obs, self.norm_reward], dtype=np.int64))

    def load_state_dict(self, sd, settings=True):
        """Statistics always; ``settings``: also clips, gamma, epsilon and the three flags.  ``returns`` is taken when it fits this
        batch, else zeroed."""
        t, D = self._torch, self.obs_dim
        if np.shape(sd["obs_mean"]) != (D,) or np.shape(sd["obs_var"]) != (D,):
            raise ValueError("load_state_dict: statistics of %r columns for an env of %d" % (np.shape(sd["obs_mean"]), D))
        flat = np.concatenate([np.asarray(sd[k], np.float64).reshape(-1) for k in ("obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count")])
        self._state.copy_(t.as_tensor(flat))
        self._rebase()                       # a synchronised object: what was loaded is what the ranks agree on, nothing pending
        ret = np.asarray(sd.get("returns", ()), np.float64).reshape(-1)
        if ret.size == self.num_envs:
            self.returns.copy_(t.as_tensor(ret))
        else:
            self.returns.zero_()
        if settings:
            self.clip_obs, self.clip_reward, self.gamma, self.epsilon = (float(x) for x in np.asarray(sd["settings"]).reshape(-1))
            self.training, self.norm_obs, self.norm_reward = (bool(x) for x in np.asarray(sd["flags"]).reshape(-1))

    def save(self, path):
        """One .npz-format file at exactly ``path`` (no pickle)."""
        with open(path, "wb") as f:
            np.savez(f, **self.state_dict())

    @classmethod
    def load(cls, path, venv, sync_group=None):
        with np.load(path, allow_pickle=False) as z:
            sd = {k: z[k] for k in z.files}
        vn = cls(venv, sync_group=sync_group)
        vn.load_state_dict(sd)
        return vn
