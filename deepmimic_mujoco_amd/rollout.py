"""The rollout side of PPO: one collector for every rollout path, the rollout's tail (``RolloutFinish``) and GAE.

A rollout is T steps of every env sub-batch followed by one tail.  ``Collector`` is the product of two choices, both made by
``route()``:

  step of sub-batch k at time t      policy_forward   dm_policy_forward + dm_step, both writing row t of the buffers in place
                                     sample_store     library GEMMs, dm_policy_sample, env step, dm_rollout_store
                                     plain            PyTorch ops only (the only one that runs on the CPU)
  driver of the T x K steps          serial           the current stream, one batch
                                     streams          one stream per sub-batch, issued by the host
                                     captured         the same, recorded once into a hipGraph and replayed

Everything else exists once: the buffer allocator, the fork / join over ``concurrent_streams``, warm-up + capture
(``capture_graph``, which the learner's graphs use too), the device half of the tail (inside the graph where there is one) and its
host half (``_last_obs``, ``num_timesteps``, the statistics read).
"""
from __future__ import annotations

from contextlib import contextmanager

import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from .streams import concurrent_streams


def compute_gae(rewards, values, dones, last_values, gamma, lam):
    """SB3 ``RolloutBuffer.compute_returns_and_advantage`` [EXT]: tensors [T, N]; dones[t] is the done
    flag returned by step t (so the value after it is not bootstrapped)."""
    T = rewards.shape[0]
    adv = torch.zeros_like(rewards)
    last = torch.zeros_like(last_values)
    for t in reversed(range(T)):
        next_v = last_values if t == T - 1 else values[t + 1]
        nonterm = 1.0 - dones[t]
        delta = rewards[t] + gamma * next_v * nonterm - values[t]
        last = delta + gamma * lam * nonterm * last
        adv[t] = last
    return adv, adv + values


EP_HIST = 100        # SB3: ep_info_buffer = deque(maxlen=100)


def explained_variance64(values, returns):
    """SB3's ``explained_variance(y_pred, y_true)`` = 1 - var(y_true - y_pred) / var(y_true) in fp64 (NaN when var(y_true) is 0)."""
    y, v = np.asarray(returns, np.float64).reshape(-1), np.asarray(values, np.float64).reshape(-1)
    vy = float(np.var(y))
    return float("nan") if vy == 0.0 else 1.0 - float(np.var(y - v)) / vy


class RolloutFinish:
    """What follows the T env steps of a rollout: GAE, SB3's Monitor for the vec-env (per-env episode return / length that
    persist across rollouts, the last 100 finished episodes) and the rollout statistics.  On the GPU this is ONE call of
    ``dm_rollout_finish`` (csrc/dm_ppo.hip) on the current stream, capturable into a hipGraph, with all state on the device and
    ``read()`` as the one small device-to-host copy; on the CPU ``compute_gae`` plus the same monitor in numpy.  Episodes are
    numbered in (rollout, step, env) order, as SB3's ``_update_info_buffer`` meets them; returns are fp32 sums in step order."""

    def __init__(self, T, N, device, gamma, gae_lambda):
        self.T, self.N, self.device, self.gamma, self.gae_lambda = int(T), int(N), torch.device(device), float(gamma), float(gae_lambda)
        self.on_gpu = self.device.type == "cuda"
        if self.on_gpu:
            # one arena = one host read: [0:16) the 8 fp64 statistics, [16:216) ep_hist [2, 100], [216] ep_count (uint32)
            self.arena = torch.zeros(16 + 2 * EP_HIST + 8, device=self.device)
            self.stats64 = self.arena[:16].view(torch.float64)
            self.ep_hist = self.arena[16:16 + 2 * EP_HIST]
            self.ep_count = self.arena[16 + 2 * EP_HIST:16 + 2 * EP_HIST + 1].view(torch.int32)
            self.ep_acc = torch.zeros(2 * self.N, device=self.device)
            self.work_bytes = int(_lib.load_library().dm_rollout_finish_workspace_bytes(self.T, self.N))
            self.work = torch.zeros(self.work_bytes, dtype=torch.uint8, device=self.device)
        else:
            self._acc = np.zeros((2, self.N), np.float32)
            self._hist = np.zeros((2, EP_HIST), np.float32)
            self._count = 0
            self._stats = np.zeros(8)

    def reset(self):
        """Forget every episode, finished or running (a loaded checkpoint carries no monitor state, as in SB3)."""
        if self.on_gpu:
            self.arena.zero_()
            self.ep_acc.zero_()
        else:
            self._acc[:] = 0
            self._hist[:] = 0
            self._count = 0
            self._stats[:] = 0

    def __call__(self, rew, done, val, last_val, adv=None, ret=None):
        """rew / val [T, N] fp32, done [T, N] uint8 or fp32, last_val [N] -> (adv, ret); advances the monitor by this rollout."""
        T, N = self.T, self.N
        assert tuple(rew.shape) == (T, N) and tuple(done.shape) == (T, N) and tuple(val.shape) == (T, N) and last_val.numel() == N
        if not self.on_gpu:
            adv_, ret_ = compute_gae(rew, val, done if done.dtype == torch.float32 else done.float(), last_val, self.gamma, self.gae_lambda)
            self._monitor_numpy(rew.numpy(), done.numpy() != 0, val.numpy(), ret_.numpy())
            if adv is not None:
                adv.copy_(adv_); ret.copy_(ret_)
                return adv, ret
            return adv_, ret_
        if adv is None:
            adv, ret = torch.empty_like(rew), torch.empty_like(rew)
        last_val = last_val.reshape(-1)
        for t in (rew, val, last_val, adv, ret):
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise ValueError("dm_rollout_finish takes contiguous fp32 device tensors")
        if not (done.is_cuda and done.is_contiguous() and done.dtype in (torch.uint8, torch.float32)):
            raise ValueError("dm_rollout_finish takes done flags as a contiguous uint8 or fp32 device tensor")
        _lib.call("dm_rollout_finish", T, N, rew, done, 1 if done.dtype == torch.uint8 else 0, val, last_val, self.gamma, self.gae_lambda,
                  adv, ret, self.ep_acc, self.ep_hist, self.ep_count, self.stats64, self.work, self.work_bytes, device=self.device)
        return adv, ret

    def _monitor_numpy(self, rew, fin, val, ret):
        acc, one = self._acc, np.float32(1.0)
        for t in range(self.T):
            acc[0] += rew[t]
            acc[1] += one
            for e in np.nonzero(fin[t])[0]:                      # env order within the step
                k = self._count % EP_HIST
                self._hist[0, k], self._hist[1, k] = acc[0, e], acc[1, e]
                self._count += 1
            acc[:, fin[t]] = 0
        y, d = ret.astype(np.float64), ret.astype(np.float64) - val.astype(np.float64)
        vy, vd = float(np.var(y)), float(np.var(d))
        self._stats[:] = (float(rew.astype(np.float64).sum()), float(fin.sum()), float("nan") if vy == 0.0 else 1.0 - vd / vy, vy, vd,
                          float(rew.size), float(self._count), float(y.mean()))

    def read(self):
        """Statistics of the last rollout and the episode history, oldest episode first: one device-to-host copy on the GPU."""
        if self.on_gpu:
            host = self.arena.cpu()
            st = host[:16].view(torch.float64).numpy()
            hist = host[16:16 + 2 * EP_HIST].numpy().reshape(2, EP_HIST)
            count = int(host[16 + 2 * EP_HIST:16 + 2 * EP_HIST + 1].view(torch.int32)[0]) & 0xFFFFFFFF
        else:
            st, hist, count = self._stats, self._hist, self._count
        k = min(count, EP_HIST)
        order = (np.arange(EP_HIST) + count) % EP_HIST if count >= EP_HIST else np.arange(k)       # slot of episode count - 100 first
        ep_rew, ep_len = hist[0, order].copy(), hist[1, order].copy()
        n = float(st[5]) if st[5] > 0 else 1.0
        return dict(reward_sum=float(st[0]), dones=int(st[1]), n=int(st[5]), mean_reward=float(st[0]) / n, done_rate=float(st[1]) / n,
                    explained_variance=float(st[2]), episodes=count, ep_returns=ep_rew, ep_lengths=ep_len,
                    ep_rew_mean=float(np.mean(ep_rew.astype(np.float64))) if k else float("nan"),
                    ep_len_mean=float(np.mean(ep_len.astype(np.float64))) if k else float("nan"))


@contextmanager
def forked(device, streams):
    """Fork ``streams`` off the current stream of ``device`` and join them back into it after the block."""
    cur = torch.cuda.current_stream(device)
    for s in streams:
        s.wait_stream(cur)
    yield
    for s in streams:
        cur.wait_stream(s)


def capture_graph(device, body, warm=None, warm_iters=1):
    """Run ``warm`` on a side stream (library workspaces, allocator pools), synchronise, then capture ``body`` into a hipGraph.
    ``warm=None`` captures straight away: a further graph after one that was warmed up.  Returns (graph, what ``body`` returned)."""
    if warm is not None:
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            for _ in range(warm_iters):
                warm()
        torch.cuda.current_stream(device).wait_stream(side)
        torch.cuda.synchronize(device)
    graph = torch.cuda.CUDAGraph()
    # with a process group alive, its watchdog thread queries events while we capture: "global" capture mode would
    # fail the capture on that foreign call, "thread_local" only polices this thread
    with torch.cuda.graph(graph, **(dict(capture_error_mode="thread_local") if dist.is_initialized() else {})):
        out = body()
    return graph, out


def route(ppo):
    """(step, driver) of the rollout this configuration takes: the one place that decides it."""
    K = getattr(ppo.env, "sub_batches", 1)
    if ppo._fused_policy_ok():
        return "policy_forward", ("serial" if K == 1 else "captured" if ppo.rollout_graph else "streams")
    step = "sample_store" if ppo._fused_rollout_ok() else "plain"
    halves = K > 1 and hasattr(ppo.env, "step_sub")
    if halves and not ppo.rollout_graph and step == "sample_store":
        return step, "streams"
    if halves and ppo.rollout_graph and ppo.device.type == "cuda":
        return step, "captured"
    return step, "serial"               # one batch through env.step_tensor, whatever the env's sub-batches


class Collector:
    """Collects the rollouts of one ``PPO``: see the module docstring.  ``rb`` are the buffers of the last rollout (persistent
    except on the serial sample_store / plain rollout, which hands out fresh ones), ``last`` the observations the next rollout starts
    from, ``graph`` the captured rollout (None unless the driver is "captured")."""

    def __init__(self, ppo):
        self.ppo, self.device = ppo, ppo.device
        self.step_kind, self.driver = route(ppo)
        self.step = getattr(self, "_step_" + self.step_kind)
        env, N = ppo.env, ppo.n_envs
        K = getattr(env, "sub_batches", 1) if self.driver != "serial" else 1
        self.slices = list(env.sub_slices) if K > 1 else [slice(0, N)]
        self.streams = concurrent_streams(self.device, K) if K > 1 else []
        # under capture the sample_store / plain chains are recorded one sub-batch after the other, the policy_forward steps (as
        # everything the host issues live) step by step.  Part of the trajectory: torch numbers the plain step's draws in this order
        self.chain_major = self.driver == "captured" and self.step_kind != "policy_forward"
        self.persistent = self.driver != "serial" or self.step_kind == "policy_forward"
        self.rb = self.last = self.graph = self.fwd = None
        # a vec_normalize.HipVecNormalize around the env: the buffers gain a ``rew_raw`` row per step, which feeds the episode monitor
        from .vec_normalize import HipVecNormalize
        self.vn = env if isinstance(env, HipVecNormalize) else None
        self._scratch = {}
        if self.step_kind != "plain":
            # draw counters, advanced on the device: ONE PER SUB-BATCH — sub-batch chains run on their own streams (or as
            # independent branches of a captured graph), so a shared counter bumped by one chain would be read by the
            # others at unordered times (same noise at consecutive steps, non-reproducible rollouts)
            self.ctrs = torch.zeros(max(16, int(getattr(env, "sub_batches", 1))), dtype=torch.int32, device=self.device)
        if self.step_kind == "policy_forward":
            from .ppo import FusedPolicyForward
            self.fwd = FusedPolicyForward(ppo.policy, self.device)
            self.act_env = torch.zeros(N, ppo.act_dim, device=self.device)
            self.engines = getattr(env, "engines", None) or [env.engine]

    def _alloc(self):
        p, T, N = self.ppo, self.ppo.n_steps, self.ppo.n_envs
        z = lambda *shape, dt=torch.float32: torch.zeros(*shape, device=self.device, dtype=dt)
        rb = dict(obs=z(T, N, p.obs_dim, dt=p.buffer_dtype), act=z(T, N, p.act_dim, dt=p.buffer_dtype), rew=z(T, N), done=z(T, N), val=z(T, N),
                  logp=z(T, N), adv=z(T, N), ret=z(T, N))
        if self.step_kind == "policy_forward":
            rb["done_u8"] = z(T, N, dt=torch.uint8)         # dm_step writes its flags in place; the fp32 copy follows the finish
        if self.vn is not None:
            rb["rew_raw"] = z(T, N)                         # ``rew`` holds the normalised rewards (GAE), this the env's own (monitor)
        return rb

    # ---- the step of sub-batch k at time t, three kinds
    def _step_policy_forward(self, k, t):
        """``dm_policy_forward`` reads the observations in place and writes action / value / log-prob / observation copy straight
        into row t, ``dm_step`` writes reward and done flag into row t and the next observation over the one just consumed.  The
        draws are keyed on counter slot 0 (advanced by T once per rollout) and ``draw_offset = t``."""
        p, rb, sl, last = self.ppo, self.rb, self.slices[k], self.last
        self.fwd(last[sl], p._rollout_seed + 7919 * k, self.ctrs[0:1], t, p.act_lo, p.act_hi, rb["act"][t, sl], self.act_env[sl],
                 rb["logp"][t, sl], rb["val"][t, sl], obs_copy=rb["obs"][t, sl])
        if self.vn is None:
            self.engines[k].step(self.act_env[sl], dict(obs=last[sl], rew=rb["rew"][t, sl], done=rb["done_u8"][t, sl]))
            return
        # wrapped env (one engine): the raw reward goes to its own row, the normaliser then runs in place on what the engine wrote
        self.engines[k].step(self.act_env[sl], dict(obs=last[sl], rew=rb["rew_raw"][t, sl], done=rb["done_u8"][t, sl]))
        self.vn.step_inplace(last[sl], rb["rew_raw"][t, sl], rb["done_u8"][t, sl], rb["rew"][t, sl])

    def sample(self, obs, k=0):
        """mean / value by the MLP (library GEMMs), then one launch for sample + logp + clamp, keyed on sub-batch k's counter."""
        p, pol, n = self.ppo, self.ppo.policy, obs.shape[0]
        sc = self._scratch.get((n, k))
        if sc is None:
            z = lambda *shape: torch.zeros(*shape, device=self.device)
            sc = self._scratch[(n, k)] = dict(act=z(n, p.act_dim), act_env=z(n, p.act_dim), logp=z(n))
        mean = pol.action_net(pol.pi(obs))
        val = pol.value_net(pol.vf(obs)).squeeze(-1).contiguous()
        _lib.call("dm_policy_sample", mean.contiguous(), pol.log_std, n, p.act_dim, p._rollout_seed + 7919 * k, self.ctrs[k:k + 1],
                  p.act_lo, p.act_hi, sc["act"], sc["act_env"], sc["logp"], device=self.device)
        return sc, val

    def _env_step(self, k, act):
        return self.ppo.env.step_sub(k, act) if self.streams else self.ppo.env.step_tensor(act)

    def _step_sample_store(self, k, t):
        p, rb, sl, last = self.ppo, self.rb, self.slices[k], self.last
        sc, val = self.sample(last[sl], k)
        out = self._env_step(k, sc["act_env"])
        if rb["obs"].dtype != rb["act"].dtype or rb["obs"].dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("dm_rollout_store files obs / act as fp32 or bf16, both of one type")
        # files row t, writes the next observation over last[sl] and bumps the sub-batch's draw counter
        _lib.call("dm_rollout_store_bf16" if rb["obs"].dtype == torch.bfloat16 else "dm_rollout_store", val.shape[0], p.obs_dim, p.act_dim,
                  last[sl], sc["act"], val, sc["logp"], out["rew"], out["done"], out["obs"], rb["obs"][t, sl], rb["act"][t, sl],
                  rb["val"][t, sl], rb["logp"][t, sl], rb["rew"][t, sl], rb["done"][t, sl], last[sl], self.ctrs[k:k + 1], device=self.device)
        if self.vn is not None:
            rb["rew_raw"][t, sl].copy_(out["rew_raw"])

    def _step_plain(self, k, t):
        p, rb, sl, last = self.ppo, self.rb, self.slices[k], self.last
        obs = last[sl]
        act, val, logp = p.policy(obs)
        rb["obs"][t, sl] = obs
        rb["act"][t, sl] = act
        rb["val"][t, sl] = val
        rb["logp"][t, sl] = logp
        out = self._env_step(k, torch.clamp(act, p.act_lo, p.act_hi))
        rb["rew"][t, sl] = out["rew"]
        if self.vn is not None:
            rb["rew_raw"][t, sl] = out["rew_raw"]
        rb["done"][t, sl] = out["done"].float()
        last[sl].copy_(out["obs"])

    # ---- the driver
    def _steps(self, T):
        if not self.streams:
            for t in range(T):
                self.step(0, t)
            return
        K = len(self.streams)
        order = [(k, t) for k in range(K) for t in range(T)] if self.chain_major else [(k, t) for t in range(T) for k in range(K)]
        with forked(self.device, self.streams):
            for k, t in order:
                with torch.cuda.stream(self.streams[k]):
                    self.step(k, t)

    def _warm(self):
        """Before a capture: one step of every sub-batch.  Real env steps that ``num_timesteps`` does not count; the sample_store
        step bumps its draw counters as in any other step, the policy_forward step draws what step 0 will draw again.  The
        policy_forward steps all run on the warm-up stream and end with the tail's ``predict_values``; the sample_store / plain
        steps run on their sub-batch's stream, whose library workspaces the capture needs warmed."""
        if self.fwd is None:
            return self._steps(1)
        self.fwd.pack()
        for k in range(len(self.streams)):
            self.step(k, 0)
        self.ppo.policy.predict_values(self.last)

    def _whole(self):
        """Everything of a rollout that runs on the device, i.e. what the captured driver records."""
        p, rb = self.ppo, self.rb
        if self.fwd is not None:
            self.fwd.pack()                 # once per rollout: the weights changed since the last one
        self._steps(p.n_steps)
        if self.fwd is not None:
            self.ctrs[0:1].add_(p.n_steps)
        last_val = p.policy.predict_values(self.last)
        # GPU: dm_rollout_finish (bit for bit compute_gae), once over [T, N] after the streams joined; CPU: compute_gae itself
        p._finish(rb["rew"], rb.get("done_u8", rb["done"]), rb["val"], last_val, rb["adv"], rb["ret"])
        if self.vn is not None:
            # a Monitor inside VecNormalize sees the env's own rewards: a second finish fed rew_raw keeps the episode history and the
            # reward mean; its advantages land in scratch rows and are not used
            sc = self._scratch.setdefault("finish_raw", (torch.empty_like(rb["adv"]), torch.empty_like(rb["ret"])))
            p._finish_raw(rb["rew_raw"], rb.get("done_u8", rb["done"]), rb["val"], last_val, *sc)
        if "done_u8" in rb:
            rb["done"].copy_(rb["done_u8"])     # the returned buffer's flags are fp32 on every route; nothing here waits for it

    def _tail(self):
        """After the rollout (never inside it): the host's bookkeeping and one small read of what the finish left -> ``stats``."""
        p, rb = self.ppo, self.rb
        p._last_obs = self.last
        p.num_timesteps += p.n_steps * p.n_envs
        r = p._finish.read()
        m = r if self.vn is None else p._finish_raw.read()      # wrapped env: episodes and reward mean from the raw rewards
        p.stats.update(mean_reward=m["mean_reward"], done_rate=r["done_rate"], ep_rew_mean=m["ep_rew_mean"], ep_len_mean=m["ep_len_mean"],
                       episodes=m["episodes"], explained_variance=r["explained_variance"])
        if self.device.type != "cuda":                           # the torch path keeps its fp32 means
            p.stats["mean_reward"] = float(rb["rew" if self.vn is None else "rew_raw"].mean())
            p.stats["done_rate"] = float(rb["done"].mean())
        return {k: v for k, v in rb.items() if k != "done_u8"}

    def collect(self):
        p = self.ppo
        if self.last is None:
            self.last = (p.env.reset_tensor() if p._last_obs is None else p._last_obs).clone(memory_format=torch.contiguous_format)
        elif p._last_obs is not None and p._last_obs.data_ptr() != self.last.data_ptr():
            self.last.copy_(p._last_obs)        # assigned from outside since the last rollout
        if self.rb is None or not self.persistent:
            self.rb = self._alloc()
        if p._finish is None:
            p._finish = RolloutFinish(p.n_steps, p.n_envs, self.device, p.gamma, p.gae_lambda)
        if self.vn is not None and p._finish_raw is None:
            p._finish_raw = RolloutFinish(p.n_steps, p.n_envs, self.device, p.gamma, p.gae_lambda)
        with torch.no_grad():
            if self.driver == "captured":
                if self.graph is None:
                    self.graph, _ = capture_graph(self.device, self._whole, warm=self._warm)
                self.graph.replay()
            else:
                self._whole()
            if self.vn is not None and self.vn.synced:
                # one set of running statistics over the ranks: once per rollout, after it and before train; eager and on the
                # rollout stream like FlatAdam.all_reduce, outside the captured graph (two launches around one small all-reduce)
                self.vn.sync()
                p.stats["vecnorm_sync_calls"] = self.vn.sync_calls
        return self._tail()
