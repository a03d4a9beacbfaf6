"""Soft Actor-Critic on device tensors — the counterpart of src/sac_sb3.py (SB3 2.x ``SAC``).

src/sac_sb3.py trains ``SAC("MlpPolicy", env, policy_kwargs=dict(net_arch=[1024, 512]), buffer_size=5_000_000)`` on 32 envs and
leaves everything else at SB3's defaults [EXT]: learning_rate 3e-4, learning_starts 100, batch_size 256, tau 0.005, gamma 0.99,
train_freq 1, gradient_steps 1, ent_coef "auto" (log_ent_coef learned from 0, target_entropy = -act_dim), one Adam per actor /
critic / log_ent_coef (eps 1e-8, no clipping).  The policy is SB3's SAC MlpPolicy: ReLU MLPs with nn.Linear's default init, an
actor obs -> H1 -> H2 with heads mu and log_std (clamped to [-20, 2]) and a tanh-squashed Gaussian, twin critics
(obs | act) -> H1 -> H2 -> 1 and a Polyak-averaged target copy of the critics.

Two learners compute the same update, SB3's SAC.train in its order (alpha step, target, critic step, actor step, Polyak):
  * ``fused=False`` or CPU: plain torch (autograd), the readable statement of that update;
  * ``fused=True`` on a GPU: the GEMMs on the library, every head / activation / reduction / ring operation a HIP kernel of
    csrc/dm_sac.hip, all state on the device; one gradient step is captured once as a hipGraph and replayed.
Parameters live in three flat fp32 arenas (actor, critic, critic target) shared by both learners; an env step is
act + ``env.step_tensor`` + store, the replay ring never leaves HBM.

``SAC(env, normalizer=HipVecNormalize(env))`` is SB3's SAC on a ``VecNormalize`` env [EXT: OffPolicyAlgorithm._store_transition,
ReplayBuffer._get_samples]: the actor reads normalised observations, every env step feeds the running statistics, the ring stores RAW
transitions (the raw terminal observation for a finished env) and each sampled minibatch is normalised with the statistics of that
gradient step: ``dm_sac_gather_norm`` in the place of ``dm_sac_gather`` in the captured launch sequence, ``_norm_obs_t`` /
``_norm_rew_t`` in ``sample_torch``.  The learner steps the inner env itself; ``normalizer.training = False`` freezes the statistics
and keeps both transforms.  DESIGN §25.

``SAC(env, n_steps=n)`` is SB3's ``SAC(n_steps=)`` [EXT: NStepReplayBuffer, SB3 >= 2.7]: a sampled row keeps its observation and
action, follows its env for up to n stored steps (stopping after a done, after the newest stored step, or after n), and carries the
discounted reward sum, the chain's last next observation and ``done' = 1 - gamma^(k-1) (1 - done_last)``, which turns the one-step
target's ``(1 - done) gamma`` into the n-step ``gamma^k (1 - done_last)``: nothing after the sample changes.  ``dm_sac_gather_nstep``
(include/deepmimic_sac_nstep.h) in the place of either gather when n > 1, ``_sample_nstep_torch`` in ``sample_torch``.  DESIGN §27.
"""
from __future__ import annotations

import collections
import ctypes
import math
import time

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from ._lib import ADAM_STATE_FLOATS
from .rollout import EP_HIST, capture_graph

LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)


def actor_layout(D, H1, H2, A):
    """(name, shape) of the actor arena: latent_pi (two ReLU layers), then the head [mu ; log_std] as one [2A x H2] matrix."""
    return [("W1", (H1, D)), ("b1", (H1,)), ("W2", (H2, H1)), ("b2", (H2,)), ("Wh", (2 * A, H2)), ("bh", (2 * A,))]


def critic_layout(K, H1, H2):
    """(name, shape) of the critic arena: qf0 and qf1 stacked layer by layer (index 0 / 1 of the leading axis)."""
    return [("W1", (2, H1, K)), ("b1", (2, H1)), ("W2", (2, H2, H1)), ("b2", (2, H2)), ("W3", (2, 1, H2)), ("b3", (2, 1))]


def arena_views(flat, layout):
    out, off = {}, 0
    for name, shape in layout:
        n = int(np.prod(shape))
        out[name] = flat[off:off + n].view(shape)
        off += n
    return out


def arena_size(layout):
    return sum(int(np.prod(s)) for _, s in layout)


def actor_head(P, obs):
    """[mu | log_std] (unclamped) of the actor for obs [B x D]."""
    h = F.relu(F.linear(obs, P["W1"], P["b1"]))
    h = F.relu(F.linear(h, P["W2"], P["b2"]))
    return F.linear(h, P["Wh"], P["bh"])


def squash(head, eps):
    """SB3's SquashedDiagGaussianDistribution.log_prob_from_params with the noise given: (a = tanh(u), log pi(a))."""
    A = head.shape[1] // 2
    mu, log_std = head[:, :A], head[:, A:].clamp(-20.0, 2.0)
    std = log_std.exp()
    u = mu + std * eps
    a = torch.tanh(u)
    logp = (-((u - mu) ** 2) / (2 * std ** 2) - torch.log(std) - LOG_SQRT_2PI).sum(-1)
    return a, logp - torch.log(1 - a ** 2 + 1e-6).sum(-1)


def q_values(P, x):
    """[2, B] values of the twin critics on x = (obs | act) [B x K]."""
    out = []
    for i in range(2):
        h = F.relu(F.linear(x, P["W1"][i], P["b1"][i]))
        h = F.relu(F.linear(h, P["W2"][i], P["b2"][i]))
        out.append(F.linear(h, P["W3"][i], P["b3"][i])[:, 0])
    return torch.stack(out)


def adam_torch(p, g, m, v, step, lr, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam's single-tensor update (no weight decay, no amsgrad) on a flat arena; step counts from 1."""
    m.lerp_(g, 1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    p.addcdiv_(m, (v.sqrt() / math.sqrt(bc2)).add_(eps), value=-lr / bc1)


class SacPolicy:
    """Views of the arenas plus the inference surface the eval dashboard uses (``predict_values``)."""

    def __init__(self, sac):
        self.sac = sac

    @property
    def actor(self):
        return arena_views(self.sac.actor, self.sac._alay)

    @property
    def critic(self):
        return arena_views(self.sac.critic, self.sac._clay)

    @property
    def critic_target(self):
        return arena_views(self.sac.critic_target, self.sac._clay)

    def predict_values(self, obs):
        """min_i Q_i(obs, tanh(mu)): the value of the deterministic action."""
        with torch.no_grad():
            obs = torch.as_tensor(obs, dtype=torch.float32, device=self.sac.device)
            a = torch.tanh(actor_head(self.actor, obs)[:, :self.sac.act_dim])
            return q_values(self.critic, torch.cat([obs, a], 1)).min(0).values


class SAC:
    def __init__(self, env, net_arch=(1024, 512), buffer_size=1_000_000, learning_starts=100, batch_size=256, tau=0.005, gamma=0.99,
                 train_freq=1, gradient_steps=1, ent_coef="auto", target_entropy="auto", learning_rate=3e-4, seed=0, device=None,
                 fused=True, use_hip_graph=True, normalizer=None, n_steps=1):
        from .vec_normalize import HipVecNormalize
        if isinstance(env, HipVecNormalize):
            raise ValueError("SAC does not take a HipVecNormalize env: SB3 normalises at replay-sample time there, which this wrapper "
                             "does not do; pass the inner env")
        if normalizer is not None and not (isinstance(normalizer, HipVecNormalize) and normalizer.venv is env):
            raise ValueError("SAC(env, normalizer=...) takes a HipVecNormalize built on that same env (normalizer.venv is env)")
        if not (isinstance(n_steps, (int, np.integer)) and not isinstance(n_steps, bool) and 1 <= n_steps <= _lib.SAC_NSTEP_MAX):
            raise ValueError("SAC(n_steps=%r): an integer in 1 .. %d (one lane of the gather's wave per step)" % (n_steps, _lib.SAC_NSTEP_MAX))
        self.env = env
        self.normalizer = normalizer
        self.n_steps = int(n_steps)                     # a hyperparameter fixed here: a captured graph holds it, a checkpoint does not
        self.device = torch.device(device) if device is not None else getattr(env, "device", torch.device("cpu"))
        if isinstance(self.device, int):
            self.device = torch.device("cuda", self.device)
        self.n_envs = int(env.num_envs)
        self.obs_dim = D = int(env.observation_space.shape[0])
        self.act_dim = A = int(env.action_space.shape[0])
        self.K = D + A
        self.H1, self.H2 = (int(h) for h in net_arch)
        self.learning_starts, self.batch_size, self.tau, self.gamma = int(learning_starts), int(batch_size), float(tau), float(gamma)
        self.train_freq, self.gradient_steps, self.lr = int(train_freq), int(gradient_steps), float(learning_rate)
        self.target_entropy = float(-A if target_entropy == "auto" else target_entropy)
        self.ent_auto = isinstance(ent_coef, str) and ent_coef.startswith("auto")
        init_alpha = float(ent_coef.split("_")[1]) if self.ent_auto and "_" in ent_coef else (1.0 if self.ent_auto else float(ent_coef))
        on_gpu = self.device.type == "cuda"
        self.fused = bool(fused) and on_gpu
        self.use_hip_graph = bool(use_hip_graph) and self.fused
        dev = self.device
        self._alay, self._clay = actor_layout(D, self.H1, self.H2, A), critic_layout(self.K, self.H1, self.H2)

        # nn.Linear's default init, in SB3's construction order (actor, then critic; the target is a copy), drawn from a forked
        # RNG: constructing a learner leaves the caller's torch RNG as it was
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed)
            l1, l2, mu, ls = nn.Linear(D, self.H1), nn.Linear(self.H1, self.H2), nn.Linear(self.H2, A), nn.Linear(self.H2, A)
            actor = [l1.weight, l1.bias, l2.weight, l2.bias, torch.cat([mu.weight, ls.weight]), torch.cat([mu.bias, ls.bias])]
            qs = [[nn.Linear(self.K, self.H1), nn.Linear(self.H1, self.H2), nn.Linear(self.H2, 1)] for _ in range(2)]
        critic = [torch.stack([q[k // 2].weight if k % 2 == 0 else q[k // 2].bias for q in qs]) for k in range(6)]
        self.actor = torch.cat([t.detach().reshape(-1) for t in actor]).to(dev)
        self.critic = torch.cat([t.detach().reshape(-1) for t in critic]).to(dev)
        self.critic_target = self.critic.clone()
        z = lambda n: torch.zeros(n, device=dev)
        self.actor_m, self.actor_v, self.actor_s2 = z(self.actor.numel()), z(self.actor.numel()), z(ADAM_STATE_FLOATS)
        self.critic_m, self.critic_v, self.critic_s2 = z(self.critic.numel()), z(self.critic.numel()), z(ADAM_STATE_FLOATS)
        # sac_state (csrc/dm_sac.hip): log_ent_coef, its Adam m / v / step, alpha of the step, losses, mean log pi
        self.sac_state = z(16)
        self.sac_state[0] = math.log(init_alpha)
        self.policy = SacPolicy(self)

        # replay ring: [buffer_size // n_envs steps x n_envs] transitions (SB3 ReplayBuffer), position / fill on the device
        N = self.n_envs
        self.cap_steps = max(1, int(buffer_size) // N)
        rows = self.cap_steps * N
        self.ring = dict(obs=torch.zeros(rows, D, device=dev), act=torch.zeros(rows, A, device=dev), rew=z(rows), done=z(rows),
                         next_obs=torch.zeros(rows, D, device=dev))
        self.ring_state = torch.zeros(4, dtype=torch.int32, device=dev)     # pos, fill, ticket, finished episodes
        self.ep_acc, self.ep_hist = z(2 * N), z(2 * EP_HIST)
        self._ep_deque = collections.deque(maxlen=EP_HIST)                 # torch path (host)
        self.act_lo = torch.as_tensor(env.action_space.low, dtype=torch.float32, device=dev)
        self.act_hi = torch.as_tensor(env.action_space.high, dtype=torch.float32, device=dev)
        self._roll_ctr = torch.zeros(1, dtype=torch.int32, device=dev)
        self._learn_ctr = torch.zeros(1, dtype=torch.int32, device=dev)
        self._roll_seed = (0x5AC00000 + 7919 * seed) & 0x7FFFFFFFFFFFFFFF
        self._learn_seed = (0x5AC1EA12 + 104729 * seed) & 0x7FFFFFFFFFFFFFFF
        self._gen = torch.Generator(device=dev)
        self._gen.manual_seed(seed)
        self._last_obs = None                                              # raw: what the ring stores
        # with a normaliser: what the actor reads (normalize_obs of _last_obs as of the step that produced it), and where the
        # normalised reward of normalize_step_ goes (SAC uses the raw reward: the ring and the episode monitor)
        self._obs_norm = torch.zeros(N, D, device=dev) if normalizer is not None else None
        self._rew_scratch = z(N) if normalizer is not None else None
        self._graph_norm_key = None
        self._pos = self._fill = 0                                         # torch path mirrors of ring_state[0:2]
        self.num_timesteps = 0
        self._n_updates = 0
        self._graph = None
        self._fb = None
        self.stats = {}

    # ------------------------------------------------------------------ shared helpers
    def _call(self, name, *args):
        _lib.call(name, *args, device=self.device)

    @property
    def alpha(self):
        return float(self.sac_state[0].exp())

    def state_tensors(self):
        """Every tensor one gradient step reads or writes (for snapshots around a capture, and for tests)."""
        return [self.actor, self.critic, self.critic_target, self.actor_m, self.actor_v, self.actor_s2, self.critic_m, self.critic_v,
                self.critic_s2, self.sac_state, self._learn_ctr]

    # ------------------------------------------------------------------ acting + storing
    def _act_torch(self, obs, warmup, deterministic=False):
        N, A = obs.shape[0], self.act_dim
        lo, hi = self.act_lo, self.act_hi
        if warmup:
            act_env = lo + torch.rand(N, A, device=self.device, generator=self._gen) * (hi - lo)
            return 2.0 * ((act_env - lo) / (hi - lo)) - 1.0, act_env
        head = actor_head(self.policy.actor, obs)
        if deterministic:
            a = torch.tanh(head[:, :A])
        else:
            a, _ = squash(head, torch.randn(N, A, device=self.device, generator=self._gen))
        return a, lo + 0.5 * (a + 1.0) * (hi - lo)

    def store_torch(self, last_obs, act, out):
        """SB3 ReplayBuffer.add through _store_transition: next_obs of a finished env is its terminal observation; every done is a
        true terminal (the env sets no TimeLimit.truncated)."""
        N, R = self.n_envs, self.ring
        sl = slice(self._pos * N, (self._pos + 1) * N)
        done = out["done"].bool()
        R["obs"][sl] = last_obs
        R["act"][sl] = act
        R["rew"][sl] = out["rew"]
        R["done"][sl] = done.float()
        R["next_obs"][sl] = torch.where(done[:, None], out["terminal_obs"], out["obs"])
        self._pos = (self._pos + 1) % self.cap_steps
        self._fill = min(self._fill + 1, self.cap_steps)
        self.ring_state[0], self.ring_state[1] = self._pos, self._fill
        ret, ln = self.ep_acc[:N] + out["rew"], self.ep_acc[N:] + 1
        if bool(done.any()):
            self._ep_deque.extend(zip(ret[done].tolist(), ln[done].tolist()))
        self.ep_acc[:N] = torch.where(done, torch.zeros_like(ret), ret)
        self.ep_acc[N:] = torch.where(done, torch.zeros_like(ln), ln)

    def _fused_rollout_buffers(self):
        if getattr(self, "_rb", None) is None:
            N, dev = self.n_envs, self.device
            z = lambda *s: torch.zeros(*s, device=dev)
            self._rb = dict(h1=z(N, self.H1), h2=z(N, self.H2), head=z(N, 2 * self.act_dim), act=z(N, self.act_dim),
                            act_env=z(N, self.act_dim))
        return self._rb

    def _act_fused(self, obs, warmup, deterministic=False):
        rb, P = self._fused_rollout_buffers(), self.policy.actor
        N, A = obs.shape[0], self.act_dim
        if not warmup:
            self._call("dm_sac_linear_relu", obs, self.obs_dim, P["W1"], P["b1"], rb["h1"], N, self.H1, self.obs_dim, 1)
            torch.addmm(P["b2"], rb["h1"], P["W2"].t(), out=rb["h2"]).relu_()
            torch.addmm(P["bh"], rb["h2"], P["Wh"].t(), out=rb["head"])
        self._call("dm_sac_act", None if warmup else rb["head"], N, A, 2 * A, self._roll_seed, self._roll_ctr, 1 if warmup else 0,
                   1 if deterministic else 0, self.act_lo, self.act_hi, rb["act"], rb["act_env"])
        return rb["act"], rb["act_env"]

    def _store_fused(self, out):
        N, R = self.n_envs, self.ring
        self._call("dm_sac_store", N, self.obs_dim, self.act_dim, self.cap_steps, self._last_obs, self._rb["act"], out["rew"], out["done"],
                   out["obs"], out["terminal_obs"], R["obs"], R["act"], R["rew"], R["done"], R["next_obs"], self._last_obs,
                   self.ring_state, self._roll_ctr, self.ep_acc, self.ep_hist)

    def _norm_after_step(self, out):
        """SB3's VecNormalize.step_wait around the inner step SAC just made: statistics (when training, warm-up included) and the
        next normalised observation.  The inner env's tensors stay raw."""
        self.normalizer.normalize_step_(out["obs"], out["rew"], out["done"], None, self._obs_norm, self._rew_scratch, None)

    def env_step(self):
        """One vec-env step: act (uniform before learning_starts) + env.step_tensor + store.  With a normaliser the actor reads the
        normalised last observation and the ring still gets the raw one."""
        vn = self.normalizer
        if self._last_obs is None:
            if vn is None:
                self._last_obs = self.env.reset_tensor().clone().contiguous()
            else:
                self._obs_norm.copy_(vn.reset_tensor())
                self._last_obs = vn.out["obs_raw"].clone().contiguous()
        seen = self._last_obs if vn is None else self._obs_norm
        warmup = self.num_timesteps < self.learning_starts
        if self.fused:
            _, act_env = self._act_fused(seen, warmup)
            out = self.env.step_tensor(act_env)
            if vn is not None:
                self._norm_after_step(out)
            self._store_fused(out)
        else:
            with torch.no_grad():
                act, act_env = self._act_torch(seen, warmup)
                out = self.env.step_tensor(act_env)
                if vn is not None:
                    self._norm_after_step(out)
                self.store_torch(self._last_obs, act, out)
                self._last_obs = out["obs"].clone()
        self.num_timesteps += self.n_envs

    # ------------------------------------------------------------------ torch learner (SB3 SAC.train, one gradient step)
    def sample_torch(self, idx=None):
        """A minibatch of ring rows ``idx`` (drawn uniformly when None); with a normaliser, SB3's ReplayBuffer._get_samples:
        observations and rewards through the statistics of this moment, actions and done flags as stored."""
        if idx is None:
            idx = torch.randint(0, self._fill * self.n_envs, (self.batch_size,), device=self.device, generator=self._gen)
        R, vn = self.ring, self.normalizer
        if self.n_steps > 1:
            return self._sample_nstep_torch(idx)
        b = dict(obs=R["obs"][idx], act=R["act"][idx], rew=R["rew"][idx], next_obs=R["next_obs"][idx], done=R["done"][idx])
        if vn is not None:
            b.update(obs=vn._norm_obs_t(b["obs"]), next_obs=vn._norm_obs_t(b["next_obs"]), rew=vn._norm_rew_t(b["rew"]))
        return b

    def _sample_nstep_torch(self, idx):
        """The n-step minibatch of ring rows ``idx`` with torch ops (include/deepmimic_sac_nstep.h states the semantics): row i =
        (t, e) is followed over the steps (t + j) mod cap, j <= lim = min(n - 1, distance of t to the newest stored step), up to and
        including the first done; rewards are normalised one by one, then discounted; ``k`` is the number of rows used."""
        R, vn, N, cap, n, dev = self.ring, self.normalizer, self.n_envs, self.cap_steps, self.n_steps, self.device
        pos = int(self.ring_state[0])
        idx = torch.as_tensor(idx, device=dev).long()
        t, e = idx // N, idx % N
        j = torch.arange(n, device=dev)
        lim = torch.clamp((pos + cap - 1 - t) % cap, max=n - 1)[:, None]
        rows = torch.where(j <= lim, ((t[:, None] + j) % cap) * N + e[:, None], idx[:, None])      # past lim: never used
        stop = ((R["done"][rows] != 0) | (j == lim)) & (j <= lim)
        used = (stop.cumsum(1) - stop.long()) == 0          # up to and including the first stop
        k = used.sum(1)
        last = rows.gather(1, (k - 1)[:, None])[:, 0]
        r = R["rew"][rows] if vn is None else vn._norm_rew_t(R["rew"][rows])
        g = torch.full((n,), self.gamma, dtype=torch.float32, device=dev)
        pw = torch.cat([torch.ones(1, device=dev), g[:-1].cumprod(0)])     # gamma^j by fp32 products
        b = dict(obs=R["obs"][idx], act=R["act"][idx], rew=torch.where(used, pw * r, torch.zeros_like(r)).sum(1),
                 next_obs=R["next_obs"][last], done=1.0 - pw[k - 1] * (1.0 - R["done"][last]), k=k)
        if vn is not None:
            b.update(obs=vn._norm_obs_t(b["obs"]), next_obs=vn._norm_obs_t(b["next_obs"]))
        return b

    def gradient_step_torch(self, batch=None, eps_pi=None, eps_next=None):
        """SB3's order: alpha (before its step), alpha step, target, critic step, actor loss on the stepped critics, actor step,
        Polyak.  batch / eps may be given (tests); otherwise drawn from the learner's generator."""
        B, A, dev = self.batch_size, self.act_dim, self.device
        b = batch if batch is not None else self.sample_torch()
        B = b["obs"].shape[0]
        if eps_pi is None:
            eps_pi = torch.randn(B, A, device=dev, generator=self._gen)
        if eps_next is None:
            eps_next = torch.randn(B, A, device=dev, generator=self._gen)
        step = self._n_updates + 1
        st = self.sac_state
        actor = self.actor.detach().requires_grad_(True)
        Pa = arena_views(actor, self._alay)
        a_pi, logp = squash(actor_head(Pa, b["obs"]), eps_pi)
        alpha = st[0].detach().exp()
        log_alpha = st[0:1].detach().clone().requires_grad_(True)
        alpha_loss = -(log_alpha * (logp + self.target_entropy).detach()).mean()
        if self.ent_auto:
            (g_alpha,) = torch.autograd.grad(alpha_loss, log_alpha)
            adam_torch(st[0:1], g_alpha, st[1:2], st[2:3], step, self.lr)
            st[3] = step
        with torch.no_grad():
            a_next, logp_next = squash(actor_head(Pa, b["next_obs"]), eps_next)
            qt = q_values(self.policy.critic_target, torch.cat([b["next_obs"], a_next], 1))
            y = b["rew"] + (1 - b["done"]) * self.gamma * (qt.min(0).values - alpha * logp_next)
        critic = self.critic.detach().requires_grad_(True)
        q = q_values(arena_views(critic, self._clay), torch.cat([b["obs"], b["act"]], 1))
        critic_loss = 0.5 * sum(F.mse_loss(q[i], y) for i in range(2))
        (g_critic,) = torch.autograd.grad(critic_loss, critic)
        with torch.no_grad():
            adam_torch(self.critic, g_critic, self.critic_m, self.critic_v, step, self.lr)
        critic = self.critic.detach().requires_grad_(True)          # the stepped critics; their gradient is discarded
        q_pi = q_values(arena_views(critic, self._clay), torch.cat([b["obs"], a_pi], 1))
        actor_loss = (alpha * logp - torch.min(q_pi, dim=0).values).mean()
        (g_actor,) = torch.autograd.grad(actor_loss, actor)
        with torch.no_grad():
            adam_torch(self.actor, g_actor, self.actor_m, self.actor_v, step, self.lr)
            self.critic_target.mul_(1 - self.tau).add_(self.critic, alpha=self.tau)
            st[4], st[5], st[6], st[7], st[8] = alpha, alpha_loss.detach(), critic_loss.detach(), actor_loss.detach(), logp.mean()
        self.actor_s2[1] = step
        self.critic_s2[1] = step
        self._n_updates = step
        return dict(g_actor=g_actor, g_critic=g_critic)

    # ------------------------------------------------------------------ fused learner (csrc/dm_sac.hip + library GEMMs)
    def _fused_buffers(self):
        if self._fb is None:
            B, D, A, K, H1, H2, dev = self.batch_size, self.obs_dim, self.act_dim, self.K, self.H1, self.H2, self.device
            z = lambda *s: torch.zeros(*s, device=dev)
            self._fb = dict(obs2=z(2 * B, D), xq=z(B, K), xpi=z(B, K), xt=z(B, K), rew=z(B), done=z(B),
                            idx=torch.zeros(B, dtype=torch.int32, device=dev), k=torch.zeros(B, dtype=torch.int32, device=dev),
                            h1a=z(2 * B, H1), h2a=z(2 * B, H2), head=z(2 * B, 2 * A), logp=z(2 * B),
                            h1t=z(2, B, H1), h2t=z(2, B, H2), qt=z(2, B, 1), h1q=z(2, B, H1), h2q=z(2, B, H2), q=z(2, B, 1),
                            dq=z(2, B), dh2=z(2, B, H2), dh1=z(2, B, H1),
                            h1p=z(2, B, H1), h2p=z(2, B, H2), qp=z(2, B, 1), dqp=z(2, B), dh2p=z(2, B, H2), dh1p=z(2, B, H1),
                            dxp=z(2, B, K), dhead=z(B, 2 * A), dh2a=z(B, H2), dh1a=z(B, H1),
                            g_actor=z(self.actor.numel()), g_critic=z(self.critic.numel()))
        return self._fb

    def _critic_fwd(self, P, x, h1, h2, q):
        B, K = self.batch_size, self.K
        self._call("dm_sac_linear_relu", x, K, P["W1"], P["b1"], h1, B, 2 * self.H1, K, 2)
        torch.baddbmm(P["b2"].unsqueeze(1), h1, P["W2"].transpose(1, 2), out=h2).relu_()
        torch.baddbmm(P["b3"].unsqueeze(1), h2, P["W3"].transpose(1, 2), out=q)

    def gradient_step_fused(self):
        """One gradient step as a fixed launch sequence (no host read or write): what the captured graph holds."""
        call = self._call
        fb, B, D, A, K, H1, H2 = self._fused_buffers(), self.batch_size, self.obs_dim, self.act_dim, self.K, self.H1, self.H2
        seed, ctr, st = self._learn_seed, self._learn_ctr, self.sac_state
        Pa, Pc, Pt = self.policy.actor, self.policy.critic, self.policy.critic_target
        Ga, Gc = arena_views(fb["g_actor"], self._alay), arena_views(fb["g_critic"], self._clay)
        R = self.ring
        # 1. minibatch; with a normaliser the same rows, normalised inside the launch with the statistics it finds when it runs
        gather = (B, self.n_envs, D, A, seed, ctr, self.ring_state, R["obs"], R["act"], R["rew"], R["done"], R["next_obs"],
                  fb["obs2"], fb["xq"], fb["xpi"], fb["xt"], fb["rew"], fb["done"], fb["idx"])
        if self.n_steps > 1:                   # the n-step chain of every drawn row, in the same one launch
            call("dm_sac_gather_nstep", *gather, self.cap_steps, self.n_steps, self.gamma, fb["k"],
                 None if self.normalizer is None else ctypes.byref(self.normalizer._desc))
        elif self.normalizer is None:
            call("dm_sac_gather", *gather)
        else:
            call("dm_sac_gather_norm", *gather, ctypes.byref(self.normalizer._desc))
        # 2-4. one actor pass over (obs ; next_obs), squashed heads (a_pi, a'), alpha and its Adam step
        call("dm_sac_linear_relu", fb["obs2"], D, Pa["W1"], Pa["b1"], fb["h1a"], 2 * B, H1, D, 1)
        torch.addmm(Pa["b2"], fb["h1a"], Pa["W2"].t(), out=fb["h2a"]).relu_()
        torch.addmm(Pa["bh"], fb["h2a"], Pa["Wh"].t(), out=fb["head"])
        # a_pi and a' land in the action columns of xpi / xt (row stride K)
        call("dm_sac_head_fwd", fb["head"], 2 * B, B, A, seed, ctr, fb["xpi"][:, D:], fb["xt"][:, D:], K, fb["logp"], st,
             1 if self.ent_auto else 0, self.target_entropy, self.lr)
        # 5-6. target and critic loss
        self._critic_fwd(Pt, fb["xt"], fb["h1t"], fb["h2t"], fb["qt"])
        self._critic_fwd(Pc, fb["xq"], fb["h1q"], fb["h2q"], fb["q"])
        call("dm_sac_critic_loss", fb["q"], fb["qt"], fb["logp"][B:], fb["rew"], fb["done"], B, self.gamma, st, fb["dq"], Gc["b3"])
        dq3 = fb["dq"].view(2, B, 1)
        torch.bmm(dq3.transpose(1, 2), fb["h2q"], out=Gc["W3"])
        torch.bmm(dq3, Pc["W3"], out=fb["dh2"])
        call("dm_sac_relu_bwd_colsum", fb["dh2"], fb["h2q"], fb["dh2"], Gc["b2"], B, H2, 2)
        torch.bmm(fb["dh2"].transpose(1, 2), fb["h1q"], out=Gc["W2"])
        torch.bmm(fb["dh2"], Pc["W2"], out=fb["dh1"])
        call("dm_sac_relu_bwd_colsum", fb["dh1"], fb["h1q"], fb["dh1"], Gc["b1"], B, H1, 2)
        torch.bmm(fb["dh1"].transpose(1, 2), fb["xq"].expand(2, B, K), out=Gc["W1"])
        self._adam_fused(self.critic, fb["g_critic"], self.critic_m, self.critic_v, self.critic_s2)
        # 7. actor loss on the stepped critics: input gradients only
        self._critic_fwd(Pc, fb["xpi"], fb["h1p"], fb["h2p"], fb["qp"])
        call("dm_sac_actor_loss", fb["qp"], fb["logp"], B, st, fb["dqp"])
        torch.bmm(fb["dqp"].view(2, B, 1), Pc["W3"], out=fb["dh2p"])
        call("dm_sac_relu_bwd_colsum", fb["dh2p"], fb["h2p"], fb["dh2p"], None, B, H2, 2)
        torch.bmm(fb["dh2p"], Pc["W2"], out=fb["dh1p"])
        call("dm_sac_relu_bwd_colsum", fb["dh1p"], fb["h1p"], fb["dh1p"], None, B, H1, 2)
        torch.bmm(fb["dh1p"], Pc["W1"], out=fb["dxp"])
        # 8. squashed-Gaussian backward + actor backward + actor step
        call("dm_sac_head_bwd", fb["head"], B, A, seed, ctr, fb["dxp"], K, D, st, fb["dhead"], Ga["bh"])
        h1a, h2a = fb["h1a"][:B], fb["h2a"][:B]
        torch.mm(fb["dhead"].t(), h2a, out=Ga["Wh"])
        torch.mm(fb["dhead"], Pa["Wh"], out=fb["dh2a"])
        call("dm_sac_relu_bwd_colsum", fb["dh2a"], h2a, fb["dh2a"], Ga["b2"], B, H2, 1)
        torch.mm(fb["dh2a"].t(), h1a, out=Ga["W2"])
        torch.mm(fb["dh2a"], Pa["W2"], out=fb["dh1a"])
        call("dm_sac_relu_bwd_colsum", fb["dh1a"], h1a, fb["dh1a"], Ga["b1"], B, H1, 1)
        torch.mm(fb["dh1a"].t(), fb["obs2"][:B], out=Ga["W1"])
        self._adam_fused(self.actor, fb["g_actor"], self.actor_m, self.actor_v, self.actor_s2)
        # 9. Polyak; the learner's draw counter moves on
        call("dm_sac_polyak", self.critic, self.critic_target, self.critic.numel(), self.tau, ctr)

    def _adam_fused(self, w, g, m, v, s2):
        # max_norm = +inf: the clip coefficient of dm_flat_adam_step is exactly 1 (SB3's SAC does not clip)
        self._call("dm_flat_adam_step", w, g, m, v, w.numel(), self.lr, 0.9, 0.999, 1e-8, float("inf"), 1.0, s2, ADAM_STATE_FLOATS)

    def _capture(self):
        """Capture gradient_step_fused once.  The warm-up step (library handles, workspaces) runs on a side stream and is undone."""
        snap = [t.clone() for t in self.state_tensors()]
        self._graph_norm_key = self._norm_key()
        self._graph, _ = capture_graph(self.device, self.gradient_step_fused, warm=self.gradient_step_fused)
        with torch.no_grad():
            for t, s in zip(self.state_tensors(), snap):
                t.copy_(s)

    def _norm_key(self):
        """What dm_sac_gather_norm takes by value, so what a captured graph holds of the normaliser (its statistics it reads anew)."""
        vn = self.normalizer
        return None if vn is None else (vn.norm_obs, vn.norm_reward, vn.clip_obs, vn.clip_reward, vn.epsilon)

    def train(self, gradient_steps):
        for _ in range(gradient_steps):
            if self.fused:
                if self.use_hip_graph:
                    if self._graph is not None and self._graph_norm_key != self._norm_key():
                        self._graph = None                     # a flag, a clip or epsilon changed since the capture
                    if self._graph is None:
                        self._capture()
                    self._graph.replay()
                else:
                    self.gradient_step_fused()
            else:
                self.gradient_step_torch()
            self._n_updates += 1 if self.fused else 0

    # ------------------------------------------------------------------ SB3 surface
    def _refresh_stats(self):
        st = self.sac_state.tolist()
        if self.fused:
            n = int(self.ring_state[3])
            k = min(n, EP_HIST)
            hist = self.ep_hist.view(2, EP_HIST)[:, :k].cpu().numpy()
            rew, ln = (hist[0], hist[1]) if k else ([], [])
        else:
            rew, ln = [e[0] for e in self._ep_deque], [e[1] for e in self._ep_deque]
        self.stats.update(ep_rew_mean=float(np.mean(rew)) if len(rew) else float("nan"),
                          ep_len_mean=float(np.mean(ln)) if len(ln) else float("nan"),
                          ent_coef=st[4], ent_coef_loss=st[5], critic_loss=st[6], actor_loss=st[7], n_updates=self._n_updates,
                          total_timesteps=self.num_timesteps)

    def learn(self, total_timesteps, callback=None, log_interval=100):
        """SB3 OffPolicyAlgorithm.learn with train_freq = (1, step): per vec-env step one env step, then gradient_steps updates once
        more than learning_starts transitions were collected.  Every log_interval vec-env steps the stats are refreshed (one
        synchronisation) and ``callback(self)`` is called."""
        t0, steps, n0 = time.perf_counter(), 0, self.num_timesteps
        while self.num_timesteps < total_timesteps:
            for _ in range(self.train_freq):
                self.env_step()
            steps += 1
            if self.num_timesteps > self.learning_starts and self.gradient_steps > 0:
                self.train(self.gradient_steps)
            if log_interval and (steps % log_interval == 0 or self.num_timesteps >= total_timesteps):
                self._refresh_stats()
                self.stats["fps"] = (self.num_timesteps - n0) / max(time.perf_counter() - t0, 1e-9)
                if callback is not None and callback(self) is False:
                    break
        return self

    def predict(self, obs, deterministic=True):
        """Unscaled action for obs (tensor or array [n x D]), as PPO.predict returns it."""
        with torch.no_grad():
            o = torch.as_tensor(obs, dtype=torch.float32, device=self.device).reshape(-1, self.obs_dim)
            _, act_env = self._act_torch(o, False, deterministic=deterministic)
            return act_env

    def save(self, path):
        torch.save({"actor": self.actor, "critic": self.critic, "critic_target": self.critic_target, "sac_state": self.sac_state,
                    "adam": [self.actor_m, self.actor_v, self.critic_m, self.critic_v],
                    "arch": (self.obs_dim, self.act_dim, self.H1, self.H2), "n_updates": self._n_updates,
                    "num_timesteps": self.num_timesteps}, path)

    def load(self, path):
        ck = torch.load(path, map_location=self.device)
        if tuple(ck["arch"]) != (self.obs_dim, self.act_dim, self.H1, self.H2):
            raise ValueError("checkpoint architecture %s does not match %s" % (ck["arch"], (self.obs_dim, self.act_dim, self.H1, self.H2)))
        with torch.no_grad():
            for t, k in ((self.actor, "actor"), (self.critic, "critic"), (self.critic_target, "critic_target"), (self.sac_state, "sac_state")):
                t.copy_(ck[k])
            for t, s in zip([self.actor_m, self.actor_v, self.critic_m, self.critic_v], ck["adam"]):
                t.copy_(s)
            self._n_updates = int(ck["n_updates"])
            self.actor_s2[1] = self._n_updates
            self.critic_s2[1] = self._n_updates
        self.num_timesteps = int(ck["num_timesteps"])
        self._graph = None
        return self
