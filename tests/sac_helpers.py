"""Helpers of the SAC tests (not a conftest): a contextual-bandit tensor env, the uniform and gather draws of csrc/dm_sac.hip on
the hash of tests/kernel_helpers.py, and the conversion between the SAC arenas and the named fp64 state of tests/sac_ref64.py."""
import numpy as np
import torch

from kernel_helpers import hash32, normals  # noqa: F401 (normals: the pairs of dm_normal2, used by the SAC tests)

GATHER_TAG = 0xFFFF0000


class _Box:
    def __init__(self, low, high):
        self.low, self.high = np.asarray(low, np.float32), np.asarray(high, np.float32)
        self.shape = self.low.shape


class BanditEnv:
    """Contextual bandit with the step_tensor surface of HipDeepMimicVecEnv: obs uniform in [-1, 1]^D, every step ends the episode
    (done = 1, terminal_obs = the observation acted on), reward -mean_j (a_j - a*_j)^2 with a* = 0.8 tanh(W obs) inside the
    action box [lo, hi] = [-2, 2] x A.  The optimum is 0; a uniform random action scores about -(4/3 + mean a*^2)."""

    def __init__(self, n, D, A, device="cpu", seed=0, done_every=1):
        g = torch.Generator().manual_seed(seed)
        self.num_envs, self.D, self.A, self.device = n, D, A, torch.device(device)
        self.W = (torch.randn(A, D, generator=g) / np.sqrt(D)).to(self.device)
        self.observation_space = _Box(np.full(D, -1.0), np.full(D, 1.0))
        self.action_space = _Box(np.full(A, -2.0), np.full(A, 2.0))
        self.gen = torch.Generator(device=self.device).manual_seed(seed + 1)
        self.done_every, self.t = done_every, 0
        self.obs = self._draw()

    def _draw(self):
        return torch.rand(self.num_envs, self.D, device=self.device, generator=self.gen) * 2 - 1

    def optimal(self, obs):
        return 0.8 * torch.tanh(obs @ self.W.t())

    def reward(self, obs, act):
        return -((act - self.optimal(obs)) ** 2).mean(1)

    def reset_tensor(self):
        self.obs = self._draw()
        return self.obs

    def step_tensor(self, actions):
        self.t += 1
        rew = self.reward(self.obs, actions)
        done = torch.full((self.num_envs,), 1 if self.t % self.done_every == 0 else 0, dtype=torch.uint8, device=self.device)
        term = self.obs.clone()
        nxt = self._draw()
        self.obs = torch.where(done.bool()[:, None], nxt, self.obs + 0.01)
        return dict(obs=self.obs.contiguous(), rew=rew.contiguous(), done=done, terminal_obs=term.contiguous())


# ---- csrc/dm_sac.hip draws
def uniforms(seed, rows, ctr, A):
    return np.array([[(hash32(seed, r, ctr, j) >> 8) / 16777216.0 for j in range(A)] for r in range(rows)])


def gather_rows(seed, B, ctr, total):
    return np.array([(hash32(seed, r, ctr, GATHER_TAG) * total) >> 32 for r in range(B)])


# ---- SAC arenas <-> sac_ref64 state
def _named_actor(P, A, c):
    return dict(W1=c(P["W1"]), b1=c(P["b1"]), W2=c(P["W2"]), b2=c(P["b2"]), mu_W=c(P["Wh"][:A]), mu_b=c(P["bh"][:A]),
                ls_W=c(P["Wh"][A:]), ls_b=c(P["bh"][A:]))


def _named_critic(Q, i, c):
    return {k: c(Q[k][i]) for k in ("W1", "b1", "W2", "b2", "W3", "b3")}


def _cast(dtype, device):
    return lambda t: t.detach().to(device=device, dtype=dtype).clone()


def to_ref(sac, dtype=torch.float64, device="cpu"):
    c = _cast(dtype, device)
    S = {"actor": _named_actor(sac.policy.actor, sac.act_dim, c), "log_alpha": c(sac.sac_state[0:1])}
    for name, Q in (("qf", sac.policy.critic), ("tgt", sac.policy.critic_target)):
        for i in (0, 1):
            S["%s%d" % (name, i)] = _named_critic(Q, i, c)
    return S


def named_actor(sac, flat, dtype=torch.float64):
    """A flat actor-arena-shaped tensor (weights, gradient, Adam moment) by sac_ref64's names."""
    from deepmimic_mujoco_amd.sac import arena_views
    return _named_actor(arena_views(flat, sac._alay), sac.act_dim, _cast(dtype, "cpu"))


def named_critic(sac, flat, i, dtype=torch.float64):
    from deepmimic_mujoco_amd.sac import arena_views
    return _named_critic(arena_views(flat, sac._clay), i, _cast(dtype, "cpu"))


def opt_from(sac, dtype=torch.float64):
    """sac_ref64's Adam state from the learner's moments (and its Adam step count: actor_s2[1])."""
    na = lambda f: named_actor(sac, f, dtype)
    opt = {"actor": {k: {"m": m, "v": v} for (k, m), v in zip(na(sac.actor_m).items(), na(sac.actor_v).values())}}
    for i in (0, 1):
        m, v = named_critic(sac, sac.critic_m, i, dtype), named_critic(sac, sac.critic_v, i, dtype)
        opt["qf%d" % i] = {k: {"m": m[k], "v": v[k]} for k in m}
    st = sac.sac_state.detach().to("cpu", dtype)
    opt["log_alpha"] = {"m": st[1:2].clone(), "v": st[2:3].clone()}
    return opt, int(sac.actor_s2[1]) + 1


def flat_actor(d):
    """Named actor tensors (state or gradient) -> the arena's order."""
    return torch.cat([d["W1"].reshape(-1), d["b1"], d["W2"].reshape(-1), d["b2"], torch.cat([d["mu_W"], d["ls_W"]]).reshape(-1),
                      torch.cat([d["mu_b"], d["ls_b"]])])


def flat_critic(q0, q1):
    return torch.cat([torch.stack([q0[k], q1[k]]).reshape(-1) for k in ("W1", "b1", "W2", "b2", "W3", "b3")])


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))
