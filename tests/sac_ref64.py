"""fp64 reference of one SB3 ``SAC.train`` gradient step (test helper, not a conftest).

Plain ``torch.float64`` operations only (``F.linear``, ``relu``, autograd and a hand-written Adam): no ``deepmimic_mujoco_amd``
import and no ``dm_*`` call.  State is a dict of fp64 tensors by name:

  actor:  W1 [H1 x D], b1, W2 [H2 x H1], b2, mu_W [A x H2], mu_b, ls_W [A x H2], ls_b
  qf0 / qf1 and tgt0 / tgt1 (critic_target): W1 [H1 x (D + A)], b1, W2 [H2 x H1], b2, W3 [1 x H2], b3
  log_alpha: [1]
plus Adam moments per tensor.  SB3 2.x with the defaults src/sac_sb3.py leaves unset: Adam(lr, betas (0.9, 0.999), eps 1e-8)
for actor, critic (both critics) and log_ent_coef; tau, gamma as given; target_entropy = -A.
"""
import math

import torch
import torch.nn.functional as F

LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)
ACTOR = ["W1", "b1", "W2", "b2", "mu_W", "mu_b", "ls_W", "ls_b"]
CRITIC = ["W1", "b1", "W2", "b2", "W3", "b3"]


def actor_dist(S, obs):
    h = torch.relu(F.linear(obs, S["actor"]["W1"], S["actor"]["b1"]))
    h = torch.relu(F.linear(h, S["actor"]["W2"], S["actor"]["b2"]))
    mu = F.linear(h, S["actor"]["mu_W"], S["actor"]["mu_b"])
    log_std = torch.clamp(F.linear(h, S["actor"]["ls_W"], S["actor"]["ls_b"]), -20.0, 2.0)
    return mu, log_std


def sample(S, obs, eps):
    """(a = tanh(u), log pi) with u = mu + std eps: SB3's SquashedDiagGaussianDistribution."""
    mu, log_std = actor_dist(S, obs)
    std = torch.exp(log_std)
    u = mu + std * eps
    a = torch.tanh(u)
    logp = (-((u - mu) ** 2) / (2 * std ** 2) - torch.log(std) - LOG_SQRT_2PI).sum(-1)
    return a, logp - torch.log(1 - a ** 2 + 1e-6).sum(-1)


def q(C, obs, act):
    x = torch.cat([obs, act], 1)
    h = torch.relu(F.linear(x, C["W1"], C["b1"]))
    h = torch.relu(F.linear(h, C["W2"], C["b2"]))
    return F.linear(h, C["W3"], C["b3"])[:, 0]


def _adam(p, g, st, t, lr, b1=0.9, b2=0.999, eps=1e-8):
    st["m"] = b1 * st["m"] + (1 - b1) * g
    st["v"] = b2 * st["v"] + (1 - b2) * g * g
    return p - lr / (1 - b1 ** t) * st["m"] / (torch.sqrt(st["v"]) / math.sqrt(1 - b2 ** t) + eps)


def init_adam(S):
    """Zero moments for every trainable tensor of S."""
    z = lambda t: {"m": torch.zeros_like(t), "v": torch.zeros_like(t)}
    return {"actor": {k: z(v) for k, v in S["actor"].items()}, "qf0": {k: z(v) for k, v in S["qf0"].items()},
            "qf1": {k: z(v) for k, v in S["qf1"].items()}, "log_alpha": z(S["log_alpha"])}


def train_step(S, opt, t, batch, eps_pi, eps_next, lr=3e-4, gamma=0.99, tau=0.005, target_entropy=None, ent_auto=True):
    """One gradient step in place (S, opt), Adam step t (from 1).  batch: obs, act, rew, next_obs, done (fp64).  Returns the
    gradients and the scalars of the step."""
    A = batch["act"].shape[1]
    te = -float(A) if target_entropy is None else target_entropy
    leaf = lambda d: {k: v.detach().clone().requires_grad_(True) for k, v in d.items()}
    S["actor"] = leaf(S["actor"])
    a_pi, logp = sample(S, batch["obs"], eps_pi)
    la = S["log_alpha"].detach().clone().requires_grad_(True)
    alpha = torch.exp(la.detach())
    alpha_loss = -(la * (logp + te).detach()).mean()
    if ent_auto:
        (g_la,) = torch.autograd.grad(alpha_loss, la)
        S["log_alpha"] = _adam(S["log_alpha"], g_la, opt["log_alpha"], t, lr)
    with torch.no_grad():
        a_n, logp_n = sample(S, batch["next_obs"], eps_next)
        qt = torch.stack([q(S["tgt0"], batch["next_obs"], a_n), q(S["tgt1"], batch["next_obs"], a_n)], 1)
        nq = torch.min(qt, dim=1).values - alpha * logp_n
        y = batch["rew"] + (1 - batch["done"]) * gamma * nq
    S["qf0"], S["qf1"] = leaf(S["qf0"]), leaf(S["qf1"])
    cq = [q(S["qf0"], batch["obs"], batch["act"]), q(S["qf1"], batch["obs"], batch["act"])]
    critic_loss = 0.5 * sum(F.mse_loss(c, y) for c in cq)
    cparams = [S["qf0"][k] for k in CRITIC] + [S["qf1"][k] for k in CRITIC]
    gc = torch.autograd.grad(critic_loss, cparams)
    g_critic = {"qf0": dict(zip(CRITIC, gc[:6])), "qf1": dict(zip(CRITIC, gc[6:]))}
    for name in ("qf0", "qf1"):
        S[name] = {k: _adam(S[name][k].detach(), g_critic[name][k], opt[name][k], t, lr).requires_grad_(True) for k in CRITIC}
    q_pi = torch.stack([q(S["qf0"], batch["obs"], a_pi), q(S["qf1"], batch["obs"], a_pi)], 1)
    actor_loss = (alpha * logp - torch.min(q_pi, dim=1).values).mean()
    ga = torch.autograd.grad(actor_loss, [S["actor"][k] for k in ACTOR])
    g_actor = dict(zip(ACTOR, ga))
    S["actor"] = {k: _adam(S["actor"][k].detach(), g_actor[k], opt["actor"][k], t, lr) for k in ACTOR}
    with torch.no_grad():
        for i in (0, 1):
            S["qf%d" % i] = {k: v.detach() for k, v in S["qf%d" % i].items()}
            S["tgt%d" % i] = {k: S["tgt%d" % i][k] * (1 - tau) + tau * S["qf%d" % i][k] for k in CRITIC}
    return dict(g_actor=g_actor, g_critic=g_critic, alpha=float(alpha), alpha_loss=float(alpha_loss.detach()), critic_loss=float(critic_loss.detach()),
                actor_loss=float(actor_loss.detach()), logp=logp.detach(), a_pi=a_pi.detach(), a_next=a_n, logp_next=logp_n, y=y)
