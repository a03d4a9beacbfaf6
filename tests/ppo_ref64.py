"""fp64 reference of SB3's PPO update for an ``MlpPolicy`` (test helper, not a conftest).

Plain ``torch.float64`` operations only (``F.linear``, ``tanh``, autograd): no ``MlpPolicy.forward``, no ``HipLinear`` and no
``dm_*`` call, so that a kernel test compares the project's code with something that shares none of it.  Parameters are a
dict ``name -> fp64 leaf`` in ``policy.named_parameters()`` order (the order of ``FlatAdam``'s flat buffer).
"""
import math

import torch
import torch.nn.functional as F

LOG_2PI = math.log(2.0 * math.pi)


def params64(policy, device="cpu", dtype=torch.float64):
    """Double copies of the policy's parameters (leaves that require grad), by name."""
    return {n: p.detach().to(device=device, dtype=dtype).clone().requires_grad_(True) for n, p in policy.named_parameters()}


def _layers(P, prefix):
    idx = sorted({int(n.split(".")[1]) for n in P if n.startswith(prefix + ".")})
    return [(P["%s.%d.weight" % (prefix, i)], P["%s.%d.bias" % (prefix, i)]) for i in idx]


def trunk(P, prefix, x):
    for w, b in _layers(P, prefix):
        x = torch.tanh(F.linear(x, w, b))
    return x


def heads(P, obs):
    """(mean [B, A], value [B]) of both trunks."""
    obs = obs.to(P["log_std"])
    mean = F.linear(trunk(P, "pi", obs), P["action_net.weight"], P["action_net.bias"])
    value = F.linear(trunk(P, "vf", obs), P["value_net.weight"], P["value_net.bias"]).squeeze(-1)
    return mean, value


def logp(act, mean, log_std):
    """log-density of the diagonal Gaussian, summed over the actions."""
    z = (act.to(mean) - mean) * torch.exp(-log_std)
    return (-0.5 * z * z - log_std - 0.5 * LOG_2PI).sum(-1)


def entropy(log_std):
    return (0.5 + 0.5 * LOG_2PI + log_std).sum()


def head_loss(mean, log_std, value, act, adv, ret, old_logp, clip_range=0.2, vf_coef=0.5, ent_coef=0.0, normalize=True):
    """SB3 PPO.train's minibatch loss from the heads (mean [B, A], log_std [A], value [B]).  Returns (loss, out8) with out8 as the
    kernels' record: {loss, policy_loss, value_loss, entropy, approx_kl, clip_fraction, adv_mean, 1 / (adv_std + 1e-8)}
    (adv_mean = 0 and 1 for the last two when the advantages are not normalised)."""
    d = log_std
    adv, ret, old_logp = adv.to(d), ret.to(d), old_logp.to(d)
    B = adv.shape[0]
    if normalize and B > 1:
        am, inv = adv.mean(), 1.0 / (adv.std() + 1e-8)          # unbiased std, as torch.Tensor.std
    else:
        am, inv = torch.zeros((), dtype=d.dtype, device=d.device), torch.ones((), dtype=d.dtype, device=d.device)
    a_n = (adv - am) * inv
    lp = logp(act, mean, log_std)
    log_ratio = lp - old_logp
    ratio = torch.exp(log_ratio)
    pg = -torch.min(a_n * ratio, a_n * torch.clamp(ratio, 1 - clip_range, 1 + clip_range)).mean()
    vl = F.mse_loss(ret, value)
    ent = entropy(log_std)
    total = pg + vf_coef * vl - ent_coef * ent
    with torch.no_grad():
        kl = ((ratio - 1) - log_ratio).mean()
        cf = ((ratio - 1).abs() > clip_range).to(d.dtype).mean()
        out8 = torch.stack([total.detach(), pg.detach(), vl.detach(), ent.detach(), kl, cf, am.detach(), inv.detach()])
    return total, out8


def loss(P, obs, act, adv, ret, old_logp, **kw):
    """head_loss of the policy P on the minibatch (obs, act, adv, ret, old_logp)."""
    mean, value = heads(P, obs)
    return head_loss(mean, P["log_std"], value, act, adv, ret, old_logp, **kw)


def grads(P, *batch, **kw):
    """(loss, out8, {name: d loss / d param}) of one minibatch."""
    total, out8 = loss(P, *batch, **kw)
    names = list(P)
    g = torch.autograd.grad(total, [P[n] for n in names], allow_unused=True)
    return total.detach(), out8, {n: (torch.zeros_like(P[n]) if gi is None else gi) for n, gi in zip(names, g)}


class Adam64:
    """clip_grad_norm_(max_norm) + torch.optim.Adam (betas, eps, bias correction, no weight decay) on the flat fp64 vector of
    all parameters; ``grad_scale`` multiplies the gradient first (the 1 / world of the data-parallel learner)."""

    def __init__(self, n, lr, betas=(0.9, 0.999), eps=1e-5, max_grad_norm=0.5, dtype=torch.float64, device="cpu"):
        self.lr, self.betas, self.eps, self.max_grad_norm = lr, betas, eps, max_grad_norm
        self.m = torch.zeros(n, dtype=dtype, device=device)
        self.v = torch.zeros(n, dtype=dtype, device=device)
        self.t = 0

    def step(self, p, g, grad_scale=1.0):
        """In place on the flat parameter vector p; returns the clipped gradient's pre-clip norm."""
        g = g * grad_scale
        norm = torch.linalg.vector_norm(g)
        g = g * torch.clamp(self.max_grad_norm / (norm + 1e-6), max=1.0)
        b1, b2 = self.betas
        self.t += 1
        self.m.mul_(b1).add_(g, alpha=1 - b1)
        self.v.mul_(b2).addcmul_(g, g, value=1 - b2)
        bc1, bc2 = 1 - b1 ** self.t, 1 - b2 ** self.t
        p.sub_(self.lr / bc1 * self.m / (self.v.sqrt() / math.sqrt(bc2) + self.eps))
        return float(norm)


def flat(P):
    return torch.cat([P[n].detach().reshape(-1) for n in P])


def unflat(P, vec):
    off = 0
    with torch.no_grad():
        for n in P:
            k = P[n].numel()
            P[n].copy_(vec[off:off + k].view_as(P[n]))
            off += k


def train(P, buf, perms, batch_size, opt, clip_range=0.2, vf_coef=0.5, ent_coef=0.0, normalize=True):
    """SB3 PPO.train over the flattened buffer ``buf`` (obs, act, adv, ret, logp), one epoch per permutation in ``perms``, minibatches
    perm[s:s + batch_size]; updates P in place with ``opt`` (an Adam64).  Returns the mean minibatch loss."""
    losses = []
    for perm in perms:
        perm = perm.to(buf["obs"].device)
        for s in range(0, perm.numel(), batch_size):
            i = perm[s:s + batch_size]
            l, _, g = grads(P, buf["obs"][i], buf["act"][i], buf["adv"][i], buf["ret"][i], buf["logp"][i], clip_range=clip_range,
                            vf_coef=vf_coef, ent_coef=ent_coef, normalize=normalize)
            p = flat(P)
            opt.step(p, torch.cat([g[n].reshape(-1) for n in P]))
            unflat(P, p)
            losses.append(float(l))
    return sum(losses) / max(len(losses), 1)
