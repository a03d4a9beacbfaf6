"""CPU tests that pin the fp64 PPO reference (tests/ppo_ref64.py) the G1-shape kernel tests compare against, and the
dims of a PPO built without an env."""
import math

import pytest
import torch
import torch.nn as nn

import ppo_ref64 as R
from deepmimic_mujoco_amd.ppo import PPO, MlpPolicy


def _batch(B, D, A, pol, seed, spread=0.3):
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(B, D, generator=g) * 0.7
    with torch.no_grad():
        mean = pol.action_net(pol.pi(obs))
        act = mean + pol.log_std.exp() * torch.randn(B, A, generator=g)
        old_logp = pol._logp(act, mean) + spread * torch.randn(B, generator=g)      # ratios on both sides of the clip range
    adv = torch.randn(B, generator=g) * 2 + 0.3
    ret = torch.randn(B, generator=g)
    return obs, act, adv, ret, old_logp


@pytest.mark.parametrize("normalize,ent_coef", [(True, 0.0), (False, 0.01), (True, 0.01)])
def test_ref64_loss_and_gradients_equal_ppo_loss_torch(normalize, ent_coef):
    """The reference's loss and every gradient against PPO._loss_torch (fp32 autograd on the CPU modules) at the G1 shape
    (D = 98, A = 23).  fp32 rounding of a loss that sums B = 512 terms of O(1): ~1e-6 relative; measured 2e-7 on the loss
    and 3.0e-6 of the largest entry per gradient, asserted at 2e-5 (6x margin)."""
    torch.manual_seed(1)
    pol = MlpPolicy(obs_dim=98, act_dim=23, net_arch=(64, 32))
    with torch.no_grad():
        pol.log_std.copy_(torch.linspace(-0.8, 0.4, 23))
        pol.action_net.weight.mul_(20.0)
        for m in pol.modules():
            if isinstance(m, nn.Linear):
                m.bias.normal_(0, 0.1)
    ppo = PPO(None, policy=pol, device=torch.device("cpu"), batch_size=512, normalize_advantage=normalize, ent_coef=ent_coef,
              use_hip_graph=False)
    batch = _batch(512, 98, 23, pol, 2)
    loss32 = ppo._loss_torch(*batch)
    pol.zero_grad()
    loss32.backward()
    P = R.params64(pol)
    l64, out8, g64 = R.grads(P, *batch, clip_range=ppo.clip_range, vf_coef=ppo.vf_coef, ent_coef=ent_coef, normalize=normalize)
    assert 0.05 < float(out8[5]) < 0.95                                     # the clip is active for part of the batch
    assert abs(float(loss32.detach()) - float(l64)) < 2e-5 * max(1.0, abs(float(l64)))
    assert abs(float(out8[0] - (out8[1] + ppo.vf_coef * out8[2] - ent_coef * out8[3]))) < 1e-12
    for n, p in pol.named_parameters():
        scale = float(g64[n].abs().max())
        assert scale > 0, n
        assert float((p.grad.double() - g64[n]).abs().max()) < 2e-5 * scale, n


def test_ref64_entropy_logp_and_statistics_by_formula():
    """logp / entropy of the diagonal Gaussian and the out8 statistics (approx_kl, clip fraction, advantage moments) by their
    closed forms in fp64."""
    g = torch.Generator().manual_seed(3)
    A, B = 23, 100
    ls = torch.linspace(-1, 0.5, A, dtype=torch.float64)
    mean, act = torch.randn(B, A, generator=g, dtype=torch.float64), torch.randn(B, A, generator=g, dtype=torch.float64)
    d = torch.distributions.Normal(mean, ls.exp())
    assert torch.allclose(R.logp(act, mean, ls), d.log_prob(act).sum(-1), rtol=0, atol=1e-12)
    assert abs(float(R.entropy(ls)) - float(d.entropy()[0].sum())) < 1e-12
    torch.manual_seed(0)
    pol = MlpPolicy(obs_dim=5, act_dim=3, net_arch=(8, 8))
    obs, act, adv, ret, old = _batch(B, 5, 3, pol, 4, spread=0.5)
    P = R.params64(pol)
    _, out8 = R.loss(P, obs, act, adv, ret, old, clip_range=0.2)
    m, _ = R.heads(P, obs)
    lr = R.logp(act, m, P["log_std"]).detach() - old.double()
    r = lr.exp()
    assert abs(float(out8[4]) - float(((r - 1) - lr).mean())) < 1e-14
    assert float(out8[5]) == float(((r - 1).abs() > 0.2).double().mean())
    a = adv.double()
    assert abs(float(out8[6]) - float(a.mean())) < 1e-14
    assert abs(float(out8[7]) - 1 / (math.sqrt(float(((a - a.mean()) ** 2).sum()) / (B - 1)) + 1e-8)) < 1e-12
    _, out8 = R.loss(P, obs, act, adv, ret, old, normalize=False)
    assert float(out8[6]) == 0.0 and float(out8[7]) == 1.0


def test_ref64_update_equals_clip_grad_norm_plus_torch_adam_in_fp64():
    """Adam64 against nn.utils.clip_grad_norm_(0.5) + torch.optim.Adam(eps=1e-5) on fp64 parameters, six steps that alternate
    between clipped (norm >> 0.5) and unclipped gradients; both are fp64 and do the same operations in a different grouping:
    measured 6e-17, asserted at 1e-12."""
    torch.manual_seed(2)
    pol = MlpPolicy(obs_dim=98, act_dim=23, net_arch=(32, 32)).double()
    P = R.params64(pol)
    opt_t = torch.optim.Adam(pol.parameters(), lr=4e-4, eps=1e-5)
    opt_r = R.Adam64(sum(p.numel() for p in P.values()), lr=4e-4)
    g = torch.Generator().manual_seed(5)
    norms = []
    for it in range(6):
        gv = torch.randn(sum(p.numel() for p in P.values()), generator=g, dtype=torch.float64) * (1.0 if it % 2 else 1e-3)
        off = 0
        for p in pol.parameters():
            p.grad = gv[off:off + p.numel()].view_as(p).clone()
            off += p.numel()
        norms.append(float(nn.utils.clip_grad_norm_(pol.parameters(), 0.5)))
        opt_t.step()
        p = R.flat(P)
        opt_r.step(p, gv)
        R.unflat(P, p)
        mine = torch.cat([q.detach().reshape(-1) for q in pol.parameters()])
        assert float((mine - R.flat(P)).abs().max()) < 1e-12, it
    assert min(norms) < 0.5 < max(norms)
    st = [opt_t.state[q] for q in pol.parameters()]
    assert float((torch.cat([s["exp_avg"].reshape(-1) for s in st]) - opt_r.m).abs().max()) < 1e-15
    assert float((torch.cat([s["exp_avg_sq"].reshape(-1) for s in st]) - opt_r.v).abs().max()) < 1e-15


def test_ref64_train_equals_ppo_train_on_cpu():
    """ppo_ref64.train against PPO.train on the CPU (fp32 modules, torch.optim.Adam) for the same permutations: two epochs of
    four minibatches.  fp32 vs fp64 over eight Adam steps: measured 3e-4 of lr, asserted at 5 % of lr (a different minibatch
    order moves the weights by O(lr))."""
    torch.manual_seed(4)
    pol = MlpPolicy(obs_dim=85, act_dim=23, net_arch=(32, 32))
    ppo = PPO(None, policy=pol, device=torch.device("cpu"), batch_size=64, n_epochs=2, learning_rate=4e-4, use_hip_graph=False)
    P = R.params64(pol)
    T, N = 8, 32
    g = torch.Generator().manual_seed(6)
    buf = dict(obs=torch.randn(T, N, 85, generator=g), act=torch.randn(T, N, 23, generator=g) * 0.5,
               adv=torch.randn(T, N, generator=g), ret=torch.randn(T, N, generator=g), logp=torch.randn(T, N, generator=g) - 20)
    gen = torch.Generator().manual_seed(9)
    ppo.train(buf, generator=gen)
    gen = torch.Generator().manual_seed(9)
    perms = [torch.randperm(T * N, generator=gen) for _ in range(2)]
    flat = {k: v.reshape(-1, *v.shape[2:]) for k, v in buf.items()}
    R.train(P, flat, perms, 64, R.Adam64(sum(p.numel() for p in P.values()), lr=4e-4))
    for n, p in pol.named_parameters():
        assert float((p.detach().double() - P[n].detach()).abs().max()) < 0.05 * 4e-4, n


def test_ppo_without_env_takes_its_dims_from_the_policy():
    """PPO(None, policy=...) sizes the minibatch gather and the static buffers by the policy (obs 98 / 85, 23 actions for the
    G1); without env and policy the humanoid defaults 67 / 28 stay."""
    for D, A in ((98, 23), (85, 23), (72, 28)):
        ppo = PPO(None, policy=MlpPolicy(obs_dim=D, act_dim=A, net_arch=(32, 32)), device=torch.device("cpu"), batch_size=64)
        assert (ppo.obs_dim, ppo.act_dim) == (D, A)
        mb = ppo._static_minibatch()
        assert mb["obs"].shape == (64, D) and mb["act"].shape == (64, A)
    ppo = PPO(None, device=torch.device("cpu"))
    assert (ppo.obs_dim, ppo.act_dim) == (67, 28)
    assert ppo.policy.pi[0].in_features == 67 and ppo.policy.action_net.out_features == 28
