"""The policy and learner kernels at the shapes of the reference's Unitree G1 setup (obs 98 / 85, 23 actions, [256,128],
minibatch 4096, lr 4e-4, fp32) against the fp64 reference of SB3's PPO update (tests/ppo_ref64.py).

Odd A = 23 is where the kernels special-case: the half-used last Box-Muller pair, the 32-wide action tile with 9 padding
columns, zero-padded packed weights (D 98 -> 104, 85 -> 88), two gathered rows per block.  Tolerances are fp32 error
bounds, none looser than the A = 28 counterpart in test_gpu_env.py; each docstring states the bound and the worst error
measured on an MI355X.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

import ppo_ref64 as R
from kernel_helpers import DEV, GUARD, normals  # noqa: F401
from kernel_helpers import check_out8 as _check_out8, guard_ok as _guard_ok, guarded as _guarded, lib as _lib, note as _note, ptr as _p, stream as _stream

pytestmark = pytest.mark.gpu

A = 23


def _eps64(seed, ctr, N):
    """fp64 draws [N, A] of (seed, env, counter, action index); the last pair of the odd A half used."""
    return torch.tensor(normals(seed, N, ctr, A), device=DEV)


def _g1_bounds():
    from deepmimic_mujoco_amd.g1 import load_g1_model
    g, _ = load_g1_model()                                                 # cached
    cr = np.asarray(g.act_ctrlrange, dtype=np.float64)[:A] / 20.0          # DPCombinedEnv: ctrlrange / ACT_SCALE
    return (torch.tensor(cr[:, 0], dtype=torch.float32, device=DEV), torch.tensor(cr[:, 1], dtype=torch.float32, device=DEV))


def _asym_bounds():
    """lo != -hi in every column, some bounds entirely on one side of zero."""
    lo = torch.linspace(-3.0, -0.1, A, device=DEV)
    hi = torch.linspace(0.25, 2.5, A, device=DEV).flip(0)
    lo[5], hi[5] = 0.3, 1.7
    lo[17], hi[17] = -2.2, -0.4
    return lo, hi


def _policy(D, arch, seed, bounds=None):
    from deepmimic_mujoco_amd.ppo import MlpPolicy
    torch.manual_seed(seed)
    pol = MlpPolicy(obs_dim=D, act_dim=A, net_arch=arch).to(DEV)
    with torch.no_grad():
        pol.log_std.copy_(torch.linspace(-1.0, 0.5, A))
        for m in pol.modules():
            if isinstance(m, nn.Linear):
                m.bias.normal_(0, 0.1)
        if bounds is not None:
            # per column: means centred on 0 with a spread of 2 x the widest bound, so that every column clamps at both ends
            obs = torch.randn(4096, D, device=DEV) * 0.7
            m0, _ = R.heads(R.params64(pol, DEV), obs)
            s = 2.0 * bounds / m0.std(0).float()
            pol.action_net.weight.mul_(s[:, None])
            pol.action_net.bias.copy_(-s * (m0.mean(0).float() - pol.action_net.bias))
    return pol


# ------------------------------------------------------------------------------------------------ dm_policy_forward
@pytest.mark.parametrize("arch,D,N", [((256, 128), 98, 4096), ((256, 128), 98, 4095), ((256, 128), 98, 33), ((256, 128), 98, 1),
                                      ((256, 128), 85, 4096), ((256, 128), 85, 4095), ((256, 128), 85, 33), ((256, 128), 85, 1),
                                      ((96, 160), 98, 4095), ((96, 160), 85, 33)])
def test_policy_forward_at_g1_shapes(arch, D, N):
    """dm_policy_forward, A = 23, with the G1 bounds and an asymmetric set, against fp64: mean / value within 2e-5 x max(1, |ref|)
    (fp32 GEMM of K <= 256; the A = 28 test's bound; measured margin >= 37x), the sampled action = mean + exp(log_std) x the fp64
    Box-Muller draw of the same hash within 1e-6 x max(1, |act|) + 8e-6 (fp32 expf / logf / sincosf of a few ulp on |eps| <= 5.6,
    margin >= 14x), logp of the fp64 draws within 3e-4 (A = 28 bound; margin >= 46x), act_env = clamp(act, lo[c], hi[c]) bit
    for bit with every column clamped at both ends, the dm_policy_sample draw for the same (seed, counter), the deterministic
    head; every output is a view in a NaN buffer whose guard region must stay NaN."""
    from deepmimic_mujoco_amd.ppo import FusedPolicyForward
    bset = [_g1_bounds(), _asym_bounds()]
    wide = torch.maximum(torch.maximum(bset[0][0].abs(), bset[0][1].abs()), torch.maximum(bset[1][0].abs(), bset[1][1].abs()))
    pol = _policy(D, arch, 3 + D + N, bounds=wide)
    assert FusedPolicyForward.supported(pol, DEV)
    fwd = FusedPolicyForward(pol, DEV)
    fwd.pack()
    obs = torch.randn(N, D, device=DEV) * 0.7
    P = R.params64(pol, DEV)
    with torch.no_grad():
        m64, v64 = R.heads(P, obs)
    ls64 = P["log_std"].detach()
    seed, ctr0, off = 987654321, 5, 3
    eps = _eps64(seed, ctr0 + off, N)
    (bm, mean), (ba, act), (be, act_env), (bl, logp), (bv, val), (bo, ocopy) = (
        _guarded(N, A), _guarded(N, A), _guarded(N, A), _guarded(N), _guarded(N), _guarded(N, D))
    ctr = torch.tensor([ctr0], dtype=torch.int32, device=DEV)
    for lo, hi in bset:
        fwd(obs, seed, ctr, off, lo, hi, act, act_env, logp, val, obs_copy=ocopy, mean_out=mean)
        torch.cuda.synchronize()
        assert all(_guard_ok(b, v) for b, v in ((bm, mean), (ba, act), (be, act_env), (bl, logp), (bv, val), (bo, ocopy)))
        assert torch.isfinite(mean).all() and torch.isfinite(act).all() and torch.isfinite(logp).all() and torch.isfinite(val).all()
        tm, tv = 2e-5 * max(1.0, float(m64.abs().max())), 2e-5 * max(1.0, float(v64.abs().max()))
        assert _note("policy_forward mean", float((mean.double() - m64).abs().max()), tm) < tm
        assert _note("policy_forward value", float((val.double() - v64).abs().max()), tv) < tv
        assert torch.equal(ocopy, obs)
        act64 = mean.double() + ls64.exp() * eps
        ta = 1e-6 * max(1.0, float(act64.abs().max())) + 8e-6
        assert _note("policy_forward act", float((act.double() - act64).abs().max()), ta) < ta
        lp64 = (-0.5 * eps * eps - ls64 - 0.5 * R.LOG_2PI).sum(-1)
        assert _note("policy_forward logp", float((logp.double() - lp64).abs().max()), 3e-4) < 3e-4
        assert torch.equal(act_env, torch.clamp(act, lo, hi))
        if N >= 4095:
            assert bool((act_env == lo).any(0).all()) and bool((act_env == hi).any(0).all())
        # dm_policy_sample on the kernel's mean, counter[0] = ctr0 + off: the same draws
        (b2, a2), (b3, e2), (b4, l2) = _guarded(N, A), _guarded(N, A), _guarded(N)
        c8 = torch.tensor([ctr0 + off], dtype=torch.int32, device=DEV)
        rc = _lib().dm_policy_sample(_p(mean), _p(pol.log_std), N, A, C.c_uint64(seed), _p(c8), _p(lo), _p(hi), _p(a2), _p(e2), _p(l2),
                                     _stream())
        assert rc == 0
        torch.cuda.synchronize()
        assert _guard_ok(b2, a2) and _guard_ok(b3, e2) and _guard_ok(b4, l2)
        assert torch.allclose(a2, act, rtol=2.0 ** -22, atol=1e-6) and torch.allclose(l2, logp, atol=3e-4)
        assert torch.equal(e2, torch.clamp(a2, lo, hi))
    # deterministic head: act = mean, logp of eps = 0
    fwd(obs, seed, ctr, 0, bset[0][0], bset[0][1], act, act_env, logp, val, deterministic=True)
    torch.cuda.synchronize()
    assert _guard_ok(ba, act) and _guard_ok(be, act_env) and _guard_ok(bl, logp)
    assert float((act.double() - m64).abs().max()) < 2e-5 * max(1.0, float(m64.abs().max()))
    assert float((logp.double() - (-ls64 - 0.5 * R.LOG_2PI).sum()).abs().max()) < 3e-4
    assert torch.equal(act_env, torch.clamp(act, bset[0][0], bset[0][1]))


def test_policy_forward_unpaired_last_action_is_standard_normal():
    """Column 22 takes the cosine half of a Box-Muller pair whose sine half is unused: over 16 draw counters x 4096 envs its eps
    has mean 0, std 1, skewness 0 and kurtosis 3 within ~5 standard errors (0.02, 0.015, 0.05, 0.1), and is uncorrelated with
    column 21 (|r| < 0.02) and with itself at the next counter."""
    from deepmimic_mujoco_amd.ppo import FusedPolicyForward
    N = 4096
    pol = _policy(98, (256, 128), 17)
    fwd = FusedPolicyForward(pol, DEV)
    fwd.pack()
    obs = torch.randn(N, 98, device=DEV) * 0.7
    z = lambda *s: torch.zeros(*s, device=DEV)
    mean, act, act_env, logp, val = z(N, A), z(N, A), z(N, A), z(N), z(N)
    lo, hi = torch.full((A,), -1e30, device=DEV), torch.full((A,), 1e30, device=DEV)
    ctr = torch.zeros(1, dtype=torch.int32, device=DEV)
    eps = []
    for k in range(16):
        fwd(obs, 42, ctr, k, lo, hi, act, act_env, logp, val, mean_out=mean)
        eps.append(((act.double() - mean.double()) / pol.log_std.detach().double().exp()).clone())
    E = torch.stack(eps)                        # [16, N, A]
    e22, e21 = E[:, :, 22].reshape(-1), E[:, :, 21].reshape(-1)
    assert abs(float(e22.mean())) < 0.02 and abs(float(e22.std()) - 1) < 0.015
    assert abs(float((e22 ** 3).mean())) < 0.05 and abs(float((e22 ** 4).mean()) - 3) < 0.1
    assert abs(float(torch.corrcoef(torch.stack([e21, e22]))[0, 1])) < 0.02
    assert abs(float((E[:-1, :, 22] * E[1:, :, 22]).mean())) < 0.02


# ------------------------------------------------------------------------------------------------ dm_policy_sample / dm_rollout_store
@pytest.mark.parametrize("N", [4096, 4095])
def test_policy_sample_and_rollout_store_at_g1_shapes(N):
    """dm_policy_sample at A = 23 with the G1 bounds: the action is mean + exp(log_std) x the fp64 draw (1e-6 relative + 8e-6; margin
    >= 11x), logp of the fp64 draws within 3e-4 (the A = 28 bound; margin >= 38x), act_env clamped per column bit for bit; dm_rollout_store at
    D = 98: every store bit-exact, the counter advanced by one, nothing written behind the last row."""
    lo, hi = _g1_bounds()
    D = 98
    g = torch.Generator(device=DEV); g.manual_seed(8)
    mean = torch.randn(N, A, device=DEV, generator=g) * 3.0
    log_std = torch.linspace(-1.2, 0.6, A, device=DEV)
    ctr = torch.tensor([77], dtype=torch.int32, device=DEV)
    (ba, act), (be, act_env), (bl, logp) = _guarded(N, A), _guarded(N, A), _guarded(N)
    rc = _lib().dm_policy_sample(_p(mean), _p(log_std), N, A, C.c_uint64(2024), _p(ctr), _p(lo), _p(hi), _p(act), _p(act_env), _p(logp),
                                 _stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert _guard_ok(ba, act) and _guard_ok(be, act_env) and _guard_ok(bl, logp)
    eps = _eps64(2024, 77, N)
    ls64 = log_std.double()
    act64 = mean.double() + ls64.exp() * eps
    ta = 1e-6 * max(1.0, float(act64.abs().max())) + 8e-6
    assert _note("policy_sample act", float((act.double() - act64).abs().max()), ta) < ta
    assert _note("policy_sample logp", float((logp.double() - (-0.5 * eps * eps - ls64 - 0.5 * R.LOG_2PI).sum(-1)).abs().max()), 3e-4) < 3e-4
    assert torch.equal(act_env, torch.clamp(act, lo, hi))
    assert bool((act_env == lo).any(0).all()) and bool((act_env == hi).any(0).all())
    last = torch.randn(N, D, device=DEV, generator=g)
    new = torch.randn(N, D, device=DEV, generator=g)
    val, rew = torch.randn(N, device=DEV, generator=g), torch.randn(N, device=DEV, generator=g)
    done = (torch.rand(N, device=DEV, generator=g) < 0.3).to(torch.uint8)
    (b0, bo), (b1, bac), (b2, bv), (b3, bl_), (b4, br), (b5, bd), (b6, lo_out) = (
        _guarded(N, D), _guarded(N, A), _guarded(N), _guarded(N), _guarded(N), _guarded(N), _guarded(N, D))
    rc = _lib().dm_rollout_store(N, D, A, _p(last), _p(act), _p(val), _p(logp), _p(rew), _p(done), _p(new), _p(bo), _p(bac), _p(bv),
                                 _p(bl_), _p(br), _p(bd), _p(lo_out), _p(ctr), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert all(_guard_ok(b, v) for b, v in ((b0, bo), (b1, bac), (b2, bv), (b3, bl_), (b4, br), (b5, bd), (b6, lo_out)))
    assert torch.equal(bo, last) and torch.equal(bac, act) and torch.equal(bv, val) and torch.equal(bl_, logp)
    assert torch.equal(br, rew) and torch.equal(bd, done.float()) and torch.equal(lo_out, new)
    assert int(ctr[0]) == 78


# ------------------------------------------------------------------------------------------------ dm_ppo_mlp_grad
def _minibatch(pol, D, B, seed):
    g = torch.Generator(device=DEV); g.manual_seed(seed)
    with torch.no_grad():
        obs = torch.randn(B, D, device=DEV, generator=g) * 0.7
        mean = pol.action_net(pol.pi(obs))
        act = mean + pol.log_std.exp() * torch.randn(B, A, device=DEV, generator=g)
        old_logp = pol._logp(act, mean) + 0.15 * torch.randn(B, device=DEV, generator=g)       # ratios straddle [0.8, 1.2]
        adv = torch.randn(B, device=DEV, generator=g) * 2 + 0.3
        ret = torch.randn(B, device=DEV, generator=g)
    return obs, act, adv, ret, old_logp


@pytest.mark.parametrize("D,B,normalize,ent", [(98, 4096, True, 0.0), (98, 4096, False, 0.01), (98, 4096, True, 0.01), (98, 4096, False, 0.0),
                                               (85, 4096, True, 0.01), (98, 512, False, 0.0), (85, 512, True, 0.0), (98, 64, True, 0.01),
                                               (85, 64, False, 0.0)])
def test_fused_mlp_grad_at_g1_shapes(D, B, normalize, ent):
    """dm_ppo_mlp_grad through FusedMlpGrad ([256,128], A = 23) against the fp64 reference: loss and out8 statistics (see
    _check_out8), every parameter gradient incl. each of the 23 log_std entries within 3e-4 of the tensor's largest entry (the A = 28
    bound; fp32 sums over B; measured margin >= 98x; out8 terms >= 60x), on a minibatch whose ratios straddle the clip range."""
    from deepmimic_mujoco_amd.ppo import PPO, FusedMlpGrad
    pol = _policy(D, (256, 128), 7)
    with torch.no_grad():
        pol.action_net.weight.mul_(20.0)
    ppo = PPO(None, policy=pol, device=DEV, batch_size=B, ent_coef=ent, normalize_advantage=normalize, use_hip_graph=False)
    assert (ppo.obs_dim, ppo.act_dim) == (D, A)
    batch = _minibatch(pol, D, B, 100 + B)
    P = R.params64(pol, DEV)
    l64, ref8, g64 = R.grads(P, *batch, clip_range=ppo.clip_range, vf_coef=ppo.vf_coef, ent_coef=ent, normalize=normalize)
    with torch.no_grad():
        m64, _ = R.heads(P, batch[0])
        ratio64 = torch.exp(R.logp(batch[1], m64, P["log_std"]) - batch[4].double())
    assert 0.05 < float(ref8[5]) < 0.95
    assert FusedMlpGrad.supported(pol, B)
    opt = ppo.optimizer
    opt.zero_grad()
    mg = FusedMlpGrad(pol, opt, B)
    loss = mg(*batch, ppo.clip_range, ppo.vf_coef, ent, normalize)
    torch.cuda.synchronize()
    assert abs(float(loss) - float(l64)) < 2e-5 * max(1.0, abs(float(l64)))
    _check_out8(mg.out8, ref8, ratio64, ppo.clip_range, B)
    names = {id(p): n for n, p in pol.named_parameters()}
    for p, g in zip(opt.params, opt.slices):
        n = names[id(p)]
        r = g64[n]
        scale = float(r.abs().max())
        assert scale > 0, n
        assert _note("mlp_grad d/d " + n, float((g.double() - r).abs().max()), 3e-4 * scale) < 3e-4 * scale, n
    gl = opt.slices[[id(q) for q in opt.params].index(id(pol.log_std))]
    assert gl.numel() == A and bool(((gl.double() - g64["log_std"]).abs() < 3e-4 * float(g64["log_std"].abs().max())).all())


# ------------------------------------------------------------------------------------------------ dm_ppo_loss
@pytest.mark.parametrize("B,normalize", [(4096, True), (257, False), (257, True)])
def test_fused_ppo_loss_at_a23(B, normalize):
    """dm_ppo_loss through FusedPPOLoss.raw (the loss of the library-GEMM learner), A = 23: loss / out8 (see _check_out8), d loss / d
    mean, d value and d log_std within 2e-5 of each tensor's largest entry (the A = 28 bound; measured margin >= 6.6x)."""
    from deepmimic_mujoco_amd.ppo import FusedPPOLoss
    g = torch.Generator(device=DEV); g.manual_seed(B)
    mean = torch.randn(B, A, device=DEV, generator=g) * 2
    log_std = torch.linspace(-0.7, 0.4, A, device=DEV)
    value = torch.randn(B, device=DEV, generator=g)
    act = mean + log_std.exp() * torch.randn(B, A, device=DEV, generator=g)
    m64, ls64, v64 = (t.double().requires_grad_(True) for t in (mean, log_std, value))
    with torch.no_grad():
        old_logp = (R.logp(act, m64, ls64) + 0.15 * torch.randn(B, device=DEV, generator=g, dtype=torch.float64)).float()
    adv = torch.randn(B, device=DEV, generator=g) * 2 + 0.3
    ret = torch.randn(B, device=DEV, generator=g)
    l64, ref8 = R.head_loss(m64, ls64, v64, act, adv, ret, old_logp, clip_range=0.2, vf_coef=0.5, ent_coef=0.01, normalize=normalize)
    gm64, gl64, gv64 = torch.autograd.grad(l64, [m64, ls64, v64])
    with torch.no_grad():
        ratio64 = torch.exp(R.logp(act, m64, ls64) - old_logp.double())
    assert 0.05 < float(ref8[5]) < 0.95
    gls = torch.full((A + GUARD,), float("nan"), device=DEV)
    loss, gm, gv = FusedPPOLoss.raw(mean, log_std, value, act, old_logp, adv, ret, 0.2, 0.5, 0.01, normalize, grad_log_std=gls[:A])
    torch.cuda.synchronize()
    assert bool(torch.isnan(gls[A:]).all())
    out8 = FusedPPOLoss.buffers(B, A, DEV)["out"]
    assert abs(float(loss) - float(l64.detach())) < 1e-5 * max(1.0, abs(float(l64.detach())))
    _check_out8(out8, ref8, ratio64, 0.2, B)
    for what, got, ref in (("mean", gm, gm64), ("log_std", gls[:A], gl64), ("value", gv, gv64)):
        tol = 2e-5 * float(ref.abs().max())
        assert _note("ppo_loss d/d " + what, float((got.double() - ref).abs().max()), tol) < tol


# ------------------------------------------------------------------------------------------------ gathers
@pytest.mark.parametrize("B", [4096, 4095, 513, 1])
def test_minibatch_gathers_at_d98_a23(B):
    """dm_ppo_gather (PPO._gather_minibatch, sized by the policy's dims) and the gather riding on Adam's norm launch
    (dm_flat_adam_step_gather), D = 98, A = 23, even and odd B: the gathered rows equal index_select bit for bit, nothing is
    written behind row B - 1."""
    from deepmimic_mujoco_amd.ppo import PPO, MlpPolicy
    n, D = 8192, 98
    g = torch.Generator(device=DEV); g.manual_seed(31)
    flat = dict(obs=torch.randn(n, D, device=DEV, generator=g), act=torch.randn(n, A, device=DEV, generator=g),
                adv=torch.randn(n, device=DEV, generator=g), ret=torch.randn(n, device=DEV, generator=g), logp=torch.randn(n, device=DEV, generator=g))
    idx = torch.randperm(n, device=DEV, generator=g)[:B].contiguous()
    ppo = PPO(None, policy=MlpPolicy(obs_dim=D, act_dim=A, net_arch=(64, 64)).to(DEV), device=DEV, batch_size=B, use_hip_graph=False)
    for ride in (False, True):
        bufs = {k: _guarded(B, D) if k == "obs" else _guarded(B, A) if k == "act" else _guarded(B) for k in flat}
        out = {k: v for k, (_, v) in bufs.items()}
        if ride:
            ppo.optimizer.flat_g.normal_()
            ppo.optimizer.step(begin=True, gather_next=(flat, idx, out))
        else:
            ppo._gather_minibatch(flat, idx, out)
        torch.cuda.synchronize()
        for k in flat:
            assert _guard_ok(*bufs[k]), (ride, k)
            assert torch.equal(out[k], torch.index_select(flat[k], 0, idx)), (ride, k)


# ------------------------------------------------------------------------------------------------ dm_flat_adam_step
N_G1 = 119599          # [256,128] at D = 98, A = 23


def test_g1_parameter_count():
    from deepmimic_mujoco_amd.ppo import MlpPolicy
    assert sum(p.numel() for p in MlpPolicy(obs_dim=98, act_dim=A).parameters()) == N_G1 and N_G1 % 4 == 3


@pytest.mark.parametrize("n,offset,grad_scale", [(N_G1, 0, 1.0), (N_G1, 1, 1.0), (1000, 0, 1.0), (2049, 0, 0.5), (4098, 0, 1.0),
                                                 (8195, 1, 0.5), (2 * 1024 * 2048 + 7, 0, 0.5), (2 * 1024 * 2048 + 7, 1, 1.0)])
def test_flat_adam_step_against_fp64(n, offset, grad_scale):
    """dm_flat_adam_step over six steps (clipped and unclipped norms alternating) against fp64 clip_grad_norm_ + Adam: n = the G1
    parameter count (n = 3 mod 4: the scalar tail runs), one block (n < 2048), n = 1, 2, 3 mod 4, n > 1024 x 2048 (the partial
    sums hit their cap and the strided loops wrap), views offset by one float (no float4 path), grad_scale != 1.  Parameters within
    6 x (2^-22 max|p| + 1e-4 lr) (fp32 rounding of p per step plus the update's relative error; measured margin >= 16x), first moment within 1e-5
    relative, second moment within 4e-5 (beta2 = 0.999 in fp32), step count exact."""
    lr, K = 1e-3, 6
    g = torch.Generator(device=DEV); g.manual_seed(n + offset)
    buf = lambda: torch.zeros(n + 1 + GUARD, device=DEV)
    bp, bg, bm, bv = buf(), buf(), buf(), buf()
    p, gr, m, v = (b[offset:offset + n] for b in (bp, bg, bm, bv))
    p.copy_(torch.randn(n, device=DEV, generator=g) * 0.1)
    state2 = torch.zeros(2 + 1024, device=DEV)
    p64 = p.double().clone()
    ref = R.Adam64(n, lr, device=DEV)
    norms = []
    for k in range(K):
        x = torch.randn(n, device=DEV, generator=g)
        gr.copy_(x if k % 2 == 0 else x * (0.2 / math.sqrt(n) / grad_scale))
        rc = _lib().dm_flat_adam_step(_p(p), _p(gr), _p(m), _p(v), n, C.c_float(lr), C.c_float(0.9), C.c_float(0.999), C.c_float(1e-5),
                                      C.c_float(0.5), C.c_float(grad_scale), _p(state2), int(state2.numel()), _stream())
        assert rc == 0
        norms.append(ref.step(p64, gr.double(), grad_scale=grad_scale) * 1.0)
    torch.cuda.synchronize()
    assert min(norms) < 0.5 < max(norms)
    assert float(state2[1]) == K
    for b in (bp, bg, bm, bv):       # nothing in front of or behind the view
        assert not bool(b[:offset].any()) and not bool(b[offset + n:].any())
    pmax = float(p64.abs().max())
    tol = K * (2.0 ** -22 * pmax + 1e-4 * lr)
    assert _note("flat_adam p (n=%d)" % n, float((p.double() - p64).abs().max()), tol) < tol
    assert float((m.double() - ref.m).abs().max()) < 1e-5 * float(ref.m.abs().max())
    # 1 - beta2 with beta2 = 0.999 rounded to fp32 is off by 1.3e-5 relative (half an ulp of 0.999 over 1e-3 is up to 3e-5)
    assert float((v.double() - ref.v).abs().max()) < 4e-5 * float(ref.v.abs().max())


# ------------------------------------------------------------------------------------------------ PPO.train end to end
def _fp32_train(pol, flat, perms, B, lr):
    """Plain fp32 PyTorch: F.linear trunks (ppo_ref64 in float32), clip_grad_norm_ + torch.optim.Adam."""
    P = R.params64(pol, DEV, dtype=torch.float32)
    opt = torch.optim.Adam(list(P.values()), lr=lr, eps=1e-5)
    for perm in perms:
        for s in range(0, perm.numel(), B):
            i = perm[s:s + B]
            loss, _ = R.loss(P, flat["obs"][i], flat["act"][i], flat["adv"][i], flat["ret"][i], flat["logp"][i])
            opt.zero_grad()
            loss.backward()
            nn.utils.clip_grad_norm_(list(P.values()), 0.5)
            opt.step()
    return P


@pytest.mark.parametrize("D,B", [(98, 4096), (85, 512)])
def test_ppo_train_matches_the_fp64_reference(D, B):
    """PPO.train on the product path (epoch graph, dm_ppo_mlp_grad, flat Adam with the next gather riding on the norm launch, the
    warm-up / restore around the capture), called twice on a synthetic 8 x 1024 buffer (graph reused, Adam's step count carried
    across), against the fp64 reference for the same permutations.  The product's parameter error (max and L2) is at most 4x
    that of plain fp32 PyTorch on the same run (Adam amplifies fp32 noise on near-zero gradients, so an absolute bound would be
    fragile; measured 1.0-1.1x), and the update itself is far larger than either error."""
    from deepmimic_mujoco_amd.ppo import PPO, MlpPolicy
    lr, T, N, E = 4e-4, 8, 1024, 2
    torch.manual_seed(12)
    pol = MlpPolicy(obs_dim=D, act_dim=A, net_arch=(256, 128))
    ppo = PPO(None, policy=pol, device=DEV, batch_size=B, learning_rate=lr, n_epochs=E)
    assert (ppo.obs_dim, ppo.act_dim) == (D, A) and ppo.use_hip_graph and ppo.flat_adam and ppo.epoch_graph and ppo.fused_mlp
    pol = ppo.policy
    P64 = R.params64(pol, DEV)
    p0 = R.flat(P64).clone()
    g = torch.Generator(device=DEV); g.manual_seed(5)
    with torch.no_grad():
        obs = torch.randn(T, N, D, device=DEV, generator=g) * 0.7
        mean, _ = R.heads(P64, obs)
        act = (mean + P64["log_std"].exp() * torch.randn(T, N, A, device=DEV, generator=g, dtype=torch.float64)).float()
        logp = (R.logp(act, mean, P64["log_std"]) + 0.1 * torch.randn(T, N, device=DEV, generator=g, dtype=torch.float64)).float()
    buf = dict(obs=obs, act=act, adv=torch.randn(T, N, device=DEV, generator=g) + 0.2, ret=torch.randn(T, N, device=DEV, generator=g),
               logp=logp, val=torch.zeros(T, N, device=DEV), rew=torch.zeros(T, N, device=DEV), done=torch.zeros(T, N, device=DEV))
    pol32 = MlpPolicy(obs_dim=D, act_dim=A, net_arch=(256, 128)).to(DEV)
    pol32.load_state_dict(pol.state_dict())
    gen = torch.Generator(device=DEV); gen.manual_seed(77)
    ppo.train(buf, generator=gen)
    ppo.train(buf, generator=gen)
    assert ppo._eg is not None and float(ppo.optimizer.state2[1]) == 2 * E * (T * N // B)
    gen = torch.Generator(device=DEV); gen.manual_seed(77)
    perm = torch.empty(T * N, dtype=torch.int64, device=DEV)
    perms = []
    for _ in range(2 * E):
        torch.randperm(T * N, device=DEV, generator=gen, out=perm)
        perms.append(perm.clone())
    flat = {k: v.reshape(-1, *v.shape[2:]) for k, v in buf.items() if k in ("obs", "act", "adv", "ret", "logp")}
    R.train(P64, flat, perms, B, R.Adam64(p0.numel(), lr, device=DEV))
    P32 = _fp32_train(pol32, flat, perms, B, lr)
    ref, prod, f32 = R.flat(P64), torch.cat([p.detach().double().reshape(-1) for p in pol.parameters()]), R.flat(P32).double()
    e_prod, e_32 = (prod - ref).abs(), (f32 - ref).abs()
    _note("train max|err| / fp32 torch's", float(e_prod.max()) / float(e_32.max()), 4.0)
    _note("train L2 err / fp32 torch's", float(e_prod.norm()) / float(e_32.norm()), 4.0)
    assert float(e_prod.max()) <= 4 * float(e_32.max()), (float(e_prod.max()), float(e_32.max()))
    assert float(e_prod.norm()) <= 4 * float(e_32.norm()), (float(e_prod.norm()), float(e_32.norm()))
    assert float((ref - p0).norm()) > 50 * float(e_prod.norm())


# ------------------------------------------------------------------------------------------------ G1 rollout buffers
@pytest.mark.parametrize("sub_batches,graph", [(1, False), (2, False), (2, True)])
def test_g1_one_launch_policy_rollout(sub_batches, graph):
    """PPO.collect_rollouts on the dm_policy_forward path with the G1 DPCombinedEnv batch (512 envs, D = 98, A = 23): replaying the
    stored actions (clamped to the per-joint bounds) on a twin env of the same seed gives bit-equal rewards, dones and next
    observations; logp / value of the stored rows match the fp64 policy (3e-4 / 2e-5, the humanoid test's bounds; measured
    margins >= 50x / 32x); the last env
    action lies inside the bounds and equals the clamped stored action.  With the captured graph the uncounted warm-up step is
    reproduced first (its draws are those of step 0)."""
    from deepmimic_mujoco_amd.combined_env import HipCombinedVecEnv
    from deepmimic_mujoco_amd.ppo import PPO, FusedPolicyForward
    Nn, T = 512, 4
    env = HipCombinedVecEnv(Nn, seed=11, sub_batches=sub_batches)
    twin = HipCombinedVecEnv(Nn, seed=11, sub_batches=sub_batches)
    ppo = PPO(env, net_arch=(256, 128), n_steps=T, batch_size=512, n_epochs=1, rollout_graph=graph, seed=2)
    assert (ppo.obs_dim, ppo.act_dim) == (98, A) and ppo._fused_policy_ok()
    with torch.no_grad():
        ppo.policy.log_std.copy_(torch.linspace(-0.5, 0.5, A))
    buf = ppo.collect_rollouts()
    lo, hi = ppo.act_lo, ppo.act_hi
    P = R.params64(ppo.policy, DEV)
    with torch.no_grad():
        for t in range(T):
            m64, v64 = R.heads(P, buf["obs"][t])
            assert _note("rollout logp", float((buf["logp"][t].double() - R.logp(buf["act"][t], m64, P["log_std"])).abs().max()), 3e-4) < 3e-4
            assert _note("rollout value", float((buf["val"][t].double() - v64).abs().max()), 2e-5) < 2e-5
        last_env = ppo._collector.act_env
        assert torch.equal(last_env, torch.clamp(buf["act"][T - 1], lo, hi))
        assert bool(((last_env >= lo) & (last_env <= hi)).all()) and bool((last_env == hi).any() and (last_env == lo).any())
        o = twin.reset_tensor().clone()
        if graph:
            fwd = FusedPolicyForward(ppo.policy, DEV)
            fwd.pack()
            z = lambda *s: torch.zeros(*s, device=DEV)
            a0, e0, l0, v0 = z(Nn, A), z(Nn, A), z(Nn), z(Nn)
            c0 = torch.zeros(1, dtype=torch.int32, device=DEV)
            for k in range(sub_batches):
                sl = env.sub_slices[k]
                fwd(o[sl].contiguous(), ppo._rollout_seed + 7919 * k, c0, 0, lo, hi, a0[sl], e0[sl], l0[sl], v0[sl])
            o = twin.step_tensor(e0)["obs"].clone()
        assert torch.equal(buf["obs"][0], o)
        for t in range(T):
            out = twin.step_tensor(torch.clamp(buf["act"][t], lo, hi))
            assert torch.equal(out["rew"], buf["rew"][t]) and torch.equal(out["done"].float(), buf["done"][t]), t
            if t + 1 < T:
                assert torch.equal(out["obs"], buf["obs"][t + 1]), t
        assert torch.equal(out["obs"], ppo._last_obs)
    env.close(); twin.close()
