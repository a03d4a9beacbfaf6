"""PPO(mlp_dtype="bf16x3") end to end: the routing of the learner, the minibatch gradient of the [1024,512] net against the fp64
reference of SB3's update (tests/ppo_ref64.py), and five optimizer steps against the fp32 library-GEMM learner.

Setup: net_arch (1024, 512), batch_size 256, n_epochs 2, a synthetic buffer of T x N = 4 x 256 rows, D = 67, A = 28, built by
ppo_wide3_ref64.make_batch (actions drawn from the policy, ratios on both sides of the clip range, no row within 1e-2 of a clip
boundary in log ratio: a clip decision that differs between two evaluations would move a gradient by a whole row's worth)."""
import functools

import pytest
import torch
import torch.nn as nn

import ppo_ref64 as R
import ppo_wide_ref64 as W
import ppo_wide3_ref64 as W3
from kernel_helpers import DEV

pytestmark = pytest.mark.gpu

ARCH, D, A, B, T = (1024, 512), 67, 28, 256, 4


def _policy(arch=ARCH, seed=13):
    from deepmimic_mujoco_amd.ppo import MlpPolicy
    torch.manual_seed(seed)
    pol = MlpPolicy(obs_dim=D, act_dim=A, net_arch=arch).to(DEV)
    with torch.no_grad():
        pol.log_std.add_(0.1 * torch.randn(A, device=DEV))
        for m in pol.modules():
            if isinstance(m, nn.Linear):
                m.bias.normal_(0, 0.1)
    return pol


@functools.lru_cache(maxsize=None)
def _rows():
    """(obs, act, adv, ret, old_logp) of the T x N = 4 x 256 rows, flat, for the policy of _policy()."""
    return W3.make_batch(R.params64(_policy(), DEV), D, A, T * B, W.SEEDS[0])


def _ppo(mlp_dtype, arch=ARCH, **kw):
    from deepmimic_mujoco_amd.ppo import PPO
    return PPO(None, net_arch=arch, batch_size=B, n_epochs=2, device=DEV, policy=_policy(arch), mlp_dtype=mlp_dtype, **kw)


def _minibatch(i):
    return tuple(t[i * B:(i + 1) * B].contiguous() for t in _rows())


def test_bf16x3_routes_the_wide_net_to_wide3_and_the_epoch_graph_replays():
    """PPO(net_arch=(1024,512), mlp_dtype="bf16x3") selects WideMlpGrad3 (dm_ppo_wide3_grad), the epoch graph applies and two
    PPO.train calls replay it: n_epochs x 4 optimizer steps counted on the device each time, a finite loss, moved parameters."""
    from deepmimic_mujoco_amd.ppo import WideMlpGrad3
    ppo = _ppo("bf16x3")
    assert ppo._wide_ok and ppo.learner_path() == "wide_bf16x3"
    obs, act, adv, ret, logp = _rows()
    buf = dict(obs=obs.view(T, B, D), act=act.view(T, B, A), adv=adv.view(T, B), ret=ret.view(T, B), logp=logp.view(T, B))
    flat = {k: v.reshape(-1, *v.shape[2:]) for k, v in buf.items()}
    assert ppo._epoch_graph_ok(flat, T * B)
    before = torch.cat([p.detach().reshape(-1) for p in ppo.policy.parameters()]).clone()
    for _ in range(2):
        loss = ppo.train(buf)
        torch.cuda.synchronize()
        assert loss == loss and abs(loss) < 1e3
        assert float(ppo._loss_acc[1]) == 2 * T
    assert ppo._eg["graph"] is not None and isinstance(ppo._mlp_grads[("wide", B)], WideMlpGrad3)
    after = torch.cat([p.detach().reshape(-1) for p in ppo.policy.parameters()])
    assert torch.isfinite(after).all() and float((after - before).abs().max()) > 1e-4


def test_bf16x3_keeps_the_fused_fp32_kernel_for_the_small_net():
    """PPO(net_arch=(256,128), mlp_dtype="bf16x3") still takes dm_ppo_mlp_grad (exact fp32, already fused)."""
    from deepmimic_mujoco_amd.ppo import FusedMlpGrad
    ppo = _ppo("bf16x3", arch=(256, 128), use_hip_graph=False)
    assert not ppo._wide_ok and ppo.learner_path() == "fused_fp32"
    ppo._minibatch_grad(*_minibatch(0))
    torch.cuda.synchronize()
    assert isinstance(ppo._mlp_grads[B], FusedMlpGrad) and ("wide", B) not in ppo._mlp_grads


def test_bf16x3_minibatch_gradient_is_within_1e_4_of_the_fp64_gradient():
    """The flat gradient of the first minibatch (optimizer.flat_g after _minibatch_grad, named_parameters order) against
    ppo_ref64.grads in fp64: relative L2 <= 1e-4."""
    ppo = _ppo("bf16x3", use_hip_graph=False)
    mb = _minibatch(0)
    P = R.params64(ppo.policy, DEV)
    _, _, g64 = R.grads(P, *mb, clip_range=ppo.clip_range, vf_coef=ppo.vf_coef, ent_coef=ppo.ent_coef, normalize=True)
    ppo._minibatch_grad(*mb)
    torch.cuda.synchronize()
    assert [id(p) for p in ppo.optimizer.params] == [id(p) for _, p in ppo.policy.named_parameters()]
    ref = torch.cat([g64[n].reshape(-1) for n in P])
    d = W.rel_l2(ppo.optimizer.flat_g, ref)
    print("bf16x3 flat gradient against fp64: relative L2 %.3g" % d)
    assert d <= 1e-4, d


def test_bf16x3_five_optimizer_steps_track_the_fp32_library_learner():
    """The same five optimizer steps (minibatches 0, 1, 2, 3, 0) from the same initial weights through the bf16x3 learner and
    through the fp32 library-GEMM learner: every loss agrees to 1e-4 relative, the parameters to rtol 1e-4 / atol 2e-6 (the rule
    of the fused fp32 [256,128] learner against its fp32 twin, test_gpu_env.py)."""
    res = {}
    for dt in ("bf16x3", torch.float32):
        ppo = _ppo(dt, use_hip_graph=False)
        assert ppo.learner_path() == ("wide_bf16x3" if dt == "bf16x3" else "library_fp32")
        losses = [float(ppo._minibatch_step(*_minibatch(i % T))) for i in range(5)]
        torch.cuda.synchronize()
        res[dt] = (losses, torch.cat([p.detach().reshape(-1) for p in ppo.policy.parameters()]))
    (l3, p3), (l32, p32) = res["bf16x3"], res[torch.float32]
    print("losses bf16x3 %s fp32 %s, max |d param| %.3g" % (l3, l32, float((p3 - p32).abs().max())))
    for a, b in zip(l3, l32):
        assert abs(a - b) <= 1e-4 * abs(b), (l3, l32)
    assert torch.allclose(p3, p32, rtol=1e-4, atol=2e-6), float((p3 - p32).abs().max())
