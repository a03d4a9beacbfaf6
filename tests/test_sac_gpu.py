"""The fused SAC learner (csrc/dm_sac.hip + library GEMMs) on the MI355X against the fp64 reference of SB3's SAC.train, at the
humanoid3d (67 / 28) and Unitree G1 (98 / 23) shapes with the [256,128] and [1024,512] nets of the reference scripts.  Every
draw (minibatch rows, noise) is restated from the kernels' hash (tests/sac_helpers.py)."""
import numpy as np
import pytest
import torch

import sac_ref64 as ref
from sac_helpers import BanditEnv, gather_rows, named_actor, named_critic, normals, opt_from, rel_l2, to_ref, uniforms

pytestmark = pytest.mark.gpu

SHAPES = [(67, 28, (256, 128)), (67, 28, (1024, 512)), (98, 23, (256, 128)), (98, 23, (1024, 512))]
# (D, A, arch, batch size, envs): the four nets at SB3's batch of 256 (one full pass of the 256-thread heads), and a batch of 100
# on 7 envs with hidden widths 96 and 40, where every one-workgroup loop ends in a partial pass and both layers straddle the
# 64-column tiles of the first-layer and ReLU-backward kernels
RAGGED = (5, 3, (96, 40), 100, 7)
STEP_CASES = [pytest.param(*s, 256, 64, id="%d-%d-arch%d" % (s[0], s[1], i)) for i, s in enumerate(SHAPES)] + \
             [pytest.param(*RAGGED, id="5-3-arch4-b100-n7")]
# Tolerance basis.  fp32 rounds at 6e-8; a dot product of <= 1024 terms carries ~sqrt(1024) x 6e-8 = 2e-6 relative error and a
# gradient passes through at most six of them (critic forward, backward into the action, head, actor backward): ~1e-5.  A
# handful of ReLU units whose pre-activation lies within that error of 0 switch between fp32 and fp64 and move a gradient by
# a few 1e-4 at most: GRAD_TOL = 1e-3.  After one Adam step every parameter moves by +-lr (m / sqrt(v) = sign(g) at step 1),
# so an element whose gradient is ~0 may move the other way: 2 lr = 6e-4 on weights of size ~1 / sqrt(fan_in) >= 0.03, a
# relative-L2 of sqrt(fraction) x 0.02 -> PARAM_TOL = 1e-4 allows a fraction of 2.5e-5 of such elements.
GRAD_TOL, PARAM_TOL, HEAD_TOL = 1e-3, 1e-4, 1e-4


def _sac(D, A, arch, B=256, n=64, steps=8, done_every=3, **kw):
    from deepmimic_mujoco_amd.sac import SAC
    torch.manual_seed(0)
    env = BanditEnv(n, D, A, device="cuda", seed=3, done_every=done_every)
    sac = SAC(env, net_arch=arch, batch_size=B, learning_starts=kw.pop("learning_starts", 10 ** 9), seed=1,
              device="cuda", **kw)
    for _ in range(steps):
        sac.env_step()
    return env, sac


def _per_tensor(got, want, tol, what):
    for k in want:
        assert rel_l2(got[k], want[k]) < tol, (what, k, rel_l2(got[k], want[k]))


@pytest.mark.parametrize("D,A,arch,B,n", STEP_CASES)
def test_fused_gradient_steps_match_fp64(D, A, arch, B, n):
    """Three fused gradient steps from a state where every part of the update shows: the target critics differ from the online
    ones, alpha = 0.2, a third of the transitions are not terminal (the target network enters y), Adam is past its first step
    after the first compared step, and one log_std output sits below the clamp.  Before each step the fp64 reference takes the
    learner's state (weights, targets, Adam moments and step count, log_ent_coef), so each step is compared on its own, per
    tensor, with its rows and noise restated from the hash for that counter value."""
    env, sac = _sac(D, A, arch, B, n)
    assert sac.n_envs == n and sac.batch_size == B
    g = torch.Generator(device="cuda").manual_seed(11)
    with torch.no_grad():
        sac.critic_target.add_(0.3 * sac.critic.abs() * torch.randn(sac.critic.shape, device="cuda", generator=g))
        sac.sac_state[0] = float(np.log(0.2))
        sac.policy.actor["bh"][A + 1] = -25.0                 # log_std column 1 clamped at -20 for every row
    total = int(sac.ring_state[1]) * n
    for step in range(3):
        S = to_ref(sac)
        opt, t = opt_from(sac)
        assert t == step + 1
        ctr = int(sac._learn_ctr)
        target_old, alpha = sac.critic_target.clone(), float(torch.exp(sac.sac_state[0]))
        sac.gradient_step_fused()
        torch.cuda.synchronize()
        fb, R = sac._fb, sac.ring
        # gather: rows restated from the hash, contents bit-exact
        rows = gather_rows(sac._learn_seed, B, ctr, total)
        assert np.array_equal(fb["idx"].cpu().numpy(), rows)
        idx = torch.as_tensor(rows, device="cuda", dtype=torch.long)
        batch = {k: R[k][idx] for k in ("obs", "act", "rew", "done", "next_obs")}
        assert 0.0 < float(batch["done"].mean()) < 1.0
        assert torch.equal(fb["obs2"][:B], batch["obs"]) and torch.equal(fb["obs2"][B:], batch["next_obs"])
        assert torch.equal(fb["xq"], torch.cat([batch["obs"], batch["act"]], 1))
        assert torch.equal(fb["xt"][:, :D], batch["next_obs"]) and torch.equal(fb["xpi"][:, :D], batch["obs"])
        assert torch.equal(fb["rew"], batch["rew"]) and torch.equal(fb["done"], batch["done"])
        eps = torch.as_tensor(normals(sac._learn_seed, 2 * B, ctr, A))
        r = ref.train_step(S, opt, t, {k: v.double().cpu() for k, v in batch.items()}, eps[:B], eps[B:])
        # squashed-Gaussian head forward (a_pi, a', log pi, log pi'), alpha and its Adam step
        assert rel_l2(fb["xpi"][:, D:], r["a_pi"]) < HEAD_TOL and rel_l2(fb["xt"][:, D:], r["a_next"]) < HEAD_TOL
        assert rel_l2(fb["logp"][:B], r["logp"]) < HEAD_TOL and rel_l2(fb["logp"][B:], r["logp_next"]) < HEAD_TOL
        st = sac.sac_state.cpu()
        assert abs(float(st[4]) - alpha) <= 1e-6 * alpha and abs(r["alpha"] - alpha) <= 1e-6 * alpha
        assert abs(float(st[0]) - float(S["log_alpha"])) < 1e-6
        assert abs(float(st[5]) - r["alpha_loss"]) < 1e-4 * max(1.0, abs(r["alpha_loss"]))
        # critic target + loss (a target read from the online critics, or no Polyak, moves these by O(1)), actor loss
        assert abs(float(st[6]) - r["critic_loss"]) < 1e-4 * max(1.0, abs(r["critic_loss"]))
        assert abs(float(st[7]) - r["actor_loss"]) < 1e-4 * max(1.0, abs(r["actor_loss"]))
        # gradients tensor by tensor: head backward (mu / log_std halves of Wh, bh), ReLU backward + bias sums (b1, b2), loss heads
        _per_tensor(named_actor(sac, fb["g_actor"]), r["g_actor"], GRAD_TOL, "g_actor")
        for i in (0, 1):
            _per_tensor(named_critic(sac, fb["g_critic"], i), r["g_critic"]["qf%d" % i], GRAD_TOL, "g_qf%d" % i)
        assert float(r["g_actor"]["ls_b"][1]) == 0.0 and float(named_actor(sac, fb["g_actor"])["ls_b"][1]) == 0.0   # clamp mask
        # Adam steps, tensor by tensor
        _per_tensor(named_actor(sac, sac.actor), S["actor"], PARAM_TOL, "actor")
        for i in (0, 1):
            _per_tensor(named_critic(sac, sac.critic, i), S["qf%d" % i], PARAM_TOL, "qf%d" % i)
            _per_tensor(named_critic(sac, sac.critic_target, i), S["tgt%d" % i], PARAM_TOL, "tgt%d" % i)
        # Polyak directly: target_new = target_old (1 - tau) + tau critic_new, to fp32 rounding (two roundings of |target_old|
        # + tau |critic_new|), and it moved by tau (critic_new - target_old), which is far above that rounding here
        t_old, c_new, t_new = target_old.double(), sac.critic.double(), sac.critic_target.double()
        want = t_old * (1 - sac.tau) + sac.tau * c_new
        bound = 3 * 2.0 ** -24 * (t_old.abs() + sac.tau * c_new.abs()) + 1e-30
        assert bool(((t_new - want).abs() <= bound).all())
        assert float((t_new - t_old).norm()) > 100 * float(bound.norm())
        assert int(sac._learn_ctr) == ctr + 1


@pytest.mark.parametrize("D,A,arch", SHAPES[:1] + SHAPES[2:3])
def test_act_and_store_kernels(D, A, arch):
    env, sac = _sac(D, A, arch, steps=0)
    n = sac.n_envs
    sac._last_obs = env.reset_tensor().clone()
    lo, hi = sac.act_lo.double().cpu(), sac.act_hi.double().cpu()
    # warm-up: uniform in the box, rescaled to [-1, 1] for the ring
    ctr = int(sac._roll_ctr)
    act, act_env = sac._act_fused(sac._last_obs, warmup=True)
    u = torch.as_tensor(uniforms(sac._roll_seed, n, ctr, A))
    assert torch.allclose(act_env.double().cpu(), lo + u * (hi - lo), atol=1e-6)
    assert torch.allclose(act.double().cpu(), 2 * u - 1, atol=1e-6)
    # policy actions: tanh(mu + exp(clamp(log_std)) eps), unscaled into the box; deterministic tanh(mu)
    S = to_ref(sac)
    obs64 = sac._last_obs.double().cpu()
    mu, ls = ref.actor_dist(S, obs64)
    eps = torch.as_tensor(normals(sac._roll_seed, n, ctr, A))
    act, act_env = sac._act_fused(sac._last_obs, warmup=False)
    a = torch.tanh(mu + ls.exp() * eps)
    assert rel_l2(act, a) < HEAD_TOL and rel_l2(act_env, lo + 0.5 * (a + 1) * (hi - lo)) < HEAD_TOL
    act_d, _ = sac._act_fused(sac._last_obs, warmup=False, deterministic=True)
    assert rel_l2(act_d, torch.tanh(mu)) < HEAD_TOL
    # store: ring row, terminal_obs substitution, last_obs, device-side position / fill / counter
    act, act_env = sac._act_fused(sac._last_obs, warmup=False)
    last = sac._last_obs.clone()
    act_keep = act.clone()
    out = env.step_tensor(act_env)
    out["done"][: n // 2] = 1
    out["done"][n // 2:] = 0
    sac._store_fused(out)
    torch.cuda.synchronize()
    R = sac.ring
    assert torch.equal(R["obs"][:n], last) and torch.equal(R["act"][:n], act_keep) and torch.equal(R["rew"][:n], out["rew"])
    assert torch.equal(R["done"][:n], out["done"].float())
    assert torch.equal(R["next_obs"][: n // 2], out["terminal_obs"][: n // 2])
    assert torch.equal(R["next_obs"][n // 2:n], out["obs"][n // 2:])
    assert torch.equal(sac._last_obs, out["obs"])
    assert sac.ring_state.tolist() == [1, 1, 0, n // 2] and int(sac._roll_ctr) == ctr + 1


def test_ring_wraps_on_device():
    env, sac = _sac(67, 28, (256, 128), n=16, steps=0, buffer_size=16 * 3)
    for t in range(7):
        sac.env_step()
    assert sac.ring_state.tolist()[:3] == [7 % 3, 3, 0]


@pytest.mark.parametrize("D,A,arch,B,n", [pytest.param(*SHAPES[1], 256, 64, id="67-28-arch0"), pytest.param(*RAGGED, id="5-3-arch1-b100-n7")])
def test_graph_replay_is_bit_identical_to_eager(D, A, arch, B, n):
    env, sac = _sac(D, A, arch, B, n)
    snap = [t.clone() for t in sac.state_tensors()]
    for _ in range(3):
        sac.gradient_step_fused()
    eager = [t.clone() for t in sac.state_tensors()] + [sac._fb["g_actor"].clone(), sac._fb["g_critic"].clone()]
    with torch.no_grad():
        for t, s in zip(sac.state_tensors(), snap):
            t.copy_(s)
    sac._capture()
    for _ in range(3):
        sac._graph.replay()
    graph = [t.clone() for t in sac.state_tensors()] + [sac._fb["g_actor"].clone(), sac._fb["g_critic"].clone()]
    for a, b in zip(eager, graph):
        assert torch.equal(a, b)


def test_gather_never_reads_unwritten_rows():
    env, sac = _sac(67, 28, (256, 128), n=32, steps=0, buffer_size=32 * 1000)
    for v in sac.ring.values():
        v.fill_(float("nan"))
    for _ in range(3):
        sac.env_step()
    sac.learning_starts = 0
    for _ in range(20):
        sac.train(1)
        assert int(sac._fb["idx"].max()) < 3 * 32
    torch.cuda.synchronize()
    for t in (sac.actor, sac.critic, sac.critic_target, sac._fb["obs2"], sac._fb["xq"]):
        assert bool(torch.isfinite(t).all())


def test_fused_sac_learns_the_bandit():
    """Contextual bandit (done every step, optimum reward 0, uniform random actions about -1.4): 700 gradient steps of the
    captured learner reach -0.05, well above random.  Fixed seeds; a few seconds."""
    from deepmimic_mujoco_amd.sac import SAC
    env = BanditEnv(32, 3, 2, device="cuda", seed=4)
    sac = SAC(env, net_arch=(64, 64), batch_size=128, learning_starts=256, learning_rate=1e-3, seed=0, device="cuda")
    sac.learn(32 * 700, log_interval=0)
    obs = torch.rand(512, 3, device="cuda") * 2 - 1
    r = float(env.reward(obs, sac.predict(obs)).mean())
    rnd = float(env.reward(obs, torch.rand(512, 2, device="cuda") * 4 - 2).mean())
    assert sac._graph is not None and sac._n_updates > 600
    assert r > -0.05 and rnd < -1.0, (r, rnd)


def test_rejected_sac_call_names_its_entry_point():
    """What the SAC driver's calls go through: dm_sac_linear_relu refuses I = 129 (one over its 128-column LDS tile) on the host,
    `_lib.call` raises with the entry point's name and -22, and nothing was launched: the output keeps its fill.  B = 2, O = 4 is
    the smallest argument set the entry point rejects."""
    from deepmimic_mujoco_amd import _lib
    DEV = torch.device("cuda", 0)
    B, O, I = 2, 4, 129
    x, w, b = torch.ones(B, I, device=DEV), torch.ones(O, I, device=DEV), torch.ones(O, device=DEV)
    y = torch.full((B, O), -7.0, device=DEV)
    with pytest.raises(RuntimeError, match=r"^dm_sac_linear_relu failed \(-22\)$"):
        _lib.call("dm_sac_linear_relu", x, I, w, b, y, B, O, I, 1, device=DEV)
    torch.cuda.synchronize(DEV)
    assert bool((y == -7.0).all())
