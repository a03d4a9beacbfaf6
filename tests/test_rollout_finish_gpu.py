"""``dm_rollout_finish`` (csrc/dm_ppo.hip) on the GPU: GAE bit for bit against ``ppo.compute_gae``, the episode monitor bit for bit
against the plain-Python reference of tests/monitor_ref.py, the fp64 statistics, reproducibility, graph capture, and the three
rollout paths of ``PPO`` that call it.  Inputs are offset views (4-byte aligned only); every output has NaN guard floats behind it."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import monitor_ref as M
from kernel_helpers import DEV, GUARD, guarded as _guarded, offset as _offset, ptr as _p  # noqa: F401
from sac_helpers import BanditEnv

pytestmark = pytest.mark.gpu

HIST = 100
GAMMA, LAM = 0.99, 0.95


class Finish:
    """Caller-side state of dm_rollout_finish, outputs with guards."""

    def __init__(self, T, N):
        from deepmimic_mujoco_amd import _lib
        self.L, self.T, self.N = _lib.load_library(), T, N
        self.adv_b, self.adv = _guarded(T, N)
        self.ret_b, self.ret = _guarded(T, N)
        self.acc_b, self.acc = _guarded(2 * N)
        self.hist_b, self.hist = _guarded(2 * HIST)
        self.stats_b, st = _guarded(16)
        self.stats = st.view(torch.float64)
        self.count = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.wb = int(self.L.dm_rollout_finish_workspace_bytes(T, N))
        self.work = torch.full((self.wb + 64,), 0xAB, dtype=torch.uint8, device=DEV)      # contents must not matter
        self.acc.zero_(); self.hist.zero_()

    def __call__(self, rew, done, val, last_val, gamma=GAMMA, lam=LAM):
        rc = self.L.dm_rollout_finish(self.T, self.N, _p(rew), _p(done), 1 if done.dtype == torch.uint8 else 0, _p(val), _p(last_val),
                                      gamma, lam, _p(self.adv), _p(self.ret), _p(self.acc), _p(self.hist), _p(self.count),
                                      _p(self.stats), _p(self.work), self.wb, C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
        assert rc == 0, rc
        return self

    def guards_ok(self):
        torch.cuda.synchronize()
        return all(bool(torch.isnan(b[n:]).all()) for b, n in ((self.adv_b, self.T * self.N), (self.ret_b, self.T * self.N),
                                                               (self.acc_b, 2 * self.N), (self.hist_b, 2 * HIST), (self.stats_b, 16)))

    def state(self):
        return [t.clone() for t in (self.adv, self.ret, self.acc, self.hist, self.count, self.stats.view(torch.int64))]


def _inputs(T, N, rate, seed, u8):
    g = torch.Generator().manual_seed(seed)
    rew, val, lv = torch.rand(T, N, generator=g), 3.0 * torch.randn(T, N, generator=g), torch.randn(N, generator=g)
    done = torch.rand(T, N, generator=g) < rate if rate < 1 else torch.ones(T, N, dtype=torch.bool)
    done = done.to(torch.uint8) if u8 else done.float()
    return _offset(rew, 1), _offset(done, 3), _offset(val, 5), _offset(lv, 7)


@pytest.mark.parametrize("rate", [0.0, 0.03, 1.0])
@pytest.mark.parametrize("u8", [True, False], ids=["done_u8", "done_f32"])
@pytest.mark.parametrize("T,N", [(32, 4096), (4096, 32), (37, 101), (1, 5)])
def test_gae_equals_compute_gae_bit_for_bit(T, N, u8, rate):
    """No tolerance: adv and ret of the kernel are torch.equal to compute_gae's on the device, for done as uint8 and as float."""
    from deepmimic_mujoco_amd.ppo import compute_gae
    rew, done, val, lv = _inputs(T, N, rate, 11 + T + N, u8)
    f = Finish(T, N)(rew, done, val, lv)
    adv, ret = compute_gae(rew, val, done.float(), lv, GAMMA, LAM)
    assert f.guards_ok()
    bad = int((f.adv != adv).sum()), int((f.ret != ret).sum())
    print("GAE (%d, %d) rate %.2f: mismatching adv %d ret %d of %d, max |adv| %.3g" % (T, N, rate, bad[0], bad[1], T * N, float(adv.abs().max())))
    assert torch.equal(f.adv, adv) and torch.equal(f.ret, ret)
    assert int(f.stats[1].item()) == int((done != 0).sum()) and int(f.count.item()) == int((done != 0).sum())


def _monitor_case(T, N, dones, seed):
    g = torch.Generator().manual_seed(seed)
    f, ref = Finish(T, N), M.MonitorRef(N)
    for k, done in enumerate(dones):
        rew, val, lv = torch.randn(T, N, generator=g), torch.randn(T, N, generator=g), torch.randn(N, generator=g)
        u8 = k % 2 == 0
        d = _offset(done.to(torch.uint8) if u8 else done.float(), 1 + k)
        f(_offset(rew, 2), d, _offset(val, 3), lv.to(DEV))
        ref.feed(rew.numpy(), done.numpy())
        assert f.guards_ok()
        assert int(f.count.item()) == ref.episodes, (k, int(f.count.item()), ref.episodes)
        assert np.array_equal(f.hist.cpu().numpy().reshape(2, HIST), ref.slots()), k         # slots, order, bits of the fp32 sums
        assert np.array_equal(f.acc.cpu().numpy().reshape(2, N), ref.running()), k
        assert int(f.stats[1].item()) == int(done.sum()) and int(f.stats[6].item()) == ref.episodes
    return f, ref


def test_monitor_many_dones_per_step_quiet_rollout_and_late_finisher():
    """N = 4096 at done rate 0.05: about 205 episodes end within one step, so the order inside a step and the wrap of the 100 slots
    both decide the answer.  The second rollout has no done at all; env 7 finishes for the first time in the third call."""
    T, N = 5, 4096
    g = torch.Generator().manual_seed(5)
    d1, d3 = torch.rand(T, N, generator=g) < 0.05, torch.rand(T, N, generator=g) < 0.05
    d1[:, 7] = False
    d3[:, 7] = False
    d3[3, 7] = True
    assert int(d1[0].sum()) > 100 and int(d3[T - 1].sum()) > 100
    f, ref = _monitor_case(T, N, [d1, torch.zeros(T, N, dtype=torch.bool), d3], 6)
    assert ref.episodes > 2000 and float(f.acc[N + 7].item()) == T - 4


def test_monitor_every_env_done_at_every_step_and_ragged_batch():
    """N = 1000 (not a multiple of the wave): a random rollout, then every env done at every step, then a random one."""
    T, N = 4, 1000
    g = torch.Generator().manual_seed(8)
    d1, d3 = torch.rand(T, N, generator=g) < 0.05, torch.rand(T, N, generator=g) < 0.03
    f, ref = _monitor_case(T, N, [d1, torch.ones(T, N, dtype=torch.bool), d3], 9)
    assert ref.episodes >= T * N


def _ev_inputs(T, N, seed):
    """Values that track the returns: var(ret) of order 1 and an explained variance inside [-1, 1]."""
    from deepmimic_mujoco_amd.ppo import compute_gae
    g = torch.Generator().manual_seed(seed)
    rew = torch.rand(T, N, generator=g) * torch.rand(1, N, generator=g)
    done = (torch.rand(T, N, generator=g) < 0.03).float()
    lv = torch.zeros(N)
    _, mc = compute_gae(rew, torch.zeros(T, N), done, lv, 0.9, 1.0)        # discounted returns
    val = mc + 0.6 * torch.randn(T, N, generator=g)
    return rew, done, val, lv


@pytest.mark.parametrize("T,N", [(32, 4096), (4096, 32), (37, 101)])
def test_statistics_against_fp64(T, N):
    """Done count exact; reward sum to 1e-6 relative (fp64 accumulation of fp32 values leaves nothing larger); explained variance
    to 1e-5 absolute on inputs with var(ret) of order 1 and the explained variance in [-1, 1]."""
    rew, done, val, lv = _ev_inputs(T, N, 21 + T)
    f = Finish(T, N)(_offset(rew, 1), _offset(done, 2), _offset(val, 3), lv.to(DEV), 0.9, 0.95)
    assert f.guards_ok()
    st = f.stats.cpu().numpy()
    ret, v = f.ret.cpu().numpy(), val.numpy()
    ev, vy = M.explained_variance(v, ret), float(np.var(ret.astype(np.float64)))
    print("stats (%d, %d): var(ret) %.4f  explained variance ref %.9f kernel %.9f  |diff| %.3g  reward sum rel %.3g" % (
        T, N, vy, ev, st[2], abs(st[2] - ev), abs(st[0] - rew.double().sum().item()) / rew.double().sum().item()))
    assert 0.1 < vy < 10.0 and -1.0 <= ev <= 1.0                           # the inputs are what the bound was set for
    assert st[1] == float(done.sum()) and st[5] == T * N
    assert abs(st[0] - rew.double().sum().item()) <= 1e-6 * abs(rew.double().sum().item())
    assert abs(st[2] - ev) <= 1e-5
    assert abs(st[3] - vy) <= 1e-9 * vy and abs(st[7] - ret.astype(np.float64).mean()) <= 1e-9


def test_explained_variance_is_nan_for_constant_returns():
    """rew = 0, val = last_val = c, gamma = lambda = 1, no done: every return is exactly c, var(ret) = 0 -> NaN as SB3's."""
    T, N = 32, 4096
    c = 1.2345678
    f = Finish(T, N)(torch.zeros(T, N, device=DEV), torch.zeros(T, N, dtype=torch.uint8, device=DEV), torch.full((T, N), c, device=DEV),
                     torch.full((N,), c, device=DEV), 1.0, 1.0)
    assert f.guards_ok() and bool((f.ret == torch.tensor(c, device=DEV)).all())
    st = f.stats.cpu().numpy()
    assert math.isnan(st[2]) and st[3] == 0.0 and st[0] == 0.0 and st[1] == 0.0
    assert math.isnan(M.explained_variance(np.full((T, N), c, np.float32), f.ret.cpu().numpy()))


@pytest.mark.parametrize("T,N", [(32, 4096), (4096, 32)])
def test_two_runs_and_a_captured_replay_give_identical_bits(T, N):
    rew, done, val, lv = _inputs(T, N, 0.05, 77, True)
    acc0, hist0 = torch.rand(2 * N, device=DEV), torch.rand(2 * HIST, device=DEV)
    acc0[N:] = torch.floor(acc0[N:] * 9)

    def start(f):
        f.acc.copy_(acc0); f.hist.copy_(hist0); f.count.fill_(12345)

    a, b = Finish(T, N), Finish(T, N)
    start(a); start(b)
    sa, sb = a(rew, done, val, lv).state(), b(rew, done, val, lv).state()
    assert a.guards_ok() and b.guards_ok()
    for x, y in zip(sa, sb):
        assert torch.equal(x, y)
    c = Finish(T, N)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        c(rew, done, val, lv)                                               # warm-up
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c(rew, done, val, lv)
    start(c)
    c.adv.fill_(float("nan")); c.ret.fill_(float("nan"))
    graph.replay()
    assert c.guards_ok()
    for x, y in zip(sa, c.state()):
        assert torch.equal(x, y)
    assert int(c.count.item()) == 12345 + int((done != 0).sum())


@pytest.mark.parametrize("path", ["fused_policy", "fused_rollout", "captured", "fused_policy_captured"])
def test_ppo_rollout_paths_use_the_kernel_and_match_the_references(path):
    """Humanoid walk, N = 256, T = 16, two rollouts per path: buf["adv"] / buf["ret"] equal compute_gae on the same buffers bit for
    bit, and PPO.stats / the episode history equal the plain-Python monitor fed with buf["rew"] / buf["done"]."""
    from deepmimic_mujoco_amd.deepmimic_env import HipDeepMimicVecEnv
    from deepmimic_mujoco_amd.ppo import PPO, compute_gae
    N, T = 256, 16
    cap = path.endswith("captured")
    venv = HipDeepMimicVecEnv(N, motion="walk", seed=3, **({"sub_batches": 2} if cap else {}))
    ppo = PPO(venv, net_arch=(256, 128), n_steps=T, batch_size=1024, n_epochs=1, fused_policy=path.startswith("fused_policy"),
              rollout_graph=cap)
    ref = M.MonitorRef(N)
    for k in range(2):
        buf = ppo.collect_rollouts()
        if path.startswith("fused_policy"):
            assert ppo._collector.step_kind == "policy_forward" and (ppo._collector.graph is not None) == cap
        else:
            assert (ppo._collector.graph is not None) == cap
        assert buf["done"].dtype == torch.float32
        with torch.no_grad():
            lv = ppo.policy.predict_values(ppo._last_obs)
            adv, ret = compute_gae(buf["rew"], buf["val"], buf["done"].float(), lv, ppo.gamma, ppo.gae_lambda)
        assert torch.equal(buf["adv"], adv) and torch.equal(buf["ret"], ret), (path, k)
        rew, done = buf["rew"].cpu().numpy(), buf["done"].cpu().numpy()
        ref.feed(rew, done)
        s = ppo.stats
        rets, lens = ppo.ep_history()
        print("%s rollout %d: episodes %d ep_rew_mean %.4f ep_len_mean %.2f explained_variance %.4f" % (
            path, k, s["episodes"], s["ep_rew_mean"], s["ep_len_mean"], s["explained_variance"]))
        assert s["episodes"] == ref.episodes and np.array_equal(rets, ref.returns()) and np.array_equal(lens, ref.lengths())
        assert M.same(s["ep_rew_mean"], ref.ep_rew_mean) and M.same(s["ep_len_mean"], ref.ep_len_mean)
        assert s["done_rate"] == float((done != 0).sum()) / (T * N)
        assert abs(s["mean_reward"] - rew.astype(np.float64).mean()) <= 1e-6 * abs(rew.astype(np.float64).mean())
        ev = M.explained_variance(buf["val"].cpu().numpy(), buf["ret"].cpu().numpy())
        assert M.same(s["explained_variance"], ev) or abs(s["explained_variance"] - ev) <= 1e-5 * max(1.0, abs(ev))
    ppo.train(buf)
    assert np.isfinite(ppo.stats["loss"])
    venv.close()


def test_gpu_ppo_learns_the_bandit():
    """The fused rollout path (dm_policy_sample + dm_rollout_store + dm_rollout_finish) and the GPU learner on the contextual bandit
    with 3-step episodes, same budget as the CPU gate (60 iterations of 32 envs x 16 steps, [64,64], lr 1e-3, 10 epochs).  Yardstick:
    ``ep_rew_mean`` after the first rollout (the untrained policy); the optimum is 0.  Measured on an MI355X, first -> final:
        seed 0   -3.239 -> -0.0639        seed 1   -3.547 -> -0.0725        seed 2   -3.200 -> -0.0641
    Gate: the midpoint between this run's first-rollout value and the worst final value (-0.0725)."""
    from deepmimic_mujoco_amd.ppo import PPO
    env = BanditEnv(32, 3, 2, device="cuda", seed=4, done_every=3)
    ppo = PPO(env, net_arch=(64, 64), n_steps=16, batch_size=128, n_epochs=10, learning_rate=1e-3, seed=0, device=DEV)
    assert ppo._fused_rollout_ok()
    curve = []
    ppo.learn(32 * 16 * 60, log_interval=0, callback=lambda p: curve.append(p.stats["ep_rew_mean"]))
    first, final = curve[0], curve[-1]
    print("bandit (gpu): ep_rew_mean first %.4f final %.4f" % (first, final))
    assert -3.8 < first < -3.0, first
    assert final > 0.5 * (first + -0.0725), (first, final)
    assert ppo.stats["ep_len_mean"] == 3.0 and ppo.stats["episodes"] == 32 * 16 * 60 // 3


def test_ppo_learns_to_stay_up_on_walk():
    """40 iterations at the defaults (4 096 envs x 32 steps, [256,128], 20 epochs, minibatch 4 096, lr 4e-4) on the humanoid walk clip.
    Yardstick: ``ep_rew_mean`` / ``ep_len_mean`` at the first iteration in which 100 episodes have finished (iteration 1: the untrained
    policy falls after ~21 steps).  Measured on an MI355X, first -> iteration 40:
        seed 0   return 1.114 -> 7.738   length 20.68 -> 74.61
        seed 1   return 1.168 -> 7.636   length 21.15 -> 73.54
        seed 2   return 1.151 -> 8.467   length 21.84 -> 76.17
    Gate: half of the smallest observed gain, i.e. return +3.234 (of 6.468) and length +26.19 (of 52.39)."""
    from deepmimic_mujoco_amd.deepmimic_env import HipDeepMimicVecEnv
    from deepmimic_mujoco_amd.ppo import PPO
    env = HipDeepMimicVecEnv(4096, motion="walk", seed=1234)
    ppo = PPO(env, n_steps=32, batch_size=4096, n_epochs=20, learning_rate=4e-4, seed=0)
    curve = []
    ppo.learn(4096 * 32 * 40, log_interval=0, callback=lambda p: curve.append((p.stats["episodes"], p.stats["ep_rew_mean"], p.stats["ep_len_mean"])))
    first = next(c for c in curve if c[0] >= 100)
    final = curve[-1]
    print("walk: first (episodes %d) ep_rew_mean %.3f ep_len_mean %.2f -> iteration %d: %.3f / %.2f" % (first + (len(curve),) + final[1:]))
    assert len(curve) == 40
    assert final[1] - first[1] >= 3.234 and final[2] - first[2] >= 26.19, (first, final)
    env.close()
