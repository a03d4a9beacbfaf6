"""The rollout finish (GAE + SB3 Monitor + rollout statistics) without a GPU: the export, the torch / numpy path of
``ppo.RolloutFinish`` against the plain-Python reference of tests/monitor_ref.py, the new ``PPO.stats`` keys and a learning gate."""
import math
import os
import re

import numpy as np
import torch

import monitor_ref as M
from sac_helpers import BanditEnv

from deepmimic_mujoco_amd.ppo import PPO, RolloutFinish, compute_gae

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


def test_rollout_finish_is_declared_and_exported():
    from deepmimic_mujoco_amd import _lib
    with open(os.path.join(ROOT, "include", "deepmimic_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+dm_rollout_finish\s*\(", header) and re.search(r"\blong long\s+dm_rollout_finish_workspace_bytes\s*\(", header)
    assert "dm_rollout_finish" in _lib.EXPORTS and "dm_rollout_finish_workspace_bytes" in _lib.EXPORTS
    L = _lib.load_library()
    assert len(L.dm_rollout_finish.argtypes) == 18 and L.dm_rollout_finish_workspace_bytes.restype is not None
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        assert "dm_rollout_finish" in f.read()


def _check(ppo, ref, buf):
    ref.feed(buf["rew"].numpy(), buf["done"].numpy())
    rets, lens = ppo.ep_history()
    assert rets.dtype == np.float32 and np.array_equal(rets, ref.returns()) and np.array_equal(lens, ref.lengths())    # contents and order
    s = ppo.stats
    assert s["episodes"] == ref.episodes
    assert M.same(s["ep_rew_mean"], ref.ep_rew_mean) and M.same(s["ep_len_mean"], ref.ep_len_mean)
    assert np.array_equal(ppo._finish._hist, ref.slots()) and np.array_equal(ppo._finish._acc, ref.running())
    ev = M.explained_variance(buf["val"].numpy(), buf["ret"].numpy())
    assert M.same(s["explained_variance"], ev) or abs(s["explained_variance"] - ev) < 1e-12
    assert s["done_rate"] == float(buf["done"].mean()) and s["mean_reward"] == float(buf["rew"].mean())


def test_torch_monitor_matches_reference_over_three_rollouts():
    """64 envs that all finish every 5th step, rollouts of 8 steps: episodes straddle both rollout boundaries, 256 episodes
    finish in all (the 100-slot history wraps twice) and the first rollout ends with every env three steps into an episode."""
    env = BanditEnv(64, 3, 2, seed=4, done_every=5)
    ppo = PPO(env, net_arch=(16, 16), n_steps=8, batch_size=128, n_epochs=1, seed=0, device=CPU)
    ref = M.MonitorRef(64)
    assert math.isnan(ppo.stats.get("ep_rew_mean", float("nan")))
    for k in range(3):
        buf = ppo.collect_rollouts()
        adv, ret = compute_gae(buf["rew"], buf["val"], buf["done"], ppo.policy.predict_values(ppo._last_obs).detach(), ppo.gamma, ppo.gae_lambda)
        assert torch.equal(buf["adv"], adv) and torch.equal(buf["ret"], ret)
        _check(ppo, ref, buf)
        assert ppo.stats["episodes"] == 64 * ((8 * (k + 1)) // 5) and ppo.stats["ep_len_mean"] == 5.0
    assert ref.episodes == 256


def test_torch_monitor_ragged_episodes_and_empty_history():
    """Random dones (rate 0.2) over three rollouts fed straight to RolloutFinish; before anything finished the means are NaN."""
    g = torch.Generator().manual_seed(3)
    T, N = 6, 37
    fin, ref = RolloutFinish(T, N, CPU, 0.99, 0.95), M.MonitorRef(N)
    for k in range(3):
        rew, val = torch.randn(T, N, generator=g), torch.randn(T, N, generator=g)
        done = (torch.rand(T, N, generator=g) < (0.0 if k == 0 else 0.2)).float()
        adv, ret = fin(rew, done, val, torch.randn(N, generator=g))
        ref.feed(rew.numpy(), done.numpy())
        r = fin.read()
        assert np.array_equal(r["ep_returns"], ref.returns()) and np.array_equal(r["ep_lengths"], ref.lengths())
        assert r["episodes"] == ref.episodes and M.same(r["ep_rew_mean"], ref.ep_rew_mean) and M.same(r["ep_len_mean"], ref.ep_len_mean)
        assert (k == 0) == math.isnan(r["ep_rew_mean"])
        assert abs(r["explained_variance"] - M.explained_variance(val.numpy(), ret.numpy())) < 1e-12
    fin.reset()
    assert fin.read()["episodes"] == 0 and math.isnan(fin.read()["ep_len_mean"])


def test_ppo_stats_have_the_monitor_keys_after_one_iteration(tmp_path):
    env = BanditEnv(16, 3, 2, seed=1, done_every=2)
    ppo = PPO(env, net_arch=(16, 16), n_steps=4, batch_size=32, n_epochs=1, seed=0, device=CPU)
    ppo.learn(16 * 4, log_interval=0)
    for k in ("mean_reward", "done_rate", "loss", "ep_rew_mean", "ep_len_mean", "episodes", "explained_variance"):
        assert k in ppo.stats, k
    assert ppo.stats["episodes"] == 32 and ppo.stats["ep_len_mean"] == 2.0 and np.isfinite(ppo.stats["ep_rew_mean"])
    path = str(tmp_path / "ppo.pt")
    ppo.save(path)
    assert "monitor" not in torch.load(path) and set(torch.load(path)) == {"policy", "optimizer", "num_timesteps"}
    ppo.load(path)                                              # a checkpoint carries no monitor state: it starts empty
    assert len(ppo.ep_history()[0]) == 0
    ppo.collect_rollouts()
    assert ppo.stats["episodes"] == 32


def test_cpu_ppo_learns_the_bandit():
    """The torch PPO on the contextual bandit with episodes of 3 steps (so ``ep_rew_mean`` is what is read; 16-step rollouts, so
    episodes straddle them).  Yardstick: ``ep_rew_mean`` after the first rollout = the untrained policy; the optimum is 0.
    Measured with this budget (60 iterations of 32 envs x 16 steps, [64,64], lr 1e-3, 10 epochs of 4 minibatches), first -> final:
        seed 0   -3.388 -> -0.0621        seed 1   -3.346 -> -0.0664        seed 2   -3.196 -> -0.0619
    Gate: the midpoint between the first-rollout value and the worst final value.  The first-rollout value is read from this very
    run (the draws do not depend on the code under test), the worst final value is -0.0664."""
    env = BanditEnv(32, 3, 2, seed=4, done_every=3)
    ppo = PPO(env, net_arch=(64, 64), n_steps=16, batch_size=128, n_epochs=10, learning_rate=1e-3, seed=0, device=CPU)
    curve = []
    ppo.learn(32 * 16 * 60, log_interval=0, callback=lambda p: curve.append(p.stats["ep_rew_mean"]))
    first, final = curve[0], curve[-1]
    print("bandit (cpu): ep_rew_mean first %.4f final %.4f" % (first, final))
    assert -3.6 < first < -3.0, first                           # the untrained policy, as recorded above
    assert final > 0.5 * (first + -0.0664), (first, final)
    assert ppo.stats["ep_len_mean"] == 3.0
