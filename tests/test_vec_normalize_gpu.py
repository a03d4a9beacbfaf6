"""HipVecNormalize around the real batch envs: PPO's two single-batch rollout routes replayed on an unwrapped twin env through the
numpy restatement (tests/vecnorm_ref.py), bf16 buffers, evaluation through the frozen statistics, train.py --normalize, SAC's refusal.

Bounds as in test_vecnorm_kernels_gpu.py: what the rollout stored is within 2^-23 |ref| + 1e-9 of the restatement fed the twin's raw
observations and rewards (one rounding to fp32 plus fp64 reordering noise); done flags, and with them the episode monitor, are exact."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from deepmimic_mujoco_amd.vec_normalize import HipVecNormalize
from monitor_ref import MonitorRef
from vecnorm_ref import VecNormalizeRef

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 8
ENVS = {"walk": 64, "combined": 64, "g1": 8}


def make_env(kind, seed=21, **kw):
    from deepmimic_mujoco_amd.combined_env import HipCombinedVecEnv
    from deepmimic_mujoco_amd.deepmimic_env import HipDeepMimicVecEnv
    if kind == "combined":
        return HipCombinedVecEnv(ENVS[kind], robot="humanoid3d", seed=seed, **kw)
    if kind == "g1":
        return HipDeepMimicVecEnv(ENVS[kind], motion="walk", robot="unitree_g1", seed=seed, **kw)
    return HipDeepMimicVecEnv(ENVS[kind], motion="walk", seed=seed, **kw)


def close(got, ref, what):
    got, ref = got.detach().float().cpu().numpy().astype(np.float64), np.asarray(ref, np.float64)
    err, bnd = np.abs(got - ref), 2.0 ** -23 * np.abs(ref) + 1e-9
    print("measured %-28s worst error / bound %.3g" % (what, float(np.max(err / bnd))))
    assert np.all(err <= bnd), (what, float(np.max(err / bnd)))


def stat_eq(a, b, rel=1e-6):
    return (math.isnan(a) and math.isnan(b)) or a == pytest.approx(b, rel=rel)


@pytest.mark.parametrize("kind,route", [("walk", "sample_store"), ("walk", "policy_forward"), ("combined", "sample_store"),
                                        ("combined", "policy_forward"), ("g1", "policy_forward")])
def test_a_rollout_replayed_on_an_unwrapped_twin(kind, route):
    from deepmimic_mujoco_amd.ppo import PPO
    env_a, env_b = make_env(kind), make_env(kind)
    N, D = env_a.num_envs, env_a.observation_space.shape[0]
    vn = HipVecNormalize(env_a)
    ppo = PPO(vn, n_steps=T, batch_size=N * T, n_epochs=1, seed=2, fused_policy=route == "policy_forward")
    assert ppo.rollout_path() == route
    ref, mon = VecNormalizeRef(N, D), MonitorRef(N)
    want_obs = ref.reset(env_b.reset_tensor().cpu().numpy())
    for call in range(2):
        buf = ppo.collect_rollouts()
        torch.cuda.synchronize()
        assert ppo.rollout_path() == route
        raws = []
        for t in range(T):
            close(buf["obs"][t], want_obs, "%s obs[%d]" % (kind, t))
            out = env_b.step_tensor(torch.clamp(buf["act"][t].float(), ppo.act_lo, ppo.act_hi))
            raw = {k: out[k].cpu().numpy() for k in ("obs", "rew", "done")}
            want_obs, want_rew, _ = ref.step(raw["obs"], raw["rew"], raw["done"])
            close(buf["rew"][t], want_rew, "%s rew[%d]" % (kind, t))
            assert np.array_equal(buf["done"][t].cpu().numpy() != 0, raw["done"] != 0)
            assert np.array_equal(buf["rew_raw"][t].cpu().numpy(), raw["rew"])
            raws.append(raw)
        close(ppo._last_obs, want_obs, "%s last obs" % kind)
        rew, done = np.stack([r["rew"] for r in raws]), np.stack([r["done"] for r in raws])
        mon.feed(rew, done)
        # the monitor and the reward mean are those of the raw rewards; GAE ran on the normalised ones
        assert stat_eq(ppo.stats["ep_rew_mean"], mon.ep_rew_mean) and stat_eq(ppo.stats["ep_len_mean"], mon.ep_len_mean)
        assert ppo.stats["episodes"] == mon.episodes
        assert ppo.stats["mean_reward"] == pytest.approx(float(rew.astype(np.float64).mean()), rel=1e-6)
        from deepmimic_mujoco_amd.rollout import compute_gae
        last_val = ppo.policy.predict_values(ppo._last_obs).detach()
        adv, ret = compute_gae(buf["rew"], buf["val"], buf["done"], last_val.reshape(-1), ppo.gamma, ppo.gae_lambda)
        assert torch.allclose(buf["adv"], adv, rtol=1e-5, atol=1e-6)
    st = vn.obs_rms
    assert st.count == pytest.approx(1e-4 + N * (1 + 2 * T)) and vn.ret_rms.count == pytest.approx(1e-4 + N * 2 * T)
    assert np.max(np.abs(st.mean - ref.obs_rms.mean) / np.maximum(np.abs(ref.obs_rms.mean), 1e-300)) < 1e-10
    assert np.max(np.abs(st.var - ref.obs_rms.var) / ref.obs_rms.var) < 1e-10
    if kind != "g1":
        ppo.train(buf)                                   # the learner takes the buffer with its extra rew_raw rows
    env_a.close(), env_b.close()


def test_bf16_buffers_hold_the_same_rollout():
    from deepmimic_mujoco_amd.ppo import PPO
    got = {}
    for dt in (torch.float32, torch.bfloat16):
        env = make_env("walk")
        ppo = PPO(HipVecNormalize(env), n_steps=T, batch_size=64 * T, n_epochs=1, seed=2, buffer_dtype=dt)
        assert ppo.rollout_path() == "policy_forward"
        got[dt] = {k: v.clone() for k, v in ppo.collect_rollouts().items()}
        torch.cuda.synchronize()
        env.close()
    b32, b16 = got[torch.float32], got[torch.bfloat16]
    assert b16["obs"].dtype == torch.bfloat16 and torch.equal(b16["obs"], b32["obs"].to(torch.bfloat16))
    for k in ("rew", "rew_raw", "done", "val", "logp", "adv", "ret"):
        assert torch.equal(b16[k], b32[k]), k


def test_evaluation_through_the_frozen_statistics():
    from deepmimic_mujoco_amd.evaluation import evaluate_policy
    train_env = make_env("walk")
    vn = HipVecNormalize(train_env)
    vn.reset_tensor()
    for _ in range(5):
        vn.step_tensor(torch.zeros(64, 28, device=vn.device))
    frozen, returns = vn._state.clone(), vn.returns.clone()
    ev = make_env("walk", auto_reset=False, seed=4321)
    w = torch.linspace(-1.0, 1.0, 67 * 28, device=vn.device).reshape(67, 28)
    f = lambda o: torch.clamp(o @ w * 0.05, -0.5, 0.5)
    frames = np.arange(0, 33, 3)                          # 11 episodes; the policy is asked for all 64 rows every step
    a = evaluate_policy(f, ev, start_frames=frames, max_steps=40, return_episode_rewards=True, normalizer=vn)
    b = evaluate_policy(lambda o: f(vn.normalize_obs(o)), ev, start_frames=frames, max_steps=40, return_episode_rewards=True)
    raw = evaluate_policy(f, ev, start_frames=frames, max_steps=40, return_episode_rewards=True)
    assert a == b and a != raw and len(a[0]) == 11
    assert torch.equal(vn._state, frozen) and torch.equal(vn.returns, returns)
    x = torch.randn(5, 67, device=vn.device)             # any number of rows
    y = vn.normalize_obs(x)
    s = vn.obs_rms
    want = np.clip((x.cpu().numpy().astype(np.float64) - s.mean) / np.sqrt(s.var + 1e-8), -10, 10)
    close(y, want, "normalize_obs of 5 rows")
    assert torch.equal(vn._state, frozen)
    train_env.close(), ev.close()


def test_train_py_normalize(tmp_path):
    save = str(tmp_path / "ck.pt")
    cmd = [sys.executable, "-m", "deepmimic_mujoco_amd.train", "--normalize", "--json", "--envs", "64", "--horizon", str(T), "--total",
           str(2 * 64 * T), "--epochs", "1", "--minibatch", "256", "--save", save]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert line["normalize"] is True and line["iterations"] == 2 and line["rollout_path"] == "policy_forward"
    assert os.path.exists(save) and os.path.exists(save + ".vecnormalize")
    with np.load(save + ".vecnormalize") as z:
        sd = {k: z[k] for k in z.files}
    env = make_env("walk")
    vn = HipVecNormalize.load(save + ".vecnormalize", env)
    back = vn.state_dict()
    assert set(back) == set(sd) and all(np.array_equal(back[k], sd[k]) and back[k].dtype == sd[k].dtype for k in sd)      # bitwise
    assert vn.obs_rms.count == pytest.approx(1e-4 + 64 * (1 + 2 * T)) and float(np.abs(vn.obs_rms.mean).max()) > 0
    env.close()


def test_sac_refuses_the_wrapper():
    from deepmimic_mujoco_amd.sac import SAC
    env = make_env("walk")
    with pytest.raises(ValueError, match="HipVecNormalize"):
        SAC(HipVecNormalize(env), net_arch=(64, 64), buffer_size=1000)
    env.close()
