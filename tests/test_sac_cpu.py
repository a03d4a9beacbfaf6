"""SAC without a GPU: the torch learner against the fp64 reference of SB3's SAC.train, the replay ring, save / load and the
library's dm_sac_* exports."""
import numpy as np
import pytest
import torch

import sac_ref64 as ref
from sac_helpers import BanditEnv, flat_actor, flat_critic, rel_l2, to_ref
from deepmimic_mujoco_amd.sac import SAC


def _filled(n=8, D=6, A=3, arch=(32, 16), B=16, steps=6, **kw):
    torch.manual_seed(0)
    env = BanditEnv(n, D, A, seed=3, done_every=kw.pop("done_every", 3))
    sac = SAC(env, net_arch=arch, batch_size=B, learning_starts=10 ** 9, seed=1, device="cpu", **kw)
    for _ in range(steps):
        sac.env_step()
    return env, sac


def test_torch_step_matches_fp64_reference():
    """Five gradient steps, same minibatches and noise: alpha, all three arenas and the targets track the fp64 reference.
    Basis: fp32 arithmetic on nets of width <= 32 (relative rounding ~1e-7 per operation, a few hundred operations deep)."""
    env, sac = _filled()
    S = to_ref(sac)
    opt = ref.init_adam(S)
    g = torch.Generator().manual_seed(5)
    for t in range(1, 6):
        batch = sac.sample_torch()
        eps_pi, eps_next = torch.randn(16, 3, generator=g), torch.randn(16, 3, generator=g)
        out = sac.gradient_step_torch(batch, eps_pi, eps_next)
        r = ref.train_step(S, opt, t, {k: v.double() for k, v in batch.items()}, eps_pi.double(), eps_next.double())
        assert rel_l2(out["g_critic"], flat_critic(r["g_critic"]["qf0"], r["g_critic"]["qf1"])) < 1e-5
        assert rel_l2(out["g_actor"], flat_actor(r["g_actor"])) < 1e-5
        assert abs(float(sac.sac_state[4]) - r["alpha"]) < 1e-6
        assert abs(float(sac.sac_state[0]) - float(S["log_alpha"])) < 1e-6
        assert rel_l2(sac.actor, flat_actor(S["actor"])) < 1e-6
        assert rel_l2(sac.critic, flat_critic(S["qf0"], S["qf1"])) < 1e-6
        assert rel_l2(sac.critic_target, flat_critic(S["tgt0"], S["tgt1"])) < 1e-6
        assert abs(float(sac.sac_state[6]) - r["critic_loss"]) < 1e-4 * max(1.0, abs(r["critic_loss"]))
        assert abs(float(sac.sac_state[7]) - r["actor_loss"]) < 1e-4 * max(1.0, abs(r["actor_loss"]))
    assert float(sac.sac_state[0]) != 0.0          # log_ent_coef moved


def test_ring_wraps_substitutes_terminal_obs_and_warms_up():
    n, D, A = 4, 5, 2
    env = BanditEnv(n, D, A, seed=1, done_every=2)
    sac = SAC(env, net_arch=(8, 8), buffer_size=3 * n + 1, learning_starts=2 * n, batch_size=4, seed=0, device="cpu")
    assert sac.cap_steps == 3
    seen = []
    for t in range(5):
        last = sac._last_obs.clone() if sac._last_obs is not None else None
        sac.env_step()
        if last is None:
            last = sac.ring["obs"][(t % 3) * n:(t % 3 + 1) * n].clone()
        seen.append(dict(last=last, obs=env.obs.clone(), done=(t + 1) % 2 == 0))
    assert sac._pos == 5 % 3 and sac._fill == 3
    assert sac.ring_state.tolist()[:2] == [2, 3]
    for t in (2, 3, 4):                                   # rows of steps 3, 4 overwrote those of steps 0, 1
        rows = slice((t % 3) * n, (t % 3 + 1) * n)
        s = seen[t]
        assert torch.equal(sac.ring["obs"][rows], s["last"])
        assert torch.equal(sac.ring["done"][rows], torch.full((n,), 1.0 if s["done"] else 0.0))
        if s["done"]:                                     # next_obs is the terminal observation, not the reset one
            assert torch.equal(sac.ring["next_obs"][rows], s["last"])
            assert not torch.equal(sac.ring["next_obs"][rows], s["obs"])
        else:
            assert torch.equal(sac.ring["next_obs"][rows], s["obs"])
    # warm-up: the first learning_starts / n steps act uniformly in the box; the ring holds the actions rescaled to [-1, 1]
    env2 = BanditEnv(256, D, A, seed=2)
    sac2 = SAC(env2, net_arch=(8, 8), learning_starts=10 ** 9, seed=0, device="cpu")
    sac2.env_step()
    a = sac2.ring["act"][:256]
    assert float(a.min()) >= -1.0 and float(a.max()) <= 1.0 and float(a.std()) > 0.5      # uniform on [-1, 1]: std 0.577
    # episode bookkeeping: done every step -> every episode has length 1
    sac2._refresh_stats()
    assert sac2.stats["ep_len_mean"] == 1.0


def test_learn_with_gradient_steps_and_done_as_terminal():
    """Every done is a true terminal: with done every step the critic target is the reward alone."""
    env, sac = _filled(done_every=1)
    batch = sac.sample_torch()
    assert float(batch["done"].min()) == 1.0
    S = to_ref(sac)
    r = ref.train_step(S, ref.init_adam(S), 1, {k: v.double() for k, v in batch.items()}, torch.zeros(16, 3, dtype=torch.float64),
                       torch.zeros(16, 3, dtype=torch.float64))
    assert torch.allclose(r["y"], batch["rew"].double())
    sac.learning_starts = 0
    sac.learn(sac.num_timesteps + 4 * sac.n_envs, log_interval=2)
    assert sac._n_updates == 4 and np.isfinite(sac.stats["critic_loss"])


def test_save_load_round_trip(tmp_path):
    env, sac = _filled()
    for _ in range(3):
        sac.gradient_step_torch()
    path = str(tmp_path / "sac.pt")
    sac.save(path)
    env2 = BanditEnv(8, 6, 3, seed=9)
    other = SAC(env2, net_arch=(32, 16), batch_size=16, seed=7, device="cpu").load(path)
    for a, b in zip([sac.actor, sac.critic, sac.critic_target, sac.sac_state, sac.actor_m, sac.critic_v],
                    [other.actor, other.critic, other.critic_target, other.sac_state, other.actor_m, other.critic_v]):
        assert torch.equal(a, b)
    assert other.num_timesteps == sac.num_timesteps and other._n_updates == 3
    obs = torch.rand(5, 6)
    assert torch.equal(sac.predict(obs), other.predict(obs))
    assert torch.equal(sac.policy.predict_values(obs), other.policy.predict_values(obs))
    with pytest.raises(ValueError):
        SAC(BanditEnv(8, 7, 3), net_arch=(32, 16), device="cpu").load(path)


def test_library_exports_sac_kernels():
    from deepmimic_mujoco_amd import _lib
    names = {n for n in _lib.EXPORTS if n.startswith("dm_sac_")}
    assert names == {"dm_sac_act", "dm_sac_store", "dm_sac_gather", "dm_sac_head_fwd", "dm_sac_critic_loss", "dm_sac_actor_loss",
                     "dm_sac_head_bwd", "dm_sac_linear_relu", "dm_sac_relu_bwd_colsum", "dm_sac_polyak"}
    L = _lib.load_library()
    for n in names:
        assert getattr(L, n).argtypes, n


def test_cpu_learner_learns_the_bandit():
    """The torch learner on the contextual bandit: a quick check of the update's sign conventions (the GPU test gates the fused one)."""
    torch.manual_seed(0)
    env = BanditEnv(32, 3, 2, seed=4)
    sac = SAC(env, net_arch=(64, 64), batch_size=128, learning_starts=256, learning_rate=1e-3, seed=0, device="cpu")
    sac.learn(32 * 700, log_interval=0)
    obs = torch.rand(512, 3) * 2 - 1
    r = float(env.reward(obs, sac.predict(obs)).mean())
    rnd = float(env.reward(obs, torch.rand(512, 2) * 4 - 2).mean())
    assert r > -0.05 and rnd < -1.0, (r, rnd)


def test_constructing_a_learner_leaves_the_global_rng_alone():
    torch.manual_seed(123)
    want = torch.rand(4)
    torch.manual_seed(123)
    a = SAC(BanditEnv(4, 3, 2), net_arch=(8, 8), seed=0, device="cpu")
    assert torch.equal(torch.rand(4), want)
    b = SAC(BanditEnv(4, 3, 2), net_arch=(8, 8), seed=0, device="cpu")
    assert torch.equal(a.actor, b.actor) and torch.equal(a.critic, b.critic)      # the seed still fixes the init
    assert not torch.equal(a.actor, SAC(BanditEnv(4, 3, 2), net_arch=(8, 8), seed=1, device="cpu").actor)


def test_train_rejects_sac_under_torch_distributed(monkeypatch):
    from deepmimic_mujoco_amd import train
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        train.main(["--algo", "sac"])
