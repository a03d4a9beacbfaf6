"""SAC(env, normalizer=HipVecNormalize(env)) without a GPU: the torch learner step by step against the numpy restatement of SB3's
sequence (tests/sac_vecnorm_ref.py), the refusals, the export of dm_sac_gather_norm and its host-side argument checks, and a
learning check on a bandit with badly scaled observation columns.

Bounds, none taken from the code under test: the ring holds the env's raw outputs bit for bit; the running statistics agree with
the restatement to 1e-12 relative (both are fp64 and apply RunningMeanStd's formulas in the same order: the bound of
test_vecnorm_cpu.py); a normalised output is within 2^-23 |ref| + 1e-9 (one rounding to fp32)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from sac_helpers import BanditEnv
from sac_vecnorm_ref import RecordingBandit, SacVecNormRef, ScaledBanditEnv, out_bound, stats_rel_err
from deepmimic_mujoco_amd import _lib
from deepmimic_mujoco_amd.sac import SAC, actor_head, squash
from deepmimic_mujoco_amd.vec_normalize import HipVecNormalize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _within(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err, bnd = np.abs(got - ref), out_bound(ref)
    print("measured %-24s worst error / bound %.3g" % (what, float(np.max(err / bnd))))
    assert np.all(err <= bnd), (what, float(np.max(err / bnd)))


def test_torch_path_follows_the_restatement_step_by_step():
    """Eleven vec-env steps on 8 envs (done every third step, three warm-up steps, a ring of five steps that wraps twice), clips of
    1.5 / 0.5 so that both are hit; then minibatches of given rows; then the same with the statistics frozen."""
    n, D, A, cap, warm = 8, 6, 3, 5, 3
    env = RecordingBandit(n, D, A, seed=3, done_every=3)
    kw = dict(clip_obs=1.5, clip_reward=0.5, gamma=0.9)
    vn = HipVecNormalize(env, **kw)
    sac = SAC(env, net_arch=(32, 16), batch_size=16, buffer_size=cap * n, learning_starts=warm * n, seed=1, device="cpu", normalizer=vn)
    assert sac.normalizer is vn and sac.cap_steps == cap
    ref = SacVecNormRef(n, D, A, cap, **kw)
    lo, hi = sac.act_lo, sac.act_hi
    ep_ret, episodes = np.zeros(n), []
    for t in range(11):
        gen = torch.Generator().set_state(sac._gen.get_state())
        sac.env_step()
        if t == 0:
            ref.reset(env.first.numpy())
        seen, rec = ref.obs_norm.copy(), env.log[-1]
        rows = slice(ref.pos * n, (ref.pos + 1) * n)
        act = sac.ring["act"][rows].clone()
        # the action: uniform in the box before learning_starts, then the actor on the NORMALISED last observation
        if t < warm:
            act_env = lo + torch.rand(n, A, generator=gen) * (hi - lo)
            assert torch.equal(rec["act_env"], act_env) and torch.equal(act, 2.0 * ((act_env - lo) / (hi - lo)) - 1.0)
        else:
            want, _ = squash(actor_head(sac.policy.actor, torch.from_numpy(seen)), torch.randn(n, A, generator=gen))
            # `seen` is within one fp32 rounding of what the learner fed its actor; two 32-wide layers carry that to ~1e-6
            assert float((act - want).abs().max()) < 1e-5
            assert torch.allclose(rec["act_env"], lo + 0.5 * (act + 1.0) * (hi - lo), atol=1e-6)
        ref.step(act.numpy(), rec["obs"].numpy(), rec["rew"].numpy(), rec["done"].numpy(), rec["terminal_obs"].numpy())
        # the ring: raw, bit for bit
        for k in ("obs", "act", "rew", "done", "next_obs"):
            assert np.array_equal(sac.ring[k].numpy(), ref.ring[k]), (t, k)
        d = rec["done"].numpy() != 0
        assert np.array_equal(sac.ring["next_obs"][rows].numpy(), np.where(d[:, None], rec["terminal_obs"].numpy(), rec["obs"].numpy()))
        assert torch.equal(sac._last_obs, rec["obs"]) and (sac._pos, sac._fill) == (ref.pos, ref.fill)
        # statistics (updated in warm-up too) and the next normalised observation
        assert stats_rel_err(vn, ref.vn) < 1e-12, (t, stats_rel_err(vn, ref.vn))
        _within(sac._obs_norm.numpy(), ref.obs_norm, "obs_norm step %d" % t)
        ep_ret += rec["rew"].numpy().astype(np.float64)
        episodes += list(ep_ret[d])
        ep_ret[d] = 0
    assert vn.obs_rms.count == pytest.approx(1e-4 + n * 12) and ref.fill == cap and ref.pos == 11 % cap
    # the episode monitor keeps raw rewards
    assert np.allclose([e[0] for e in sac._ep_deque], episodes, rtol=1e-6) and len(episodes) == 3 * n
    # minibatches of given rows, with the statistics of the moment
    idx = torch.tensor([0, 1, 7, 8, 15, 16, 23, 24, 31, 39, 39, 5, 12, 20, 33, 38])
    for frozen in (False, True):
        b, r = sac.sample_torch(idx), ref.sample(idx.numpy())
        for k in ("obs", "next_obs", "rew"):
            assert b[k].dtype == torch.float32
            _within(b[k].numpy(), r[k], "sample %s" % k)
        assert torch.equal(b["act"], sac.ring["act"][idx]) and torch.equal(b["done"], sac.ring["done"][idx])
        assert float(np.abs(r["obs"]).max()) == 1.5 and float(np.abs(r["rew"]).max()) == 0.5          # both clips are hit
        assert not np.array_equal(r["obs"], ref.ring["obs"][idx.numpy()])
        if not frozen:                                     # training = False: statistics frozen, both transforms kept
            vn.training = ref.vn.training = False
            state = vn._state.clone()
            gen = torch.Generator().set_state(sac._gen.get_state())
            sac.env_step()
            rec = env.log[-1]
            ref.step(sac.ring["act"][ref.pos * n:(ref.pos + 1) * n].numpy(), rec["obs"].numpy(), rec["rew"].numpy(), rec["done"].numpy(),
                     rec["terminal_obs"].numpy())
            assert torch.equal(vn._state, state)
            _within(sac._obs_norm.numpy(), ref.obs_norm, "obs_norm frozen")
    # a gradient step of the torch learner draws its own rows and runs on the normalised batch
    sac.gradient_step_torch()
    assert np.isfinite(float(sac.sac_state[6])) and sac._n_updates == 1


def test_without_a_normalizer_nothing_changes():
    """normalizer=None: the same ring, the same draws and the same minibatch as a learner built without the argument."""
    out = []
    for kw in ({}, {"normalizer": None}):
        env = BanditEnv(8, 6, 3, seed=3, done_every=3)
        sac = SAC(env, net_arch=(32, 16), batch_size=16, learning_starts=16, seed=1, device="cpu", **kw)
        for _ in range(5):
            sac.env_step()
        sac.gradient_step_torch()
        out.append([sac.ring[k].clone() for k in sac.ring] + [sac.actor.clone(), sac.critic.clone()])
        assert sac.normalizer is None and sac._obs_norm is None
    assert all(torch.equal(a, b) for a, b in zip(*out))


def test_refusals_and_flags(monkeypatch):
    from deepmimic_mujoco_amd import train
    from deepmimic_mujoco_amd.eval_dashboard import training_normalizer
    env, other = BanditEnv(4, 3, 2), BanditEnv(4, 3, 2)
    with pytest.raises(ValueError, match="normalizer.venv is env"):
        SAC(env, net_arch=(8, 8), device="cpu", normalizer=HipVecNormalize(other))
    with pytest.raises(ValueError, match="normalizer.venv is env"):
        SAC(env, net_arch=(8, 8), device="cpu", normalizer=object())
    with pytest.raises(ValueError, match="pass the inner env"):
        SAC(HipVecNormalize(env), net_arch=(8, 8), device="cpu")
    vn = HipVecNormalize(env)
    sac = SAC(env, net_arch=(8, 8), device="cpu", normalizer=vn)
    assert training_normalizer(sac) is vn
    assert training_normalizer(SAC(other, net_arch=(8, 8), device="cpu")) is None
    args = train.build_parser().parse_args(["--algo", "sac", "--normalize", "--norm-clip-obs", "5", "--no-norm-reward"])
    assert args.algo == "sac" and args.normalize and args.norm_clip_obs == 5.0 and args.no_norm_reward
    src = open(os.path.join(ROOT, "deepmimic_mujoco_amd", "train.py")).read()
    assert "not implemented" not in src and "normalizer=vn" in src
    monkeypatch.setenv("WORLD_SIZE", "2")                  # the multi-rank refusal stays
    with pytest.raises(SystemExit):
        train.main(["--normalize"])


def test_a_setting_changed_on_the_normalizer_reaches_the_learner():
    """clip_obs set between steps is what the next sample uses (on the device: what the descriptor holds, and what SAC.train compares
    with the values its graph was captured with)."""
    env = BanditEnv(4, 3, 2, done_every=2)
    vn = HipVecNormalize(env)
    sac = SAC(env, net_arch=(8, 8), device="cpu", learning_starts=10 ** 9, normalizer=vn)
    for _ in range(4):
        sac.env_step()
    key = sac._norm_key()
    assert key == (True, True, 10.0, 10.0, 1e-8)
    vn.clip_obs = 0.25
    assert sac._norm_key() != key and sac._norm_key()[2] == 0.25
    assert float(sac.sample_torch(torch.arange(16))["obs"].abs().max()) == 0.25
    vn.norm_obs = False
    assert torch.equal(sac.sample_torch(torch.arange(16))["obs"], sac.ring["obs"][:16])


def test_gather_norm_is_declared_listed_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "deepmimic_sac_norm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(dm_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_lib.SAC_NORM_EXPORTS) == {"dm_sac_gather_norm"}
    for other in (_lib.EXPORTS, _lib.RENDER_EXPORTS, _lib.TRACE_EXPORTS, _lib.VECNORM_EXPORTS):
        assert not set(_lib.SAC_NORM_EXPORTS) & set(other)
    L = _lib.load_library()
    at = L.dm_sac_gather_norm.argtypes
    assert len(at) == len(L.dm_sac_gather.argtypes) + 1 and at[:-2] == L.dm_sac_gather.argtypes[:-1] and at[-2] is C.POINTER(_lib.DmVecNorm)
    assert "dm_sac_gather_norm" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    # one statement of the transform: the kernels of both files call the header's
    csrc = os.path.join(ROOT, "deepmimic_mujoco_amd", "csrc")
    for f in ("dm_sac.hip", "dm_vecnorm.hip"):
        src = open(os.path.join(csrc, f)).read()
        assert "dm_vn_norm_one(" in src and "float dm_vn_norm_one" not in src and "rsqrt" not in src, f
    assert open(os.path.join(ROOT, "include", "deepmimic_vecnorm.h")).read().count("float dm_vn_norm_one(") == 1


def test_gather_norm_refuses_bad_arguments_on_the_host(monkeypatch):
    """Every refusal comes back as -22 before any HIP call (this machine has no device: a launch would return -5), and the
    driver's call helper names the entry point.  The non-NULL pointers are never dereferenced by a refused call."""
    L = _lib.load_library()
    st = np.zeros(16)                                       # host memory standing in for the statistics: never read
    p = C.c_void_p(st.ctypes.data)

    def desc(**kw):
        d = dict(N=3, D=5, device=0, training=1, norm_obs=1, norm_reward=1, gamma=0.99, epsilon=1e-8, clip_obs=10.0, clip_reward=10.0,
                 obs_mean=p.value, obs_var=p.value, obs_count=p.value, ret_stats=p.value)
        d.update(kw)
        return _lib.DmVecNorm(**d)

    def args(B=4, N=3, D=5, A=2, null=None, vn=None):
        ptrs = [None if i == null else p for i in range(14)]          # counter, ring, 5 ring arrays, 6 outputs, idx_out
        return [B, N, D, A, 7] + ptrs + [C.byref(vn) if vn is not None else None, None]

    good = desc()
    for what, a in [("B < 1", args(B=0, vn=good)), ("N < 1", args(N=0, vn=good)), ("D < 1", args(D=0, vn=good)), ("A < 1", args(A=0, vn=good)),
                    ("null struct", args()), ("D of the struct", args(vn=desc(D=6))), ("null statistics", args(vn=desc(obs_var=None))),
                    ("null ret_stats", args(vn=desc(ret_stats=None))), ("clip_obs 0", args(vn=desc(clip_obs=0.0))),
                    ("clip_reward nan", args(vn=desc(clip_reward=float("nan")))), ("epsilon < 0", args(vn=desc(epsilon=-1e-8))),
                    ("gamma", args(vn=desc(gamma=1.5))), ("struct N", args(vn=desc(N=0)))] + \
                   [("null pointer %d" % i, args(null=i, vn=good)) for i in range(13)]:
        assert L.dm_sac_gather_norm(*a) == -22, what

    class _Stream:
        cuda_stream = 0
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: _Stream())
    with pytest.raises(RuntimeError, match=r"^dm_sac_gather_norm failed \(-22\)$"):
        _lib.call("dm_sac_gather_norm", *args(B=0, vn=good)[:-1], device=torch.device("cpu"))


# Measured on the CPU (seeds 0 and 1, every 100 vec-env steps, 512 fixed contexts): the plain torch learner on the plain bandit of
# test_sac_cpu.py is above that test's bar of -0.05 from 200 steps on (-0.012 / -0.015); the learner below, with the normaliser on the
# badly scaled bandit, from 300 steps on but only just (-0.046 / -0.050) and with margin from 400 (-0.022 / -0.015).  It needs more
# than the plain one, so it gets the existing test's own budget of 700 steps (the allowance is twice that); DESIGN §25 has the table.
BANDIT_STEPS = 700


def test_normalised_learner_learns_the_badly_scaled_bandit():
    """test_sac_cpu.py's bandit, net, batch, learning rate and bar, behind sensors that present half the columns as 50 + 1e-3 x and
    half as 1e3 x, with the normaliser and the budget the plain learner has on the plain bandit."""
    torch.manual_seed(0)
    env = ScaledBanditEnv(32, 3, 2, seed=4)
    vn = HipVecNormalize(env)
    sac = SAC(env, net_arch=(64, 64), batch_size=128, learning_starts=256, learning_rate=1e-3, seed=0, device="cpu", normalizer=vn)
    sac.learn(32 * BANDIT_STEPS, log_interval=0)
    x = torch.rand(512, 3) * 2 - 1
    seen = vn.normalize_obs(env.present(x))                    # predict takes what the policy sees
    r = float(BanditEnv.reward(env, x, sac.predict(seen)).mean())
    rnd = float(BanditEnv.reward(env, x, torch.rand(512, 2) * 4 - 2).mean())
    print("measured reward %.4f after %d steps (random %.3f)" % (r, BANDIT_STEPS, rnd))
    assert r > -0.05 and rnd < -1.0, (r, rnd)
    assert vn.obs_rms.count == pytest.approx(1e-4 + 32 * (BANDIT_STEPS + 1))
