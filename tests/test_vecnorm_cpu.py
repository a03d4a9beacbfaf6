"""HipVecNormalize, the parts that need no GPU: the numpy restatement (tests/vecnorm_ref.py) against a closed form, the C ABI's
names and refusals (include/deepmimic_vecnorm.h), and the wrapper's logic over a CPU stub env, step by step against the
restatement.  On a CPU device the wrapper runs the same formulas as torch fp64 ops, so the comparisons below hold to fp64 reordering
noise (1e-12 on the statistics) and one fp32 rounding (2^-23 |ref| + 1e-9 on the outputs)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from deepmimic_mujoco_amd import _lib
from deepmimic_mujoco_amd.vec_env import Box
from deepmimic_mujoco_amd.vec_normalize import HipVecNormalize
from monitor_ref import MonitorRef
from vecnorm_ref import RunningMeanStd, VecNormalizeRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DM_EINVAL = -22


# ------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("shape", [(), (5,)])
def test_restatement_equals_the_closed_form(shape):
    """k updates = the moments of the concatenated data merged with a prior of weight 1e-4 at mean 0, variance 1 (Chan's merge is
    associative): to 1e-12."""
    rng = np.random.default_rng(0)
    rms = RunningMeanStd(shape)
    chunks = [rng.standard_normal((n,) + shape) * 3.0 + 50.0 for n in (1, 7, 64, 3, 129)]
    for c in chunks:
        rms.update(c)
    x = np.concatenate(chunks)
    n, w = x.shape[0], 1e-4
    mean = x.mean(0) * n / (n + w)
    var = (w * 1.0 + n * x.var(0) + x.mean(0) ** 2 * w * n / (n + w)) / (n + w)
    assert rms.count == pytest.approx(n + w, rel=1e-15)
    assert np.max(np.abs(rms.mean - mean) / np.abs(mean)) < 1e-12
    assert np.max(np.abs(rms.var - var) / var) < 1e-12


# ------------------------------------------------------------------------------------------ the C ABI without a device
def test_header_exports_and_library_agree():
    hdr = open(os.path.join(ROOT, "include", "deepmimic_vecnorm.h")).read()
    declared = set(re.findall(r"\b(dm_vecnorm[a-z_0-9]*)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(_lib.VECNORM_EXPORTS), declared ^ set(_lib.VECNORM_EXPORTS)
    L = _lib.load_library()
    for name in declared:
        assert getattr(L, name).argtypes is not None, name
    for other in (_lib.EXPORTS, _lib.RENDER_EXPORTS, _lib.TRACE_EXPORTS):
        assert not set(_lib.VECNORM_EXPORTS) & set(other)
    assert "dm_vecnorm" not in open(os.path.join(ROOT, "include", "deepmimic_hip.h")).read()
    src = open(os.path.join(ROOT, "deepmimic_mujoco_amd", "csrc", "dm_vecnorm.hip")).read()
    assert re.findall(r'#include\s+"([^"]+)"', src) == ["../../include/deepmimic_vecnorm.h"]      # no engine header
    assert "atomic" not in src.lower().replace("no atomics", "")
    body = re.search(r"typedef struct DmVecNorm \{(.*?)\} DmVecNorm;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip(" *") for decl in body.split(";") for f in re.sub(r"^\s*(const\s+)?\w+\s*\**\s", "", decl.strip()).split(",") if f.strip()]
    assert fields == [n for n, _ in _lib.DmVecNorm._fields_]


FAKE = 0x1000      # stands for a device pointer: a refused call dereferences none


def _desc(**kw):
    N, D = kw.get("N", 8), kw.get("D", 5)
    L = _lib.load_library()
    d = dict(N=N, D=D, device=0, training=1, norm_obs=1, norm_reward=1, gamma=0.99, epsilon=1e-8, clip_obs=10.0, clip_reward=10.0,
             obs_mean=FAKE, obs_var=FAKE, obs_count=FAKE, ret_stats=FAKE, returns=FAKE, scratch=FAKE,
             scratch_bytes=max(0, L.dm_vecnorm_scratch_bytes(max(N, 1), max(D, 1))))
    d.update(kw)
    return _lib.DmVecNorm(**d)


BAD = [dict(N=0), dict(D=0), dict(device=-1), dict(obs_mean=None), dict(obs_var=None), dict(obs_count=None), dict(ret_stats=None),
       dict(gamma=1.5), dict(gamma=-0.1), dict(gamma=float("nan")), dict(epsilon=-1.0), dict(clip_obs=0.0), dict(clip_reward=-1.0)]
BAD_STATEFUL = [dict(returns=None), dict(scratch=None), dict(scratch_bytes=8)]


@pytest.mark.parametrize("bad", BAD + BAD_STATEFUL, ids=[str(b) for b in BAD + BAD_STATEFUL])
def test_a_bad_struct_is_refused_without_a_device(bad):
    L = _lib.load_library()
    d = _desc(**bad)
    assert L.dm_vecnorm_step(C.byref(d), FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None) == DM_EINVAL
    assert len(L.dm_vecnorm_last_error()) > 0
    assert L.dm_vecnorm_reset(C.byref(d), FAKE, FAKE, None) == DM_EINVAL
    if bad in BAD:
        assert L.dm_vecnorm_apply(C.byref(d), 3, FAKE, FAKE, FAKE, FAKE, None) == DM_EINVAL
        assert len(L.dm_vecnorm_last_error()) > 0


def test_bad_arguments_are_refused_without_a_device():
    L = _lib.load_library()
    d = _desc()
    assert L.dm_vecnorm_step(None, *[FAKE] * 7, None) == DM_EINVAL
    assert L.dm_vecnorm_reset(None, FAKE, FAKE, None) == DM_EINVAL
    assert L.dm_vecnorm_apply(None, 3, FAKE, FAKE, None, None, None) == DM_EINVAL
    for k in (0, 1, 2, 4, 5):                            # obs, rew, done, obs_out, rew_out
        args = [FAKE] * 7
        args[k] = None
        assert L.dm_vecnorm_step(C.byref(d), *args, None) == DM_EINVAL, k
        assert len(L.dm_vecnorm_last_error()) > 0
    for args in ([FAKE, FAKE, FAKE, None, FAKE, FAKE, FAKE], [FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None]):      # tobs without its output, or the reverse
        assert L.dm_vecnorm_step(C.byref(d), *args, None) == DM_EINVAL
    for args in ((None, FAKE), (FAKE, None)):
        assert L.dm_vecnorm_reset(C.byref(d), *args, None) == DM_EINVAL
    for n in (0, -3):
        assert L.dm_vecnorm_apply(C.byref(d), n, FAKE, FAKE, None, None, None) == DM_EINVAL
        assert b"n < 1" in L.dm_vecnorm_last_error()
    for args in ((FAKE, None, None, None), (None, None, FAKE, None), (None, None, None, None)):
        assert L.dm_vecnorm_apply(C.byref(d), 3, *args, None) == DM_EINVAL
    assert L.dm_vecnorm_scratch_bytes(0, 5) < 0 and L.dm_vecnorm_scratch_bytes(5, 0) < 0
    # [chunks, 2, D + 1] doubles and one more: 64-row chunks up to 16 384 envs, at most 256 chunks beyond
    assert L.dm_vecnorm_scratch_bytes(1, 1) == (2 * 2 + 1) * 8 and L.dm_vecnorm_scratch_bytes(65, 98) == (2 * 2 * 99 + 1) * 8
    assert L.dm_vecnorm_scratch_bytes(4096, 98) == (64 * 2 * 99 + 1) * 8 and L.dm_vecnorm_scratch_bytes(1 << 20, 3) == (256 * 2 * 4 + 1) * 8


# ------------------------------------------------------------------------------------------ the wrapper over a CPU stub env
class StubEnv:
    """The tensor surface of a batch env on the CPU: scripted observations (one offset column, one constant column, one column
    beyond the clip), rewards and done flags, none of which depend on the actions."""

    def __init__(self, n=6, d=5, a=3, seed=0, done_every=5):
        self.num_envs, self.device = n, torch.device("cpu")
        self.observation_space, self.action_space = Box(-np.inf, np.inf, (d,), np.float32), Box(-1.0, 1.0, (a,), np.float32)
        self.rng, self.t, self.done_every = np.random.default_rng(seed), 0, done_every
        self.d = d
        self.closed = False

    def _obs(self):
        x = self.rng.standard_normal((self.num_envs, self.d))
        x[:, 0] = 50.0 + 1e-3 * x[:, 0]
        x[:, 1] = 0.25
        x[:, 2] *= 40.0
        return torch.tensor(x, dtype=torch.float32)

    def reset_tensor(self):
        return self._obs()

    def step_tensor(self, actions):
        assert tuple(actions.shape) == (self.num_envs, self.action_space.shape[0])
        self.t += 1
        done = torch.tensor([(self.t + 2 * e) % self.done_every == 0 for e in range(self.num_envs)], dtype=torch.uint8)
        rew = torch.tensor(self.rng.random(self.num_envs), dtype=torch.float32)
        return dict(obs=self._obs(), rew=rew, done=done, terminal_obs=self._obs())

    def close(self):
        self.closed = True


def _close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    assert np.all(np.abs(got - ref) <= 2.0 ** -23 * np.abs(ref) + 1e-9), (what, float(np.abs(got - ref).max()))


def _stats_close(vn, ref, tol=1e-12):
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(np.abs(np.asarray(b)), 1e-300)))
    assert rel(vn.obs_rms.mean, ref.obs_rms.mean) < tol and rel(vn.obs_rms.var, ref.obs_rms.var) < tol
    assert rel(vn.obs_rms.count, ref.obs_rms.count) < tol
    assert rel(vn.ret_rms.mean, ref.ret_rms.mean) < tol and rel(vn.ret_rms.var, ref.ret_rms.var) < tol
    assert rel(vn.ret_rms.count, ref.ret_rms.count) < tol
    assert np.allclose(vn.returns.numpy(), ref.returns, rtol=tol, atol=0)


FLAGS = [dict(), dict(norm_obs=False), dict(norm_reward=False), dict(norm_obs=False, norm_reward=False), dict(gamma=0.5, clip_obs=2.0, clip_reward=0.5)]


@pytest.mark.parametrize("kw", FLAGS, ids=[str(k) for k in FLAGS])
def test_wrapper_follows_the_restatement_step_by_step(kw):
    env, twin = StubEnv(seed=3), StubEnv(seed=3)
    vn = HipVecNormalize(env, **kw)
    ref = VecNormalizeRef(env.num_envs, env.d, **kw)
    _close(vn.reset_tensor(), ref.reset(twin.reset_tensor().numpy()), "reset")
    _stats_close(vn, ref)
    act = torch.zeros(env.num_envs, 3)
    saw_done = 0
    for t in range(12):
        out = vn.step_tensor(act)
        raw = twin.step_tensor(act)
        before = ref.returns.copy()
        o, r, tb = ref.step(raw["obs"].numpy(), raw["rew"].numpy(), raw["done"].numpy(), raw["terminal_obs"].numpy())
        _close(out["obs"], o, "obs %d" % t)              # normalised with the statistics this very step updated
        _close(out["rew"], r, "rew %d" % t)
        dn = raw["done"].numpy() != 0
        saw_done += int(dn.sum())
        _close(out["terminal_obs"], tb, "terminal_obs %d" % t)
        assert np.array_equal(out["terminal_obs"].numpy()[~dn], raw["terminal_obs"].numpy()[~dn])      # rows of live envs pass through
        assert np.array_equal(out["obs_raw"].numpy(), raw["obs"].numpy()) and np.array_equal(out["rew_raw"].numpy(), raw["rew"].numpy())
        assert np.array_equal(vn.get_original_obs(), raw["obs"].numpy()) and np.array_equal(vn.get_original_reward(), raw["rew"].numpy())
        # returns: discounted before the reward is normalised, zeroed for done envs after it
        assert np.all(vn.returns.numpy()[dn] == 0) and np.allclose(vn.returns.numpy()[~dn], (before * ref.gamma + raw["rew"].numpy().astype(np.float64))[~dn], rtol=1e-12)
        _stats_close(vn, ref)
    assert saw_done > 3
    if kw.get("norm_obs", True):
        assert float(out["obs"][:, 2].abs().max()) <= kw.get("clip_obs", 10.0)
        # update-then-normalise: the statistics of step 0 already hold step 0's batch
        assert vn.obs_rms.count == pytest.approx(1e-4 + 13 * env.num_envs)
    else:
        assert vn.obs_rms.count == 1e-4 and np.array_equal(out["obs"].numpy(), raw["obs"].numpy())
    assert vn.ret_rms.count == pytest.approx(1e-4 + 12 * env.num_envs)          # updated whenever training, norm_reward or not


def test_training_false_leaves_the_statistics_alone_and_flags_can_be_set_between_steps():
    env, twin = StubEnv(seed=5), StubEnv(seed=5)
    vn, ref = HipVecNormalize(env), VecNormalizeRef(env.num_envs, env.d)
    vn.reset_tensor(), ref.reset(twin.reset_tensor().numpy())
    act = torch.zeros(env.num_envs, 3)
    for _ in range(4):
        vn.step_tensor(act)
        raw = twin.step_tensor(act)
        ref.step(*[raw[k].numpy() for k in ("obs", "rew", "done", "terminal_obs")])
    vn.training = ref.training = False
    frozen = vn._state.clone()
    for _ in range(3):
        out = vn.step_tensor(act)
        raw = twin.step_tensor(act)
        o, r, tb = ref.step(*[raw[k].numpy() for k in ("obs", "rew", "done", "terminal_obs")])
        _close(out["obs"], o, "obs"), _close(out["rew"], r, "rew"), _close(out["terminal_obs"], tb, "tobs")
    assert torch.equal(vn._state, frozen)                # bit for bit
    vn.training = ref.training = True
    vn.norm_reward = ref.norm_reward = False
    out = vn.step_tensor(act)
    raw = twin.step_tensor(act)
    o, r, _ = ref.step(*[raw[k].numpy() for k in ("obs", "rew", "done", "terminal_obs")])
    _close(out["obs"], o, "obs"), _close(out["rew"], r, "rew")
    assert np.array_equal(out["rew"].numpy(), raw["rew"].numpy()) and not torch.equal(vn._state, frozen)
    _stats_close(vn, ref)


def test_numpy_protocol_sb3_methods_and_save_load(tmp_path):
    env = StubEnv(seed=7)
    vn = HipVecNormalize(env, clip_obs=5.0, gamma=0.9)
    obs = vn.reset()
    assert isinstance(obs, np.ndarray) and obs.dtype == np.float32 and obs.shape == (6, 5)
    for _ in range(6):
        obs, rew, done, infos = vn.step(np.zeros((6, 3), np.float32))
    assert rew.shape == (6,) and done.dtype == bool and len(infos) == 6
    assert vn.num_envs == 6 and vn.observation_space is env.observation_space and vn.action_space is env.action_space
    assert not hasattr(vn, "step_sub") and vn.unwrapped is env
    raw = vn.get_original_obs()
    _close(vn.normalize_obs(raw), obs, "normalize_obs numpy")
    _close(vn.normalize_obs(torch.tensor(raw)), obs, "normalize_obs tensor")
    _close(vn.normalize_reward(vn.get_original_reward()), rew, "normalize_reward")
    inside = np.abs(obs) < 5.0                           # a clipped element does not come back
    assert np.allclose(vn.unnormalize_obs(obs)[inside], raw[inside], rtol=1e-5, atol=1e-5)
    assert np.allclose(vn.unnormalize_reward(rew), vn.get_original_reward(), rtol=1e-6)
    assert vn.obs_rms.mean.dtype == np.float64 and vn.obs_rms.var.shape == (5,) and isinstance(vn.ret_rms.count, float)
    m = vn.obs_rms.mean
    m[:] = 0                                             # a copy: the state cannot be written through the view
    assert np.abs(vn.obs_rms.mean).max() > 0
    path = str(tmp_path / "p.vecnormalize")
    vn.save(path)
    assert os.path.exists(path)
    back = HipVecNormalize.load(path, StubEnv(seed=8))
    assert torch.equal(back._state, vn._state) and torch.equal(back.returns, vn.returns)          # bitwise
    assert (back.clip_obs, back.gamma, back.training, back.norm_reward) == (5.0, 0.9, True, True)
    sd = vn.state_dict()
    other = HipVecNormalize(StubEnv(seed=9))
    other.load_state_dict(sd)
    assert all(np.array_equal(other.state_dict()[k], sd[k]) for k in sd)
    with pytest.raises(ValueError):
        HipVecNormalize(StubEnv(d=4)).load_state_dict(sd)
    vn.close()
    assert env.closed


def test_ppo_on_cpu_monitors_the_raw_rewards():
    from deepmimic_mujoco_amd.ppo import PPO
    env, twin = StubEnv(seed=11, done_every=4), StubEnv(seed=11, done_every=4)
    vn = HipVecNormalize(env)
    T = 16
    ppo = PPO(vn, net_arch=(16, 8), n_steps=T, batch_size=32, n_epochs=1, device=torch.device("cpu"))
    assert ppo.rollout_path() == "plain"
    ref, mon = VecNormalizeRef(env.num_envs, env.d), MonitorRef(env.num_envs)
    ref.reset(twin.reset_tensor().numpy())
    for _ in range(2):
        buf = ppo.collect_rollouts()
        raws, norms = [], []
        for t in range(T):
            raw = twin.step_tensor(torch.zeros(env.num_envs, 3))
            norms.append(ref.step(raw["obs"].numpy(), raw["rew"].numpy(), raw["done"].numpy())[1])
            raws.append((raw["rew"].numpy(), raw["done"].numpy()))
        mon.feed(np.stack([r for r, _ in raws]), np.stack([d for _, d in raws]))
        _close(buf["rew"], np.stack(norms), "normalised rewards feed GAE")
        assert np.array_equal(buf["rew_raw"].numpy(), np.stack([r for r, _ in raws]))
        assert ppo.stats["ep_rew_mean"] == pytest.approx(mon.ep_rew_mean, rel=1e-6)
        assert ppo.stats["ep_len_mean"] == pytest.approx(mon.ep_len_mean) and ppo.stats["episodes"] == mon.episodes
        assert ppo.stats["mean_reward"] == pytest.approx(float(np.mean([r for r, _ in raws])), rel=1e-5)
        assert abs(ppo.stats["mean_reward"] - float(buf["rew"].mean())) > 1e-3        # not the normalised ones
    rets, lens = ppo.ep_history()
    assert np.allclose(rets, mon.returns(), rtol=1e-6) and np.array_equal(lens, mon.lengths())
    ppo.train(buf)


def test_sac_refuses_the_wrapper_and_train_has_the_flags():
    from deepmimic_mujoco_amd.sac import SAC
    from deepmimic_mujoco_amd.train import build_parser
    with pytest.raises(ValueError, match="HipVecNormalize"):
        SAC(HipVecNormalize(StubEnv()))
    a = build_parser().parse_args([])
    assert a.normalize is False and a.norm_clip_obs == 10.0 and a.norm_clip_reward == 10.0 and a.no_norm_reward is False
    a = build_parser().parse_args(["--normalize", "--norm-clip-obs", "5", "--norm-clip-reward", "2", "--no-norm-reward"])
    assert a.normalize and a.norm_clip_obs == 5.0 and a.norm_clip_reward == 2.0 and a.no_norm_reward
    import inspect
    from deepmimic_mujoco_amd import evaluation
    for f in (evaluation.evaluate_policy, evaluation.run_episodes, evaluation.evaluation_record):
        assert inspect.signature(f).parameters["normalizer"].default is None
