"""SAC(env, n_steps=n) without a GPU: ``sample_torch`` against the fp64 restatement of the n-step semantics (tests/sac_nstep_ref.py)
on rings written directly, with and without a normaliser; n_steps = 3 where every episode has one step is n_steps = 1 bit for bit; the
torch learner with n_steps = 3 learns the bandit; the export of dm_sac_gather_nstep, its host-side refusals and the constructor's.

Bounds, none taken from the code under test (u = 2^-24, S = sum_{j<k} gamma^j |r_j|): |rew - ref| <= (2k + 1) u S, with a normaliser
plus sum_j gamma^j out_bound(r_j); |done' - ref| <= (k + 1) u; observations are the ring's bits without a normaliser and within
out_bound (2^-23 |ref| + 1e-9) with one; actions and k are exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from sac_helpers import BanditEnv
from sac_nstep_ref import SHAPES, done_bound, nstep_batch64, rew_bound, states, written_ring
from sac_vecnorm_ref import out_bound
from vecnorm_ref import VecNormalizeRef
from deepmimic_mujoco_amd import _lib
from deepmimic_mujoco_amd.sac import SAC
from deepmimic_mujoco_amd.vec_normalize import HipVecNormalize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMA, CLIP_REW = 0.9, 1.5
KINDS = {"full", "cut by done", "cut at newest", "done at newest", "wraps"}


def _within(got, ref, bnd, what):
    err = np.abs(np.asarray(got, np.float64) - ref)
    print("measured %-34s worst error / bound %.3g" % (what, float(np.max(np.where(err == 0, 0.0, err / bnd)))))
    assert np.all(err <= bnd), (what, float(np.max(err / bnd)))


def _learner(N, cap, D, A, n, normalize):
    """A CPU learner whose normaliser (if any) has seen four real steps, with a ring of `cap` steps to be written directly."""
    env = BanditEnv(N, D, A, seed=2, done_every=3)
    vn = HipVecNormalize(env, clip_reward=CLIP_REW) if normalize else None
    sac = SAC(env, net_arch=(8, 8), batch_size=8, buffer_size=cap * N, learning_starts=10 ** 9, gamma=GAMMA, seed=1, device="cpu",
              normalizer=vn, n_steps=n)
    assert sac.cap_steps == cap and sac.n_steps == n
    vref = None
    if normalize:
        for _ in range(4):
            sac.env_step()
        vref = VecNormalizeRef(N, D, clip_reward=CLIP_REW)
        vref.obs_rms.mean, vref.obs_rms.var, vref.ret_rms.var = vn.obs_rms.mean, vn.obs_rms.var, float(vn.ret_rms.var[0])
    return sac, vref


def _write(sac, ring, N, fill, pos):
    """The ring and its state as `fill` stored steps with the write position at `pos`; rows never stored are NaN: a read shows."""
    for k, v in ring.items():
        sac.ring[k].copy_(torch.as_tensor(v))
        sac.ring[k][fill * N:] = float("nan")
    sac._pos, sac._fill = pos, fill
    sac.ring_state[0], sac.ring_state[1] = pos, fill


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalizer"])
@pytest.mark.parametrize("shape,mod", SHAPES, ids=["3-7-5-2", "7-5-98-23"])
def test_sample_torch_follows_the_restatement(shape, mod, normalize):
    """Every stored row of both small rings in all three ring states, n = 1, 2, 3, 5 and 64.  At (cap, 3) with n = 3 all five kinds of
    chain occur: full, cut by a done, cut at the newest step, a done at the newest step, and one that goes from step cap - 1 to 0."""
    N, cap, D, A = shape
    ring = written_ring(N, cap, D, A, mod)
    for n in (1, 2, 3, 5, 64):
        sac, vref = _learner(N, cap, D, A, n, normalize)
        for fill, pos in states(cap):
            _write(sac, ring, N, fill, pos)
            idx = np.arange(fill * N)
            ref = nstep_batch64(ring, idx, N, cap, pos, n, GAMMA, vref)
            b = sac.sample_torch(torch.as_tensor(idx))
            tag = "n%d fill%d pos%d " % (n, fill, pos)
            assert all(b[k].dtype == torch.float32 for k in ("obs", "act", "rew", "next_obs", "done"))
            if n > 1:
                assert np.array_equal(b["k"].numpy(), ref["k"]), tag
            else:
                assert int(ref["k"].max()) == 1
            assert np.array_equal(b["act"].numpy(), ring["act"][idx])
            if normalize:
                _within(b["obs"].numpy(), ref["obs"], out_bound(ref["obs"]), tag + "obs")
                _within(b["next_obs"].numpy(), ref["next_obs"], out_bound(ref["next_obs"]), tag + "next_obs")
                assert float(np.abs(ref["rew"]).max()) > 0 and not np.array_equal(b["obs"].numpy(), ring["obs"][idx])
            else:
                assert np.array_equal(b["obs"].numpy(), ring["obs"][idx]) and np.array_equal(b["next_obs"].numpy(), ring["next_obs"][ref["last"]])
            _within(b["rew"].numpy(), ref["rew"], rew_bound(ref), tag + "rew")
            _within(b["done"].numpy(), ref["done"], done_bound(ref), tag + "done'")
            one = ref["k"] == 1                              # a chain of one row: the stored flag itself
            assert np.array_equal(b["done"].numpy()[one], ring["done"][idx][one])
            if (fill, pos) == (cap, 3) and n == 3:
                assert set().union(*ref["kinds"]) >= KINDS, set().union(*ref["kinds"])
            if n == 64:                                      # no chain is longer than the ring, none reads past the newest step
                assert int(ref["k"].max()) <= cap
    assert bool(torch.isfinite(b["rew"]).all())


def _bandit_run(n_steps, done_every, steps, seed=0, **kw):
    torch.manual_seed(0)
    env = BanditEnv(32, 3, 2, seed=4, done_every=done_every)
    sac = SAC(env, net_arch=(64, 64), batch_size=128, learning_starts=256, learning_rate=1e-3, seed=seed, device="cpu", n_steps=n_steps, **kw)
    sac.learn(32 * steps, log_interval=0)
    return env, sac


def test_one_step_episodes_make_n_steps_3_the_one_step_learner():
    """done every step: every chain is cut at its first row, so n_steps = 3 is n_steps = 1 bit for bit after the same learn call:
    weights, targets, sac_state and Adam moments."""
    (_, a), (_, b) = _bandit_run(1, 1, 40), _bandit_run(3, 1, 40)
    assert a._n_updates == b._n_updates > 20
    for x, y in zip(a.state_tensors() + [a.ring["rew"]], b.state_tensors() + [b.ring["rew"]]):
        assert torch.equal(x, y)


def test_cpu_learner_with_n_steps_3_learns_the_bandit():
    """test_cpu_learner_learns_the_bandit's settings, budget and bar with episodes of four steps and n_steps = 3."""
    env, sac = _bandit_run(3, 4, 700)
    obs = torch.rand(512, 3) * 2 - 1
    r = float(env.reward(obs, sac.predict(obs)).mean())
    rnd = float(env.reward(obs, torch.rand(512, 2) * 4 - 2).mean())
    print("measured reward %.4f after 700 steps with n_steps = 3 (random %.3f)" % (r, rnd))
    assert r > -0.05 and rnd < -1.0, (r, rnd)
    assert 0.0 < float(sac.ring["done"][:sac._fill * 32].mean()) < 1.0


def test_constructor_and_flag_refuse_bad_n_steps():
    from deepmimic_mujoco_amd import train
    env = BanditEnv(4, 3, 2)
    for bad in (0, -1, 65, 2.0, "3", None, True):
        with pytest.raises(ValueError, match="n_steps"):
            SAC(env, net_arch=(8, 8), device="cpu", n_steps=bad)
    assert SAC(env, net_arch=(8, 8), device="cpu").n_steps == 1 and SAC(env, net_arch=(8, 8), device="cpu", n_steps=64).n_steps == 64
    args = train.build_parser().parse_args(["--algo", "sac", "--n-step", "3"])
    assert args.n_step == 3 and train.build_parser().parse_args([]).n_step == 1
    for argv in (["--algo", "sac", "--n-step", "0"], ["--algo", "sac", "--n-step", "65"], ["--n-step", "3"]):
        with pytest.raises(SystemExit):
            train.main(argv)
    src = open(os.path.join(ROOT, "deepmimic_mujoco_amd", "train.py")).read()
    assert "n_steps=args.n_step" in src and '"n_steps": sac.n_steps' in src


def test_n_steps_is_not_checkpoint_state(tmp_path):
    _, a = _bandit_run(3, 4, 12)
    path = str(tmp_path / "sac.pt")
    a.save(path)
    assert "n_steps" not in torch.load(path)
    b = SAC(BanditEnv(32, 3, 2), net_arch=(64, 64), device="cpu").load(path)
    assert b.n_steps == 1 and torch.equal(a.actor, b.actor)


def test_gather_nstep_is_declared_listed_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "deepmimic_sac_nstep.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(dm_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_lib.SAC_NSTEP_EXPORTS) == {"dm_sac_gather_nstep"}
    from deepmimic_mujoco_amd import g1
    for other in (_lib.EXPORTS, _lib.RENDER_EXPORTS, _lib.TRACE_EXPORTS, _lib.VECNORM_EXPORTS, _lib.SAC_NORM_EXPORTS, g1.EXPORTS):
        assert not set(_lib.SAC_NSTEP_EXPORTS) & set(other)
    for other in ("deepmimic_hip.h", "deepmimic_sac_norm.h"):
        assert "dm_sac_gather_nstep" not in open(os.path.join(ROOT, "include", other)).read()
    assert int(re.search(r"#define DM_SAC_NSTEP_MAX (\d+)", hdr).group(1)) == _lib.SAC_NSTEP_MAX == 64
    L = _lib.load_library()
    at, base = L.dm_sac_gather_nstep.argtypes, L.dm_sac_gather.argtypes
    assert at[:len(base) - 1] == base[:-1] and at[len(base) - 1:] == [C.c_int, C.c_int, C.c_float, C.c_void_p, C.POINTER(_lib.DmVecNorm), C.c_void_p]
    assert "dm_sac_gather_nstep" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    # one kernel, templated on the normaliser, that calls the header's transform
    src = open(os.path.join(ROOT, "deepmimic_mujoco_amd", "csrc", "dm_sac.hip")).read()
    assert src.count("void __launch_bounds__(64) sac_gather_nstep_kernel(") == 1 and "template <bool NORM>" in src


def test_gather_nstep_refuses_bad_arguments_on_the_host(monkeypatch):
    """Every refusal comes back as -22 before any HIP call (without a device a launch would return -5); the non-NULL pointers are never
    dereferenced by a refused call."""
    L = _lib.load_library()
    st = np.zeros(16)
    p = C.c_void_p(st.ctypes.data)

    def desc(**kw):
        d = dict(N=3, D=5, device=0, training=1, norm_obs=1, norm_reward=1, gamma=0.99, epsilon=1e-8, clip_obs=10.0, clip_reward=10.0,
                 obs_mean=p.value, obs_var=p.value, obs_count=p.value, ret_stats=p.value)
        d.update(kw)
        return _lib.DmVecNorm(**d)

    def args(B=4, N=3, D=5, A=2, null=None, cap=7, n=3, gamma=0.99, vn=None):
        ptrs = [None if i == null else p for i in range(14)]          # counter, ring, 5 ring arrays, 6 outputs, idx_out
        return [B, N, D, A, 7] + ptrs + [cap, n, gamma, p, C.byref(vn) if vn is not None else None, None]

    good = desc()
    cases = [("B < 1", args(B=0)), ("N < 1", args(N=0)), ("D < 1", args(D=0)), ("A < 1", args(A=0)), ("cap_steps < 1", args(cap=0)),
             ("n_steps 0", args(n=0)), ("n_steps -1", args(n=-1)), ("n_steps 65", args(n=65)), ("gamma < 0", args(gamma=-0.1)),
             ("gamma > 1", args(gamma=1.0001)), ("gamma nan", args(gamma=float("nan"))), ("n_steps 65 with struct", args(n=65, vn=good)),
             ("D of the struct", args(vn=desc(D=6))), ("null statistics", args(vn=desc(obs_var=None))),
             ("null ret_stats", args(vn=desc(ret_stats=None))), ("clip_obs 0", args(vn=desc(clip_obs=0.0))),
             ("clip_reward nan", args(vn=desc(clip_reward=float("nan")))), ("epsilon < 0", args(vn=desc(epsilon=-1e-8))),
             ("gamma of the struct", args(vn=desc(gamma=1.5))), ("struct N", args(vn=desc(N=0)))]
    cases += [("null pointer %d" % i, args(null=i)) for i in range(13)] + [("null pointer %d with struct" % i, args(null=i, vn=good)) for i in (0, 12)]
    for what, a in cases:
        assert L.dm_sac_gather_nstep(*a) == -22, what

    class _Stream:
        cuda_stream = 0
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: _Stream())
    with pytest.raises(RuntimeError, match=r"^dm_sac_gather_nstep failed \(-22\)$"):
        _lib.call("dm_sac_gather_nstep", *args(n=0)[:-1], device=torch.device("cpu"))
