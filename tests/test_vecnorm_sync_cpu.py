"""HipVecNormalize(sync_group=...) without a GPU: the torch fp64 path of the base / acc / sync scheme on two gloo ranks
over a scripted env, against the numpy restatement (tests/vecnorm_sync_ref.py) and against ONE VecNormalizeRef that saw the rows of
both ranks; the C ABI's new names and refusals; persistence between synchronised and plain objects.

Bounds: statistics 1e-10 relative (the bound of tests/test_vecnorm_kernels_gpu.py; every merge is a sum of non-negative terms, so
regrouping the same rows costs a few ulp: the restatement against the single normaliser is asserted on its own first), outputs one
fp32 rounding (2^-23 |ref| + 1e-9), across ranks after a sync(): torch.equal."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from deepmimic_mujoco_amd import _lib
from deepmimic_mujoco_amd.vec_env import Box
from deepmimic_mujoco_amd.vec_normalize import HipVecNormalize
from vecnorm_ref import VecNormalizeRef
from vecnorm_sync_ref import SyncRankRef, sync as ref_sync

W, N, D, A = 2, 3, 5, 2
ROLLOUTS, T = 3, 5
DM_EINVAL = -22
FAKE = 0x1000


def script(rank):
    """What rank ``rank``'s env returns: obs [1 + ROLLOUTS * T, N, D] (row 0: the reset), rew and done [ROLLOUTS * T, N].  Column
    scales 1e-3, 1, 1e3 and 30, column 1 constant; column 0 has a large mean beside its small spread."""
    rng = np.random.default_rng(100 + rank)
    steps = ROLLOUTS * T
    x = rng.standard_normal((steps + 1, N, D))
    x[:, :, 0] = 50.0 + 1e-3 * x[:, :, 0]
    x[:, :, 1] = 0.25
    x[:, :, 3] *= 1e3
    x[:, :, 4] = 30.0 * x[:, :, 4] - 7.0 * rank
    rew = rng.random((steps, N)) * (1.0 + rank)
    done = (rng.random((steps, N)) < 0.25).astype(np.uint8)
    return x.astype(np.float32), rew.astype(np.float32), done


class ScriptedEnv:
    """The tensor surface of a batch env on the CPU, replaying ``script(rank)``; the actions are ignored."""

    def __init__(self, rank=0, n=N, d=D):
        self.num_envs, self.device = n, torch.device("cpu")
        self.observation_space, self.action_space = Box(-np.inf, np.inf, (d,), np.float32), Box(-1.0, 1.0, (A,), np.float32)
        self.obs, self.rew, self.done = (torch.tensor(a) for a in script(rank))
        if (n, d) != (N, D):
            self.obs = torch.zeros(self.obs.shape[0], n, d)
        self.t = 0

    def reset_tensor(self):
        return self.obs[0].clone()

    def step_tensor(self, actions):
        t = self.t
        self.t = (t + 1) % self.rew.shape[0]
        return dict(obs=self.obs[t + 1].clone(), rew=self.rew[t].clone(), done=self.done[t].clone(), terminal_obs=self.obs[t].clone())

    def close(self):
        pass


def _rank_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    # rank 0 names the default group, rank 1 passes it: both spellings of the same group
    vn = HipVecNormalize(ScriptedEnv(rank), sync_group="world" if rank == 0 else dist.group.WORLD)
    act = torch.zeros(N, A)
    steps, synced = [], []
    first = vn.reset_tensor().numpy().copy()
    after_reset = vn._state.numpy().copy()
    for _ in range(ROLLOUTS):
        for _ in range(T):
            out = vn.step_tensor(act)
            steps.append((out["obs"].numpy().copy(), out["rew"].numpy().copy(), out["terminal_obs"].numpy().copy(), vn._state.numpy().copy(),
                          vn.returns.numpy().copy()))
        vn.sync()
        synced.append((vn._state.numpy().copy(), vn._base.numpy().copy(), vn._acc.numpy().copy()))
    q.put((rank, first, after_reset, steps, synced, vn.sync_calls))
    dist.barrier()
    dist.destroy_process_group()


def rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(got == ref, 0.0, np.abs(got - ref) / np.abs(ref))))


def _close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    assert np.all(np.abs(got - ref) <= 2.0 ** -23 * np.abs(ref) + 1e-9), (what, float(np.abs(got - ref).max()))


def single_row(one):
    return np.concatenate([one.obs_rms.mean, one.obs_rms.var, [one.obs_rms.count], [one.ret_rms.mean, one.ret_rms.var, one.ret_rms.count]])


def restated():
    """-> per rank the restatement's (reset obs, state after reset, per step (obs, rew, tobs, running, returns)), per sync the agreed
    row, and per sync the row of ONE VecNormalizeRef fed both ranks' rows, rank 0's first."""
    scripts = [script(r) for r in range(W)]
    ranks = [SyncRankRef(N, D) for _ in range(W)]
    one = VecNormalizeRef(W * N, D)
    cat = lambda k, t: np.concatenate([s[k][t] for s in scripts])
    first = [r.reset(s[0][0]) for r, s in zip(ranks, scripts)]
    after_reset = [r.running_row() for r in ranks]
    one.reset(cat(0, 0))
    steps, agreed, single = [[] for _ in range(W)], [], []
    for t in range(ROLLOUTS * T):
        for k, (r, s) in enumerate(zip(ranks, scripts)):
            o, rw, tb = r.step(s[0][t + 1], s[1][t], s[2][t], s[0][t])
            steps[k].append((o, rw, tb, r.running_row(), r.returns.copy()))
        one.step(cat(0, t + 1), cat(1, t), cat(2, t))
        if (t + 1) % T == 0:
            ref_sync(ranks)
            assert all(np.array_equal(r.running_row(), ranks[0].running_row()) and np.array_equal(r.base_row(), r.running_row()) for r in ranks)
            assert all(not r.acc_row().any() for r in ranks)
            agreed.append(ranks[0].running_row())
            single.append(single_row(one))
    return first, after_reset, steps, agreed, single


def test_the_restatement_alone_equals_one_normaliser_that_saw_every_row():
    """The claim of the scheme, on the reference side only: after every synchronisation the agreed statistics are, to rounding, those
    of one VecNormalize fed the concatenated rows."""
    _, _, steps, agreed, single = restated()
    assert len(agreed) == ROLLOUTS
    for k, (a, s) in enumerate(zip(agreed, single)):
        worst = rel(a, s)
        print("restatement against one normaliser, sync %d: %.3g (bound 1e-10)" % (k, worst))
        assert worst <= 1e-10
        assert a[2 * D] == pytest.approx(1e-4 + W * N * (1 + (k + 1) * T), rel=1e-14)
    # between synchronisations the ranks do differ: each normalises with the agreed statistics plus its own rows
    assert rel(steps[0][2][3], steps[1][2][3]) > 1e-3


@pytest.fixture(scope="module")
def two_ranks():
    port = 29700 + (os.getpid() % 2000)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, W, port, q)) for r in range(W)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=180) for _ in range(W)], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


def test_two_gloo_ranks_follow_the_restatement_step_by_step(two_ranks):
    first, after_reset, steps, agreed, _ = restated()
    for rank, g_first, g_reset, g_steps, g_synced, calls in two_ranks:
        assert calls == ROLLOUTS
        _close(g_first, first[rank], "reset obs")
        assert rel(g_reset, after_reset[rank]) <= 1e-10
        assert len(g_steps) == ROLLOUTS * T
        for t, (got, want) in enumerate(zip(g_steps, steps[rank])):
            _close(got[0], want[0], "obs %d" % t), _close(got[1], want[1], "rew %d" % t), _close(got[2], want[2], "terminal_obs %d" % t)
            assert rel(got[3], want[3]) <= 1e-10, (rank, t)
            assert rel(got[4], want[4]) <= 1e-12, (rank, t)
        for k, (state, base, acc) in enumerate(g_synced):
            assert rel(state, agreed[k]) <= 1e-10
            assert np.array_equal(state, base) and not acc.any()


def test_after_every_sync_the_ranks_are_bit_identical_and_equal_one_normaliser(two_ranks):
    single = restated()[4]
    (_, _, _, steps0, sync0, _), (_, _, _, steps1, sync1, _) = two_ranks
    for k in range(ROLLOUTS):
        assert torch.equal(torch.tensor(sync0[k][0]), torch.tensor(sync1[k][0]))
        worst = rel(sync0[k][0], single[k])
        print("two ranks against one normaliser, sync %d: %.3g (bound 1e-10)" % (k, worst))
        assert worst <= 1e-10
    # and in between they are not: each rank's own rows are in its statistics
    assert not np.array_equal(steps0[T - 1][3], steps1[T - 1][3])


def test_state_dict_save_and_load_between_synchronised_and_plain_objects(tmp_path):
    """A synchronised object in a process without a process group is a world of one.  What it saves is ``running``; loading sets
    base = running and empties acc; the file loads into a plain object and back."""
    act = torch.zeros(N, A)
    vs = HipVecNormalize(ScriptedEnv(0), sync_group="world", clip_obs=5.0)
    plain = HipVecNormalize(ScriptedEnv(0), clip_obs=5.0)
    assert vs.synced and not plain.synced
    vs.reset_tensor(), plain.reset_tensor()
    for _ in range(4):
        a, b = vs.step_tensor(act), plain.step_tensor(act)
    assert float(vs._acc[2 * D]) == 5 * N and float(vs._base[2 * D]) == 1e-4           # nothing synchronised yet
    assert rel(vs._state.numpy(), plain._state.numpy()) <= 1e-10                         # one rank: the same statistics, regrouped
    _close(a["obs"], b["obs"].numpy(), "obs")
    path = str(tmp_path / "s.vecnormalize")
    vs.save(path)
    sd = vs.state_dict()
    assert sorted(sd) == sorted(plain.state_dict())
    back = HipVecNormalize.load(path, ScriptedEnv(0))                                    # synchronised -> plain
    assert not back.synced and torch.equal(back._state, vs._state) and torch.equal(back.returns, vs.returns) and back.clip_obs == 5.0
    again = HipVecNormalize.load(path, ScriptedEnv(0), sync_group="world")               # -> synchronised
    assert again.synced and torch.equal(again._state, vs._state) and torch.equal(again._base, vs._state) and not again._acc.any()
    path2 = str(tmp_path / "p.vecnormalize")
    plain.save(path2)                                                                    # plain -> synchronised
    other = HipVecNormalize(ScriptedEnv(1), sync_group="world")
    other.load_state_dict(plain.state_dict())
    assert torch.equal(other._state, plain._state) and torch.equal(other._base, plain._state) and not other._acc.any()
    # both continue alike from the loaded statistics, and a sync() of the world of one changes nothing but the bookkeeping
    o1, o2 = other.step_tensor(act), back.step_tensor(act)
    before = other._state.clone()
    other.sync()
    assert torch.equal(other._state, before) and torch.equal(other._base, before) and not other._acc.any() and other.sync_calls == 1
    with pytest.raises(RuntimeError, match="sync_group"):
        plain.sync()
    with pytest.raises(ValueError, match="sync_group"):
        HipVecNormalize(ScriptedEnv(0), sync_group="everyone")


def test_ppo_synchronises_once_per_rollout_and_a_plain_wrapper_never():
    from deepmimic_mujoco_amd.ppo import PPO
    vn = HipVecNormalize(ScriptedEnv(0), sync_group="world")
    ppo = PPO(vn, net_arch=(8, 8), n_steps=T, batch_size=N * T, n_epochs=1, device=torch.device("cpu"))
    for it in range(2):
        buf = ppo.collect_rollouts()
        assert vn.sync_calls == it + 1 == ppo.stats["vecnorm_sync_calls"] and not vn._acc.any() and torch.equal(vn._base, vn._state)
        ppo.train(buf)
    plain = HipVecNormalize(ScriptedEnv(0))
    ppo = PPO(plain, net_arch=(8, 8), n_steps=T, batch_size=N * T, n_epochs=1, device=torch.device("cpu"))
    ppo.collect_rollouts()
    assert plain.sync_calls == 0 and "vecnorm_sync_calls" not in ppo.stats and plain._base is None


# ------------------------------------------------------------------------------------------ the C ABI without a device
def _descs(**kw):
    L = _lib.load_library()
    v = _lib.DmVecNorm(N=8, D=5, device=0, training=1, norm_obs=1, norm_reward=1, gamma=0.99, epsilon=1e-8, clip_obs=10.0, clip_reward=10.0,
                       obs_mean=FAKE, obs_var=FAKE, obs_count=FAKE, ret_stats=FAKE, returns=FAKE, scratch=FAKE,
                       scratch_bytes=L.dm_vecnorm_scratch_bytes(8, 5))
    y = dict(world=2, rank=1, base=FAKE, acc=FAKE, gather=FAKE)
    y.update(kw)
    return v, _lib.DmVecNormSync(**y)


BAD_SYNC = [dict(world=0), dict(world=-1), dict(rank=-1), dict(rank=2), dict(world=1, rank=1), dict(base=None), dict(acc=None), dict(gather=None)]


@pytest.mark.parametrize("bad", BAD_SYNC, ids=str)
def test_a_bad_sync_descriptor_is_refused_without_a_device(bad):
    """-22 before any HIP call (this machine may have no device: a launch would return -5); FAKE pointers are never dereferenced."""
    L = _lib.load_library()
    v, y = _descs(**bad)
    assert L.dm_vecnorm_step_sync(C.byref(v), *[FAKE] * 7, C.byref(y), None) == DM_EINVAL
    assert len(L.dm_vecnorm_last_error()) > 0
    assert L.dm_vecnorm_reset_sync(C.byref(v), FAKE, FAKE, C.byref(y), None) == DM_EINVAL
    assert L.dm_vecnorm_sync_pack(C.byref(v), C.byref(y), None) == DM_EINVAL
    assert L.dm_vecnorm_sync_merge(C.byref(v), C.byref(y), None) == DM_EINVAL
    assert len(L.dm_vecnorm_last_error()) > 0


def test_null_descriptors_and_the_step_arguments_are_refused_without_a_device():
    L = _lib.load_library()
    v, y = _descs()
    for f in (L.dm_vecnorm_sync_pack, L.dm_vecnorm_sync_merge):
        assert f(None, C.byref(y), None) == DM_EINVAL and f(C.byref(v), None, None) == DM_EINVAL
    assert L.dm_vecnorm_step_sync(C.byref(v), *[FAKE] * 7, None, None) == DM_EINVAL
    assert L.dm_vecnorm_step_sync(None, *[FAKE] * 7, C.byref(y), None) == DM_EINVAL
    assert L.dm_vecnorm_reset_sync(C.byref(v), FAKE, FAKE, None, None) == DM_EINVAL
    for k in (0, 1, 2, 4, 5):                            # obs, rew, done, obs_out, rew_out: as dm_vecnorm_step
        args = [FAKE] * 7
        args[k] = None
        assert L.dm_vecnorm_step_sync(C.byref(v), *args, C.byref(y), None) == DM_EINVAL, k
    for args in ([FAKE, FAKE, FAKE, None, FAKE, FAKE, FAKE], [FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None]):
        assert L.dm_vecnorm_step_sync(C.byref(v), *args, C.byref(y), None) == DM_EINVAL
    for args in ((None, FAKE), (FAKE, None)):
        assert L.dm_vecnorm_reset_sync(C.byref(v), *args, C.byref(y), None) == DM_EINVAL
    v.scratch_bytes = 8                                  # the stateful checks of the struct hold for the twins too
    assert L.dm_vecnorm_step_sync(C.byref(v), *[FAKE] * 7, C.byref(y), None) == DM_EINVAL
    v.obs_mean = None                                    # and the struct checks for pack / merge
    assert L.dm_vecnorm_sync_pack(C.byref(v), C.byref(y), None) == DM_EINVAL


def test_the_sync_struct_mirror_and_the_one_merge_function():
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "deepmimic_vecnorm.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct DmVecNormSync \{(.*?)\} DmVecNormSync;", hdr, re.S).group(1), flags=re.S)
    fields = [f.strip(" *") for decl in body.split(";") for f in re.sub(r"^\s*(const\s+)?\w+\s*\**\s", "", decl.strip()).split(",") if f.strip()]
    assert fields == [n for n, _ in _lib.DmVecNormSync._fields_]
    for name in ("dm_vecnorm_step_sync", "dm_vecnorm_reset_sync", "dm_vecnorm_sync_pack", "dm_vecnorm_sync_merge"):
        assert name in _lib.VECNORM_EXPORTS and name in open(os.path.join(root, "INTEGRATION.md")).read()
    # one statement of the merge: in the header, called (not restated) by the kernels
    assert hdr.count("void dm_vn_merge(") == 1
    src = open(os.path.join(root, "deepmimic_mujoco_amd", "csrc", "dm_vecnorm.hip")).read()
    assert src.count("dm_vn_merge(") >= 3 and "void dm_vn_merge" not in src


def test_train_builds_the_synchronised_wrapper_for_several_ranks():
    from deepmimic_mujoco_amd import train
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "deepmimic_mujoco_amd", "train.py")).read()
    assert "would diverge per rank" not in src and 'sync_group="world" if world > 1 else None' in src
    assert "--algo sac runs one learner on one GPU" in src                    # that refusal stays
    text = " ".join(train.build_parser().format_help().split())
    assert "one rank only" not in text and "several ranks" in text
