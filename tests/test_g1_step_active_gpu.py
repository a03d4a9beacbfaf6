"""``dmg1_step_active`` (csrc/dm_g1.hip) and the evaluator route built on it (``BatchEvaluator(compact="all")``) on the GPU.

Engine level, both pipelines and both tasks: a step over a slot list gives every listed env the bits the plain ``dmg1_step`` gives it,
whatever the order of the list and however many envs are listed, and leaves an env that is not listed alone: its state row, counters,
motion slot and output rows.  Evaluator level: the compacted G1 evaluation equals the reference loop and the uncompacted run bit for
bit.  Every comparison is bitwise: the arithmetic is that of ``dmg1_step``, only the set of workgroups differs."""
import ctypes as C

import numpy as np
import pytest
import torch

from deepmimic_mujoco_amd import evaluation
from deepmimic_mujoco_amd.config import MotionConfig
from deepmimic_mujoco_amd.evaluation import BatchEvaluator
from deepmimic_mujoco_amd.mocap import MocapDM

pytestmark = pytest.mark.gpu

N = 24
SENTINEL = -12345
DM_EINVAL = -22                # include/deepmimic_hip.h
MOTIONS = {}
CASES = [(pl, task) for pl in (1, 2) for task in ("dpenv", "combined")]


def _clip(motion):
    if motion not in MOTIONS:
        mc = MocapDM(robot="unitree_g1")
        mc.load_mocap(MotionConfig(motion, robot="unitree_g1").mocap_path)
        MOTIONS[motion] = mc
    return MOTIONS[motion]


def _engine(pl, task, seed=9, auto_reset=False, max_ep_length=None):
    from deepmimic_mujoco_amd.g1 import COMBINED_CLIPS, TASK_COMBINED, TASK_DPENV, G1HipEngine
    combined = task == "combined"
    e = G1HipEngine(N, auto_reset=auto_reset, seed=seed, pipeline=pl, task=TASK_COMBINED if combined else TASK_DPENV,
                    max_ep_length=max_ep_length or (2000 if combined else 1000))
    if combined:
        for cid, m in enumerate(COMBINED_CLIPS):
            e.load_clip(_clip(m), clip_id=cid)
    else:
        e.load_clip(_clip("walk"))
    return e


def _reset(e, out, task):
    """Spread start frames: every third frame of the walk clip (DPEnv); the combined task's own seeded draw of motion and frame
    (walk or getup; the same for twins of one seed)."""
    e.reset(out["obs"], idx_init=None if task == "combined" else torch.arange(N, dtype=torch.int32, device=e.device) * 3)


def _actions(g, dev, task):
    """Random actions at the scale of the teacher-forced runs of tests/test_g1_gpu.py: full scale (DPEnv), 0.2 (combined)."""
    return ((torch.rand(N, 23, generator=g) * 2 - 1) * (0.2 if task == "combined" else 1.0)).to(dev)


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _same(a, b, rows=None):
    a, b = _bits(a), _bits(b)
    return torch.equal(a, b) if rows is None else torch.equal(a[rows], b[rows])


def _engine_state(e):
    """Everything of an env that the C-ABI shows: qpos, qvel, warm start | idx_curr, episode length, episode reward | motion slot."""
    return [x.clone() for x in (*e.get_state(), *e.get_counters(), e.get_motion())]


def _poison(out):
    for k in ("obs", "rew", "terms"):
        out[k].fill_(float("nan"))
    out["done"].fill_(0xAB)
    out["reason"].fill_(SENTINEL)
    return {k: out[k].clone() for k in ("obs", "rew", "terms", "done", "reason")}


def _warm_twins(pl, task, count, steps=4):
    """``count`` engines of one seed after the same reset and the same ``steps`` plain steps: equal states, robots already thrashing."""
    engs = [_engine(pl, task) for _ in range(count)]
    outs = [e.alloc_outputs() for e in engs]
    g = torch.Generator(device="cpu").manual_seed(4)
    for e, o in zip(engs, outs):
        _reset(e, o, task)
    for _ in range(steps):
        act = _actions(g, engs[0].device, task)
        for e, o in zip(engs, outs):
            e.step(act, o)
    ref = _engine_state(engs[0])
    for e in engs[1:]:
        assert all(_same(x, y) for x, y in zip(_engine_state(e), ref))
    return engs, outs, g


def _slot_list(live, dev):
    """The ascending list of ``live`` with one -1 in the middle and a -1 tail; nslots covers the middle one and two of the tail."""
    ids = list(live)
    ids.insert(len(ids) // 2, -1)
    nslots = len(ids) + 2
    assert nslots <= N
    return torch.tensor(ids + [-1] * (N - len(ids)), dtype=torch.int32, device=dev), nslots


@pytest.mark.parametrize("pl, task", CASES)
def test_subset_equals_full_step_and_unlisted_envs_are_untouched(pl, task):
    (A, B), (oa, ob), g = _warm_twins(pl, task, 2)
    try:
        dev = A.device
        live = [i for i in range(N) if i % 3 != 1]
        snap = {i: [x[i].clone() for x in _engine_state(A)] for i in range(N) if i not in live}
        for step in range(8):
            act = _actions(g, dev, task)
            B.step(act, ob)
            ids, nslots = _slot_list(live, dev)
            ids_before = ids.clone()
            poison = _poison(oa)
            A.step_active(act, ids, nslots, oa)
            torch.cuda.synchronize()
            assert torch.equal(ids, ids_before), "the caller's list was written"
            rows = torch.tensor(live, device=dev)
            rest = torch.tensor([i for i in range(N) if i not in live], device=dev)
            for k in ("obs", "rew", "done", "terms", "reason"):
                assert _same(oa[k], ob[k], rows), (step, k)
                assert _same(oa[k], poison[k], rest), (step, k, "an output row of an env that is not listed was written")
            sa, sb = _engine_state(A), _engine_state(B)
            for x, y in zip(sa, sb):
                assert _same(x, y, rows), step
            for i in rest.tolist():
                for x, want in zip(sa, snap[i]):
                    assert _same(x[i], want), (step, i, "an env that is not listed moved")
            drop = live[1::4][:2]                                                    # a few more leave every step: 16, 14, ... 2 listed
            for i in drop:
                snap[i] = [x[i].clone() for x in sa]
            live = [i for i in live if i not in drop]
        assert 0 < len(live) <= 4
    finally:
        A.close()
        B.close()


@pytest.mark.parametrize("pl, task", CASES)
def test_order_of_the_list_does_not_matter(pl, task):
    engs, outs, g = _warm_twins(pl, task, 3)
    try:
        dev = engs[0].device
        live = [i for i in range(N) if i % 3 != 1]
        ids0, nslots = _slot_list(live, dev)
        perm = torch.randperm(nslots, generator=torch.Generator(device="cpu").manual_seed(7)).to(dev)
        lists = [ids0, torch.cat([ids0[:nslots].flip(0), ids0[nslots:]]).contiguous(), torch.cat([ids0[:nslots][perm], ids0[nslots:]]).contiguous()]
        rows = torch.tensor(live, device=dev)
        for step in range(3):
            act = _actions(g, dev, task)
            for e, o, ids in zip(engs, outs, lists):
                _poison(o)
                e.step_active(act, ids, nslots, o)
            torch.cuda.synchronize()
            states = [_engine_state(e) for e in engs]
            for o, s in zip(outs[1:], states[1:]):
                for k in ("obs", "rew", "done", "terms", "reason"):
                    assert _same(o[k], outs[0][k]), (step, k)                       # listed rows equal, the others still poison
                for x, y in zip(s, states[0]):
                    assert _same(x, y), step
            assert not torch.isnan(outs[0]["obs"][rows]).any()
    finally:
        for e in engs:
            e.close()


@pytest.mark.parametrize("pl, task", CASES)
def test_auto_reset_is_forced_off(pl, task):
    """An ``auto_reset=True`` engine under ``step_active``: an env that ends reports done and keeps its terminal state, as the
    ``auto_reset=False`` twin does under the plain step; its reset count does not advance (the next seeded reset draws the twin's
    frames)."""
    A, B = _engine(pl, task, auto_reset=True, max_ep_length=6), _engine(pl, task, auto_reset=False, max_ep_length=6)
    try:
        dev = A.device
        oa, ob = A.alloc_outputs(), B.alloc_outputs()
        ep0 = (torch.arange(N, device=dev) % 6).to(torch.int32).contiguous()         # envs 6 k + 3, + 4, + 5 reach the cap within 3 steps
        for e, o in ((A, oa), (B, ob)):
            _reset(e, o, task)
            e.set_counters(episode_length=ep0)
        g = torch.Generator(device="cpu").manual_seed(11)
        live, ended = list(range(N)), {}
        for step in range(3):
            act = _actions(g, dev, task) * 0.05
            B.step(act, ob)
            ids, nslots = _slot_list(live, dev) if len(live) + 3 <= N else (torch.tensor(live, dtype=torch.int32, device=dev), len(live))
            A.step_active(act, ids, nslots, oa)
            torch.cuda.synchronize()
            rows = torch.tensor(live, device=dev)
            for k in ("obs", "rew", "done", "terms", "reason"):
                assert _same(oa[k], ob[k], rows), (step, k)
            sa, sb = _engine_state(A), _engine_state(B)
            for x, y in zip(sa, sb):
                assert _same(x, y, rows), step
            for i in [i for i in live if int(oa["done"][i])]:
                ended[i] = [x[i].clone() for x in sb]                                 # the twin's terminal state
                live.remove(i)
        print("ended", sorted(ended), "episode lengths", _engine_state(A)[4].tolist())
        assert len(ended) >= 3 and len(live) >= 3
        sa = _engine_state(A)
        for i, want in ended.items():
            for x, w in zip(sa, want):
                assert _same(x[i], w), (i, "an env that ended did not keep its terminal state")
            assert int(sa[4][i]) >= 6                                                  # the episode length of the terminal step, not 0
        A.reset(oa["obs"])
        B.reset(ob["obs"])                                                             # seeded draws keyed by the reset count
        sa, sb = _engine_state(A), _engine_state(B)                                    # (the warm start survives a reset: not compared)
        assert _same(oa["obs"], ob["obs"]) and all(_same(sa[k], sb[k]) for k in (0, 1, 3, 4, 5, 6))
    finally:
        A.close()
        B.close()


@pytest.mark.parametrize("pl", [1, 2])
def test_argument_errors_launch_nothing(pl):
    from deepmimic_mujoco_amd._lib import _ptr
    (A,), (oa,), g = _warm_twins(pl, "dpenv", 1, steps=2)
    try:
        before = _engine_state(A)
        poison = _poison(oa)
        act = _actions(g, A.device, "dpenv")
        ids = torch.arange(N + 1, dtype=torch.int32, device=A.device)
        stream = C.c_void_p(torch.cuda.current_stream(A.device).cuda_stream)
        good = dict(actions=_ptr(act), ids=_ptr(ids), nslots=N, obs=_ptr(oa["obs"]))
        for bad in (dict(nslots=0), dict(nslots=N + 1), dict(ids=None), dict(obs=None)):
            a = dict(good, **bad)
            rc = A.L.dmg1_step_active(A.h, a["actions"], a["ids"], a["nslots"], a["obs"], _ptr(oa["rew"]), _ptr(oa["done"]),
                                      _ptr(oa["terms"]), _ptr(oa["reason"]), stream)
            assert rc == DM_EINVAL, (bad, rc)
            assert len(A.L.dmg1_last_error(A.h) or b"") > 0
        assert A.L.dmg1_step_active(None, good["actions"], good["ids"], N, good["obs"], _ptr(oa["rew"]), _ptr(oa["done"]), None, None, stream) == DM_EINVAL
        assert len(A.L.dmg1_last_error(None) or b"") > 0
        torch.cuda.synchronize()
        assert all(_same(x, y) for x, y in zip(_engine_state(A), before))
        assert all(_same(oa[k], poison[k]) for k in poison)
    finally:
        A.close()


# ------------------------------------------------------------------------------------------ evaluator level
def reference_loop(env, act_fn, start_frames, max_steps):
    """``reference_loop`` of tests/test_evaluation_gpu.py with the per-term sums added: the plain ``step_tensor`` on ALL envs every
    step, bookkeeping on the host in Python floats, a ``get_state`` snapshot after every step."""
    n = env.num_envs
    obs = env.reset_tensor(torch.as_tensor(np.asarray(start_frames, np.int32), device=env.device))
    alive, ep_len, ep_ret = [True] * n, [0] * n, [0.0] * n
    ep_terms = np.zeros((n, env.out["terms"].shape[1]), np.float64)
    ep_reason, last_obs, snap = [None] * n, [None] * n, [None] * n
    with torch.no_grad():
        for _ in range(max_steps):
            out = env.step_tensor(act_fn(obs))
            rew, done, reason, o, terms = (out[k].cpu().numpy() for k in ("rew", "done", "reason", "obs", "terms"))
            state = [s.cpu().numpy() for s in env.engine.get_state()]
            for i in range(n):
                if not alive[i]:
                    continue
                ep_len[i] += 1
                ep_ret[i] += float(rew[i])
                ep_terms[i] += terms[i].astype(np.float64)
                if done[i] or ep_len[i] == max_steps:
                    ep_reason[i] = int(reason[i]) if done[i] else evaluation.TRUNCATED
                    last_obs[i] = o[i].copy()
                    snap[i] = [s[i].copy() for s in state]
                    alive[i] = False
    assert not any(alive)
    return dict(ep_len=np.array(ep_len, np.int32), ep_ret=np.array(ep_ret, np.float64), ep_reason=np.array(ep_reason, np.int32),
                ep_terms=ep_terms, last_obs=np.stack(last_obs), snap=snap)


def use(env, steps=3):
    """Leave ``env`` mid-episode with warm starts and controls of its own, as an earlier run would (tests/test_evaluation_gpu.py)."""
    g = torch.Generator(device="cpu").manual_seed(5)
    env.reset_tensor()
    for _ in range(steps):
        a = (torch.rand(env.num_envs, env.action_space.shape[0], generator=g) - 0.5).to(env.device)
        env.step_tensor(a * torch.as_tensor(env.action_space.high, device=env.device))


def check_all_frozen(result, ref, env, max_steps):
    """``check(..., all_frozen=True)`` of tests/test_evaluation_gpu.py, with the per-term sums."""
    ep_len, ep_reason = result.ep_len.cpu().numpy(), result.ep_reason.cpu().numpy()
    print("lengths", ep_len.tolist(), "reasons", ep_reason.tolist())
    assert result.ep_len.dtype == torch.int32 and result.ep_ret.dtype == torch.float64
    assert np.array_equal(ep_len, ref["ep_len"])
    assert np.array_equal(ep_reason, ref["ep_reason"])
    assert np.array_equal(result.ep_ret.cpu().numpy().view(np.int64), ref["ep_ret"].view(np.int64))
    assert np.array_equal(result.ep_terms.cpu().numpy().view(np.int64), ref["ep_terms"].view(np.int64))
    assert np.array_equal(result.last_obs.cpu().numpy().view(np.int32), ref["last_obs"].view(np.int32))
    assert result.steps_run <= max_steps
    state = [s.cpu().numpy() for s in env.engine.get_state()]
    for i in range(len(ep_len)):
        for got, want in zip(state, ref["snap"][i]):
            assert np.array_equal(got[i].view(np.int32), want.view(np.int32)), "env %d is not frozen at its terminal state" % i


FIELDS = ("ep_len", "ep_reason", "ep_ret", "ep_terms", "last_obs")


def _equal_results(a, b):
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        if x.dtype.is_floating_point:
            x, y = x.view(torch.int64 if x.dtype == torch.float64 else torch.int32), y.view(torch.int64 if y.dtype == torch.float64 else torch.int32)
        assert torch.equal(x, y), f


def _g1_walk_env(n, **kw):
    from deepmimic_mujoco_amd.deepmimic_env import HipDeepMimicVecEnv
    return HipDeepMimicVecEnv(n, motion="walk", robot="unitree_g1", auto_reset=False, **kw)


def test_g1_walk_compacted_evaluation_equals_the_reference_loop():
    n, max_steps = 16, 17
    frames = np.linspace(0, 75, n).astype(np.int32)
    env, ref_env = _g1_walk_env(n), _g1_walk_env(n)
    try:
        zero = torch.zeros(n, env.action_space.shape[0], device=env.device)
        act_fn = lambda obs: zero
        ref = reference_loop(ref_env, act_fn, frames, max_steps)
        assert int(np.sum(ref["ep_reason"] != evaluation.TRUNCATED)) >= 3 and int(np.sum(ref["ep_reason"] == evaluation.TRUNCATED)) >= 3
        live_steps = int(ref["ep_len"].sum())
        assert not BatchEvaluator(env, compact=True).compact           # True keeps its meaning: humanoid engines only
        for sync_every in (16, 1):                                      # first on the env as built, then used
            ev = BatchEvaluator(env, compact="all", sync_every=sync_every)
            assert ev.compact
            check_all_frozen(ev.run(act_fn, frames, max_steps), ref, env, max_steps)
            # finished envs leave the launch at the next read of the live count at the latest
            assert live_steps <= ev.launched_env_steps <= n * max_steps
            if sync_every == 1:
                assert ev.launched_env_steps == live_steps
            use(env)
    finally:
        env.close()
        ref_env.close()


def test_g1_split_pipeline_engine_compacted_equals_uncompacted():
    """512 envs: the smallest engine that takes the split pipeline by itself, and the longest-first pass over the slot list."""
    n, max_steps = 512, 24
    env = _g1_walk_env(n)
    try:
        assert env.engine.split
        zero = torch.zeros(n, env.action_space.shape[0], device=env.device)
        frames = np.arange(n) % evaluation.clip_length(env)
        ev = BatchEvaluator(env, compact="all", sync_every=2)
        a = ev.run(lambda obs: zero, frames, max_steps)
        assert ev.launched_env_steps < n * a.steps_run
        ln = a.ep_len.cpu().numpy()
        print("lengths", sorted(set(ln.tolist())), "launched", ev.launched_env_steps, "live", int(ln.sum()))
        assert ln.min() + 2 < ln.max()
        b = BatchEvaluator(env, compact=False).run(lambda obs: zero, frames, max_steps)
        _equal_results(a, b)
    finally:
        env.close()


def test_g1_two_engines_compacted_equals_uncompacted():
    n, max_steps = 32, 17
    env = _g1_walk_env(n, sub_batches=2)
    try:
        zero = torch.zeros(n, env.action_space.shape[0], device=env.device)
        frames = np.linspace(0, 75, n).astype(np.int32)
        ev = BatchEvaluator(env, compact="all", sync_every=2)
        assert ev.compact and len(env.engines) == 2
        a = ev.run(lambda obs: zero, frames, max_steps)
        b = BatchEvaluator(env, compact=False).run(lambda obs: zero, frames, max_steps)
        _equal_results(a, b)
        assert ev.launched_env_steps < n * a.steps_run
    finally:
        env.close()


COMBINED_MAX_STEPS = 120       # zero actions: 4 of the 16 seeded episodes end early (fallen without amnesty), 12 are cut


def test_g1_combined_task_compacted_equals_uncompacted():
    """The combined task starts from the engine's seeded draw, keyed by the env's reset count: the two runs are on twin envs of one
    seed, each on its first evaluation."""
    from deepmimic_mujoco_amd.g1 import HipG1CombinedVecEnv
    n = 16
    env, twin = HipG1CombinedVecEnv(n, auto_reset=False), HipG1CombinedVecEnv(n, auto_reset=False)
    try:
        zero = torch.zeros(n, env.action_space.shape[0], device=env.device)
        ev = BatchEvaluator(env, compact="all", sync_every=4)
        assert ev.compact
        a = ev.run(lambda obs: zero, None, COMBINED_MAX_STEPS)
        ln, reason = a.ep_len.cpu().numpy(), a.ep_reason.cpu().numpy()
        print("combined lengths", ln.tolist(), "reasons", reason.tolist())
        assert int(np.sum(reason != evaluation.TRUNCATED)) >= 2 and int(np.sum(reason == evaluation.TRUNCATED)) >= 2
        b = BatchEvaluator(twin, compact=False).run(lambda obs: zero, None, COMBINED_MAX_STEPS)
        assert torch.equal(a.start_frames, b.start_frames)
        _equal_results(a, b)
        assert ev.launched_env_steps < n * a.steps_run
    finally:
        env.close()
        twin.close()
