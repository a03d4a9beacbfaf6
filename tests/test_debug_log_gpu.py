"""Episode debug log on the GPU (csrc/dm_trace.hip, deepmimic_mujoco_amd/debug_log.py) against tests/trace_ref.py.

The recorder copies: every comparison of a ring, a capture or a count is bit for bit against the numpy restatement fed with the
host loop's own ``get_state`` snapshots, actions and step outputs.  An engine with a recorder attached computes what its twin
without one computes.  The only arithmetic gate is the one-step re-simulation (test 7): |dqpos| <= 1e-4, the project's gate.
The sim-error and out-of-bounds exits are the handled ones tests/test_gpu_env.py::test_sim_error_and_obs_bound_paths takes."""
import os

import numpy as np
import pytest
import torch

from deepmimic_mujoco_amd import debug_log
from deepmimic_mujoco_amd.debug_log import FlightRecorder

from trace_ref import TraceRef

pytestmark = pytest.mark.gpu

MASK = (1 << 5) | (1 << 6)
HUM = (35, 34, 28)
G1D = (44, 43, 23)


def _np(x):
    return x.detach().cpu().numpy()


def _state(eng):
    """(qpos, qvel, warm) of every env as the engine's get_state returns them."""
    return [_np(x) for x in eng.get_state()[:3]]


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float32:
        a, b = a.view(np.int32), b.view(np.int32)
    return a.shape == b.shape and np.array_equal(a, b)


def _check_against(rec, ref, envs=None):
    """Ring, heads, captures and counts of ``rec`` equal ``ref``'s; ``read`` / ``captures`` decode them in time order."""
    torch.cuda.synchronize()
    assert np.array_equal(_np(rec.head).astype(np.int64) & 0xFFFFFFFF, ref.head)
    assert _same(_np(rec.ring), ref.ring)
    assert _same(_np(rec.cap), ref.cap), "a capture differs, or a row that was never written is not zero"
    assert np.array_equal(_np(rec.cap_meta), ref.cap_meta) and np.array_equal(_np(rec.cap_count), ref.cap_count)
    assert not _np(rec.trig).any()
    nq, nv, na = rec.nq, rec.nv, rec.na
    for e in (range(ref.N) if envs is None else envs):
        got, want = rec.read(e), debug_log.decode(ref.ordered(e), nq, nv, na)
        assert got["env"] == e + rec.env_offset
        for k in debug_log.FIELDS:
            assert _same(got[k], want[k]), (e, k)
        h = int(ref.head[e])
        assert got["step"].tolist() == list(range(h - min(h, ref.K), h))


# ------------------------------------------------------------------------------------------ humanoid
def _humanoid(model, clips, n, auto_reset, **kw):
    from deepmimic_mujoco_amd._lib import HipEngine
    eng = HipEngine(model, n, auto_reset=auto_reset, seed=77, **kw)
    eng.load_clip(0, clips["walk"])
    return eng


def _reset(eng, out):
    idx = (torch.arange(eng.N, dtype=torch.int32, device=eng.device) * 3) % 30
    eng.reset(out["obs"], idx_init=idx.contiguous())


RING_RUNS = {}


def _ring_run(model, clips, N, K, auto_reset):
    """Test 1's run, kept for test 7: an engine with a recorder next to a twin without one, 2K+1 random steps.  ``max_ep_length=3``
    makes episodes end (reason 3, not a trigger) inside the run, so done flags, reasons and, with auto-reset, reset states are in
    the rings."""
    key = (N, K, auto_reset)
    if key in RING_RUNS:
        return RING_RUNS[key]
    eng, twin = (_humanoid(model, clips, N, auto_reset, max_ep_length=3) for _ in range(2))
    try:
        rec = FlightRecorder(eng, steps=K, captures=4)
        assert rec.W == 136 and eng._recorder is rec and twin._recorder is None
        ref = TraceRef(N, K, 4, *HUM, MASK)
        out, tout = eng.alloc_outputs(), twin.alloc_outputs()
        _reset(eng, out)
        _reset(twin, tout)
        ref.mark(*_state(eng))
        assert _same(_np(out["obs"]), _np(tout["obs"]))
        act = torch.zeros(N, 28, device=eng.device)
        dones = 0
        for t in range(2 * K + 1):
            eng.fill_random_actions(act, t)
            eng.step(act, out)
            twin.step(act, tout)
            s, o = _state(eng), {k: _np(v) for k, v in out.items()}
            ref.record(*s, _np(act), o["rew"], o["done"], o["reason"])
            dones += int(o["done"].sum())
            for k in ("obs", "rew", "done", "reason", "terms", "terminal_obs"):
                assert _same(o[k], _np(tout[k])), (t, k)
            for a, b in zip(s, _state(twin)):
                assert _same(a, b), t
            _check_against(rec, ref, envs=[0, N - 1])
        _check_against(rec, ref)
        assert dones >= N                               # every env's episode ended at least once
        assert rec.counts() == (0, 0)
        RING_RUNS[key] = dict(rings=[rec.read(e) for e in range(N)], ref=ref)
    finally:
        eng.close()
        twin.close()
    return RING_RUNS[key]


@pytest.mark.parametrize("auto_reset", [True, False])
@pytest.mark.parametrize("K", [2, 5])
@pytest.mark.parametrize("N", [1, 63, 65, 130])
def test_ring_against_a_host_loop(model, clips, N, K, auto_reset):
    run = _ring_run(model, clips, N, K, auto_reset)
    assert all(len(r["kind"]) == K and (r["kind"] == 0).all() for r in run["rings"])      # 2K+2 entries went through K rows


def _inject(eng, nan_envs, fast_envs):
    q, v, w, c = eng.get_state()
    for e in nan_envs:
        q[e, 10] = float("nan")          # -> reason 5 (src/deepmimic_env.py:366-378)
    for e in fast_envs:
        v[e, 8] = 5000.0                 # -> reason 6 (:465-476)
    eng.set_state(q, v, w, c)
    return q, v, w


@pytest.mark.parametrize("reasons, filed", [(("sim_error", "obs_out_of_bounds"), [1, 2, 63]), (("sim_error",), [1, 64])])
def test_triggers_take_slots_in_env_order(model, clips, reasons, filed):
    N, K, Cn = 65, 4, 3
    eng = _humanoid(model, clips, N, False)
    try:
        rec = FlightRecorder(eng, steps=K, captures=Cn, reasons=reasons)
        ref = TraceRef(N, K, Cn, *HUM, debug_log.reason_mask(reasons))
        out = eng.alloc_outputs()
        _reset(eng, out)
        ref.mark(*_state(eng))
        act = torch.zeros(N, 28, device=eng.device)

        def step(t):
            eng.fill_random_actions(act, t)
            eng.step(act, out)
            ref.record(*_state(eng), _np(act), _np(out["rew"]), _np(out["done"]), _np(out["reason"]))
        for t in range(3):
            step(t)
        assert rec.counts() == (0, 0)
        q, v, w = _inject(eng, [1, 64], [2, 63])
        ref.mark(*_state(eng))
        step(3)
        reason = _np(out["reason"])
        assert reason[[1, 64]].tolist() == [5, 5] and reason[[2, 63]].tolist() == [6, 6] and _np(out["done"])[[1, 2, 63, 64]].all()
        seen = 4 if len(reasons) == 2 else 2
        assert rec.counts() == (len(filed), seen)
        _check_against(rec, ref, envs=[0, 1, 2, 63, 64])
        caps = rec.captures()
        assert [c["meta"]["env"] for c in caps] == filed
        for c in caps:
            e = c["meta"]["env"]
            assert c["meta"] == dict(env=e, entries=K, head=6, reason=int(reason[e]))
            assert c["kind"].tolist() == [0, 0, 1, 0] and c["step"].tolist() == [2, 3, 4, 5]
            # the second-to-last entry is the mark holding the injected state
            assert _same(c["qpos"][-2], _np(q)[e]) and _same(c["qvel"][-2], _np(v)[e]) and _same(c["warm"][-2], _np(w)[e])
            assert not c["action"][-2].any() and c["reward"][-2] == 0 and c["done"][-2] == 0 and c["reason"][-2] == 0
            assert (np.isnan(c["qpos"][-2, 10]) if int(reason[e]) == 5 else c["qvel"][-2, 8] == 5000.0)
            assert c["done"][-1] == 1 and c["reason"][-1] == reason[e] and _same(c["action"][-1], _np(act)[e])
        if len(reasons) == 1:
            assert not _np(rec.cap)[2].any() and not _np(rec.cap_meta)[2].any()      # a slot never filed stays zero
        # one more trigger: counted; filed only while a slot is free
        _inject(eng, [7], [])
        ref.mark(*_state(eng))
        before = _np(rec.cap).copy()
        step(4)
        assert _np(out["reason"])[7] == 5
        n_filed, n_seen = rec.counts()           # (an env left at 5000 rad/s may add a trigger of its own: the reference counts it too)
        assert n_filed == 3 and n_seen >= seen + 1 and (n_filed, n_seen) == tuple(ref.cap_count)
        if len(reasons) == 2:
            assert _same(_np(rec.cap), before)
        _check_against(rec, ref, envs=[7])
        # a log of a capture: the sim-error step is last_action, the rest of the ring its steps
        log = debug_log.to_episode_log(caps[0], "walk", "humanoid3d", model)
        assert log["last_action"] == caps[0]["action"][-1].astype(np.float64).tolist()
        assert len(log["qpos"]) == 2 and "DM_REASON_SIM_ERROR" in log["full_traceback"]
        rec.clear()
        assert rec.counts() == (0, 0) and not _np(rec.ring).any() and not _np(rec.head).any() and not _np(rec.cap).any()
    finally:
        eng.close()


def test_slot_lists(model, clips):
    N, K = 65, 4
    eng = _humanoid(model, clips, N, False)
    try:
        rec = FlightRecorder(eng, steps=K, captures=2)
        ref = TraceRef(N, K, 2, *HUM, MASK)
        out = eng.alloc_outputs()
        _reset(eng, out)
        ref.mark(*_state(eng))
        act = torch.zeros(N, 28, device=eng.device)
        eng.fill_random_actions(act, 0)
        ids = torch.full((N,), -1, dtype=torch.int32, device=eng.device)
        ids[:4] = torch.tensor([64, -1, 3, 0], dtype=torch.int32)
        for nslots in (N, 4):
            eng.step_active(act, ids, nslots, out)
            ref.record(*_state(eng), _np(act), _np(out["rew"]), _np(out["done"]), _np(out["reason"]), env_ids=_np(ids), nslots=nslots)
        head = _np(rec.head)
        assert head[[64, 3, 0]].tolist() == [3, 3, 3] and (np.delete(head, [64, 3, 0]) == 1).all()
        _check_against(rec, ref)
        # a mark over a list, and a reset under a mask
        some = torch.tensor([64, 3, 0], dtype=torch.int32, device=eng.device)
        q, v, w, c = eng.get_state(some, 3)
        eng.set_state(q, v, w, c, env_ids=some)
        ref.mark(*_state(eng), env_ids=[64, 3, 0], nslots=3)
        mask = torch.zeros(N, dtype=torch.uint8, device=eng.device)
        mask[[5, 64]] = 1
        eng.reset(out["obs"], mask=mask)
        ref.mark(*_state(eng), env_ids=[5, 64], nslots=2)
        _check_against(rec, ref)
        assert _np(rec.head)[[64, 3, 0, 5, 6]].tolist() == [5, 4, 4, 2, 1]
    finally:
        eng.close()


def test_a_recorder_is_refused_on_the_device_too(model, clips):
    """The refusals of tests/test_debug_log_cpu.py with real buffers: nothing is written."""
    eng = _humanoid(model, clips, 8, False)
    try:
        rec = FlightRecorder(eng, steps=3, captures=1)
        out = eng.alloc_outputs()
        act = torch.zeros(8, 28, device=eng.device)
        for nslots in (0, 9):
            with pytest.raises(RuntimeError, match="nslots"):
                rec.record(act, out, nslots=nslots)
        with pytest.raises(ValueError):
            rec.record(act, dict(rew=out["rew"], done=out["done"]))
        with pytest.raises(ValueError):
            FlightRecorder(eng, steps=1, attach=False)
        torch.cuda.synchronize()
        assert not _np(rec.head).any() and not _np(rec.ring).any()
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------ Unitree G1
G1_CASES = [(pl, task) for pl in (1, 2) for task in ("dpenv", "combined")]
G1_MOTIONS = {}


def _g1_clip(motion):
    from deepmimic_mujoco_amd.config import MotionConfig
    from deepmimic_mujoco_amd.mocap import MocapDM
    if motion not in G1_MOTIONS:
        mc = MocapDM(robot="unitree_g1")
        mc.load_mocap(MotionConfig(motion, robot="unitree_g1").mocap_path)
        G1_MOTIONS[motion] = mc
    return G1_MOTIONS[motion]


def _g1_engine(n, pl, task, auto_reset):
    from deepmimic_mujoco_amd.g1 import COMBINED_CLIPS, TASK_COMBINED, TASK_DPENV, G1HipEngine
    combined = task == "combined"
    e = G1HipEngine(n, auto_reset=auto_reset, seed=9, pipeline=pl, task=TASK_COMBINED if combined else TASK_DPENV,
                    max_ep_length=2000 if combined else 1000)
    if combined:
        for cid, m in enumerate(COMBINED_CLIPS):
            e.load_clip(_g1_clip(m), clip_id=cid)
    else:
        e.load_clip(_g1_clip("walk"))
    return e


@pytest.mark.parametrize("pl, task", G1_CASES)
def test_g1_ring_and_nan_trigger(pl, task):
    N, K = 5, 3
    eng, twin = _g1_engine(N, pl, task, False), _g1_engine(N, pl, task, False)
    try:
        rec = FlightRecorder(eng, steps=K, captures=2)
        assert rec.W == 158
        ref = TraceRef(N, K, 2, *G1D, MASK)
        out, tout = eng.alloc_outputs(), twin.alloc_outputs()
        idx = None if task == "combined" else torch.arange(N, dtype=torch.int32, device=eng.device) * 3
        eng.reset(out["obs"], idx_init=idx)
        twin.reset(tout["obs"], idx_init=idx)
        ref.mark(*_state(eng))
        g = torch.Generator(device="cpu").manual_seed(4)
        for t in range(2 * K + 1):
            act = ((torch.rand(N, 23, generator=g) * 2 - 1) * (0.2 if task == "combined" else 1.0)).to(eng.device)
            eng.step(act, out)
            twin.step(act, tout)
            s = _state(eng)
            ref.record(*s, _np(act), _np(out["rew"]), _np(out["done"]), _np(out["reason"]))
            for k in ("obs", "rew", "done", "reason", "terms"):
                assert _same(_np(out[k]), _np(tout[k])), (t, k)
            for a, b in zip(s, _state(twin)):
                assert _same(a, b), t
            _check_against(rec, ref)
        assert rec.counts() == (0, 0)
        # the NaN trigger of tests/g1_task_cases.py: a stored state with a NaN joint position, then a real step
        q, v, w = eng.get_state()
        q[1, 10] = float("nan")
        eng.set_state(q, v, warm=w, run_forward=False)
        ref.mark(*_state(eng))
        eng.step(act, out)
        ref.record(*_state(eng), _np(act), _np(out["rew"]), _np(out["done"]), _np(out["reason"]))
        assert int(out["reason"][1]) == 5 and int(out["done"][1]) == 1
        assert rec.counts() == (1, 1)
        _check_against(rec, ref)
        cap = rec.captures()[0]
        assert cap["meta"] == dict(env=1, entries=K, head=2 * K + 4, reason=5)
        assert cap["kind"].tolist() == [0, 1, 0] and np.isnan(cap["qpos"][1, 10]) and cap["qpos"].shape == (3, 44) and cap["action"].shape == (3, 23)
    finally:
        eng.close()
        twin.close()


# ------------------------------------------------------------------------------------------ every rollout route
def _last_step_entries(dlog, n):
    """(reward [n, N], done [n, N], heads [N]) of the last ``n`` step entries of every env, from one download per recorder."""
    rews, dones, heads = [], [], []
    torch.cuda.synchronize()
    for rec in dlog.recorders:
        ring, head = _np(rec.ring), _np(rec.head).astype(np.int64) & 0xFFFFFFFF
        o4 = rec.W - 5
        for e in range(rec.N):
            h = int(head[e])
            rows = ring[e, [(h - n + r) % rec.K for r in range(n)]]
            assert (rows[:, o4 + 3].view(np.int32) == 0).all(), "a mark among the last %d entries" % n
            assert rows[:, o4 + 4].view(np.int32).tolist() == list(range(h - n, h))
            rews.append(rows[:, o4])
            dones.append(rows[:, o4 + 1].view(np.int32))
        heads += head.tolist()
    return np.stack(rews, 1), np.stack(dones, 1), np.asarray(heads)


ROUTES = [("policy_forward", "serial", dict(), 1), ("sample_store", "serial", dict(fused_policy=False), 1),
          ("policy_forward", "captured", dict(rollout_graph=True), 2)]


@pytest.mark.parametrize("step_kind, driver, kw, sub_batches", ROUTES, ids=["policy_forward", "fused_policy_off", "captured"])
def test_every_rollout_route_records(step_kind, driver, kw, sub_batches):
    from deepmimic_mujoco_amd.deepmimic_env import HipDeepMimicVecEnv
    from deepmimic_mujoco_amd.ppo import PPO
    T, N = 8, 128
    venv = HipDeepMimicVecEnv(N, motion="walk", sub_batches=sub_batches)
    try:
        dlog = venv.enable_debug_log(steps=16)
        assert len(dlog.recorders) == sub_batches and [r.env_offset for r in dlog.recorders] == [k * N // sub_batches for k in range(sub_batches)]
        ppo = PPO(venv, net_arch=(64, 32), n_steps=T, batch_size=512, n_epochs=1, **kw)
        col = ppo.collector()
        assert (col.step_kind, col.driver) == (step_kind, driver)
        rb = ppo.collect_rollouts()
        rew, done, heads = _last_step_entries(dlog, T)
        assert _same(rew, _np(rb["rew"])) and np.array_equal(done, _np(rb["done"]).astype(np.int32))
        assert np.abs(rew).max() > 0
        warm = 1 if driver == "captured" else 0             # the capture's warm-up step is a real env step
        assert (heads == 1 + warm + T).all()
        rb = ppo.collect_rollouts()                           # captured: a second replay of the graph appends 8 more
        rew2, done2, heads2 = _last_step_entries(dlog, T)
        assert (heads2 == heads + T).all()
        assert _same(rew2, _np(rb["rew"])) and np.array_equal(done2, _np(rb["done"]).astype(np.int32))
        assert not _same(rew2, rew)
        assert dlog.counts() == (0, 0) and dlog.dump(os.devnull) == []
    finally:
        venv.close()


def test_batch_dump_writes_the_captures_once(model, tmp_path):
    from deepmimic_mujoco_amd.deepmimic_env import HipDeepMimicVecEnv
    N = 8
    venv = HipDeepMimicVecEnv(N, motion=["walk", "run"], sub_batches=2, auto_reset=False)
    try:
        dlog = venv.enable_debug_log(steps=4, captures=2)
        venv.reset_tensor()
        act = torch.zeros(N, 28, device=venv.device)
        venv.step_tensor(act)
        eng = venv.engines[1]                                 # envs 4..7
        q, v, w, c = eng.get_state()
        v[3, 8] = 5000.0
        eng.set_state(q, v, w, c)
        venv.step_tensor(act)
        assert int(venv.out["reason"][7]) == 6 and dlog.counts() == (1, 1)
        paths = dlog.dump(str(tmp_path))
        assert len(paths) == 1 and paths[0].endswith("_env7.json") and os.path.basename(paths[0]).startswith("deepmimic_episode_")
        log = debug_log.load(paths[0])
        assert log["robot"] == "humanoid3d" and log["motion"] == "run" and log["full_traceback"] == debug_log.OBS_BOUNDS_TRACEBACK
        assert log["capture"] == dict(env=7, entries=4, head=4, reason=6) and log["entries"]["env"] == 7 and log["auto_reset"] is False
        assert log["entries"]["kind"] == [1, 0, 1, 0] and len(log["qpos"]) == 2 and len(log["body_xpos"][0]) == len(model.body_parent)
        assert dlog.dump(str(tmp_path)) == [] and dlog.counts() == (1, 1) and dlog.files == paths
    finally:
        venv.close()


def test_train_json_line_gains_debug_log(tmp_path, capsys):
    import json
    from deepmimic_mujoco_amd import train
    train.main(["--envs", "128", "--horizon", "8", "--total", "2048", "--arch", "64,32", "--minibatch", "512", "--epochs", "1", "--json",
                "--debug-log", str(tmp_path / "logs"), "--debug-log-steps", "8"])
    line = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])
    assert set(line["debug_log"]) == {"captures", "triggers", "files"}
    assert line["debug_log"]["captures"] == len(line["debug_log"]["files"]) <= line["debug_log"]["triggers"]
    assert line["rollout_path"].startswith("policy_forward")


# ------------------------------------------------------------------------------------------ surfaces
@pytest.mark.parametrize("robot, renderer", [("humanoid3d", "raycast"), ("unitree_g1", "stick")])
def test_single_env_surface_file_and_frames(robot, renderer, tmp_path, capsys):
    from PIL import Image
    from deepmimic_mujoco_amd.deepmimic_env import DPEnv
    env = DPEnv("walk", robot=robot)
    path = None
    try:
        assert env.episode_debug_log == {}
        env.enable_debug_log()
        env.reset()
        assert env.episode_debug_log == {}
        zero = np.zeros(env.action_space.shape[0])
        for n in range(1, 4):
            env.step(zero)
            log = env.episode_debug_log
            assert [len(log[k]) for k in ("action", "body_xpos", "qpos", "qvel", "reward")] == [n] * 5
            assert log["robot"] == robot and log["motion"] == "walk" and "full_traceback" not in log
        env.reset()
        assert env.episode_debug_log == {}
        for n in range(1, 4):
            env.step(zero)
        assert len(env.episode_debug_log["qpos"]) == 3
        q, v = env._state()
        v[8] = 5000.0
        env.set_state(q, v)
        capsys.readouterr()
        obs, rew, done, info = env.step(zero)
        assert done and rew == 0 and info == {} and not obs.any()
        path = env._debug_log.files[-1]
        assert "Observation out of bounds in step, debug log written to %s" % path in capsys.readouterr().out
        assert os.path.dirname(path) == "/tmp" and os.path.basename(path).startswith("deepmimic_episode_")
        log = debug_log.load(path)
        assert log == env.episode_debug_log
        assert len(log["qpos"]) == 4 and log["full_traceback"] == "Observation out of bounds (deepmimic_env step)"
        assert log["entries"]["kind"] == [1, 0, 0, 0, 1, 0] and log["entries"]["reason"][-1] == 6
        assert len(log["qpos"][0]) == env._eng.NQ and len(log["body_xpos"][0]) == env._eng.NBODY
        frames = str(tmp_path / "frames")
        assert debug_log.main([path, "--frames", frames, "--renderer", renderer, "--size", "32x24", "--last", "3"]) == 0
        names = sorted(os.listdir(frames))
        assert names == ["frame_0001.png", "frame_0002.png", "frame_0003.png"]
        imgs = [np.asarray(Image.open(os.path.join(frames, f))) for f in names]
        assert all(i.shape == (24, 32, 3) and i.std() > 0 for i in imgs)
    finally:
        env.close()
        if path and os.path.exists(path):
            os.remove(path)


# ------------------------------------------------------------------------------------------ re-simulation
def test_one_step_resimulation_from_the_rings(model, clips):
    """From test 1's rings at N = 65 (K = 5, no auto-reset): every logged state with its warm start goes back into a second engine,
    which takes one step with the next logged action.  Gate: |dqpos| <= 1e-4 on every step entry that is not a sim error, the
    project's north_star gate (nobody had shown that a restart from get_state data is bit-exact); the measured maximum is printed.
    Measured on the MI355X: 260 steps, max|dqpos| = 0 and max|dqvel| = 0, every bit of qpos, qvel and warm start equal."""
    N = 65
    run = _ring_run(model, clips, N, 5, False)
    eng = _humanoid(model, clips, N, False)
    try:
        r = debug_log.resimulate(eng, run["rings"])
    finally:
        eng.close()
    use = r["compared"] & (r["reason"] != 5)
    assert use.shape == (4, N) and use.all()
    dq, dv = r["dqpos"][use], r["dqvel"][use]
    print("re-simulation: %d steps  max|dqpos| %.3e  max|dqvel| %.3e  all bits agree on %d of them (zero: %s)"
          % (use.sum(), dq.max(), dv.max(), int(r["same"][use].sum()), bool(dq.max() == 0 and dv.max() == 0)))
    assert dq.max() <= 1e-4
