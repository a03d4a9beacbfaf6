"""Euler integrator of the Unitree G1 engine (DmG1Config.integrator, csrc/dm_g1_task.h::euler_advance) on the GPU against the
mj_Euler branch of the fp64 oracle (oracle/dm_oracle.c::dmo_step), on both pipelines and both tasks, and the surfaces that select it.

The teacher-forced cases follow tests/test_g1_gpu.py::_teacher_forced with its gates: before every step the oracle takes the engine's
state and warm start, both step.  Under Euler a step has one forward evaluation, so only RK stage 0 of the per-stage records exists."""
import ctypes as C

import numpy as np
import pytest

from deepmimic_mujoco_amd.config import MotionConfig
from deepmimic_mujoco_amd.mocap import MocapDM

pytestmark = pytest.mark.gpu

MOTIONS = {}


def _clip(motion):
    if motion not in MOTIONS:
        mc = MocapDM(robot="unitree_g1")
        mc.load_mocap(MotionConfig(motion, robot="unitree_g1").mocap_path)
        MOTIONS[motion] = mc
    return MOTIONS[motion]


def _euler_model():
    """(oracle module, GModel, a copy of the G1 model struct with integrator = DM_INT_EULER)"""
    from deepmimic_mujoco_amd.g1 import DmModelG1
    from oracle import oracle_g1 as og
    g, cm = og.g1_model()
    ce = DmModelG1.from_buffer_copy(cm)
    ce.integrator = 0
    return og, g, ce


def _teacher_forced(n, steps, act_scale, seed, stride=4, pipeline=0):
    import torch
    from deepmimic_mujoco_amd.g1 import G1HipEngine
    og, g, ce = _euler_model()
    mc = _clip("walk")
    clip = og.G1Clip(*mc.tables())
    eng = G1HipEngine(n, auto_reset=False, pipeline=pipeline, integrator="Euler")
    eng.load_clip(mc)
    out = eng.alloc_outputs()
    idx = torch.arange(n, dtype=torch.int32, device=eng.device) * stride
    eng.reset(out["obs"], idx_init=idx)
    sims = [og.G1Sim(g, ce) for _ in range(n)]
    for i, s in enumerate(sims):
        s.set_caps(48, 256)
        s.env_reset(clip, int(idx[i]))
    rng = np.random.default_rng(seed)
    alive = np.ones(n, bool)
    dbg = eng.enable_debug()
    recs = []   # qpos err, qvel rel err, obs err, reward err, the evaluation had a non-analytic (MPR) contact, warm start rel err
    for t in range(steps):
        q, v, w = [x.cpu().numpy().astype(np.float64) for x in eng.get_state()]
        act = (rng.uniform(-1, 1, (n, 23)) * act_scale).astype(np.float32)
        eng.step(torch.tensor(act, device=eng.device), out)
        torch.cuda.synchronize()
        q2, v2, w2 = [x.cpu().numpy() for x in eng.get_state()]
        obs, rew, done = out["obs"].cpu().numpy(), out["rew"].cpu().numpy(), out["done"].cpu().numpy()
        d = dbg.cpu().numpy()
        for i, s in enumerate(sims):
            if not alive[i]:
                continue
            s.set("qpos", q[i]); s.set("qvel", v[i]); s.set("qacc_warmstart", w[i])
            o, r, dn, terms, reason = s.env_step(clip, act[i].astype(np.float64))
            mpr = any(not (g.geom_type[c["geom1"]] == 0 and g.geom_type[c["geom2"]] in (2, 5, 6))
                      and not (g.geom_type[c["geom1"]] == 2 and g.geom_type[c["geom2"]] in (2, 6))
                      and not (g.geom_type[c["geom1"]] == 6 and g.geom_type[c["geom2"]] == 6) for c in s.contacts())
            ws = s.get("qacc_warmstart")
            recs.append((np.abs(q2[i] - s.get("qpos")).max(),
                         np.abs(v2[i] - s.get("qvel")).max() / max(1.0, np.abs(s.get("qvel")).max()),
                         np.abs(obs[i] - o).max(), abs(rew[i] - r), mpr,
                         np.abs(w2[i] - ws).max() / max(1.0, np.abs(ws).max())))
            # the (geom1, geom2) list of the step's evaluation, by count and by hash, and its row count
            assert (int(d[i][1000]), int(d[i][1012])) == (s.geti("stage_ncon0"), s.geti("stage_chash0")), ("contact list differs", t, i)
            assert int(d[i][1004]) == (s.geti("stage_nefc0") & 0xFF), ("row count differs", t, i)
            # the RK stages that an Euler step does not have read 0
            assert not d[i][1001:1004].any() and not d[i][1005:1008].any() and not d[i][1013:1016].any(), (t, i)
            assert bool(done[i]) == dn, ("termination differs", t, i, done[i], dn, reason)
            if dn:
                alive[i] = False
    eng.close()
    return np.array(recs, float)


def test_g1_euler_teacher_forced_steps_small_actions():
    """16 envs on the walk clip, 25 steps of small torques.  State, observation and reward to the RK4 test's gates on every step;
    the warm start kept for the next step is the evaluation's qacc (not the damped qacc'), to _forward_parity's qacc gate."""
    r = _teacher_forced(16, 25, 0.05, 1)
    print("G1 Euler teacher-forced, small actions: %d env-steps (%d with MPR contacts); max qpos %.2e (median %.2e) qvel %.2e obs %.2e "
          "rew %.2e warm %.2e" % (len(r), int(r[:, 4].sum()), r[:, 0].max(), np.median(r[:, 0]), r[:, 1].max(), r[:, 2].max(),
                                  r[:, 3].max(), r[:, 5].max()))
    assert len(r) >= 200 and r[:, 4].sum() >= 50
    assert r[:, 0].max() < 2e-5 and r[:, 1].max() < 5e-4 and r[:, 2].max() < 5e-4 and r[:, 3].max() < 5e-4
    assert np.median(r[:, 0]) < 1e-6
    assert r[:, 5].max() < 5e-3


@pytest.mark.parametrize("pipeline", [1, 2])
def test_g1_euler_teacher_forced_steps_large_actions(pipeline):
    """Full-scale random torques on the monolithic kernel (1) and the split pipeline (2): north_star's gate on every env-step, no
    exclusion set."""
    r = _teacher_forced(24, 60, 1.0, 1, stride=3, pipeline=pipeline)
    e = r[:, 0]
    print("G1 Euler teacher-forced, full-scale actions: %d env-steps (%d with MPR contacts); qpos err median %.2e p99 %.2e max %.2e; "
          "qvel rel max %.2e obs %.2e rew %.2e warm %.2e" % (len(e), int(r[:, 4].sum()), np.median(e), np.percentile(e, 99), e.max(),
                                                             r[:, 1].max(), r[:, 2].max(), r[:, 3].max(), r[:, 5].max()))
    assert len(e) >= 300 and r[:, 4].sum() >= 100
    assert e.max() < 1e-4, "north_star: per-step qpos L-inf error < 1e-4"
    assert np.median(e) < 1e-6 and np.percentile(e, 99) < 1e-5
    assert r[:, 1].max() < 2e-3 and r[:, 2].max() < 2e-3 and r[:, 3].max() < 1e-3


def test_g1_euler_combined_env_matches_the_oracle():
    """The envs, motions and step counts of tests/test_g1_gpu.py::test_g1_combined_env_matches_the_oracle with Euler on both sides:
    every decision equals the oracle's, state, obs, reward and terms to that test's gates.  The getup envs lie on the floor with more
    than 128 constraint rows: the four-rows-per-lane constraint path runs in front of the Euler advance."""
    import torch
    from deepmimic_mujoco_amd.g1 import G1HipEngine, TASK_COMBINED, COMBINED_CLIPS
    og, g, ce = _euler_model()
    n, steps = 12, 100
    mocaps = [_clip(m) for m in COMBINED_CLIPS]
    clips = [og.G1Clip(*mc.tables()) for mc in mocaps]
    eng = G1HipEngine(n, auto_reset=False, task=TASK_COMBINED, max_ep_length=2000, integrator="Euler")
    for cid, mc in enumerate(mocaps):
        eng.load_clip(mc, clip_id=cid)
    out = eng.alloc_outputs()
    motion0 = np.array([0, 0, 0, 0, 2, 2, 2, 2, 3, 3, 0, 2], np.int32)
    nst0 = np.array([170, 300, 10, 161, 0, 100, 250, 340, 0, 170, 200, 345], np.int32)
    eng.set_motion(torch.tensor(motion0, device=eng.device))
    eng.reset(out["obs"], idx_init=torch.tensor(nst0, device=eng.device))
    torch.cuda.synchronize()
    sims = [og.G1CombSim(clips) for _ in range(n)]
    obs0 = out["obs"].cpu().numpy()
    for i, s in enumerate(sims):
        s.cm = ce
        s.set_caps(48, 256)
        o, err = s.comb_reset(int(motion0[i]), int(nst0[i]))
        assert err == 0 and np.abs(o - obs0[i]).max() < 1e-4, (i, np.abs(o - obs0[i]).max())
    rng = np.random.default_rng(5)
    alive = np.ones(n, bool)
    worst = dict(obs=0.0, rew=0.0, terms=0.0, state=0.0, vel=0.0)
    transitions = compared = many_rows = max_rows = 0
    for t in range(steps):
        q, v, w = [x.cpu().numpy().astype(np.float64) for x in eng.get_state()]
        act = (rng.uniform(-1, 1, (n, 23)) * 0.2).astype(np.float32)
        eng.step(torch.tensor(act, device=eng.device), out)
        torch.cuda.synchronize()
        obs, rew, done = out["obs"].cpu().numpy(), out["rew"].cpu().numpy(), out["done"].cpu().numpy()
        terms, reason = out["terms"].cpu().numpy(), out["reason"].cpu().numpy()
        mot, nst = eng.get_motion().cpu().numpy(), eng.get_counters()[0].cpu().numpy()
        q2, v2 = [x.cpu().numpy() for x in eng.get_state()[:2]]
        for i, s in enumerate(sims):
            if not alive[i]:
                continue
            m_before = s.cenv.motion
            s.set("qpos", q[i]); s.set("qvel", v[i]); s.set("qacc_warmstart", w[i])
            o, r, d, tr, rs = s.comb_step(act[i].astype(np.float64))
            state_err = np.abs(q2[i] - s.get("qpos")).max()
            assert state_err < 1e-4, (t, i, state_err)
            assert (int(mot[i]), int(nst[i]), bool(done[i]), int(reason[i])) == (s.cenv.motion, s.cenv.n_steps, d, rs), (t, i)
            transitions += int(s.cenv.motion != m_before)
            compared += 1
            rows = s.geti("stage_nefc0")
            many_rows += int(rows > 128)
            max_rows = max(max_rows, rows)
            vel_err = np.abs(v2[i] - s.get("qvel")).max() if not d else 0.0
            worst["state"] = max(worst["state"], state_err)
            worst["vel"] = max(worst["vel"], vel_err)
            worst["obs"] = max(worst["obs"], np.abs(obs[i] - o).max())
            worst["rew"] = max(worst["rew"], abs(rew[i] - r))
            worst["terms"] = max(worst["terms"], np.abs(terms[i, :7] - tr[:7]).max())
            assert int(terms[i, 7]) == int(tr[7]) or state_err > 1e-7
            if d:
                alive[i] = False
    print("G1 Euler DPCombinedEnv parity:", {k: float(x) for k, x in worst.items()}, "motion transitions", transitions,
          "compared env-steps", compared, "with more than 128 rows", many_rows, "max rows", max_rows)
    assert transitions >= 3 and many_rows >= 10
    assert compared > 600 and worst["obs"] < 3e-4 and worst["rew"] < 5e-4 and worst["terms"] < 5e-4 and worst["vel"] < 5e-3
    eng.close()


@pytest.mark.parametrize("task", ["dpenv", "combined"])
def test_g1_euler_split_pipeline_is_bit_identical_to_the_monolithic_kernel(task):
    """Under Euler the split pipeline is 3 per-env launches around 2 narrowphase launches (the evaluation, and the evaluation at the
    reset state of envs that ended, in the third env launch): bit-identical to the one-launch kernel over a rollout with auto-resets,
    and only rounds 0 and 1 file tickets."""
    import torch
    from deepmimic_mujoco_amd.g1 import G1HipEngine, TASK_COMBINED, TASK_DPENV, COMBINED_CLIPS
    n, steps = 96, 60
    engs = []
    for pl in (1, 2):
        e = G1HipEngine(n, auto_reset=True, seed=9, pipeline=pl, task=TASK_COMBINED if task == "combined" else TASK_DPENV,
                        max_ep_length=2000 if task == "combined" else 1000, integrator="Euler")
        if task == "combined":
            for cid, m in enumerate(COMBINED_CLIPS):
                e.load_clip(_clip(m), clip_id=cid)
        else:
            e.load_clip(_clip("walk"))
        engs.append((e, e.alloc_outputs()))
    for e, o in engs:
        e.reset(o["obs"])
    assert torch.equal(engs[0][1]["obs"], engs[1][1]["obs"])
    g = torch.Generator(device=engs[0][0].device).manual_seed(4)
    ndone = reset_tickets = 0
    for t in range(steps):
        act = (torch.rand(n, 23, device=engs[0][0].device, generator=g) * 2 - 1) * (0.25 if task == "combined" else 1.0)
        for e, o in engs:
            e.step(act, o)
        torch.cuda.synchronize()
        a, b = engs[0][1], engs[1][1]
        for k in ("obs", "rew", "done", "terms", "reason", "terminal_obs"):
            assert torch.equal(a[k], b[k]), (task, t, k, int((a[k] != b[k]).sum()))
        for x, y in zip(engs[0][0].get_state(), engs[1][0].get_state()):
            assert torch.equal(x, y), (task, t)
        for x, y in zip(engs[0][0].get_counters(), engs[1][0].get_counters()):
            assert torch.equal(x, y), (task, t)
        ndone += int(a["done"].sum())
        qc = engs[1][0].queue_counters()
        assert qc[0][0] + qc[0][1] > 0 and qc[0][2] >= qc[0][0] + qc[0][1], (t, qc)     # the evaluation: tickets filed, all pulled
        assert all(c == (0, 0, 0) for c in qc[2:]), (t, qc)                              # rounds that an Euler step does not run
        reset_tickets += qc[1][0] + qc[1][1]
        assert engs[0][0].queue_counters() == [(0, 0, 0)] * 6
    assert ndone >= (3 if task == "combined" else 20) and reset_tickets > 0
    for e, _ in engs:
        e.close()


def _walk_engine(n, **kw):
    from deepmimic_mujoco_amd.g1 import G1HipEngine
    e = G1HipEngine(n, auto_reset=False, seed=3, **kw)
    e.load_clip(_clip("walk"))
    return e, e.alloc_outputs()


def _equal_outputs(ea, oa, eb, ob):
    import torch
    same = all(torch.equal(oa[k], ob[k]) for k in ("obs", "rew", "done", "terms", "reason"))
    return same and all(torch.equal(x, y) for x, y in zip(ea.get_state(), eb.get_state()))


def test_g1_integrator_selector():
    """None and "RK4" are the same engine; "Euler" is another one; a model struct with integrator = DM_INT_EULER under the default
    config is the "Euler" engine bit for bit; a selector outside DM_CFG_INT_* fails dmg1_create with a text."""
    import torch
    from deepmimic_mujoco_amd import g1
    _, _, ce = _euler_model()
    n = 16
    engs = [_walk_engine(n), _walk_engine(n, integrator="RK4"), _walk_engine(n, integrator="Euler"), _walk_engine(n, cmodel=ce)]
    idx = torch.arange(n, dtype=torch.int32, device=engs[0][0].device) * 4      # clip frames: the joints move
    for e, o in engs:
        e.reset(o["obs"], idx_init=idx)
    gen = torch.Generator(device=engs[0][0].device).manual_seed(2)
    for t in range(20):
        act = (torch.rand(n, 23, device=engs[0][0].device, generator=gen) * 2 - 1) * 0.3
        for e, o in engs:
            e.step(act, o)
        torch.cuda.synchronize()
        assert _equal_outputs(*engs[0], *engs[1]), ("model / RK4", t)
        assert _equal_outputs(*engs[2], *engs[3]), ("Euler by config / by model", t)
        if t == 0:
            assert not torch.equal(engs[0][0].get_state()[1], engs[2][0].get_state()[1]), "Euler moved nothing"
            assert not torch.equal(engs[0][1]["obs"], engs[2][1]["obs"])
    for e, _ in engs:
        e.close()
    L = g1._lib()
    cfg = g1.DmG1Config()
    L.dmg1_default_config(C.byref(cfg))
    cfg.num_envs, cfg.integrator = 4, 7
    h = C.c_void_p()
    gm, cm = g1.load_g1_model()
    assert L.dmg1_create(C.byref(cm), C.sizeof(g1.DmModelG1), C.byref(cfg), C.byref(h)) == -22 and not h.value
    assert b"integrator" in (L.dmg1_last_error(None) or b"")
    with pytest.raises(KeyError):
        g1.G1HipEngine(4, integrator="implicit")


def test_g1_euler_step_active_equals_the_plain_step():
    """dmg1_step_active on the shorter launch sequence: the compacted evaluator and the uncompacted one give the same episodes."""
    import torch
    from deepmimic_mujoco_amd.evaluation import BatchEvaluator
    from deepmimic_mujoco_amd.g1 import HipG1VecEnv
    n, max_steps = 16, 60
    env = HipG1VecEnv(n, motion="walk", auto_reset=False, integrator="Euler")
    try:
        zero = torch.zeros(n, env.action_space.shape[0], device=env.device)
        frames = np.linspace(0, 75, n).astype(np.int32)
        ev = BatchEvaluator(env, compact="all", sync_every=2)
        assert ev.compact
        a = ev.run(lambda obs: zero, frames, max_steps)
        b = BatchEvaluator(env, compact=False).run(lambda obs: zero, frames, max_steps)
        assert torch.equal(a.ep_len, b.ep_len) and torch.equal(a.ep_reason, b.ep_reason)
        assert torch.equal(a.ep_ret, b.ep_ret)
        ln = a.ep_len.cpu().numpy()
        print("Euler evaluation: lengths", ln.tolist(), "launched env-steps", ev.launched_env_steps, "of", n * a.steps_run)
        assert ln.min() < ln.max() and ev.launched_env_steps < n * a.steps_run      # envs did drop out of the launches
    finally:
        env.close()


def test_euler_on_the_vec_env_surfaces_of_both_robots():
    import torch
    from deepmimic_mujoco_amd import g1
    from deepmimic_mujoco_amd.combined_env import HipCombinedVecEnv
    from deepmimic_mujoco_amd.deepmimic_env import HipDeepMimicVecEnv
    for make, cls, na in ((lambda: HipDeepMimicVecEnv(8, robot="unitree_g1", integrator="Euler"), g1.HipG1VecEnv, 23),
                          (lambda: HipCombinedVecEnv(8, integrator="Euler"), g1.HipG1CombinedVecEnv, 23)):
        env = make()
        assert isinstance(env, cls)
        obs = env.reset()
        for t in range(5):
            obs, rew, done, infos = env.step(np.zeros((8, na), np.float32))
            assert np.isfinite(obs).all() and np.isfinite(rew).all() and len(infos) == 8
        assert env.engine.queue_counters() == [(0, 0, 0)] * 6      # 8 envs: the monolithic kernel
        env.close()
    # the humanoid engine had the integrator all along; its vec-env now passes the keyword on
    envs = [HipDeepMimicVecEnv(8, seed=7, auto_reset=False, integrator=i) for i in ("Euler", "RK4", None)]
    idx = torch.arange(8, dtype=torch.int32, device=envs[0].device) * 3
    act = torch.zeros(8, envs[0].action_space.shape[0], device=envs[0].device)
    outs = []
    for env in envs:
        env.reset_tensor(idx)
        outs.append(env.step_tensor(act)["obs"].clone())
    assert all(torch.isfinite(o).all() for o in outs)
    assert torch.equal(outs[1], outs[2]) and not torch.equal(outs[0], outs[1])
    for env in envs:
        env.close()
