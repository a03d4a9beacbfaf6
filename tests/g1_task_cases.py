"""Single-step cases for the task layer of the Unitree G1 engine (csrc/dm_g1_task.h: step_enter, task_and_finish, the in-kernel
auto-reset), for DPEnv(robot="unitree_g1") and DPCombinedEnv().  A plain module: it builds the cases, runs them on the fp64
oracle and restates the RSI draw; it touches no GPU and holds no test.  tests/test_g1_task_cases_cpu.py proves on the oracle alone
that every case reaches the branch it names; tests/test_g1_task_layer_gpu.py runs the same cases on the engine.

A case starts from a clip frame with a small, fixed edit (a pelvis height, a roll composed onto the root quaternion, one joint
velocity of 5000) rounded to fp32, so engine and oracle see the same input.  Three kinds:
  forced    the state goes in through step_forced / force_state=: one forward evaluation, physics plays no part
  stepped   the state is stored without evaluation (set_state(run_forward=False)) and one real step with an action follows: this is
            the only road through the split pipeline, whose launches serve MODE_STEP alone (step_forced takes the monolithic
            kernel whatever DmG1Config.pipeline says)
  sim_error a stored state with a NaN joint position, then a real step: mj_checkPos fails before any evaluation runs

Episode cap: the reference tests `episode_length >= MAX_EP_LENGTH` BEFORE the increment (src/deepmimic_env.py:435-438 against
:455, src/combined_env.py:442-445 against :456), so the step taken with the counter at 999 / 1999 is alive and the one at
1000 / 2000 reports max_ep_len (as tests/test_gpu_configs.py::test_max_ep_len_on_the_dpenv_task holds for the humanoid).
The cases sit at cap - 2, cap - 1 and cap.
"""
import math

import numpy as np

from deepmimic_mujoco_amd.config import MotionConfig
from deepmimic_mujoco_amd.mocap import MocapDM
from deepmimic_mujoco_amd.model import quat_mul

G1_CLIPS = ("walk", "run", "getup_facedown", "getup_facedown_slow", "getup_facedown_slow_FSI", "getup_facedown_towalk")
COMBINED_CLIPS = ("walk", "run", "getup_facedown_towalk")      # src/combined_env.py:168-170
# clip slots of the DPEnv engine that runs the single-step cases: (motion, flags)
DPENV_SLOTS = (("walk", {}), ("run", dict(run_rule=True)), ("run", {}), ("getup_facedown", dict(floor=True, acyclic=True)),
               ("walk", dict(acyclic=True)))
WALK, RUNRULE, RUNPLAIN, FLOOR, WALKACYC = range(5)
CAP_DPENV, CAP_COMBINED, AMNESTY, TO_GETUP_LEN = 1000, 2000, 150, 180      # the oracle's compile-time constants
M_WALK, M_RUN, M_GETUP, M_TO_GETUP = 0, 1, 2, 3
NACT = 23

_MOCAP = {}


def mocap(motion):
    if motion not in _MOCAP:
        mc = MocapDM(robot="unitree_g1")
        mc.load_mocap(MotionConfig(motion, robot="unitree_g1").mocap_path)
        _MOCAP[motion] = mc
    return _MOCAP[motion]


def clip_flags(motion):
    """The flags g1._load gives a clip (src/config.py:36-37, src/deepmimic_env.py:426)."""
    cfg = MotionConfig(motion, robot="unitree_g1")
    return dict(floor=motion in cfg.floor_motions, acyclic=motion in cfg.acyclical_motions, run_rule=motion == "run")


def oracle_clip(motion, **flags):
    from oracle import oracle_g1 as og
    return og.G1Clip(*mocap(motion).tables(), **flags)


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def frame(motion, i, z=None, roll_deg=None, vel8=None, zero_vel=False):
    """(qpos, qvel) of frame i of a clip, fp32-rounded, with the edits of tests/test_g1_oracle.py::test_g1_termination_rules."""
    mc = mocap(motion)
    q, v = np.array(mc.get_qpos(i), np.float64), np.array(mc.get_qvel(i), np.float64)
    if zero_vel:
        v[:] = 0
    if z is not None:
        q[2] = z
    if roll_deg is not None:      # R = Rz Ry Rx: a rotation about x composed on the right adds exactly roll_deg to the roll
        a = math.radians(roll_deg)
        q[3:7] = quat_mul(q[3:7] / np.linalg.norm(q[3:7]), [math.cos(a / 2), math.sin(a / 2), 0, 0])
    if vel8 is not None:
        v[8] = vel8
    return f32(q), f32(v)


def _case(name, task, kind, state, expect_reason, expect_done, **kw):
    c = dict(name=name, task=task, kind=kind, qpos=state[0], qvel=state[1], reason=expect_reason, done=expect_done,
             slot=WALK, motion=M_WALK, idx=0, ep_len=0, action=np.zeros(NACT), zeroed=expect_reason in (5, 6), boundary=False,
             next_idx=None, next_motion=None, on_frame=None, phase=None)
    c.update(kw)
    return c


def dpenv_cases():
    Lw, Lr = len(mocap("walk").data_config), len(mocap("run").data_config)
    D = lambda name, state, reason, done, **kw: _case(name, "dpenv", kw.pop("kind", "forced"), state, reason, done, **kw)
    cap = CAP_DPENV
    cases = [
        D("alive", frame("walk", 10), 2, False, idx=10, on_frame=10),                       # low / high is written every step (:424)
        D("low_z", frame("walk", 10, z=0.30), 1, True, idx=10),
        D("high_z", frame("walk", 10, z=2.5), 2, True, idx=10),
        D("floor clip, lying", frame("getup_facedown", 3), 0, False, slot=FLOOR, idx=3, on_frame=3),
        D("run rule", frame("run", 0, z=1.0, roll_deg=70.0, zero_vel=True), 8, True, slot=RUNRULE),
        D("run rule off", frame("run", 0, z=1.0, roll_deg=70.0, zero_vel=True), 2, False, slot=RUNPLAIN),
        D("run rule, just inside", frame("run", 0, z=1.0, roll_deg=59.9, zero_vel=True), 2, False, slot=RUNRULE, boundary=True),
        D("run rule, just outside", frame("run", 0, z=1.0, roll_deg=60.1, zero_vel=True), 8, True, slot=RUNRULE),
        D("run rule over low_z", frame("run", 0, z=0.30, roll_deg=70.0, zero_vel=True), 8, True, slot=RUNRULE),
        D("cap - 2", frame("walk", 10), 2, False, idx=10, ep_len=cap - 2, boundary=True),
        D("cap - 1", frame("walk", 10), 2, False, idx=10, ep_len=cap - 1, boundary=True),
        D("cap", frame("walk", 10), 3, True, idx=10, ep_len=cap),
        D("cap over low_z", frame("walk", 10, z=0.30), 3, True, idx=10, ep_len=cap),
        D("acyclic, L - 2", frame("walk", Lw - 2), 2, False, slot=WALKACYC, idx=Lw - 2, boundary=True, on_frame=Lw - 2),
        D("acyclic end", frame("walk", Lw - 1), 4, True, slot=WALKACYC, idx=Lw - 1, next_idx=0),
        D("acyclic end over cap", frame("walk", Lw - 1), 4, True, slot=WALKACYC, idx=Lw - 1, ep_len=cap, next_idx=0),
        D("cyclic wrap", frame("walk", Lw - 1), 2, False, idx=Lw - 1, next_idx=0, on_frame=Lw - 1),
        D("obs bound", frame("walk", 10, vel8=5000.0), 6, True, idx=10),
        D("obs bound over low_z", frame("walk", 10, z=0.30, vel8=5000.0), 6, True, idx=10),
        D("obs bound over cap and acyclic end", frame("walk", Lw - 1, vel8=5000.0), 6, True, slot=WALKACYC, idx=Lw - 1, ep_len=cap, next_idx=0),
    ]
    # the same rules through a real step (the split pipeline's road): margins are wide enough for one step of physics
    lying = frame("getup_facedown", 3)
    cases += [
        D("stepped alive", frame("walk", 10), 2, False, kind="stepped", idx=10),
        D("stepped low_z", lying, 1, True, kind="stepped", idx=10),
        D("stepped high_z", frame("walk", 10, z=2.5), 2, True, kind="stepped", idx=10),
        D("stepped floor clip", lying, 0, False, kind="stepped", slot=FLOOR, idx=3),
        D("stepped run rule", frame("run", 0, z=1.0, roll_deg=70.0, zero_vel=True), 8, True, kind="stepped", slot=RUNRULE),
        D("stepped cap - 1", frame("walk", 10), 2, False, kind="stepped", idx=10, ep_len=cap - 1, boundary=True),
        D("stepped cap", frame("walk", 10), 3, True, kind="stepped", idx=10, ep_len=cap),
        D("stepped acyclic end", frame("walk", Lw - 1), 4, True, kind="stepped", slot=WALKACYC, idx=Lw - 1, next_idx=0),
        D("stepped cyclic wrap", frame("run", Lr - 1), 2, False, kind="stepped", slot=RUNPLAIN, idx=Lr - 1, next_idx=0),
    ]
    q, v = frame("walk", 10)
    q[10] = float("nan")
    cases.append(D("sim error", (q, v), 5, True, kind="sim_error", idx=10, ep_len=17, next_idx=10))
    for c in cases:
        if c["next_idx"] is None:
            c["next_idx"] = c["idx"] + 1
    return cases


def combined_cases():
    L = [len(mocap(m).data_config) for m in COMBINED_CLIPS]
    C = lambda name, state, reason, done, **kw: _case(name, "combined", kw.pop("kind", "forced"), state, reason, done, **kw)
    cap = CAP_COMBINED
    fell = dict(next_motion=M_TO_GETUP, next_idx=1)
    lying, standing_up = frame("getup_facedown_towalk", 1), frame("getup_facedown_towalk", L[2] - 1)
    cases = [
        C("walk alive", frame("walk", 200 % L[0]), 0, False, idx=200, on_frame=200 % L[0]),
        C("walk fall, no amnesty", frame("walk", 10, z=0.30), 7, True, idx=10, **fell),
        C("walk fall at the amnesty boundary", frame("walk", AMNESTY % L[0], z=0.30), 7, True, idx=AMNESTY, **fell),
        C("walk fall with amnesty", frame("walk", (AMNESTY + 1) % L[0], z=0.30), 0, False, idx=AMNESTY + 1, **fell),
        C("walk fall by high_z", frame("walk", 10, z=2.5), 7, True, idx=10, **fell),
        C("run fall by roll, with amnesty", frame("run", 200 % L[1], z=1.0, roll_deg=70.0, zero_vel=True), 0, False, motion=M_RUN, idx=200, **fell),
        C("run fall by roll, no amnesty", frame("run", 10, z=1.0, roll_deg=70.0, zero_vel=True), 7, True, motion=M_RUN, idx=10, **fell),
        C("run roll just inside", frame("run", 10, z=1.0, roll_deg=59.9, zero_vel=True), 0, False, motion=M_RUN, idx=10, boundary=True),
        C("to_getup success", lying, 0, False, motion=M_TO_GETUP, idx=5, next_motion=M_GETUP, next_idx=1),
        C("to_getup, one short of the time-out", frame("walk", 10), 0, False, motion=M_TO_GETUP, idx=TO_GETUP_LEN - 2, boundary=True),
        C("to_getup time-out", frame("walk", 10), 0, False, motion=M_TO_GETUP, idx=TO_GETUP_LEN - 1, next_motion=M_GETUP, next_idx=1),
        C("getup, one short of the time-out", lying, 0, False, motion=M_GETUP, idx=L[2] - 2, boundary=True),
        C("getup time-out, lying: run, then fallen", lying, 7, True, motion=M_GETUP, idx=L[2] - 1, **fell),
        C("getup time-out, standing: run", standing_up, 0, False, motion=M_GETUP, idx=L[2] - 1, next_motion=M_RUN, next_idx=1, on_frame=L[2] - 1),
        C("walk past one clip", frame("walk", 37), 0, False, idx=L[0] + 37, on_frame=37, phase=37.0 / L[0]),
        C("cap - 2", frame("walk", 10), 0, False, idx=200, ep_len=cap - 2, boundary=True),
        C("cap - 1", frame("walk", 10), 0, False, idx=200, ep_len=cap - 1, boundary=True),
        C("cap", frame("walk", 10), 3, True, idx=200, ep_len=cap),
        C("cap over a fall without amnesty", frame("walk", 10, z=0.30), 3, True, idx=10, ep_len=cap, **fell),
        C("obs bound", frame("walk", 10, vel8=5000.0), 6, True, idx=200),
        C("obs bound over a fall and the cap", frame("walk", 10, z=0.30, vel8=5000.0), 6, True, idx=10, ep_len=cap, **fell),
    ]
    cases += [
        C("stepped walk alive", frame("walk", 200 % L[0]), 0, False, kind="stepped", idx=200),
        C("stepped walk fall, no amnesty", lying, 7, True, kind="stepped", idx=AMNESTY, **fell),
        C("stepped walk fall with amnesty", lying, 0, False, kind="stepped", idx=AMNESTY + 1, **fell),
        C("stepped getup time-out, lying", lying, 7, True, kind="stepped", motion=M_GETUP, idx=L[2] - 1, **fell),
        C("stepped to_getup time-out", frame("walk", 10), 0, False, kind="stepped", motion=M_TO_GETUP, idx=TO_GETUP_LEN - 1, next_motion=M_GETUP, next_idx=1),
        C("stepped walk past one clip", frame("walk", 37), 0, False, kind="stepped", idx=L[0] + 37, phase=37.0 / L[0]),
        C("stepped cap - 1", frame("walk", 10), 0, False, kind="stepped", idx=200, ep_len=cap - 1, boundary=True),
        C("stepped cap", frame("walk", 10), 3, True, kind="stepped", idx=200, ep_len=cap),
    ]
    q, v = frame("walk", 10)
    q[10] = float("nan")
    cases.append(C("sim error", (q, v), 5, True, kind="sim_error", motion=M_RUN, idx=31, ep_len=17, next_idx=31, next_motion=M_RUN))
    for c in cases:
        if c["next_idx"] is None:
            c["next_idx"] = c["idx"] + 1
        if c["next_motion"] is None:
            c["next_motion"] = c["motion"]
    return cases


def all_cases():
    return dpenv_cases() + combined_cases()


_ORACLE = {}


def oracle_clips(task):
    if task not in _ORACLE:
        if task == "dpenv":
            _ORACLE[task] = [oracle_clip(m, **fl) for m, fl in DPENV_SLOTS]
        else:
            _ORACLE[task] = [oracle_clip(m) for m in COMBINED_CLIPS]
    return _ORACLE[task]


def run_on_oracle(case):
    """The case on a fresh fp64 environment.  forced: force_state=; stepped / sim_error: the state stored as it is (zero warm
    start), then a step with the case's action.  Returns what the engine is compared with."""
    from oracle import oracle_g1 as og
    clips = oracle_clips(case["task"])
    comb = case["task"] == "combined"
    s = og.G1CombSim(clips) if comb else og.G1Sim()
    s.set_caps(48, 256)
    if comb:
        s.cenv.motion, s.cenv.n_steps, s.cenv.episode_length = case["motion"], case["idx"], case["ep_len"]
        step = s.comb_step
    else:
        s.env.idx_curr, s.env.episode_length = case["idx"], case["ep_len"]
        step = lambda a, force_state=None: s.env_step(clips[case["slot"]], a, force_state=force_state)
    if case["kind"] == "forced":
        obs, rew, done, terms, reason = step(np.zeros(NACT), force_state=(case["qpos"], case["qvel"]))
    else:
        s.set("qpos", case["qpos"]); s.set("qvel", case["qvel"]); s.set("qacc_warmstart", np.zeros(og.NV))
        obs, rew, done, terms, reason = step(case["action"])
    env = s.cenv if comb else s.env
    return dict(obs=obs, rew=rew, done=done, terms=terms, reason=reason, idx=env.n_steps if comb else env.idx_curr,
                ep_len=env.episode_length, motion=env.motion if comb else case["slot"], qpos=s.get("qpos"), qvel=s.get("qvel"),
                warm=s.get("qacc_warmstart"), qacc=s.get("qacc"))


# ------------------------------------------------------------------------------------------ the RSI draw of the auto-reset
def rsi_draw(task, seed, env, rcnt, lengths):
    """(motion, idx) of reset number rcnt of an env: DPEnv `hash(.., 0x5EED) % L`; DPCombinedEnv.reset(rsi=True)
    (src/combined_env.py:219-227) getup or walk from bit 0 of the 0x5EED draw, frame from the 0x5EEE draw, walk starting
    AMNESTY_STEPS + 10 steps in.  The hash is dm_hash32 of csrc/dm_rng.h as tests/kernel_helpers.py restates it."""
    from kernel_helpers import hash32
    if task == "dpenv":
        return 0, hash32(seed, env, rcnt, 0x5EED) % lengths[0]
    motion = M_GETUP if hash32(seed, env, rcnt, 0x5EED) & 1 else M_WALK
    return motion, hash32(seed, env, rcnt, 0x5EEE) % lengths[motion] + (AMNESTY + 10 if motion == M_WALK else 0)


AUTORESET = dict(seed=20, envs=32, steps=40, act_scale=0.05, act_seed=6)


def autoreset_actions():
    rng = np.random.default_rng(AUTORESET["act_seed"])
    return (rng.uniform(-1, 1, (AUTORESET["steps"], AUTORESET["envs"], NACT)) * AUTORESET["act_scale"]).astype(np.float32)


def autoreset_ep_len0(task):
    """Episode lengths stored after the first reset.  DPCombinedEnv's RSI starts walk beyond the amnesty, so a fall ends no
    episode there and getup lasts 353 steps: every fourth env starts close to the 2000-step cap instead, which adds max_ep_len
    to the reasons the auto-reset is seen after.  DPEnv: all zero (walk robots fall by themselves)."""
    n = AUTORESET["envs"]
    ep = np.zeros(n, np.int32)
    if task == "combined":
        for i in range(1, n, 4):
            ep[i] = CAP_COMBINED - 3 - i
    return ep


def oracle_autoreset_rollout(task):
    """The auto-reset rollout of the GPU test on the oracle alone (free running, same seed, same actions, resets drawn by
    rsi_draw): (dones, reasons seen)."""
    from oracle import oracle_g1 as og
    comb = task == "combined"
    clips = [oracle_clip(m) for m in COMBINED_CLIPS] if comb else [oracle_clip("walk")]
    lengths = [c.L for c in clips]
    n, seed = AUTORESET["envs"], AUTORESET["seed"]
    acts = autoreset_actions()
    ep0 = autoreset_ep_len0(task)
    sims, rcnt = [], np.zeros(n, int)
    for i in range(n):
        s = og.G1CombSim(clips) if comb else og.G1Sim()
        s.set_caps(48, 256)
        motion, idx = rsi_draw(task, seed, i, 0, lengths)
        s.comb_reset(motion, idx) if comb else s.env_reset(clips[0], idx)
        (s.cenv if comb else s.env).episode_length = int(ep0[i])
        rcnt[i] = 1
        sims.append(s)
    dones, reasons = 0, {}
    for t in range(AUTORESET["steps"]):
        for i, s in enumerate(sims):
            _, _, d, _, rs = s.comb_step(acts[t, i].astype(np.float64)) if comb else s.env_step(clips[0], acts[t, i].astype(np.float64))
            if d:
                dones += 1
                reasons[rs] = reasons.get(rs, 0) + 1
                motion, idx = rsi_draw(task, seed, i, int(rcnt[i]), lengths)
                rcnt[i] += 1
                s.comb_reset(motion, idx) if comb else s.env_reset(clips[0], idx)
    return dones, reasons


# ------------------------------------------------------------------------------------------ clip playback
def playback_frames(motion):
    """Frames of the playback test: every frame and three past the wrap for the short cyclic clips; every fourth frame plus the
    last two for the long acyclic ones."""
    L = len(mocap(motion).data_config)
    if not clip_flags(motion)["acyclic"]:
        return [t % L for t in range(L + 3)]
    return sorted(set(range(0, L, 4)) | {L - 2, L - 1})
