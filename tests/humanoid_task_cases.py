"""Single-step cases for the task layer of the humanoid3d engine (csrc/dm_kernels.hip: the part of step_body<TASK> after the
physics, and the in-kernel auto-reset), for task="dpenv" and task="combined".  A plain module: it builds the cases, runs them on
the fp64 oracle and restates the RSI draw; it touches no GPU and holds no test.  tests/test_humanoid_task_cases_cpu.py proves on
the oracle alone that every case reaches the branch it names; tests/test_humanoid_task_layer_gpu.py runs the same cases on the
engine, on the two-wave and on the three-wave kernels.

A case starts from a clip frame with a small, fixed edit (a root height, a roll or pitch put onto the root quaternion, one joint
velocity of 5000, one joint angle moved) rounded to fp32, so engine and oracle see the same input.  Three kinds:
  forced    the state goes in through step_forced / force_state=: one forward evaluation, physics plays no part
  stepped   the state is stored without evaluation (set_state(run_forward=False)), zero warm start, then one real step
  sim_error a stored state with a NaN joint position, then a real step: mj_checkPos fails before any evaluation runs

The height rule reads the centre of mass (S.com[2] / the mass-weighted xipos, src/deepmimic_env.py:420-424), not the pelvis: the
heights used here put it far from 0.7 and 2.0, and the CPU test asserts the margin from the oracle's own value.

Episode cap: the reference tests `episode_length >= MAX_EP_LENGTH` BEFORE the increment (src/deepmimic_env.py:435-438 against
:455, src/combined_env.py:442-445 against :456), so the step taken with the counter at cap - 1 is alive and the one at cap reports
max_ep_len.  The cases sit at cap - 2, cap - 1 and cap.
"""
import math

import numpy as np

from deepmimic_mujoco_amd.config import MotionConfig
from deepmimic_mujoco_amd.mocap import MocapDM
from deepmimic_mujoco_amd.model import load_model

COMBINED_CLIPS = (("walk", {}), ("run", {}), ("getup_facedown", dict(floor=True, acyclic=True)))      # tests/test_combined_env.py
# clip slots of the DPEnv engine that runs the single-step cases: (motion, flags).  The first three are the flag sets of
# tests/test_step_paths_bits_gpu.py; the run clip has another length, so a slot mix-up shows in the wrap and in the phase
DPENV_SLOTS = (("walk", {}), ("walk", dict(acyclic=True)), ("walk", dict(floor=True)), ("run", {}))
WALK, WALKACYC, WALKFLOOR, RUN = range(4)
CAP_DPENV, CAP_COMBINED, AMNESTY, TO_GETUP_LEN = 1000, 2000, 150, 180      # dm_default_config / the oracle's constants
LOW_Z, HIGH_Z, OBS_BOUND = 0.7, 2.0, 100.0
ALIM, MAX_ANGLE = math.radians(15.0), math.radians(60.0)
M_WALK, M_RUN, M_GETUP, M_TO_GETUP = 0, 1, 2, 3
NACT, NQ, NV = 28, 35, 34
ONE_FOOT_FRAME = 8           # walk: the right foot carries, the left one is 0.18 m up (the CPU test asserts both, with margins)

_MOCAP = {}


def model():
    return load_model()


def mocap(motion):
    if motion not in _MOCAP:
        mc = MocapDM(model=model())
        mc.load_mocap(MotionConfig(motion).mocap_path)
        _MOCAP[motion] = mc
    return _MOCAP[motion]


def length(motion):
    return len(mocap(motion).tables()[0])


def oracle_clip(motion, **flags):
    from oracle.oracle import OracleClip
    return OracleClip(*mocap(motion).tables(), **flags)


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def to_rpy(q):
    """py3dtf's to_rpy as the reference uses it: ZYX, the quaternion (w, x, y, z) taken as stored, not normalised."""
    w, x, y, z = q
    return np.array([math.atan2(2 * (w * x + y * z), 1 - 2 * (x * x + y * y)), math.asin(max(-1.0, min(1.0, 2 * (w * y - z * x)))),
                     math.atan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z))])


def from_rpy(r, p, y):
    cr, sr, cp, sp, cy, sy = math.cos(r / 2), math.sin(r / 2), math.cos(p / 2), math.sin(p / 2), math.cos(y / 2), math.sin(y / 2)
    return np.array([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy])


def frame(motion, i, z=None, roll_deg=None, pitch_deg=None, vel8=None, joint=None):
    """(qpos, qvel) of frame i of a clip, fp32-rounded, with the edits.  roll_deg / pitch_deg: the root quaternion becomes the
    unit quaternion whose roll / pitch is that many degrees away from the roll / pitch the rules read off this frame's stored
    quaternion (py3dtf's to_rpy does not normalise it), the other two angles as the frame's; joint = (qpos index, degrees)."""
    q, v = (np.array(t[i], np.float64) for t in mocap(motion).tables()[:2])
    if z is not None:
        q[2] = z
    if roll_deg is not None or pitch_deg is not None:
        r, p, y = to_rpy(mocap(motion).tables()[0][i][3:7])
        q[3:7] = from_rpy(r + math.radians(roll_deg or 0.0), p + math.radians(pitch_deg or 0.0), y)
    if vel8 is not None:
        v[8] = vel8
    if joint is not None:
        q[joint[0]] += math.radians(joint[1])
    return f32(q), f32(v)


def _case(name, task, kind, state, expect_reason, expect_done, **kw):
    c = dict(name=name, task=task, kind=kind, qpos=state[0], qvel=state[1], reason=expect_reason, done=expect_done,
             slot=WALK, motion=M_WALK, idx=0, ep_len=0, action=np.zeros(NACT), zeroed=expect_reason in (5, 6), boundary=False,
             next_idx=None, next_motion=None, on_frame=None, phase=None, feet=None)
    c.update(kw)
    return c


def dpenv_cases():
    Lw, Lr = length("walk"), length("run")
    D = lambda name, state, reason, done, **kw: _case(name, "dpenv", kw.pop("kind", "forced"), state, reason, done, **kw)
    cap = CAP_DPENV
    lying = frame("getup_facedown", 3)
    z_foot = float(mocap("walk").tables()[0][ONE_FOOT_FRAME][2]) - 0.02      # two centimetres into the floor: contacts beyond doubt
    cases = [
        D("alive", frame("walk", 10), 2, False, idx=10, on_frame=10),                        # low / high is written every step (:424)
        D("alive on the run clip", frame("run", 20), 2, False, slot=RUN, idx=20, on_frame=20, phase=20.0 / Lr),
        D("low_z", frame("walk", 10, z=0.30), 1, True, idx=10),
        D("high_z", frame("walk", 10, z=2.5), 2, True, idx=10),
        D("floor clip, lying", lying, 0, False, slot=WALKFLOOR, idx=3),
        D("cap - 2", frame("walk", 10), 2, False, idx=10, ep_len=cap - 2, boundary=True),
        D("cap - 1", frame("walk", 10), 2, False, idx=10, ep_len=cap - 1, boundary=True),
        D("cap", frame("walk", 10), 3, True, idx=10, ep_len=cap),
        D("cap over low_z", frame("walk", 10, z=0.30), 3, True, idx=10, ep_len=cap),
        D("acyclic, L - 2", frame("walk", Lw - 2), 2, False, slot=WALKACYC, idx=Lw - 2, boundary=True, on_frame=Lw - 2),
        D("acyclic end", frame("walk", Lw - 1), 4, True, slot=WALKACYC, idx=Lw - 1, next_idx=0),
        D("acyclic end over cap", frame("walk", Lw - 1), 4, True, slot=WALKACYC, idx=Lw - 1, ep_len=cap, next_idx=0),
        D("cyclic wrap", frame("walk", Lw - 1), 2, False, idx=Lw - 1, next_idx=0, on_frame=Lw - 1),
        D("cyclic wrap on the run clip", frame("run", Lr - 1), 2, False, slot=RUN, idx=Lr - 1, next_idx=0, phase=(Lr - 1.0) / Lr),
        D("obs bound", frame("walk", 10, vel8=5000.0), 6, True, idx=10),
        D("obs bound over low_z", frame("walk", 10, z=0.30, vel8=5000.0), 6, True, idx=10),
        D("obs bound over cap and acyclic end", frame("walk", Lw - 1, vel8=5000.0), 6, True, slot=WALKACYC, idx=Lw - 1, ep_len=cap, next_idx=0),
        D("one foot on the floor", frame("walk", ONE_FOOT_FRAME, z=z_foot), 2, False, idx=ONE_FOOT_FRAME, feet=(1.0, 0.0)),
        D("no foot on the floor", frame("walk", 10, z=1.5), 2, False, idx=10, feet=(0.0, 0.0)),
    ]
    # the same rules through a real step: the margins are wide enough for one step of physics
    cases += [
        D("stepped alive", frame("walk", 10), 2, False, kind="stepped", idx=10),
        D("stepped low_z", lying, 1, True, kind="stepped", idx=10),
        D("stepped high_z", frame("walk", 10, z=2.5), 2, True, kind="stepped", idx=10),
        D("stepped floor clip", lying, 0, False, kind="stepped", slot=WALKFLOOR, idx=3),
        D("stepped cap - 1", frame("walk", 10), 2, False, kind="stepped", idx=10, ep_len=cap - 1, boundary=True),
        D("stepped cap", frame("walk", 10), 3, True, kind="stepped", idx=10, ep_len=cap),
        D("stepped acyclic end", frame("walk", Lw - 1), 4, True, kind="stepped", slot=WALKACYC, idx=Lw - 1, next_idx=0),
        D("stepped cyclic wrap", frame("run", Lr - 1), 2, False, kind="stepped", slot=RUN, idx=Lr - 1, next_idx=0),
    ]
    q, v = frame("walk", 10)
    q[10] = float("nan")
    cases.append(D("sim error", (q, v), 5, True, kind="sim_error", idx=10, ep_len=17, next_idx=10))
    for c in cases:
        if c["next_idx"] is None:
            c["next_idx"] = c["idx"] + 1
    return cases


def combined_cases():
    L = [length(m) for m, _ in COMBINED_CLIPS]
    C = lambda name, state, reason, done, **kw: _case(name, "combined", kw.pop("kind", "forced"), state, reason, done, **kw)
    cap = CAP_COMBINED
    fell = dict(next_motion=M_TO_GETUP, next_idx=1)
    lying, standing_up = frame("getup_facedown", 1), frame("getup_facedown", L[2] - 1)
    A, Z = AMNESTY, 1.3            # Z: a root height at which the tilted body touches nothing and its centre of mass stays between the limits

    def tilted(motion, n, **kw):
        return frame(motion, n % L[M_RUN if motion == "run" else M_WALK], z=Z, **kw)
    cases = [
        C("walk alive, past one clip", frame("walk", 37), 0, False, idx=L[0] + 37, on_frame=37, phase=37.0 / L[0]),
        C("run alive, past two clips", frame("run", 5), 0, False, motion=M_RUN, idx=2 * L[1] + 5, on_frame=5, phase=5.0 / L[1]),
        C("walk fall by low_z, no amnesty", frame("walk", 10, z=0.30), 7, True, idx=10, **fell),
        C("walk fall by low_z at the amnesty boundary", frame("walk", A % L[0], z=0.30), 7, True, idx=A, **fell),
        C("walk fall by low_z with amnesty", frame("walk", (A + 1) % L[0], z=0.30), 0, False, idx=A + 1, **fell),
        C("walk fall by high_z", frame("walk", 10, z=2.5), 7, True, idx=10, **fell),
        C("fall by roll, no amnesty", tilted("walk", 10, roll_deg=70.0), 7, True, idx=10, **fell),
        C("fall by roll with amnesty", tilted("run", 200, roll_deg=-70.0), 0, False, motion=M_RUN, idx=200, **fell),
        C("fall by pitch, no amnesty", tilted("run", 10, pitch_deg=-70.0), 7, True, motion=M_RUN, idx=10, **fell),
        C("fall by pitch with amnesty", tilted("walk", 200, pitch_deg=70.0), 0, False, idx=200, **fell),
        C("roll just inside", tilted("walk", 10, roll_deg=59.9), 0, False, idx=10, boundary=True),
        C("roll just outside", tilted("walk", 10, roll_deg=60.1), 7, True, idx=10, **fell),
        C("pitch just inside", tilted("run", 10, pitch_deg=-59.9), 0, False, motion=M_RUN, idx=10, boundary=True),
        C("pitch just outside", tilted("run", 10, pitch_deg=-60.1), 7, True, motion=M_RUN, idx=10, **fell),
        C("to_getup success", lying, 0, False, motion=M_TO_GETUP, idx=5, next_motion=M_GETUP, next_idx=1),
        C("to_getup, one joint 16 degrees off", frame("getup_facedown", 1, joint=(10, 16.0)), 0, False, motion=M_TO_GETUP, idx=5, boundary=True),
        C("to_getup, one short of the time-out", frame("walk", 10), 0, False, motion=M_TO_GETUP, idx=TO_GETUP_LEN - 2, boundary=True),
        C("to_getup time-out", frame("walk", 10), 0, False, motion=M_TO_GETUP, idx=TO_GETUP_LEN - 1, next_motion=M_GETUP, next_idx=1),
        C("getup, one short of the time-out", lying, 0, False, motion=M_GETUP, idx=L[2] - 2, boundary=True),
        C("getup time-out, lying: run, then fallen", lying, 7, True, motion=M_GETUP, idx=L[2] - 1, **fell),
        C("getup time-out, standing: run", standing_up, 0, False, motion=M_GETUP, idx=L[2] - 1, next_motion=M_RUN, next_idx=1, on_frame=L[2] - 1),
        C("cap - 2", frame("walk", 10), 0, False, idx=200, ep_len=cap - 2, boundary=True),
        C("cap - 1", frame("walk", 10), 0, False, idx=200, ep_len=cap - 1, boundary=True),
        C("cap", frame("walk", 10), 3, True, idx=200, ep_len=cap),
        C("cap over a fall without amnesty", frame("walk", 10, z=0.30), 3, True, idx=10, ep_len=cap, **fell),
        C("obs bound", frame("walk", 10, vel8=5000.0), 6, True, idx=200),
        C("obs bound over a fall and the cap", frame("walk", 10, z=0.30, vel8=5000.0), 6, True, idx=10, ep_len=cap, **fell),
    ]
    cases += [
        C("stepped walk alive", frame("walk", 200 % L[0]), 0, False, kind="stepped", idx=200),
        C("stepped walk fall, no amnesty", lying, 7, True, kind="stepped", idx=A, **fell),
        C("stepped walk fall with amnesty", frame("getup_facedown", 3), 0, False, kind="stepped", idx=A + 1, **fell),
        C("stepped to_getup success", lying, 0, False, kind="stepped", motion=M_TO_GETUP, idx=5, next_motion=M_GETUP, next_idx=1),
        C("stepped to_getup time-out", frame("walk", 10), 0, False, kind="stepped", motion=M_TO_GETUP, idx=TO_GETUP_LEN - 1, next_motion=M_GETUP, next_idx=1),
        C("stepped getup time-out, lying", lying, 7, True, kind="stepped", motion=M_GETUP, idx=L[2] - 1, **fell),
        C("stepped getup time-out, standing", standing_up, 0, False, kind="stepped", motion=M_GETUP, idx=L[2] - 1, next_motion=M_RUN, next_idx=1),
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
        _ORACLE[task] = [oracle_clip(m, **fl) for m, fl in (DPENV_SLOTS if task == "dpenv" else COMBINED_CLIPS)]
    return _ORACLE[task]


def new_sim(task):
    from oracle.oracle import OracleCombined, OracleSim
    s = OracleCombined(model(), oracle_clips(task)) if task == "combined" else OracleSim(model())
    s.set_caps(32, 128)
    return s


def target_frame(case):
    """(clip tables, frame) the reward and the angle rules of the case's step read: the to_getup transition aims at frame 1 of
    getup (src/combined_env.py:72-79)."""
    if case["task"] == "dpenv":
        return mocap(DPENV_SLOTS[case["slot"]][0]).tables(), case["idx"]
    if case["motion"] == M_TO_GETUP:
        return mocap(COMBINED_CLIPS[M_GETUP][0]).tables(), 1
    tab = mocap(COMBINED_CLIPS[case["motion"]][0]).tables()
    return tab, case["idx"] % len(tab[0])


def tested_quantities(case, s):
    """What the rules of the case's step compare with their thresholds, from the oracle's own fp64 state after the evaluation:
    centre-of-mass height, |roll - target roll|, |pitch - target pitch| and the 28 joint differences."""
    cm = model().cstruct
    xi = s.get("xipos")
    mass = np.array([cm.body_mass[b] for b in range(len(xi))])
    q = s.get("qpos")
    tab, fi = target_frame(case)
    tq = tab[0][fi]
    rc, rt = to_rpy(q[3:7]), to_rpy(tq[3:7])
    return dict(zc=float((mass * xi[:, 2]).sum() / mass.sum()), droll=abs(rc[0] - rt[0]), dpitch=abs(rc[1] - rt[1]),
                djoint=np.abs(q[7:] - tq[7:]))


def run_on_oracle(case, dz=0.0):
    """The case on a fresh fp64 environment.  forced: force_state=; stepped / sim_error: the state stored as it is (zero warm
    start), then a step with the case's action.  Returns what the engine is compared with, and the tested quantities.  dz moves
    the root that far up (the CPU test's look at how firmly the contacts of a forced case stand)."""
    clips = oracle_clips(case["task"])
    comb = case["task"] == "combined"
    s = new_sim(case["task"])
    if comb:
        s.cenv.motion, s.cenv.n_steps, s.cenv.episode_length = case["motion"], case["idx"], case["ep_len"]
        step = s.comb_step
    else:
        s.env.idx_curr, s.env.episode_length = case["idx"], case["ep_len"]
        step = lambda a, force_state=None: s.env_step(clips[case["slot"]], a, force_state=force_state)
    qpos = case["qpos"].copy()
    qpos[2] += dz
    if case["kind"] == "forced":
        obs, rew, done, terms, reason = step(np.zeros(NACT), force_state=(qpos, case["qvel"]))
    else:
        s.set("qpos", qpos); s.set("qvel", case["qvel"]); s.set("qacc_warmstart", np.zeros(NV))
        obs, rew, done, terms, reason = step(case["action"])
    env = s.cenv if comb else s.env
    r = dict(obs=obs, rew=rew, done=done, terms=terms, reason=reason, idx=env.n_steps if comb else env.idx_curr,
             ep_len=env.episode_length, motion=env.motion if comb else case["slot"], qpos=s.get("qpos"), qvel=s.get("qvel"),
             warm=s.get("qacc_warmstart"), qacc=s.get("qacc"), ncon=s.ncon, contact=s.get("contact"), geom_xpos=s.get("geom_xpos"))
    if case["kind"] != "sim_error":
        r.update(tested_quantities(case, s))
    return r


# ------------------------------------------------------------------------------------------ the RSI draw of the auto-reset
def rsi_draw(task, seed, env, rcnt, lengths):
    """(motion, idx) of reset number rcnt of an env, as step_body draws it: DPEnv `hash(.., 0x5EED) % L`; DPCombinedEnv.reset(rsi=True)
    (src/combined_env.py:219-227) getup or walk from bit 0 of the 0x5EED draw, frame from the 0x5EEE draw, walk starting
    AMNESTY_STEPS + 10 steps in.  The hash is dm_hash32 of csrc/dm_rng.h as tests/kernel_helpers.py restates it."""
    from kernel_helpers import hash32
    if task == "dpenv":
        return 0, hash32(seed, env, rcnt, 0x5EED) % lengths[0]
    motion = M_GETUP if hash32(seed, env, rcnt, 0x5EED) & 1 else M_WALK
    return motion, hash32(seed, env, rcnt, 0x5EEE) % lengths[motion] + (AMNESTY + 10 if motion == M_WALK else 0)


AUTORESET = dict(seed=20, envs=32, steps=40, act_scale=0.05, act_seed=6, min_dones=10)


def autoreset_actions():
    rng = np.random.default_rng(AUTORESET["act_seed"])
    return (rng.uniform(-1, 1, (AUTORESET["steps"], AUTORESET["envs"], NACT)) * AUTORESET["act_scale"]).astype(np.float32)


def autoreset_counters0(task, draws):
    """(idx_curr / n_steps, episode length) stored after the first reset; draws: the (motion, idx) of that reset.  Every fourth
    env starts close to the cap, which adds max_ep_len to the reasons the auto-reset is seen after.  DPCombinedEnv's RSI starts
    walk beyond the amnesty, where a fall ends no episode, and getup lasts 183 steps: every other fourth env that drew walk has
    its n_steps taken back by whole clip lengths to below the amnesty (same frame), so that its fall is one without amnesty."""
    n = AUTORESET["envs"]
    idx, ep = np.array([d[1] for d in draws], np.int32), np.zeros(n, np.int32)
    cap = CAP_COMBINED if task == "combined" else CAP_DPENV
    for i in range(1, n, 4):
        ep[i] = cap - 3 - i
    if task == "combined":
        Lw = length("walk")
        for i in range(3, n, 4):
            if draws[i][0] == M_WALK:
                idx[i] = idx[i] % Lw
    return idx, ep


def oracle_autoreset_rollout(task):
    """The auto-reset rollout of the GPU test on the oracle alone (free running, same seed, same actions, resets drawn by
    rsi_draw): (dones, reasons seen)."""
    comb = task == "combined"
    clips = oracle_clips("combined") if comb else [oracle_clips("dpenv")[WALK]]
    lengths = [c.L for c in clips]
    n, seed = AUTORESET["envs"], AUTORESET["seed"]
    acts = autoreset_actions()
    draws = [rsi_draw(task, seed, i, 0, lengths) for i in range(n)]
    idx0, ep0 = autoreset_counters0(task, draws)
    sims, rcnt = [], np.ones(n, int)
    for i in range(n):
        s = new_sim(task)
        s.comb_reset(*draws[i]) if comb else s.env_reset(clips[0], draws[i][1])
        env = s.cenv if comb else s.env
        env.episode_length = int(ep0[i])
        if comb:
            env.n_steps = int(idx0[i])
        sims.append(s)
    dones, reasons = 0, {}
    for t in range(AUTORESET["steps"]):
        for i, s in enumerate(sims):
            a = acts[t, i].astype(np.float64)
            _, _, d, _, rs = s.comb_step(a) if comb else s.env_step(clips[0], a)
            if d:
                dones += 1
                reasons[rs] = reasons.get(rs, 0) + 1
                motion, idx = rsi_draw(task, seed, i, int(rcnt[i]), lengths)
                rcnt[i] += 1
                s.comb_reset(motion, idx) if comb else s.env_reset(clips[0], idx)
    return dones, reasons
