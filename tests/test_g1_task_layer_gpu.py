"""The task layer of the Unitree G1 engine (csrc/dm_g1_task.h: step_enter, task_and_finish, the in-kernel auto-reset) against the fp64
oracle on every exit path, for DPEnv(robot="unitree_g1") and DPCombinedEnv(), through both pipelines.  The cases come from
tests/g1_task_cases.py; tests/test_g1_task_cases_cpu.py proves on the oracle alone that they reach what they name.

step_forced runs the monolithic kernel whatever DmG1Config.pipeline says (the split pipeline's launches serve MODE_STEP), so under
pipeline 2 the forced cases go through the same kernel as under pipeline 1; the stepped cases, the simulation error and the
auto-reset test are what reaches the task layer inside g1_env_kernel.
"""
import numpy as np
import pytest

import g1_task_cases as tc

pytestmark = pytest.mark.gpu

OBS_TOL, REW_TOL, TERMS_TOL, RESET_OBS_TOL = 3e-4, 5e-4, 5e-4, 1e-4      # tests/test_g1_gpu.py::test_g1_combined_env_matches_the_oracle
_REF = {}


def _reference(task):
    """The oracle's result of every single-step case of a task, computed once for both pipelines."""
    if task not in _REF:
        cases = [c for c in tc.all_cases() if c["task"] == task]
        _REF[task] = (cases, [tc.run_on_oracle(c) for c in cases])
    return _REF[task]


def _engine(task, pipeline, n, clips, auto_reset=False, seed=0):
    """clips: [(motion, flags)] by slot."""
    from deepmimic_mujoco_amd.g1 import G1HipEngine, TASK_COMBINED, TASK_DPENV
    comb = task == "combined"
    eng = G1HipEngine(n, auto_reset=auto_reset, seed=seed, pipeline=pipeline, task=TASK_COMBINED if comb else TASK_DPENV,
                      max_ep_length=tc.CAP_COMBINED if comb else tc.CAP_DPENV)
    for slot, (m, fl) in enumerate(clips):
        eng.load_clip(tc.mocap(m), clip_id=slot, **fl)
    return eng


def _i32(eng, a):
    import torch
    return torch.tensor(np.asarray(a, np.int32), device=eng.device).contiguous()


def _f32(eng, a):
    import torch
    return torch.tensor(np.asarray(a, np.float32), device=eng.device).contiguous()


def _read(eng, out):
    import torch
    torch.cuda.synchronize()
    r = {k: out[k].cpu().numpy() for k in ("obs", "rew", "done", "terms", "reason", "terminal_obs")}
    idx, ep, _ = eng.get_counters()
    r["idx"], r["ep_len"], r["motion"] = idx.cpu().numpy(), ep.cpu().numpy(), eng.get_motion().cpu().numpy()
    r["qpos"], r["qvel"], r["warm"] = [x.cpu().numpy() for x in eng.get_state()]
    return r


@pytest.mark.parametrize("pipeline", [1, 2])
@pytest.mark.parametrize("task", ["dpenv", "combined"])
def test_g1_single_step_cases_match_the_oracle(task, pipeline):
    """Every case of tests/g1_task_cases.py, each in its own env of one engine per task: the forced cases in one step_forced
    launch, then the stepped cases and the simulation error in one step launch (state stored with set_state(run_forward=False)).
    done, reason, the next idx_curr / n_steps, the episode length and the combined motion equal the oracle's as integers; obs
    within 3e-4, reward and terms within 5e-4, terms[7] as an integer; reasons 5 and 6 return obs, reward and terms of exact
    zeros; after the simulation error the stored state is qpos0 (bit-exact in fp32), zero velocity and warm start, counters and
    motion untouched.  No evaluation runs on the NaN state in either pipeline: g1_step_kernel skips forward() while
    X.sim_err is set, g1_env_kernel's round 0 goes from step_enter straight to task_and_finish and the write-back.

    DPEnv: 30 cases, reasons 0, 1, 2, 3, 4, 5, 6, 8; combined: 30 cases, reasons 0, 3, 5, 6, 7 and the transitions walk / run ->
    to_getup with and without done, to_getup -> getup by success and by time-out, getup -> run, getup -> run -> to_getup.
    Measured on an MI355X, both pipelines alike.  DPEnv: obs 2.7e-7, reward 1.8e-7, terms 1.0e-6, position after a stepped case
    8.2e-8; cases per reason {0: 2, 1: 2, 2: 12, 3: 3, 4: 3, 5: 1, 6: 3, 8: 4}.  Combined: obs 1.5e-6, reward 2.4e-7, terms 1.5e-6,
    position 6.2e-8; cases per reason {0: 17, 3: 3, 5: 1, 6: 2, 7: 7}; cases per transition walk -> to_getup 6 done + 2 with
    amnesty, run -> to_getup 1 + 1, to_getup -> getup 1 by success + 2 by time-out, getup -> run 1, getup -> run -> to_getup 2."""
    from oracle import oracle_g1 as og
    cases, ref = _reference(task)
    comb = task == "combined"
    n = len(cases)
    clips = [(m, {}) for m in tc.COMBINED_CLIPS] if comb else list(tc.DPENV_SLOTS)
    eng = _engine(task, pipeline, n, clips)
    out = eng.alloc_outputs()
    where = _i32(eng, [c["motion"] if comb else c["slot"] for c in cases])
    idx, ep = _i32(eng, [c["idx"] for c in cases]), _i32(eng, [c["ep_len"] for c in cases])

    def arm():
        eng.set_motion(where) if comb else eng.set_env_clips(where)
        eng.set_counters(idx, ep)
    arm()
    eng.reset(out["obs"], idx_init=_i32(eng, np.zeros(n)))
    benign = tc.frame("walk", 0)

    def rows(kinds):
        st = [(c["qpos"], c["qvel"]) if c["kind"] in kinds else benign for c in cases]
        return _f32(eng, [s[0] for s in st]), _f32(eng, [s[1] for s in st])
    got = [None] * n
    arm()
    q, v = rows(("forced",))
    eng.step_forced(q, v, out)
    r = _read(eng, out)
    for i, c in enumerate(cases):
        if c["kind"] == "forced":
            got[i] = {k: x[i] for k, x in r.items()}
    arm()
    q, v = rows(("stepped", "sim_error"))
    eng.set_state(q, v, warm=_f32(eng, np.zeros((n, og.NV))), run_forward=False)
    eng.step(_f32(eng, [c["action"] for c in cases]), out)
    r = _read(eng, out)
    for i, c in enumerate(cases):
        if c["kind"] != "forced":
            got[i] = {k: x[i] for k, x in r.items()}
    eng.close()

    g, _ = og.g1_model()
    worst = dict(obs=0.0, rew=0.0, terms=0.0, stepped_qpos=0.0)
    bad, reasons, compared = [], {}, 0
    for c, o, e in zip(cases, ref, got):
        assert e is not None, c["name"]
        compared += 1
        ints = (bool(e["done"]), int(e["reason"]), int(e["idx"]), int(e["ep_len"]))
        want = (bool(o["done"]), int(o["reason"]), int(o["idx"]), int(o["ep_len"]))
        if comb:
            ints, want = ints + (int(e["motion"]),), want + (int(o["motion"]),)
        if ints != want:
            bad.append((c["name"], "done / reason / idx / episode length / motion", ints, want))
        reasons[int(e["reason"])] = reasons.get(int(e["reason"]), 0) + 1
        if c["zeroed"]:
            if e["obs"].any() or e["rew"] != 0 or e["terms"].any():
                bad.append((c["name"], "obs, reward and terms must be exact zeros"))
        else:
            nt = 7 if comb else 5
            worst["obs"] = max(worst["obs"], np.abs(e["obs"] - o["obs"]).max())
            worst["rew"] = max(worst["rew"], abs(e["rew"] - o["rew"]))
            worst["terms"] = max(worst["terms"], np.abs(e["terms"][:nt] - o["terms"][:nt]).max())
            if comb and int(e["terms"][7]) != int(o["terms"][7]):
                bad.append((c["name"], "terms[7]", e["terms"][7], o["terms"][7]))
            if not (np.abs(e["obs"] - o["obs"]).max() < OBS_TOL and abs(e["rew"] - o["rew"]) < REW_TOL and
                    np.abs(e["terms"][:nt] - o["terms"][:nt]).max() < TERMS_TOL):
                bad.append((c["name"], "obs / reward / terms", np.abs(e["obs"] - o["obs"]).max(), abs(e["rew"] - o["rew"]),
                            np.abs(e["terms"][:nt] - o["terms"][:nt]).max()))
        if c["kind"] == "sim_error":
            if not (np.array_equal(e["qpos"], g.qpos0.astype(np.float32)) and not e["qvel"].any() and not e["warm"].any()):
                bad.append((c["name"], "the stored state must be qpos0, zero velocity, zero warm start"))
        elif c["kind"] == "stepped":
            worst["stepped_qpos"] = max(worst["stepped_qpos"], np.abs(e["qpos"] - o["qpos"]).max())
        else:
            f = c["qpos"].astype(np.float32)          # (the root quaternion is normalised in place)
            if not (np.array_equal(e["qpos"][:3], f[:3]) and np.array_equal(e["qpos"][7:], f[7:])):
                bad.append((c["name"], "a forced step stores the forced position"))
    print("G1 task layer, %s, pipeline %d: %d cases compared, worst %s, reasons %s" %
          (task, pipeline, compared, {k: float(x) for k, x in worst.items()}, dict(sorted(reasons.items()))))
    for b in bad:
        print("   MISMATCH", b)
    assert compared == n and not bad, bad
    assert worst["stepped_qpos"] < 1e-4          # north_star's per-step gate, as the teacher-forced tests hold it


@pytest.mark.parametrize("pipeline", [1, 2])
@pytest.mark.parametrize("task", ["dpenv", "combined"])
def test_g1_autoreset_matches_the_hash_and_the_oracle(task, pipeline):
    """auto_reset=True, seed 20, 32 envs, 40 steps of small random actions from reset() without idx_init (1280 oracle env-steps).
    The first reset is the RSI draw with reset count 0.  Before every step the oracle takes the engine's state and counters and
    both step: done and reason are equal on every env-step.  At every done: terminal_obs is the oracle's observation of the
    pre-reset state (3e-4); idx_curr / n_steps and the motion are the draw recomputed on the host (kernel_helpers.hash32 of seed,
    env, reset count) with the keys 0x5EED / 0x5EEE and, for walk, the amnesty + 10 offset; the episode length is 0; the returned obs is the
    oracle's reset observation at that draw (1e-4) and differs from terminal_obs.  Envs that go on are compared as well (obs
    3e-4, counters).  DPCombinedEnv's RSI starts walk beyond the amnesty, so every fourth env is put close to the 2000-step cap
    after the first reset (tests/g1_task_cases.py::autoreset_ep_len0): its resets follow max_ep_len and fallen-without-amnesty.
    At least 8 dones per task (the oracle alone: 64 and 10, tests/test_g1_task_cases_cpu.py).  Last, a simulation error
    under auto-reset: a NaN stored into env 0's position, one step: done, reason 5, zeros in reward, terms and terminal_obs, and the
    env reset to its next draw.

    Measured on an MI355X, both pipelines alike.  DPEnv: 64 dones (all low_z), up to 3 resets per env; reset obs 5.9e-8, terminal
    obs 5.4e-7, obs 1.2e-6, reward 2.4e-7; smallest |terminal_obs - obs| 1.05.  Combined: 10 dones (7 max_ep_len, 3 fallen without
    amnesty); reset obs 3.9e-6, terminal obs 8.9e-7, obs 7.4e-5, reward 5.7e-5; smallest |terminal_obs - obs| 0.91."""
    from oracle import oracle_g1 as og
    A = tc.AUTORESET
    n, seed, comb = A["envs"], A["seed"], task == "combined"
    names = tc.COMBINED_CLIPS if comb else ("walk",)
    eng = _engine(task, pipeline, n, [(m, tc.clip_flags(m) if not comb else {}) for m in names], auto_reset=True, seed=seed)
    oclips = [tc.oracle_clip(m) for m in names]
    lengths = [c.L for c in oclips]
    out = eng.alloc_outputs()
    eng.reset(out["obs"])
    r = _read(eng, out)
    sims = []
    worst = dict(reset_obs=0.0, terminal_obs=0.0, obs=0.0, rew=0.0)
    bad = []

    def check_reset(i, rcnt, r):
        motion, ix = tc.rsi_draw(task, seed, i, rcnt, lengths)
        if (int(r["idx"][i]), int(r["ep_len"][i])) != (ix, 0) or (comb and int(r["motion"][i]) != motion):
            bad.append(("reset", i, rcnt, int(r["idx"][i]), int(r["ep_len"][i]), int(r["motion"][i]), "drawn", motion, ix))
        o, err = sims[i].comb_reset(motion, ix) if comb else sims[i].env_reset(oclips[0], ix)
        worst["reset_obs"] = max(worst["reset_obs"], np.abs(r["obs"][i] - o).max())
    for i in range(n):
        s = og.G1CombSim(oclips) if comb else og.G1Sim()
        s.set_caps(48, 256)
        sims.append(s)
        check_reset(i, 0, r)
    eng.set_counters(None, _i32(eng, tc.autoreset_ep_len0(task)))
    acts = tc.autoreset_actions()
    rcnt = np.ones(n, int)
    dones, reasons, min_gap = 0, {}, np.inf
    r = _read(eng, out)
    for t in range(A["steps"]):
        b = r
        eng.step(_f32(eng, acts[t]), out)
        r = _read(eng, out)
        for i, s in enumerate(sims):
            env = s.cenv if comb else s.env
            if comb:
                env.motion, env.n_steps = int(b["motion"][i]), int(b["idx"][i])
            else:
                env.idx_curr = int(b["idx"][i])
            env.episode_length = int(b["ep_len"][i])
            s.set("qpos", b["qpos"][i].astype(np.float64)); s.set("qvel", b["qvel"][i].astype(np.float64))
            s.set("qacc_warmstart", b["warm"][i].astype(np.float64))
            a = acts[t, i].astype(np.float64)
            o, rew, d, terms, rs = s.comb_step(a) if comb else s.env_step(oclips[0], a)
            if (bool(r["done"][i]), int(r["reason"][i])) != (d, rs):
                bad.append(("done / reason", t, i, int(r["done"][i]), int(r["reason"][i]), d, rs))
                continue
            worst["rew"] = max(worst["rew"], abs(r["rew"][i] - rew))
            if d:
                dones += 1
                reasons[rs] = reasons.get(rs, 0) + 1
                worst["terminal_obs"] = max(worst["terminal_obs"], np.abs(r["terminal_obs"][i] - o).max())
                min_gap = min(min_gap, np.abs(r["terminal_obs"][i] - r["obs"][i]).max())
                check_reset(i, int(rcnt[i]), r)
                rcnt[i] += 1
            else:
                worst["obs"] = max(worst["obs"], np.abs(r["obs"][i] - o).max())
                after = (env.n_steps, env.episode_length, env.motion) if comb else (env.idx_curr, env.episode_length, 0)
                if (int(r["idx"][i]), int(r["ep_len"][i]), int(r["motion"][i]) if comb else 0) != after:
                    bad.append(("counters", t, i, int(r["idx"][i]), int(r["ep_len"][i]), int(r["motion"][i]), after))
    # a simulation error under auto-reset (src/deepmimic_env.py:366-378 inside a SubprocVecEnv worker): env 0's stored position gets
    # a NaN, the others keep their state; the step reports done / reason 5 with zeros and resets env 0 like after any other done
    q = r["qpos"].copy()
    q[0, 10] = np.nan
    eng.set_state(_f32(eng, q), _f32(eng, r["qvel"]), warm=_f32(eng, r["warm"]), run_forward=False)
    eng.step(_f32(eng, np.zeros((n, tc.NACT))), out)
    r = _read(eng, out)
    if not (r["done"][0] == 1 and r["reason"][0] == 5 and r["rew"][0] == 0 and not r["terminal_obs"][0].any() and not r["terms"][0].any()):
        bad.append(("simulation error under auto-reset", int(r["done"][0]), int(r["reason"][0]), float(r["rew"][0])))
    check_reset(0, int(rcnt[0]), r)
    if not np.isfinite(r["obs"]).all():
        bad.append(("a NaN reached an observation",))
    eng.close()
    print("G1 auto-reset, %s, pipeline %d: %d dones, reasons %s, resets per env up to %d, worst %s, smallest |terminal_obs - obs| %.3g" %
          (task, pipeline, dones, dict(sorted(reasons.items())), int(rcnt.max()), {k: float(x) for k, x in worst.items()}, min_gap))
    for x in bad:
        print("   MISMATCH", x)
    assert not bad, bad
    assert dones >= 8
    assert worst["reset_obs"] < RESET_OBS_TOL and worst["terminal_obs"] < OBS_TOL and worst["obs"] < OBS_TOL and worst["rew"] < REW_TOL
    assert min_gap > 1e-3, "terminal_obs must be the observation before the reset, not the one after it"


def _playback_reference():
    if "playback" not in _REF:
        from oracle import oracle_g1 as og
        pairs, ref = [], []
        for slot, m in enumerate(tc.G1_CLIPS):
            clip = tc.oracle_clip(m, **tc.clip_flags(m))
            s = og.G1Sim()
            s.set_caps(48, 256)
            for i in tc.playback_frames(m):
                s.env.idx_curr, s.env.episode_length = i, 0
                st = tc.frame(m, i)
                obs, rew, done, terms, reason = s.env_step(clip, np.zeros(tc.NACT), force_state=st)
                pairs.append((slot, i, clip.L, st))
                ref.append(dict(obs=obs, rew=rew, done=done, terms=terms, reason=reason, idx=s.env.idx_curr))
        _REF["playback"] = (pairs, ref)
    return _REF["playback"]


@pytest.mark.parametrize("pipeline", [1, 2])
def test_g1_every_clip_plays_back_on_its_own_tables(pipeline):
    """The six G1 clips in six slots of one engine, with the flags g1._load gives them, forced along their own frames: walk and
    run frame by frame through the wrap (L + 3 steps), the four getup clips every fourth frame and their last two (438 forced
    steps in 14 launches of 32 envs).  Against the oracle's result of the same forced step: terms within 5e-4, reward within
    5e-4, done, reason and the next idx_curr equal; the phase observation is idx / L; the acyclic clips report reason 4 on their
    last frame and nowhere else; the cyclic ones wrap to 0.

    terms[0..3] stay within 1e-5 of 1 plus the oracle's own distance from 1.  That distance is below 7e-7 for the velocity,
    end-effector and centre-of-mass terms on every frame and for the pose term of getup_facedown; the pose term of the other
    clips is below 1 in the reference itself, by up to 1e-4 (walk), 8e-4 (run) and 0.10 (the slow getup clips): their stored root
    quaternions are off unit length, MuJoCo normalises the state's, and the target pitch comes from the stored one
    (tests/test_g1_task_cases_cpu.py::test_every_clip_scores_one_on_its_own_frames).

    Measured on an MI355X, both pipelines alike: terms 4.7e-5, reward 3.5e-5, obs 4.9e-6 against the oracle; phase exact;
    |terms - 1| beyond the oracle's own 3.7e-6 (pose term), 0 for the other three; 4 acyclic ends, 6 wraps to frame 0."""
    pairs, ref = _playback_reference()
    n = 32
    eng = _engine("dpenv", pipeline, n, [(m, tc.clip_flags(m)) for m in tc.G1_CLIPS])
    out = eng.alloc_outputs()
    eng.reset(out["obs"], idx_init=_i32(eng, np.zeros(n)))
    worst = dict(terms=0.0, rew=0.0, obs=0.0, phase=0.0, above_oracle=np.zeros(4))
    bad, ends, wraps, launches = [], 0, 0, 0
    for k in range(0, len(pairs), n):
        chunk = list(range(k, min(k + n, len(pairs))))
        chunk += [chunk[-1]] * (n - len(chunk))
        eng.set_env_clips(_i32(eng, [pairs[j][0] for j in chunk]))
        eng.set_counters(_i32(eng, [pairs[j][1] for j in chunk]), _i32(eng, np.zeros(n)))
        eng.step_forced(_f32(eng, [pairs[j][3][0] for j in chunk]), _f32(eng, [pairs[j][3][1] for j in chunk]), out)
        r = _read(eng, out)
        launches += 1
        for e, j in enumerate(chunk[:min(n, len(pairs) - k)]):
            slot, i, L, _ = pairs[j]
            o = ref[j]
            if (bool(r["done"][e]), int(r["reason"][e]), int(r["idx"][e])) != (bool(o["done"]), int(o["reason"]), int(o["idx"])):
                bad.append((tc.G1_CLIPS[slot], i, int(r["done"][e]), int(r["reason"][e]), int(r["idx"][e]), o["done"], o["reason"], o["idx"]))
            ends += int(r["reason"][e]) == 4
            wraps += int(r["idx"][e]) == 0
            worst["terms"] = max(worst["terms"], np.abs(r["terms"][e] - o["terms"]).max())
            worst["rew"] = max(worst["rew"], abs(r["rew"][e] - o["rew"]))
            worst["obs"] = max(worst["obs"], np.abs(r["obs"][e] - o["obs"]).max())
            worst["phase"] = max(worst["phase"], abs(r["obs"][e][84] - i / L))
            worst["above_oracle"] = np.maximum(worst["above_oracle"], np.abs(r["terms"][e][:4] - 1) - np.abs(o["terms"][:4] - 1))
    eng.close()
    print("G1 clip playback, pipeline %d: %d forced steps in %d launches, acyclic ends %d, wraps to 0 %d, worst against the oracle: terms %.3g "
          "reward %.3g obs %.3g; phase against idx / L %.3g; |terms[0..3] - 1| beyond the oracle's own %s" %
          (pipeline, len(pairs), launches, ends, wraps, worst["terms"], worst["rew"], worst["obs"], worst["phase"],
           ["%.2g" % x for x in worst["above_oracle"]]))
    for b in bad:
        print("   MISMATCH", b)
    assert not bad, bad
    assert ends == 4 and wraps == 6          # four acyclic clips end; walk and run wrap, the acyclic ends wrap their counter too
    assert worst["terms"] < TERMS_TOL and worst["rew"] < REW_TOL and worst["obs"] < OBS_TOL
    assert worst["phase"] < 1e-6
    assert worst["above_oracle"].max() < 1e-5
