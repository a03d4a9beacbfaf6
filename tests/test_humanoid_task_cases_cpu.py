"""The cases of tests/humanoid_task_cases.py on the fp64 oracle alone (no GPU): every case reaches the reason, the done flag and the
counter changes it names, the set covers every reason and every motion transition of both tasks, every quantity a rule tests is
at least 1e-3 away from its threshold in the oracle's own fp64 value (so no case may be left out of the GPU comparison for
being too close), the boundary cases are alive and their twins on the other side are not, and the oracle's auto-reset rollout
ends enough episodes.  This is what keeps tests/test_humanoid_task_layer_gpu.py from passing on cases that never reach their
branch."""
import numpy as np
import pytest

import humanoid_task_cases as tc

MARGIN = 1e-3


@pytest.fixture(scope="module")
def results():
    return [(c, tc.run_on_oracle(c)) for c in tc.all_cases()]


def test_cases_are_named_once_and_fp32_exact():
    cases = tc.all_cases()
    names = [(c["task"], c["name"]) for c in cases]
    assert len(set(names)) == len(names)
    for c in cases:
        ok = np.isfinite(c["qpos"])
        assert c["qpos"].shape == (tc.NQ,) and c["qvel"].shape == (tc.NV,)
        assert np.array_equal(c["qpos"][ok], tc.f32(c["qpos"][ok])) and np.array_equal(c["qvel"], tc.f32(c["qvel"])), c["name"]
        assert (~ok).sum() == (1 if c["kind"] == "sim_error" else 0)
        assert c["kind"] in ("forced", "stepped", "sim_error")


def test_every_case_reaches_what_it_names(results):
    for c, r in results:
        tag = (c["task"], c["name"])
        assert (r["reason"], r["done"]) == (c["reason"], c["done"]), (tag, r["reason"], r["done"])
        assert r["idx"] == c["next_idx"], (tag, r["idx"])
        # the counters advance on every path but the simulation error, which returns before them (src/deepmimic_env.py:366-378)
        assert r["ep_len"] == c["ep_len"] + (0 if c["kind"] == "sim_error" else 1), (tag, r["ep_len"])
        if c["task"] == "combined":
            assert r["motion"] == c["next_motion"], (tag, r["motion"])
        if c["zeroed"]:
            assert not r["obs"].any() and r["rew"] == 0 and not r["terms"].any(), tag
        else:
            assert np.isfinite(r["obs"]).all() and r["obs"].any() and np.abs(r["obs"]).max() <= tc.OBS_BOUND - 1.0, tag
        if c["kind"] != "sim_error":
            # far from mj_checkAcc's 1e10, so that an fp32 evaluation cannot turn the case into a simulation error
            assert np.abs(r["qacc"]).max() < 1e8, (tag, np.abs(r["qacc"]).max())
        if c["on_frame"] is not None:
            # the reward was taken against this frame: forced onto it, the pose and velocity terms are 1 (the pose term up to what a
            # root quaternion stored off unit length costs); one frame off costs more than 1e-3 (test_reward_frames_are_told_apart).
            # The end-effector term is left out: the clips' end-effector tables are up to 7 mm off their own frames (0.998)
            assert np.abs(r["terms"][:2] - 1).max() < 2e-4, (tag, r["terms"])
        if c["phase"] is not None:
            assert abs(r["obs"][66 if c["task"] == "dpenv" else 64] - c["phase"]) < 1e-12, tag
        if c["feet"] is not None:
            assert tuple(r["obs"][64:66]) == c["feet"], (tag, r["obs"][64:66])


def test_reward_frames_are_told_apart(results):
    """The cases that pin the reward frame would notice a neighbouring frame: the same state scored one frame off is not 1."""
    by = {(c["task"], c["name"]): c for c, _ in results}
    for key, other in ((("dpenv", "cyclic wrap"), 0), (("dpenv", "alive on the run clip"), 19),
                       (("combined", "walk alive, past one clip"), 36), (("combined", "run alive, past two clips"), 2 * 48 + 4)):
        c = dict(by[key])
        c["idx"] = other
        r = tc.run_on_oracle(c)
        assert np.abs(r["terms"][:2] - 1).max() > 1e-3, (key, r["terms"])


def test_every_tested_quantity_is_far_from_its_threshold(results):
    """In the oracle's own fp64 values, after the evaluation the rules read: the centre of mass at least 1e-3 from 0.7 and 2.0;
    under the combined task the roll and pitch differences at least 1e-3 from 15 and 60 degrees and every one of the 28 joint
    differences at least 1e-3 from 15 degrees (terms[7] counts them, and the GPU test compares it as an integer); the largest
    |obs| at least 1 from the bound of 100 (a guard case has an entry of 500).  The "just inside" / "just outside" pairs sit
    1.7e-3 rad from 60 degrees, the 16-degree joint 1.7e-2 from 15.  An fp32 evaluation is within 1e-5 of these."""
    worst = {}
    for c, r in results:
        if c["kind"] == "sim_error":
            continue
        tag = (c["task"], c["name"])
        m = dict(zc=min(abs(r["zc"] - tc.LOW_Z), abs(r["zc"] - tc.HIGH_Z)))
        if c["task"] == "combined":
            for k in ("droll", "dpitch"):
                m[k] = min(abs(r[k] - tc.ALIM), abs(r[k] - tc.MAX_ANGLE))
            m["djoint"] = np.abs(r["djoint"] - tc.ALIM).min()
        largest = abs(c["qvel"][8]) * 0.1 if c["reason"] == 6 else np.abs(r["obs"]).max()      # a guarded observation comes back as zeros
        assert abs(largest - tc.OBS_BOUND) >= 1.0 and (largest > tc.OBS_BOUND) == (c["reason"] == 6), (tag, largest)
        for k, x in m.items():
            assert x >= MARGIN, (tag, k, x)
            if x < worst.get(k, (np.inf,))[0]:
                worst[k] = (float(x), c["name"])
    print("smallest distance from a threshold:", worst)


def test_boundary_twins(results):
    """Each case on the alive side of a boundary has a twin on the other side that is not alive, from the same state."""
    by = {(c["task"], c["name"]): (c, r) for c, r in results}
    pairs = [("dpenv", "cap - 1", "cap"), ("dpenv", "acyclic, L - 2", "acyclic end"), ("dpenv", "stepped cap - 1", "stepped cap"),
             ("combined", "cap - 1", "cap"), ("combined", "stepped cap - 1", "stepped cap"),
             ("combined", "roll just inside", "roll just outside"), ("combined", "pitch just inside", "pitch just outside"),
             ("combined", "to_getup, one joint 16 degrees off", "to_getup success"),
             ("combined", "to_getup, one short of the time-out", "to_getup time-out"),
             ("combined", "getup, one short of the time-out", "getup time-out, lying: run, then fallen"),
             ("combined", "walk fall by low_z with amnesty", "walk fall by low_z at the amnesty boundary")]
    for task, inside, outside in pairs:
        (ci, ri), (co, ro) = by[(task, inside)], by[(task, outside)]
        assert not ri["done"] and ri["reason"] in (0, 2), (task, inside)
        changed = ro["done"] or (task == "combined" and ro["motion"] != co["motion"] and ri["motion"] == ci["motion"])
        assert changed, (task, outside)
    # the angle pairs differ by 0.2 degrees and nothing else; the joint pair by one joint
    for a, b, k in (("roll just inside", "roll just outside", "droll"), ("pitch just inside", "pitch just outside", "dpitch")):
        ri, ro = by[("combined", a)][1], by[("combined", b)][1]
        assert ri[k] < tc.MAX_ANGLE - MARGIN and ro[k] > tc.MAX_ANGLE + MARGIN and abs(ro[k] - ri[k] - np.radians(0.2)) < 1e-6
    r16, r0 = by[("combined", "to_getup, one joint 16 degrees off")][1], by[("combined", "to_getup success")][1]
    assert (r16["djoint"] > tc.ALIM).sum() == 1 and r16["terms"][7] == 1 and r0["terms"][7] == 0
    assert max(r16["droll"], r16["dpitch"]) < tc.ALIM - MARGIN


def test_foot_contact_cases_stand_firmly(results):
    """One foot: the right foot's contacts are all deeper than 5 mm and the left foot is more than 0.1 m higher; none: both feet
    more than 0.5 m up.  And no forced DPEnv case changes its foot-contact observation when the root moves 2e-4 up or down, two
    hundred times what fp32 kinematics are off by (the combined observation has no contact entries, and a forced step observes
    nothing else that a contact changes)."""
    cm = tc.model().cstruct
    by = {(c["task"], c["name"]): (c, r) for c, r in results}
    c, r = by[("dpenv", "one foot on the floor")]
    feet = r["geom_xpos"][[cm.rfoot_geom, cm.lfoot_geom], 2]
    assert r["ncon"] >= 1 and r["contact"][:r["ncon"], 0].max() < -5e-3 and feet[1] - feet[0] > 0.1, (r["contact"][:, 0], feet)
    c, r = by[("dpenv", "no foot on the floor")]
    assert r["ncon"] == 0 and r["geom_xpos"][[cm.rfoot_geom, cm.lfoot_geom], 2].min() > 0.5
    for c, r in results:
        if c["task"] == "dpenv" and c["kind"] == "forced" and not c["zeroed"]:
            for dz in (-2e-4, 2e-4):
                assert np.array_equal(tc.run_on_oracle(c, dz=dz)["obs"][64:66], r["obs"][64:66]), (c["name"], dz)


def test_sim_error_resets_the_state(results):
    qpos0 = np.array(tc.model().qpos0, np.float64)
    seen = 0
    for c, r in results:
        if c["kind"] == "sim_error":
            seen += 1
            assert np.array_equal(r["qpos"], qpos0) and not r["qvel"].any() and not r["warm"].any(), c["task"]
            assert (c["idx"], c["ep_len"]) != (0, 0) and (r["idx"], r["ep_len"], r["motion"]) == (c["idx"], c["ep_len"], c["next_motion"] or 0)
    assert seen == 2


def test_quotas(results):
    """Every reason a task has, every transition of the combined state machine, and the boundaries on their alive side."""
    for task, reasons in (("dpenv", (0, 1, 2, 3, 4, 5, 6)), ("combined", (0, 3, 5, 6, 7))):
        for kind in ("any", "stepped"):
            got = {}
            for c, r in results:
                if c["task"] == task and (kind == "any" or c["kind"] != "forced"):
                    got[r["reason"]] = got.get(r["reason"], 0) + 1
            want = set(reasons) - ({6} if kind == "stepped" else set())      # the obs bound has forced cases only
            print(task, kind, "cases per reason", dict(sorted(got.items())))
            assert want <= set(got), (task, kind, sorted(want - set(got)))
    assert not any(r["reason"] == 4 for c, r in results if c["task"] == "combined")
    assert not any(r["reason"] == 7 for c, r in results if c["task"] == "dpenv")
    trans = {}
    Lg = tc.length("getup_facedown")
    for c, r in results:
        if c["task"] == "combined" and r["motion"] != c["motion"]:
            by_timeout = (c["motion"] == tc.M_TO_GETUP and c["idx"] >= tc.TO_GETUP_LEN - 1 or c["motion"] == tc.M_GETUP and c["idx"] >= Lg - 1)
            key = (c["motion"], r["motion"], bool(r["done"]), by_timeout)
            trans[key] = trans.get(key, 0) + 1
    print("combined transitions (from, to, done, out of time):", trans)
    W, R, G, T = tc.M_WALK, tc.M_RUN, tc.M_GETUP, tc.M_TO_GETUP
    for key in ((W, T, True, False), (W, T, False, False), (R, T, True, False), (R, T, False, False), (T, G, False, False),
                (T, G, False, True), (G, R, False, True), (G, T, True, True)):
        assert trans.get(key, 0) >= 1, key
    by = {(c["task"], c["name"]): (c, r) for c, r in results}
    c, r = by[("combined", "walk fall by low_z at the amnesty boundary")]
    assert c["idx"] == tc.AMNESTY and r["reason"] == 7 and r["done"]                      # !(150 > 150): no amnesty yet
    c, r = by[("combined", "walk fall by low_z with amnesty")]
    assert c["idx"] == tc.AMNESTY + 1 and r["reason"] == 0 and not r["done"] and r["motion"] == T
    bnd = [(c, r) for c, r in results if c["boundary"]]
    assert len(bnd) >= 12
    for c, r in bnd:
        assert not r["done"] and r["reason"] in (0, 2) and (c["task"] == "dpenv" or r["motion"] == c["motion"]), (c["task"], c["name"])
    # precedence: 3 over 1, 4 over 3, 3 over 7, 6 over everything, each from a state in which the lower rule fires as well
    for task, name, lower in (("dpenv", "cap over low_z", "low_z"),
                              ("dpenv", "obs bound over low_z", "low_z"), ("dpenv", "obs bound over cap and acyclic end", "acyclic end over cap"),
                              ("combined", "cap over a fall without amnesty", "walk fall by low_z, no amnesty"),
                              ("combined", "obs bound over a fall and the cap", "cap over a fall without amnesty")):
        (c, r), (cl, rl) = by[(task, name)], by[(task, lower)]
        assert r["done"] and rl["done"] and r["reason"] != rl["reason"], (task, name)
        assert abs(r["zc"] - rl["zc"]) < 1e-9 and (c["idx"], c["slot"], c["motion"]) == (cl["idx"], cl["slot"], cl["motion"]), (task, name)
        assert c["ep_len"] >= cl["ep_len"]
    c, r = by[("dpenv", "acyclic end over cap")]          # the cap fires on any state: the counter alone decides
    assert c["ep_len"] == tc.CAP_DPENV and r["reason"] == 4 and by[("dpenv", "cap")][1]["reason"] == 3


def test_rsi_draw_ranges():
    """DPCombinedEnv.reset(rsi=True): getup anywhere in its clip, walk AMNESTY_STEPS + 10 steps in; both motions are drawn."""
    L = [tc.length(m) for m, _ in tc.COMBINED_CLIPS]
    draws = [tc.rsi_draw("combined", 20, i, 0, L) for i in range(64)]
    assert {m for m, _ in draws} == {tc.M_WALK, tc.M_GETUP}
    assert all((160 <= i < 160 + L[0]) if m == tc.M_WALK else (0 <= i < L[2]) for m, i in draws)
    assert all(m == 0 and 0 <= i < L[0] for m, i in (tc.rsi_draw("dpenv", 20, i, 3, L) for i in range(64)))
    assert len({tc.rsi_draw("dpenv", 20, 5, k, L) for k in range(8)}) > 4          # the reset count moves the draw


@pytest.mark.parametrize("task", ["dpenv", "combined"])
def test_oracle_autoreset_rollout_ends_enough_episodes(task):
    dones, reasons = tc.oracle_autoreset_rollout(task)
    print(task, "oracle alone: dones", dones, "reasons", reasons)
    assert dones >= tc.AUTORESET["min_dones"] and len(reasons) >= 2
    assert 3 in reasons and (7 if task == "combined" else 1) in reasons
