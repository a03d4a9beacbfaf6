"""The cases of tests/g1_task_cases.py on the fp64 oracle alone (no GPU): every case reaches the reason, the done flag and the
counter changes it names, the set covers every reason and every motion transition of both tasks, the "just inside" cases are
alive, and the oracle's auto-reset rollout ends enough episodes.  This is what keeps tests/test_g1_task_layer_gpu.py from passing
on cases that never reach their branch."""
import numpy as np
import pytest

import g1_task_cases as tc


@pytest.fixture(scope="module")
def results():
    cases = tc.all_cases()
    return [(c, tc.run_on_oracle(c)) for c in cases]


def test_cases_are_named_once_and_fp32_exact():
    cases = tc.all_cases()
    names = [(c["task"], c["name"]) for c in cases]
    assert len(set(names)) == len(names)
    for task in ("dpenv", "combined"):
        assert sum(c["task"] == task for c in cases) <= 32, "one engine of at most 32 envs per task"
    for c in cases:
        ok = np.isfinite(c["qpos"])
        assert np.array_equal(c["qpos"][ok], tc.f32(c["qpos"][ok])) and np.array_equal(c["qvel"], tc.f32(c["qvel"])), c["name"]
        assert (~ok).sum() == (1 if c["kind"] == "sim_error" else 0)


def test_every_case_reaches_what_it_names(results):
    for c, r in results:
        tag = (c["task"], c["name"])
        assert (r["reason"], r["done"]) == (c["reason"], c["done"]), (tag, r["reason"], r["done"])
        assert r["idx"] == c["next_idx"], (tag, r["idx"])
        # the counters advance on every path but the simulation error, which returns before them (:366-378)
        assert r["ep_len"] == c["ep_len"] + (0 if c["kind"] == "sim_error" else 1), (tag, r["ep_len"])
        if c["task"] == "combined":
            assert r["motion"] == c["next_motion"], (tag, r["motion"])
        if c["zeroed"]:
            assert not r["obs"].any() and r["rew"] == 0 and not r["terms"].any(), tag
        else:
            assert np.isfinite(r["obs"]).all() and r["obs"].any() and np.abs(r["obs"]).max() <= 100.0, tag
        if c["kind"] == "forced":
            # far from mj_checkAcc's 1e10, so that an fp32 evaluation cannot turn the case into a simulation error
            assert np.abs(r["qacc"]).max() < 1e8, (tag, np.abs(r["qacc"]).max())
        if c["on_frame"] is not None:
            # the reward was taken against this frame: forced onto it, the imitation terms are 1, up to what a root quaternion
            # stored off unit length costs the pose term (1e-4 on the walk clip, see the playback test below); one frame off
            # costs more than 1e-3 (test_reward_frames_are_told_apart)
            assert np.abs(r["terms"][:4] - 1).max() < 2e-4, (tag, r["terms"])
        if c["phase"] is not None:
            assert abs(r["obs"][90] - c["phase"]) < 1e-12, tag


def test_reward_frames_are_told_apart(results):
    """The cases that pin the reward frame would notice a neighbouring frame: the same state scored one frame off is not 1."""
    by = {(c["task"], c["name"]): c for c, _ in results}
    for key, other in ((("dpenv", "cyclic wrap"), 0), (("combined", "walk past one clip"), 36)):
        c = dict(by[key])
        c["idx"] = other
        r = tc.run_on_oracle(c)
        assert np.abs(r["terms"][:4] - 1).max() > 1e-3, (key, r["terms"])


def test_sim_error_resets_the_state(results):
    from oracle import oracle_g1 as og
    g, _ = og.g1_model()
    seen = 0
    for c, r in results:
        if c["kind"] == "sim_error":
            seen += 1
            assert np.array_equal(r["qpos"], g.qpos0) and not r["qvel"].any() and not r["warm"].any(), c["task"]
    assert seen == 2


def test_quotas(results):
    """Every reason a task has, every transition of the combined state machine, and the boundaries on their alive side."""
    for task, reasons in (("dpenv", (0, 1, 2, 3, 4, 5, 6, 8)), ("combined", (0, 3, 5, 6, 7))):
        for kind in ("any", "stepped"):
            got = {r["reason"] for c, r in results if c["task"] == task and (kind == "any" or c["kind"] != "forced")}
            want = set(reasons) - ({6} if kind == "stepped" else set())      # the obs bound has forced cases only
            print(task, kind, "reasons reached", sorted(got))
            assert want <= got, (task, kind, sorted(want - got))
    assert not any(r["reason"] in (4, 8) for c, r in results if c["task"] == "combined")
    assert not any(r["reason"] == 7 for c, r in results if c["task"] == "dpenv")
    trans = {}
    for c, r in results:
        if c["task"] == "combined" and r["motion"] != c["motion"]:
            by_timeout = (c["motion"] == tc.M_TO_GETUP and c["idx"] >= tc.TO_GETUP_LEN - 1 or
                          c["motion"] == tc.M_GETUP and c["idx"] >= tc.oracle_clips("combined")[tc.M_GETUP].L - 1)
            key = (c["motion"], r["motion"], bool(r["done"]), by_timeout)
            trans[key] = trans.get(key, 0) + 1
    print("combined transitions (from, to, done, out of time):", trans)
    W, R, G, T = tc.M_WALK, tc.M_RUN, tc.M_GETUP, tc.M_TO_GETUP
    for key in ((W, T, True, False), (W, T, False, False), (R, T, True, False), (R, T, False, False), (T, G, False, False),
                (T, G, False, True), (G, R, False, True), (G, T, True, True)):
        assert trans.get(key, 0) >= 1, key
    bnd = [(c, r) for c, r in results if c["boundary"]]
    assert len(bnd) >= 10
    for c, r in bnd:
        assert not r["done"] and r["reason"] in (0, 2) and (c["task"] == "dpenv" or r["motion"] == c["motion"]), (c["task"], c["name"])
    # precedence: 3 over 1, 4 over 3, 8 over 1, 6 over everything, each from a state in which the lower rule fires as well
    names = {c["name"] for c, _ in results}
    assert {"cap over low_z", "acyclic end over cap", "run rule over low_z", "obs bound over low_z",
            "obs bound over cap and acyclic end", "cap over a fall without amnesty", "obs bound over a fall and the cap"} <= names


def test_rsi_draw_ranges():
    """DPCombinedEnv.reset(rsi=True): getup anywhere in its clip, walk AMNESTY_STEPS + 10 steps in; both motions are drawn."""
    L = [76, 48, 353]
    draws = [tc.rsi_draw("combined", 20, i, 0, L) for i in range(64)]
    assert {m for m, _ in draws} == {tc.M_WALK, tc.M_GETUP}
    assert all((160 <= i < 160 + 76) if m == tc.M_WALK else (0 <= i < 353) for m, i in draws)
    assert all(m == 0 and 0 <= i < 76 for m, i in (tc.rsi_draw("dpenv", 20, i, 3, L) for i in range(64)))


@pytest.mark.parametrize("task", ["dpenv", "combined"])
def test_oracle_autoreset_rollout_ends_enough_episodes(task):
    dones, reasons = tc.oracle_autoreset_rollout(task)
    print(task, "oracle alone: dones", dones, "reasons", reasons)
    assert dones >= 8
    assert (3 if task == "combined" else 1) in reasons


def test_every_clip_scores_one_on_its_own_frames():
    """The oracle's own numbers for the playback test: forced along each clip, the velocity, end-effector and centre-of-mass terms
    are 1 within 1e-5 on every frame.  The pose term is 1 within 1e-5 only where the clip stores unit root quaternions
    (getup_facedown): MuJoCo normalises the quaternion of the state it is given while the target's pitch is taken from the stored
    one (py3dtf's to_rpy does not normalise), so a clip whose root quaternion is off unit length scores its own frame below 1:
    by 1e-4 on walk, 8e-4 on run and 0.10 on the three slow getup clips (norm off by 1.7 %).  The acyclic clips end with reason 4
    on their last frame and nowhere else."""
    from oracle import oracle_g1 as og
    for m in tc.G1_CLIPS:
        fl = tc.clip_flags(m)
        clip = tc.oracle_clip(m, **fl)
        s = og.G1Sim()
        s.set_caps(48, 256)
        worst, norm_err = np.zeros(4), 0.0
        for i in tc.playback_frames(m):
            s.env.idx_curr, s.env.episode_length = i, 0
            obs, rew, done, terms, reason = s.env_step(clip, np.zeros(tc.NACT), force_state=tc.frame(m, i))
            worst = np.maximum(worst, np.abs(terms[:4] - 1))
            norm_err = max(norm_err, abs(np.linalg.norm(tc.mocap(m).get_qpos(i)[3:7]) - 1))
            assert (reason == 4) == (fl["acyclic"] and i == clip.L - 1), (m, i, reason)
            assert s.env.idx_curr == (i + 1) % clip.L
        print("%-28s L %3d frames %3d worst |terms - 1| %s root quaternion norm off by %.1e" %
              (m, clip.L, len(tc.playback_frames(m)), ["%.1e" % x for x in worst], norm_err))
        assert worst[1:].max() < 1e-5, (m, worst)
        assert worst[0] < 1e-5 or norm_err > 1e-6, (m, worst)
