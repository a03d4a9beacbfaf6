"""Everything a launch of the Unitree G1 engine leaves behind, bit for bit against a recording, on every exit path of its task
layer (csrc/dm_g1_task.h: step_enter, rk_advance, task_and_finish, the in-kernel auto-reset) and through both pipelines.  The
other G1 suites compare with the fp64 oracle inside tolerances, which a refactor could move within unnoticed; this one holds the
arithmetic itself, down to which products the compiler contracts into FMAs, and the order of effects.

tests/golden/g1_step_bits.npz was recorded on an MI355X by tests/golden/make_g1_step_bits.py from the library of the commit the
file names ("commit"), before dm_g1.hip was cut into layers.  The inputs are those of tests/test_g1_task_layer_gpu.py:

  cases     the 30 DPEnv and 30 DPCombinedEnv cases of tests/g1_task_cases.py, one env per case: one step_forced launch
            ("forced"), then one step launch after set_state(run_forward=False) ("stepped").  Recorded in full: obs, rew, done,
            terms, reason, terminal_obs, the stored qpos / qvel / warm start, idx, episode length and reward, motion, and the whole
            DMG1_DEBUG_STRIDE debug row of every env (body positions, qacc_smooth, qacc, counts, contacts, constraint forces, the
            per-stage counts and contact hashes: the physics).
  rollout   the AUTORESET rollout of that module (32 envs, 40 steps, auto-reset on), the first reset and the closing step with a
            NaN in env 0 included.  rew, done, reason, the counters and the motion are recorded in full for every launch, the
            wide arrays (obs, terms, terminal_obs, state, debug rows) as one SHA-256 per launch and array: the file stays small.

The pipelines are bit-identical (tests/test_g1_gpu.py), so the file holds ONE copy and both pipelines are compared with it.  One
thing is left out of the comparison: the debug row of an env that reports a simulation error (reason 5).  mj_checkPos fails
before any evaluation runs on such an env, so the row is copied from LDS arrays that nothing wrote in that launch.  The envs, the
shapes and the steps are the smallest that reach every exit (tests/test_g1_task_cases_cpu.py proves that on the oracle)."""
import hashlib
import os

import numpy as np
import pytest

import g1_task_cases as tc

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g1_step_bits.npz")
TASKS = ("dpenv", "combined")
OUTPUTS = ("obs", "rew", "done", "terms", "reason", "terminal_obs")
FULL = ("rew", "done", "reason", "idx", "ep_len", "ep_rew", "motion")      # the rollout's arrays that are stored as they are
SIM_ERROR = 5


def _bits(a):
    a = np.ascontiguousarray(a)
    a = a.view(np.int32) if a.dtype == np.float32 else a.astype(np.int32)
    return a.reshape(a.shape[0], -1)


def _snap(eng, out, dbg):
    """field -> int32 [envs, k] of everything the last launch left (fp32 as bit patterns)."""
    import torch
    torch.cuda.synchronize()
    r = {k: out[k] for k in OUTPUTS}
    r["idx"], r["ep_len"], r["ep_rew"] = eng.get_counters()
    r["motion"] = eng.get_motion()
    r["qpos"], r["qvel"], r["warm"] = eng.get_state()
    r["debug"] = dbg
    r = {k: _bits(x.cpu().numpy()) for k, x in r.items()}
    r["debug"][r["reason"][:, 0] == SIM_ERROR] = 0          # see the module's docstring
    return r


def _engine(task, pipeline, n, clips, **kw):
    from deepmimic_mujoco_amd.g1 import G1HipEngine, TASK_COMBINED, TASK_DPENV
    comb = task == "combined"
    eng = G1HipEngine(n, pipeline=pipeline, task=TASK_COMBINED if comb else TASK_DPENV,
                      max_ep_length=tc.CAP_COMBINED if comb else tc.CAP_DPENV, **kw)
    for slot, (m, fl) in enumerate(clips):
        eng.load_clip(tc.mocap(m), clip_id=slot, **fl)
    return eng, eng.alloc_outputs(), eng.enable_debug()


def _cases(task, pipeline, sink):
    """The flow of tests/test_g1_task_layer_gpu.py::test_g1_single_step_cases_match_the_oracle."""
    import torch
    cases = [c for c in tc.all_cases() if c["task"] == task]
    comb, n = task == "combined", len(cases)
    eng, out, dbg = _engine(task, pipeline, n, [(m, {}) for m in tc.COMBINED_CLIPS] if comb else list(tc.DPENV_SLOTS),
                            auto_reset=False, seed=0)
    dev = lambda a, dt: torch.tensor(np.asarray(a, dt), device=eng.device).contiguous()
    where = dev([c["motion"] if comb else c["slot"] for c in cases], np.int32)
    idx, ep = dev([c["idx"] for c in cases], np.int32), dev([c["ep_len"] for c in cases], np.int32)

    def arm():
        eng.set_motion(where) if comb else eng.set_env_clips(where)
        eng.set_counters(idx, ep)
    benign = tc.frame("walk", 0)

    def rows(kinds):
        st = [(c["qpos"], c["qvel"]) if c["kind"] in kinds else benign for c in cases]
        return dev([s[0] for s in st], np.float32), dev([s[1] for s in st], np.float32)
    arm()
    eng.reset(out["obs"], idx_init=dev(np.zeros(n), np.int32))
    arm()
    q, v = rows(("forced",))
    eng.step_forced(q, v, out)
    sink.update({"cases/%s/forced/%s" % (task, k): a for k, a in _snap(eng, out, dbg).items()})
    arm()
    q, v = rows(("stepped", "sim_error"))
    eng.set_state(q, v, warm=dev(np.zeros((n, 43)), np.float32), run_forward=False)
    eng.step(dev([c["action"] for c in cases], np.float32), out)
    sink.update({"cases/%s/stepped/%s" % (task, k): a for k, a in _snap(eng, out, dbg).items()})
    eng.close()


def _rollout(task, pipeline, sink):
    """The flow of tests/test_g1_task_layer_gpu.py::test_g1_autoreset_matches_the_hash_and_the_oracle, the oracle left out."""
    import torch
    A, comb = tc.AUTORESET, task == "combined"
    names = tc.COMBINED_CLIPS if comb else ("walk",)
    eng, out, dbg = _engine(task, pipeline, A["envs"], [(m, tc.clip_flags(m) if not comb else {}) for m in names],
                            auto_reset=True, seed=A["seed"])
    dev = lambda a, dt: torch.tensor(np.asarray(a, dt), device=eng.device).contiguous()
    full = {k: [] for k in FULL}
    sha = {}

    def keep():
        for k, a in _snap(eng, out, dbg).items():
            if k in FULL:
                full[k].append(a[:, 0])
            else:
                sha.setdefault(k, []).append(np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8))
    eng.reset(out["obs"])
    keep()
    eng.set_counters(None, dev(tc.autoreset_ep_len0(task), np.int32))
    acts = tc.autoreset_actions()
    for t in range(A["steps"]):
        eng.step(dev(acts[t], np.float32), out)
        keep()
    q, v, w = [x.cpu().numpy() for x in eng.get_state()]
    q[0, 10] = np.nan                       # a simulation error under auto-reset
    eng.set_state(dev(q, np.float32), dev(v, np.float32), warm=dev(w, np.float32), run_forward=False)
    eng.step(dev(np.zeros((A["envs"], tc.NACT)), np.float32), out)
    keep()
    eng.close()
    sink.update({"rollout/%s/%s" % (task, k): np.stack(x) for k, x in full.items()})            # int32 [launches, envs]
    sink.update({"rollout/%s/sha256/%s" % (task, k): np.stack(x) for k, x in sha.items()})      # uint8 [launches, 32]


def compute(pipeline):
    """What the fixture holds, from the library under test on one pipeline (1 monolithic, 2 split): name -> array."""
    sink = {}
    for task in TASKS:
        _cases(task, pipeline, sink)
        _rollout(task, pipeline, sink)
    return sink


def differing(got, want):
    """Names of the arrays that are not equal (shape included), each with the rows that differ."""
    keys = sorted(set(got) | set(want))
    bad = []
    for k in keys:
        if k not in got or k not in want or got[k].shape != want[k].shape:
            bad.append("%s (missing or another shape)" % k)
        elif not np.array_equal(got[k], want[k]):
            rows = np.nonzero((got[k] != want[k]).reshape(len(got[k]), -1).any(axis=1))[0].tolist()
            cols = np.nonzero((got[k] != want[k]).reshape(len(got[k]), -1).any(axis=0))[0].tolist()
            bad.append("%s (rows %s, columns %s)" % (k, rows[:16], cols[:16]))
    return bad


@pytest.fixture(scope="module")
def golden():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files if k != "commit"}


def test_fixture_takes_every_exit(golden):
    """The recording holds what the cases are there for: every reason code the two tasks can report, with done set; the
    combined task's four transitions; dones of the rollout with the env reset in the same launch (episode length 0); and a
    debug row with contacts and constraint rows in it for every env that ran an evaluation."""
    g = golden
    for task, reasons in (("dpenv", {0, 1, 2, 3, 4, 5, 6, 8}), ("combined", {0, 3, 5, 6, 7})):
        seen = set()
        for launch in ("forced", "stepped"):
            p = "cases/%s/%s/" % (task, launch)
            seen |= set(g[p + "reason"][:, 0].tolist())
            ran = g[p + "reason"][:, 0] != SIM_ERROR
            assert g[p + "debug"].shape == (30, 1024)
            assert (g[p + "debug"][ran, 204] != 0).all() and (g[p + "debug"][ran, 203] != 0).sum() >= 15      # nefc, ncon
            assert (g[p + "debug"][~ran] == 0).all()
        assert seen == reasons, (task, seen)
        done, ep_len = g["rollout/%s/done" % task], g["rollout/%s/ep_len" % task]
        assert done.shape == (tc.AUTORESET["steps"] + 2, tc.AUTORESET["envs"])
        assert done.sum() >= 8 and (ep_len[done != 0] == 0).all()
        assert done[-1, 0] == 1 and g["rollout/%s/reason" % task][-1, 0] == SIM_ERROR
    before = np.array([c["motion"] for c in tc.combined_cases()])
    after = np.concatenate([g["cases/combined/%s/motion" % launch][:, 0] for launch in ("forced", "stepped")])
    moves = set(zip(np.tile(before, 2).tolist(), after.tolist()))
    assert {(tc.M_WALK, tc.M_TO_GETUP), (tc.M_RUN, tc.M_TO_GETUP), (tc.M_TO_GETUP, tc.M_GETUP), (tc.M_GETUP, tc.M_RUN),
            (tc.M_GETUP, tc.M_TO_GETUP)} <= moves


@pytest.mark.parametrize("pipeline", [1, 2])
def test_g1_step_bits(golden, pipeline):
    """Every recorded array equals what this library leaves on this pipeline, bit for bit; no case and no field is left out."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    got = compute(pipeline)
    bad = differing(got, golden)
    assert not bad, "%d of %d arrays differ from the recording: %s" % (len(bad), len(golden), "; ".join(bad[:12]))
