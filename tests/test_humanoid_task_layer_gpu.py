"""The task layer of the humanoid3d engine (csrc/dm_kernels.hip: what step_body<TASK> does after the physics, and the in-kernel
auto-reset) against the fp64 oracle on every exit path, for task="dpenv" and task="combined", on the two-wave kernels (w2: an
engine of exactly the cases) and on the three-wave kernels (w3: the cases tiled to >= 3072 envs, dm_abi.hip: launch()).  Every
tile of w3 must hold the bits of tile 0; tile 0 is compared with the oracle.  The cases come from tests/humanoid_task_cases.py;
tests/test_humanoid_task_cases_cpu.py proves on the oracle alone that they reach what they name and that every quantity a rule
tests is at least 1e-3 from its threshold, so no case is left out here: integers are compared exactly.

Floating-point gates: ten times the worst error measured on an MI355X (the reward terms are expf of sums whose FMA contraction
may change with a reschedule), and never above what the humanoid's older oracle comparisons hold (tests/test_combined_env.py:
obs 2e-3, reward 1e-4, terms 2e-4, qpos 1e-4; tests/test_gpu_configs.py: TOL_OBS 2e-3, TOL_REW 1e-4).  The measured values are
at GATE / ROLLOUT_GATE and in the docstrings of the tests.  Reset observations are copies of a table row evaluated once: 1e-5.
"""
import numpy as np
import pytest

import humanoid_task_cases as tc

pytestmark = pytest.mark.gpu

CEILING = dict(obs=2e-3, rew=1e-4, terms=2e-4, stepped_qpos=1e-4, terminal_obs=2e-3)
# Ten times the worst measured on an MI355X (w2 and w3 gave the same figures), rounded up to two digits; all are far below CEILING.
# GATE: the single-step cases, through step / step_forced and through step_active.  Measured: DPEnv obs 8.66e-8, reward 1.79e-7,
# terms 3.68e-7, position after a stepped case 7.86e-8; combined obs 1.11e-7, reward 3.58e-7, terms 8.49e-7, position 8.48e-8.
GATE = dict(dpenv=dict(obs=8.7e-7, rew=1.8e-6, terms=3.7e-6, stepped_qpos=7.9e-7),
            combined=dict(obs=1.2e-6, rew=3.6e-6, terms=8.5e-6, stepped_qpos=8.5e-7))
# ROLLOUT_GATE: the 40-step teacher-forced auto-reset rollout, whose states are less tame than clip frames.  Measured: DPEnv obs
# 1.60e-6, terminal obs 6.15e-7, reward 2.38e-7; combined obs 6.52e-6, terminal obs 9.79e-7, reward 4.77e-7.
ROLLOUT_GATE = dict(dpenv=dict(obs=1.7e-5, terminal_obs=6.2e-6, rew=2.4e-6),
                    combined=dict(obs=6.6e-5, terminal_obs=9.8e-6, rew=4.8e-6))
RESET_OBS_TOL = 1e-5
VARIANTS = ("w2", "w3")
_REF = {}


def _reference(task):
    """The oracle's result of every single-step case of a task, computed once for both kernel variants and both tests."""
    if task not in _REF:
        cases = [c for c in tc.all_cases() if c["task"] == task]
        _REF[task] = (cases, [tc.run_on_oracle(c) for c in cases])
    return _REF[task]


class _Engine:
    """One engine of n envs (two-wave kernels) or of n envs tiled to >= 3072 (three-wave); arrays go in tiled, come out as
    [tile, n, ...]."""

    def __init__(self, model, task, variant, n, auto_reset=False, seed=0):
        import torch
        from deepmimic_mujoco_amd import _lib
        self.torch, self.n, self.comb = torch, n, task == "combined"
        self.tile = 1 if variant == "w2" else -(-3072 // n)
        assert (n * self.tile >= 3072) == (variant == "w3")
        self.eng = eng = _lib.HipEngine(model, n * self.tile, task=_lib.TASK_COMBINED if self.comb else _lib.TASK_DPENV,
                                        auto_reset=auto_reset, seed=seed, max_ep_length=tc.CAP_COMBINED if self.comb else tc.CAP_DPENV)
        for slot, (m, fl) in enumerate(tc.COMBINED_CLIPS if self.comb else tc.DPENV_SLOTS):
            eng.load_clip(slot, tc.mocap(m), **fl)
        self.out = eng.alloc_outputs()

    def dev(self, a, dtype):
        a = np.asarray(a, dtype)
        return self.torch.tensor(np.tile(a, (self.tile,) + (1,) * (a.ndim - 1)), device=self.eng.device).contiguous()

    def i32(self, a):
        return self.dev(a, np.int32)

    def f32(self, a):
        return self.dev(a, np.float32)

    def ids(self, a):
        """Env ids of tile 0 -> the same envs of every tile; -1 (skipped by the kernel) stays."""
        a = np.asarray(a, np.int32)
        return self.torch.tensor(np.concatenate([np.where(a < 0, a, a + k * self.n) for k in range(self.tile)]),
                                 dtype=self.torch.int32, device=self.eng.device)

    def read(self):
        eng = self.eng
        self.torch.cuda.synchronize()
        r = {k: self.out[k] for k in ("obs", "rew", "done", "terms", "reason", "terminal_obs")}
        r["idx"], r["ep_len"], _ = eng.get_counters()
        r["motion"] = eng.get_env_clips()
        r["qpos"], r["qvel"], r["warm"], r["ctrl"] = eng.get_state()
        return {k: x.cpu().numpy().reshape((self.tile, self.n) + tuple(x.shape[1:])) for k, x in r.items()}

    def close(self):
        self.eng.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _tiles_equal(r, rows, label):
    """Every tile holds tile 0's bits in the given rows (identical inputs, no hash draw)."""
    for k, x in r.items():
        b = _bits(x)
        for t in range(1, b.shape[0]):
            assert np.array_equal(b[0][rows], b[t][rows]), "%s: %s of tile %d differs from tile 0" % (label, k, t)


def _arm(E, cases):
    E.eng.set_env_clips(E.i32([c["motion"] if E.comb else c["slot"] for c in cases]))
    E.eng.set_counters(E.i32([c["idx"] for c in cases]), E.i32([c["ep_len"] for c in cases]))


def _rows(E, cases, kinds):
    benign = tc.frame("walk", 0)
    st = [(c["qpos"], c["qvel"]) if c["kind"] in kinds else benign for c in cases]
    return E.f32([s[0] for s in st]), E.f32([s[1] for s in st])


def _compare(task, cases, ref, got, qpos0, worst, bad, reasons):
    """One engine row per case against the oracle: integers exactly, floats into `worst` and against GATE[task]."""
    comb, gate = task == "combined", GATE[task]
    compared = 0
    for c, o, e in zip(cases, ref, got):
        if e is None:
            continue
        compared += 1
        ints = (bool(e["done"]), int(e["reason"]), int(e["idx"]), int(e["ep_len"]), int(e["motion"]))
        want = (bool(o["done"]), int(o["reason"]), int(o["idx"]), int(o["ep_len"]), int(o["motion"]))
        if ints != want:
            bad.append((c["name"], "done / reason / idx / episode length / motion", ints, want))
        reasons[int(e["reason"])] = reasons.get(int(e["reason"]), 0) + 1
        if c["zeroed"]:
            if e["obs"].any() or e["rew"] != 0 or e["terms"].any():
                bad.append((c["name"], "obs, reward and terms must be exact zeros"))
        else:
            nt = 7 if comb else 5
            err = dict(obs=np.abs(e["obs"] - o["obs"]).max(), rew=abs(e["rew"] - o["rew"]), terms=np.abs(e["terms"][:nt] - o["terms"][:nt]).max())
            for k, x in err.items():
                worst[k] = max(worst[k], float(x))
            if comb and (e["terms"][7] != int(e["terms"][7]) or int(e["terms"][7]) != int(o["terms"][7])):
                bad.append((c["name"], "terms[7]", e["terms"][7], o["terms"][7]))
            if not all(err[k] < gate[k] for k in err):
                bad.append((c["name"], "obs / reward / terms", err))
        if c["kind"] == "sim_error":
            if not (np.array_equal(e["qpos"], qpos0.astype(np.float32)) and not e["qvel"].any() and not e["warm"].any()):
                bad.append((c["name"], "the stored state must be qpos0, zero velocity, zero warm start"))
        elif c["kind"] == "stepped":
            x = float(np.abs(e["qpos"] - o["qpos"]).max())
            worst["stepped_qpos"] = max(worst["stepped_qpos"], x)
            if not x < gate["stepped_qpos"]:
                bad.append((c["name"], "position after the step", x))
        else:
            f = c["qpos"].astype(np.float32)          # (the root quaternion may be normalised in place)
            if not (np.array_equal(e["qpos"][:3], f[:3]) and np.array_equal(e["qpos"][7:], f[7:])):
                bad.append((c["name"], "a forced step stores the forced position"))
    return compared


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("task", ["dpenv", "combined"])
def test_single_step_cases_match_the_oracle(model, task, variant):
    """Every case of tests/humanoid_task_cases.py, each in its own env of one engine per task and variant: a reset, then the
    forced cases in one step_forced launch, then the stepped cases and the simulation error in one step launch (state stored with
    set_state(run_forward=False), zero warm start).  done, reason, the next idx_curr / n_steps, the episode length, the clip /
    motion id and terms[7] equal the oracle's as integers; obs, reward, terms and the position after a stepped case within
    GATE; reasons 5 and 6 return obs, reward and terms of exact zeros; after the simulation error the stored state is qpos0
    (bit-exact in fp32) with zero velocity and warm start, counters and motion untouched as in the oracle; a forced step stores
    the forced position.  No case is excluded: compared == number of cases.

    DPEnv: 28 cases, per reason {0: 2, 1: 2, 2: 14, 3: 3, 4: 3, 5: 1, 6: 3}.  Combined: 37 cases, per reason {0: 21, 3: 3, 5: 1,
    6: 2, 7: 10}; per transition walk -> to_getup 8 done + 3 with amnesty, run -> to_getup 2 + 1, to_getup -> getup 2 by success +
    2 by time-out, getup -> run 2, getup -> run -> to_getup (done, one step) 2.
    Measured on an MI355X, w2 and w3 alike, no case disagreed with the oracle.  DPEnv: obs 8.7e-8, reward 1.8e-7, terms 3.7e-7,
    position after a stepped case 7.9e-8.  Combined: obs 1.1e-7, reward 3.6e-7, terms 8.5e-7, position 8.5e-8.  The gates are
    ten times these (GATE)."""
    cases, ref = _reference(task)
    n = len(cases)
    E = _Engine(model, task, variant, n)
    eng = E.eng
    _arm(E, cases)
    eng.reset(E.out["obs"], idx_init=E.i32(np.zeros(n)))
    got = [None] * n
    _arm(E, cases)
    q, v = _rows(E, cases, ("forced",))
    eng.step_forced(q, v, E.out)
    r = E.read()
    _tiles_equal(r, slice(None), "step_forced")
    for i, c in enumerate(cases):
        if c["kind"] == "forced":
            got[i] = {k: x[0][i] for k, x in r.items()}
    _arm(E, cases)
    q, v = _rows(E, cases, ("stepped", "sim_error"))
    eng.set_state(q, v, warm=E.f32(np.zeros((n, tc.NV))), run_forward=False)
    eng.step(E.f32([c["action"] for c in cases]), E.out)
    r = E.read()
    _tiles_equal(r, slice(None), "step")
    for i, c in enumerate(cases):
        if c["kind"] != "forced":
            got[i] = {k: x[0][i] for k, x in r.items()}
    E.close()

    worst = dict(obs=0.0, rew=0.0, terms=0.0, stepped_qpos=0.0)
    bad, reasons = [], {}
    compared = _compare(task, cases, ref, got, np.asarray(model.qpos0, np.float64), worst, bad, reasons)
    print("humanoid task layer, %s, %s (%d tiles): %d cases compared, worst %s, gates %s, reasons %s" %
          (task, variant, E.tile, compared, worst, GATE[task], dict(sorted(reasons.items()))))
    for b in bad:
        print("   MISMATCH", b)
    assert compared == n and not bad, bad
    assert all(g[task][k] <= CEILING[k] for g in (GATE, ROLLOUT_GATE) for k in g[task])


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("task", ["dpenv", "combined"])
def test_step_active_takes_the_same_exits(model, task, variant):
    """The stepped cases and the simulation error again, on an engine created with auto_reset=True, through step_active: the
    slot list is the stepped envs shuffled, with a -1 in the middle and a -1 tail.  Listed envs: the same integers as the oracle
    and floats within the same gates; no reset happens (step_active forces auto-reset off), so the counters and the motion show
    the finished episode as the oracle's do.  Unlisted envs (the forced cases' rows) keep their poisoned output rows, their
    state, counters and clip id bit for bit.

    Measured on an MI355X, w2 and w3 alike: DPEnv 9 listed envs (reasons {0: 1, 1: 1, 2: 4, 3: 1, 4: 1, 5: 1}), 19 unlisted;
    combined 10 listed ({0: 6, 3: 1, 5: 1, 7: 2}), 27 unlisted; the errors are those of the step launch of the test above (DPEnv
    obs 8.7e-8, reward 1.2e-7, terms 3.7e-7, position 7.9e-8; combined obs 1.1e-7, reward 1.2e-7, terms 3.3e-7, position 8.5e-8)."""
    cases, ref = _reference(task)
    n = len(cases)
    E = _Engine(model, task, variant, n, auto_reset=True, seed=5)
    eng, torch = E.eng, E.torch
    eng.reset(E.out["obs"], idx_init=E.i32(np.zeros(n)))
    _arm(E, cases)
    q, v = _rows(E, cases, ("stepped", "sim_error"))
    eng.set_state(q, v, warm=E.f32(np.zeros((n, tc.NV))), run_forward=False)
    for k, x in E.out.items():
        x.fill_(77)
    before = E.read()
    listed = [i for i, c in enumerate(cases) if c["kind"] != "forced"]
    order = list(np.random.default_rng(11).permutation(listed))
    order = order[:len(order) // 2] + [-1] + order[len(order) // 2:] + [-1]
    ids = E.ids(order)
    assert len(ids) <= n * E.tile
    eng.step_active(E.f32([c["action"] for c in cases]), ids, len(ids), E.out)
    r = E.read()
    E.close()
    _tiles_equal(r, slice(None), "step_active")
    unlisted = np.array([i for i in range(n) if i not in listed])
    assert len(unlisted) > 0
    for k in r:
        if k == "terminal_obs":          # step_active has no terminal observation: untouched everywhere
            assert np.array_equal(_bits(r[k]), _bits(before[k])), k
        else:
            assert np.array_equal(_bits(r[k])[:, unlisted], _bits(before[k])[:, unlisted]), "unlisted envs: %s changed" % k
    got = [{k: x[0][i] for k, x in r.items()} if i in listed else None for i in range(n)]
    worst = dict(obs=0.0, rew=0.0, terms=0.0, stepped_qpos=0.0)
    bad, reasons = [], {}
    compared = _compare(task, cases, ref, got, np.asarray(model.qpos0, np.float64), worst, bad, reasons)
    print("humanoid step_active, %s, %s: %d listed envs compared, %d unlisted untouched, worst %s, reasons %s" %
          (task, variant, compared, len(unlisted), worst, dict(sorted(reasons.items()))))
    for b in bad:
        print("   MISMATCH", b)
    assert compared == len(listed) and not bad, bad


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("task", ["dpenv", "combined"])
def test_autoreset_matches_the_hash_and_the_oracle(model, task, variant):
    """auto_reset=True, seed 20, 32 envs (w3: tile 0 of 3072), 40 steps of small seeded actions from reset() without idx_init.
    The first reset is the RSI draw with reset count 0; then some counters are set (tests/humanoid_task_cases.py::
    autoreset_counters0: every fourth env close to the cap; under the combined task every other fourth env that drew walk below
    the amnesty).  Before every step the oracle takes the engine's state, warm start and counters and both step: done and reason
    are equal on every env-step.  At every done: terminal_obs is the oracle's observation of the pre-reset state; idx_curr /
    n_steps and the motion are the draw recomputed on the host (kernel_helpers.hash32 of seed, env, reset count k for the k-th
    reset) with the keys 0x5EED / 0x5EEE and, for walk, the amnesty + 10 offset; the episode length is 0; the returned obs is the
    oracle's reset observation at that draw (1e-5) and differs from terminal_obs.  Envs that go on are compared as well (obs,
    reward, counters).  At least as many dones as tests/test_humanoid_task_cases_cpu.py holds the oracle alone to (10).  Last, a
    simulation error under auto-reset: a NaN stored into env 0's position, one step: done, reason 5, zeros in reward, terms and
    terminal_obs, and the env reset to its next draw.

    Measured on an MI355X, w2 and w3 alike.  DPEnv: 37 dones (32 low_z, 5 max_ep_len), up to 3 resets per env; reset obs 5.8e-8,
    terminal obs 6.1e-7, obs 1.6e-6, reward 2.4e-7; smallest |terminal_obs - obs| 1.0.  Combined: 13 dones (8 max_ep_len, 5
    fallen without amnesty), up to 3 resets per env; reset obs 1.1e-6, terminal obs 9.8e-7, obs 6.5e-6, reward 4.8e-7; smallest
    |terminal_obs - obs| 0.69.  The gates are ten times these (ROLLOUT_GATE); the reset observation keeps the 1e-5 of the older
    reset tests."""
    A = tc.AUTORESET
    n, seed, comb = A["envs"], A["seed"], task == "combined"
    gate = ROLLOUT_GATE[task]
    E = _Engine(model, task, variant, n, auto_reset=True, seed=seed)
    eng = E.eng
    oclips = tc.oracle_clips(task)
    lengths = [c.L for c in oclips]
    eng.reset(E.out["obs"])
    r = {k: x[0] for k, x in E.read().items()}
    sims = [tc.new_sim(task) for _ in range(n)]
    worst = dict(reset_obs=0.0, terminal_obs=0.0, obs=0.0, rew=0.0)
    bad = []

    def check_reset(i, rcnt, r):
        motion, ix = tc.rsi_draw(task, seed, i, rcnt, lengths)
        if (int(r["idx"][i]), int(r["ep_len"][i]), int(r["motion"][i])) != (ix, 0, motion):
            bad.append(("reset", i, rcnt, int(r["idx"][i]), int(r["ep_len"][i]), int(r["motion"][i]), "drawn", motion, ix))
        o = sims[i].comb_reset(motion, ix) if comb else sims[i].env_reset(oclips[0], ix)
        worst["reset_obs"] = max(worst["reset_obs"], float(np.abs(r["obs"][i] - o).max()))
    for i in range(n):
        check_reset(i, 0, r)
    idx0, ep0 = tc.autoreset_counters0(task, [tc.rsi_draw(task, seed, i, 0, lengths) for i in range(n)])
    eng.set_counters(E.i32(idx0), E.i32(ep0))
    acts = tc.autoreset_actions()
    rcnt = np.ones(n, int)
    dones, reasons, min_gap = 0, {}, np.inf
    r = {k: x[0] for k, x in E.read().items()}
    for t in range(A["steps"]):
        b = r
        eng.step(E.f32(acts[t]), E.out)
        r = {k: x[0] for k, x in E.read().items()}
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
            worst["rew"] = max(worst["rew"], float(abs(r["rew"][i] - rew)))
            if d:
                dones += 1
                reasons[rs] = reasons.get(rs, 0) + 1
                worst["terminal_obs"] = max(worst["terminal_obs"], float(np.abs(r["terminal_obs"][i] - o).max()))
                min_gap = min(min_gap, float(np.abs(r["terminal_obs"][i] - r["obs"][i]).max()))
                check_reset(i, int(rcnt[i]), r)
                rcnt[i] += 1
            else:
                worst["obs"] = max(worst["obs"], float(np.abs(r["obs"][i] - o).max()))
                after = (env.n_steps, env.episode_length, env.motion) if comb else (env.idx_curr, env.episode_length, 0)
                if (int(r["idx"][i]), int(r["ep_len"][i]), int(r["motion"][i])) != after:
                    bad.append(("counters", t, i, int(r["idx"][i]), int(r["ep_len"][i]), int(r["motion"][i]), after))
    # a simulation error under auto-reset (src/deepmimic_env.py:366-378 inside a SubprocVecEnv worker): env 0's stored position gets
    # a NaN, the others keep their state; the step reports done / reason 5 with zeros and resets env 0 like after any other done
    full = E.read()
    q = full["qpos"].copy()
    q[:, 0, 10] = np.nan
    flat = lambda x: E.torch.tensor(x.reshape((-1,) + x.shape[2:]), device=eng.device).contiguous()
    eng.set_state(flat(q), flat(full["qvel"]), warm=flat(full["warm"]), ctrl=flat(full["ctrl"]), run_forward=False)
    eng.step(E.f32(np.zeros((n, tc.NACT))), E.out)
    r = {k: x[0] for k, x in E.read().items()}
    if not (r["done"][0] == 1 and r["reason"][0] == 5 and r["rew"][0] == 0 and not r["terminal_obs"][0].any() and not r["terms"][0].any()):
        bad.append(("simulation error under auto-reset", int(r["done"][0]), int(r["reason"][0]), float(r["rew"][0])))
    check_reset(0, int(rcnt[0]), r)
    if not np.isfinite(r["obs"]).all():
        bad.append(("a NaN reached an observation",))
    E.close()
    print("humanoid auto-reset, %s, %s: %d dones, reasons %s, resets per env up to %d, worst %s, smallest |terminal_obs - obs| %.3g" %
          (task, variant, dones, dict(sorted(reasons.items())), int(rcnt.max()), worst, min_gap))
    for x in bad:
        print("   MISMATCH", x)
    assert not bad, bad
    assert dones >= A["min_dones"] and len(reasons) >= 2
    assert worst["reset_obs"] < RESET_OBS_TOL and worst["terminal_obs"] < gate["terminal_obs"] and worst["obs"] < gate["obs"] and worst["rew"] < gate["rew"]
    assert min_gap > 1e-3, "terminal_obs must be the observation before the reset, not the one after it"
