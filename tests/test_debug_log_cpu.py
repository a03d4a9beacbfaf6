"""Episode debug log, the parts that need no GPU: the C ABI's names and refusals (include/deepmimic_trace.h), the reference-shaped
dict and file (deepmimic_mujoco_amd/debug_log.py against src/deepmimic_env.py:366-378, 457-476 of the reference, whose key names
are written out here), the CLI summary and scripts/debug_log_vs_oracle.py on a log made from an oracle rollout."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from deepmimic_mujoco_amd import _lib, debug_log

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DM_EINVAL = -22
NQ, NV, NA = 35, 34, 28
W = NQ + 2 * NV + NA + 5


def test_header_exports_and_library_agree():
    hdr = open(os.path.join(ROOT, "include", "deepmimic_trace.h")).read()
    declared = set(re.findall(r"\b(dm_trace[a-z_0-9]*)\s*\(", hdr))
    assert declared == set(_lib.TRACE_EXPORTS), declared ^ set(_lib.TRACE_EXPORTS)
    L = _lib.load_library()
    for name in declared:
        assert getattr(L, name).argtypes is not None, name
    assert not set(_lib.TRACE_EXPORTS) & set(_lib.EXPORTS)
    assert "dm_trace" not in open(os.path.join(ROOT, "include", "deepmimic_hip.h")).read()
    src = open(os.path.join(ROOT, "deepmimic_mujoco_amd", "csrc", "dm_trace.hip")).read()
    assert re.findall(r'#include\s+"([^"]+)"', src) == ["../../include/deepmimic_trace.h"]      # no engine header
    assert W == 136 and 44 + 2 * 43 + 23 + 5 == 158
    # the ctypes mirror has the header's fields, in its order
    body = re.search(r"typedef struct DmTraceBufs \{(.*?)\} DmTraceBufs;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip(" *") for decl in body.split(";") for f in re.sub(r"^\s*(const\s+)?\w+\s*\**\s", "", decl.strip()).split(",") if f.strip()]
    assert fields == [n for n, _ in _lib.DmTraceBufs._fields_]


FAKE = 0x1000      # stands for a device pointer: a refused call dereferences none


def _bufs(**kw):
    d = dict(N=8, K=4, C=2, nq=NQ, nv=NV, na=NA, W=W, device=0, ring=FAKE, head=FAKE, cap=FAKE, cap_meta=FAKE, cap_count=FAKE, trig=FAKE)
    d.update(kw)
    return _lib.DmTraceBufs(**d)


BAD_BUFS = [dict(N=0), dict(K=1), dict(C=0), dict(W=W + 1), dict(W=W - 5), dict(nq=NQ + 1), dict(ring=None), dict(head=None), dict(cap=None),
            dict(cap_meta=None), dict(cap_count=None), dict(trig=None)]


@pytest.mark.parametrize("bad", BAD_BUFS, ids=[str(b) for b in BAD_BUFS])
def test_a_bad_struct_is_refused_without_a_device(bad):
    L = _lib.load_library()
    b = _bufs(**bad)
    assert L.dm_trace_record(C.byref(b), FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None, 8, 0x60, None) == DM_EINVAL
    assert len(L.dm_trace_last_error()) > 0
    assert L.dm_trace_mark(C.byref(b), FAKE, FAKE, FAKE, None, 8, None) == DM_EINVAL
    assert len(L.dm_trace_last_error()) > 0


def test_bad_arguments_are_refused_without_a_device():
    L = _lib.load_library()
    b = _bufs()
    good = [FAKE] * 7
    assert L.dm_trace_record(None, *good, None, 8, 0x60, None) == DM_EINVAL
    assert L.dm_trace_mark(None, FAKE, FAKE, FAKE, None, 8, None) == DM_EINVAL
    for k in range(7):                                   # qpos, qvel, warm, actions, rew, done, reason
        args = list(good)
        args[k] = None
        assert L.dm_trace_record(C.byref(b), *args, None, 8, 0x60, None) == DM_EINVAL, k
        assert len(L.dm_trace_last_error()) > 0
    for k in range(3):
        args = [FAKE] * 3
        args[k] = None
        assert L.dm_trace_mark(C.byref(b), *args, None, 8, None) == DM_EINVAL, k
    for nslots in (0, -1, 9):
        assert L.dm_trace_record(C.byref(b), *good, FAKE, nslots, 0x60, None) == DM_EINVAL, nslots
        assert L.dm_trace_mark(C.byref(b), FAKE, FAKE, FAKE, FAKE, nslots, None) == DM_EINVAL, nslots
        assert b"nslots" in L.dm_trace_last_error()


def test_reason_names_go_through_the_table():
    from deepmimic_mujoco_amd import g1
    assert debug_log.reason_mask(("sim_error", "obs_out_of_bounds")) == (1 << 5) | (1 << 6)
    assert debug_log.reason_mask(("sim_error",)) == 1 << 5
    assert debug_log.reason_mask(("run roll/pitch limit",), g1.REASONS) == 1 << 8
    with pytest.raises(ValueError):
        debug_log.reason_mask(("no such reason",))


# ------------------------------------------------------------------------------------------ the reference's dict
def _ring(n, last_reason, marks=(0,), seed=0):
    """``n`` finite entries; those of ``marks`` are marks, the last is a done step with ``last_reason``."""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    ent = dict(qpos=f(n, NQ), qvel=f(n, NV), warm=f(n, NV), action=f(n, NA), reward=rng.random(n).astype(np.float32),
               done=np.zeros(n, np.int32), reason=np.zeros(n, np.int32), kind=np.zeros(n, np.int32), step=np.arange(n, dtype=np.int32) + 7,
               env=3)
    ent["qpos"][:, 3:7] = [1, 0, 0, 0]
    for m in marks:
        ent["kind"][m] = 1
        ent["action"][m], ent["reward"][m] = 0, 0
    ent["done"][-1], ent["reason"][-1] = int(last_reason != 0), last_reason
    return ent


REFERENCE_STEP_KEYS = ["action", "body_xpos", "qpos", "qvel", "reward"]          # src/deepmimic_env.py:458-463 without body_xvelp


def test_sim_error_yields_last_action_and_is_not_appended(model):
    ent = _ring(6, 5, marks=(0, 3))
    log = debug_log.to_episode_log(ent, "walk", "humanoid3d", model)
    steps = [1, 2, 4]                                    # entries 0 and 3 are marks, entry 5 raised
    for k in REFERENCE_STEP_KEYS:
        assert len(log[k]) == len(steps), k
    assert "body_xvelp" not in log
    assert log["last_action"] == ent["action"][5].astype(np.float64).tolist()
    assert log["action"] == ent["action"][steps].astype(np.float64).tolist()
    assert log["qpos"] == ent["qpos"][steps].astype(np.float64).tolist() and log["qvel"] == ent["qvel"][steps].astype(np.float64).tolist()
    assert log["reward"] == ent["reward"][steps].astype(np.float64).tolist()
    assert "DM_REASON_SIM_ERROR" in log["full_traceback"]
    assert log["motion"] == "walk" and log["robot"] == "humanoid3d"
    from deepmimic_mujoco_amd.model import forward_kinematics
    want = forward_kinematics(model, ent["qpos"][2].astype(np.float64))["xpos"]
    assert np.array_equal(np.asarray(log["body_xpos"][1]), want) and want.shape == (len(model.body_parent), 3)
    # marks only under "entries", with everything this build adds
    e = log["entries"]
    assert set(e) == {"qpos", "qvel", "warm", "action", "reward", "done", "reason", "kind", "step", "env"}
    assert e["kind"] == [1, 0, 0, 1, 0, 0] and e["step"] == list(range(7, 13)) and e["env"] == 3
    assert e["done"] == [0, 0, 0, 0, 0, 1] and e["reason"][-1] == 5 and e["warm"] == ent["warm"].astype(np.float64).tolist()
    assert set(log) == set(REFERENCE_STEP_KEYS) | {"last_action", "full_traceback", "motion", "robot", "entries"}


def test_obs_bounds_step_is_appended_with_the_reference_string(model):
    ent = _ring(5, 6)
    log = debug_log.to_episode_log(ent, "run", "humanoid3d", model)
    assert len(log["action"]) == 4 and log["action"][-1] == ent["action"][4].astype(np.float64).tolist()
    assert log["full_traceback"] == "Observation out of bounds (deepmimic_env step)"
    assert "last_action" not in log
    assert set(log) == set(REFERENCE_STEP_KEYS) | {"full_traceback", "motion", "robot", "entries"}


def test_a_running_episode_and_an_earlier_episode_in_the_ring(model):
    ent = _ring(6, 0, marks=())
    log = debug_log.to_episode_log(ent, "walk", "humanoid3d", None)
    assert len(log["qpos"]) == 6 and "full_traceback" not in log and "body_xpos" not in log
    ent["done"][2], ent["reason"][2] = 1, 1               # an auto-reset after entry 2: the last episode is entries 3..5
    log = debug_log.to_episode_log(ent, "walk", "humanoid3d", None)
    assert log["qpos"] == ent["qpos"][3:].astype(np.float64).tolist() and len(log["entries"]["kind"]) == 6


def test_the_g1_dict_uses_the_general_kinematics():
    from deepmimic_mujoco_amd import g1, mjcf
    gm = g1.load_g1_model()[0]
    rng = np.random.default_rng(1)
    n = 3
    ent = dict(qpos=np.tile(gm.qpos0.astype(np.float32), (n, 1)), qvel=np.zeros((n, 43), np.float32), warm=np.zeros((n, 43), np.float32),
               action=rng.standard_normal((n, 23)).astype(np.float32), reward=np.zeros(n, np.float32), done=np.array([0, 0, 1], np.int32),
               reason=np.array([0, 0, 6], np.int32), kind=np.array([1, 0, 0], np.int32), step=np.arange(n, dtype=np.int32), env=0)
    log = debug_log.to_episode_log(ent, "walk", "unitree_g1", gm)
    want = mjcf.forward_kinematics_general(gm, ent["qpos"][1].astype(np.float64))["xpos"]
    assert len(log["qpos"]) == 2 and len(log["qpos"][0]) == 44 and len(log["action"][0]) == 23
    assert np.array_equal(np.asarray(log["body_xpos"][0]), want) and want.shape == (39, 3)


def test_file_round_trip_and_name(tmp_path, model):
    log = debug_log.to_episode_log(_ring(6, 5, marks=(0, 3)), "walk", "humanoid3d", model)
    path = debug_log.write(str(tmp_path / "x.json"), log)
    assert debug_log.load(path) == log
    assert open(path).read().startswith("{\n    ")                              # json.dumps(indent=4), as the reference writes it
    assert re.fullmatch(r"/tmp/deepmimic_episode_\d{8}-\d{4}_\d{2}\.json", debug_log.default_path())
    assert re.fullmatch(r"/somewhere/deepmimic_episode_\d{8}-\d{4}_\d{2}_env2317\.json", debug_log.default_path("/somewhere", 2317))
    back = debug_log.entries_of(debug_log.load(path))
    ent = _ring(6, 5, marks=(0, 3))
    for k in debug_log.FIELDS:
        assert np.array_equal(back[k], ent[k]) and back[k].dtype == ent[k].dtype, k


def test_cli_summary(tmp_path, model, capsys):
    ent = _ring(5, 6)
    path = debug_log.write(str(tmp_path / "x.json"), debug_log.to_episode_log(ent, "run", "humanoid3d", model))
    assert debug_log.main([path]) == 0
    text = capsys.readouterr().out
    assert "robot   humanoid3d" in text and "motion  run" in text and "reason  obs_out_of_bounds" in text and "steps   4 " in text
    rows = re.findall(r"step +(\d+) +max\|qvel\| (\S+)", text)
    assert [int(r[0]) for r in rows] == [0, 1, 2, 3]
    assert np.allclose([float(r[1]) for r in rows], np.abs(ent["qvel"][1:]).max(1), rtol=1e-5)


def test_train_flags_and_surfaces_exist():
    from deepmimic_mujoco_amd import vec_env
    from deepmimic_mujoco_amd.train import build_parser
    a = build_parser().parse_args([])
    assert a.debug_log == "" and a.debug_log_steps == 64
    a = build_parser().parse_args(["--debug-log", "/x", "--debug-log-steps", "128"])
    assert a.debug_log == "/x" and a.debug_log_steps == 128
    assert _lib.EngineBase._recorder is None and vec_env.HipSingleEnv._debug_log is None          # off unless switched on
    assert callable(vec_env.HipBatchEnv.enable_debug_log) and callable(vec_env.HipSingleEnv.enable_debug_log)


def test_the_package_does_not_import_the_oracle():
    src = open(os.path.join(ROOT, "deepmimic_mujoco_amd", "debug_log.py")).read()
    assert not re.search(r"^\s*(from|import)\s+oracle", src, re.M)


# ------------------------------------------------------------------------------------------ scripts/debug_log_vs_oracle.py
def test_oracle_script_on_a_log_made_from_an_oracle_rollout(tmp_path, model, clips, oracle_clips):
    """The log holds fp32 roundings of an fp64 oracle rollout (states, warm starts, actions), so one oracle step from a logged state
    lands on the next logged state up to that rounding carried through one step: far under the 1e-4 gate, which every step must
    hold; a log whose last state is moved by 1e-3 must be reported."""
    from oracle.oracle import OracleSim
    sim = OracleSim(model)
    sim.set_caps(32, 128)
    sim.env_reset(oracle_clips["walk"], 5)
    rng = np.random.default_rng(3)
    n = 7
    rows = [(sim.get("qpos"), sim.get("qvel"), sim.get("qacc_warmstart"), np.zeros(NA), 0.0, 0, 0, 1)]
    for _ in range(n - 1):
        act = rng.uniform(-0.5, 0.5, NA).astype(np.float32)
        obs, rew, done, terms, reason = sim.env_step(oracle_clips["walk"], act.astype(np.float64))
        rows.append((sim.get("qpos"), sim.get("qvel"), sim.get("qacc_warmstart"), act, rew, int(done), reason, 0))
    f32 = lambda k: np.asarray([r[k] for r in rows], np.float32)
    ent = dict(qpos=f32(0), qvel=f32(1), warm=f32(2), action=f32(3), reward=f32(4), done=np.asarray([r[5] for r in rows], np.int32),
               reason=np.asarray([r[6] for r in rows], np.int32), kind=np.asarray([r[7] for r in rows], np.int32),
               step=np.arange(n, dtype=np.int32), env=0)
    assert not ent["done"].any()
    path = debug_log.write(str(tmp_path / "oracle.json"), debug_log.to_episode_log(ent, "walk", "humanoid3d", model))
    script = os.path.join(ROOT, "scripts", "debug_log_vs_oracle.py")
    r = subprocess.run([sys.executable, script, path], capture_output=True, text=True, cwd=ROOT)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    got = [float(x) for x in re.findall(r"entry +\d+ +max\|dqpos\| (\S+)", r.stdout)]
    assert len(got) == n - 1 and max(got) <= 1e-4
    assert "first step above the gate: none" in r.stdout
    ent["qpos"][4, 8] += 1e-3
    bad = debug_log.write(str(tmp_path / "moved.json"), debug_log.to_episode_log(ent, "walk", "humanoid3d", model))
    r = subprocess.run([sys.executable, script, bad], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 1 and "first step above the gate: entry 4" in r.stdout
