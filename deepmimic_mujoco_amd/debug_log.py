"""Episode debug log — the reference's ``episode_debug_log`` (src/deepmimic_env.py:299, 457-463, 499) for batched envs.

``DPEnv.step()`` of the reference appends action, body_xpos, body_xvelp, qpos, qvel and reward after every step and writes the lot
to ``/tmp/deepmimic_episode_<time>.json`` when MuJoCo throws (:366-378) or an observation leaves +-100 (:465-476);
``src/check_debug_log.py`` reads such a file back.  Here the states live on the device, so the log does too:

* :class:`FlightRecorder` keeps, per env of one engine, a ring of the last K entries (csrc/dm_trace.hip, include/deepmimic_trace.h),
  written after every engine step from the engine's own ``get_state``, and freezes a copy of an env's ring at the step that ended
  with a chosen reason.  ``_lib.EngineBase`` calls it from ``step`` / ``step_active`` (``record``) and ``reset`` / ``set_state`` /
  ``step_forced`` (``mark``), so every route that steps an engine is logged.
* :func:`to_episode_log` turns a ring into the reference's dict, :func:`write` / :func:`load` are its file.
* ``python -m deepmimic_mujoco_amd.debug_log FILE`` is ``check_debug_log.py``'s counterpart: a summary, ``--frames DIR`` (replay
  through ``set_state`` + ``render``), ``--resimulate`` (one engine step from every logged state against the next logged state).
"""
from __future__ import annotations

import ctypes as C
import json
import os
import time

import numpy as np

from . import _lib

TAIL = 5                       # reward, done, reason, kind, step (DM_TRACE_TAIL)
KIND_STEP, KIND_MARK = 0, 1    # DM_TRACE_KIND_*
OBS_BOUNDS_TRACEBACK = "Observation out of bounds (deepmimic_env step)"           # src/deepmimic_env.py:466
SIM_ERROR_TRACEBACK = "DM_REASON_SIM_ERROR (5): the engine's step refused the state (src/deepmimic_env.py:366, MujocoException)"
FIELDS = ("qpos", "qvel", "warm", "action", "reward", "done", "reason", "kind", "step")


def _dims(engine):
    """(nq, nv, na, reason table) of an engine: the humanoid steps on 28 actuator values, the G1 on the policy's 23."""
    if engine.PREFIX == "dm_":
        from .model import NU
        return engine.NQ, engine.NV, NU, _lib.REASONS
    from . import g1
    return engine.NQ, engine.NV, g1.NACT, g1.REASONS


def reason_mask(names, table=_lib.REASONS):
    """Bit ``code`` for every reason name of ``names`` (``_lib.REASONS`` / ``g1.REASONS``)."""
    codes = {v: k for k, v in table.items() if v is not None}
    mask = 0
    for n in names:
        if n not in codes:
            raise ValueError("unknown reason %r (known: %s)" % (n, sorted(codes)))
        mask |= 1 << codes[n]
    return mask


def decode(rows, nq, nv, na):
    """Entries [n, W] float32 (time order) -> dict of arrays; the last four columns are int32 bit patterns."""
    rows = np.ascontiguousarray(rows, np.float32).reshape(-1, nq + 2 * nv + na + TAIL)
    o1, o2, o3, o4 = nq, nq + nv, nq + 2 * nv, nq + 2 * nv + na
    ints = rows[:, o4 + 1:].copy().view(np.int32)
    return dict(qpos=rows[:, :o1].copy(), qvel=rows[:, o1:o2].copy(), warm=rows[:, o2:o3].copy(), action=rows[:, o3:o4].copy(),
                reward=rows[:, o4].copy(), done=ints[:, 0].copy(), reason=ints[:, 1].copy(), kind=ints[:, 2].copy(), step=ints[:, 3].copy())


class FlightRecorder:
    """The last ``steps`` entries of every env of ``engine`` and up to ``captures`` frozen rings, all on the engine's device.

    ``reasons``: the done reasons (names of ``_lib.REASONS``) whose step freezes a copy.  ``env_offset`` is added to the env numbers
    that ``read`` / ``captures`` report (the sub-batch slice of a ``HipBatchEnv``).  ``attach=True`` hooks the recorder into the
    engine: from then on every ``step`` / ``step_active`` records and every ``reset`` / ``set_state`` / ``step_forced`` marks."""

    clear_on_reset = False

    def __init__(self, engine, steps=64, captures=16, reasons=("sim_error", "obs_out_of_bounds"), env_offset=0, attach=True):
        t = engine.torch
        self.engine, self.torch, self.device = engine, t, engine.device
        self.N, self.K, self.C, self.env_offset = engine.N, int(steps), int(captures), int(env_offset)
        self.nq, self.nv, self.na, table = _dims(engine)
        self.W = self.nq + 2 * self.nv + self.na + TAIL
        if self.K < 2 or self.C < 1:
            raise ValueError("FlightRecorder needs steps >= 2 and captures >= 1")
        self.mask = reason_mask(reasons, table)
        z = lambda *shape, dt=t.float32: t.zeros(*shape, dtype=dt, device=self.device)
        self.ring, self.head = z(self.N, self.K, self.W), z(self.N, dt=t.int32)          # head: uint32 on the device
        self.cap, self.cap_meta, self.cap_count = z(self.C, self.K, self.W), z(self.C, 4, dt=t.int32), z(2, dt=t.int32)
        self.trig = z(self.N, dt=t.int32)
        # persistent staging of get_state, and the reason rows of a step whose caller asked for none
        self.qpos, self.qvel, self.warm = z(self.N, self.nq), z(self.N, self.nv), z(self.N, self.nv)
        self.reason = z(self.N, dt=t.int32)
        self._arange = t.arange(self.N, dtype=t.int32, device=self.device)
        self.bufs = _lib.DmTraceBufs(N=self.N, K=self.K, C=self.C, nq=self.nq, nv=self.nv, na=self.na, W=self.W,
                                     device=self.device.index or 0, ring=self.ring.data_ptr(), head=self.head.data_ptr(),
                                     cap=self.cap.data_ptr(), cap_meta=self.cap_meta.data_ptr(), cap_count=self.cap_count.data_ptr(),
                                     trig=self.trig.data_ptr())
        self._bufs_ref = C.byref(self.bufs)
        self.L = _lib.load_library()
        if attach:
            engine._recorder = self

    def detach(self):
        if self.engine._recorder is self:
            self.engine._recorder = None

    # ---- the two device calls
    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _stage(self):
        """The engine's existing get_state into the staging tensors (every env: the entries index them by env)."""
        if self.engine.PREFIX == "dm_":
            self.engine._call("get_state", None, self.N, self.qpos, self.qvel, self.warm, None)
        else:
            self.engine._call("get_state", self.qpos, self.qvel, self.warm)

    def _check(self, rc, name):
        if rc != 0:
            raise RuntimeError("%s failed (%d): %s" % (name, rc, (self.L.dm_trace_last_error() or b"").decode()))

    def record(self, actions, out, env_ids=None, nslots=None, reason=None):
        """One step entry for every env (for ``env_ids[:nslots]`` with a list, as ``step_active`` takes it): the state the engine
        holds now, ``actions`` and ``out``'s reward, done flag and reason (``reason``: the tensor to read when ``out`` has none)."""
        reason = out.get("reason") if reason is None else reason
        if reason is None:
            raise ValueError("FlightRecorder.record needs the step's reason rows")
        self._stage()
        p = _lib._ptr
        self._check(self.L.dm_trace_record(self._bufs_ref, p(self.qpos), p(self.qvel), p(self.warm), p(actions), p(out["rew"]), p(out["done"]),
                                           p(reason), p(env_ids), self.N if nslots is None else int(nslots), self.mask, self._stream()),
                    "dm_trace_record")

    def mark(self, env_ids=None, nslots=None, mask=None):
        """One mark entry (a state set from outside): every env, ``env_ids[:nslots]``, or the envs of a reset ``mask``."""
        if mask is not None:
            env_ids, nslots = self.torch.where(mask.reshape(-1) != 0, self._arange, -1).to(self.torch.int32).contiguous(), self.N
        self._stage()
        p = _lib._ptr
        self._check(self.L.dm_trace_mark(self._bufs_ref, p(self.qpos), p(self.qvel), p(self.warm), p(env_ids),
                                         self.N if nslots is None else int(nslots), self._stream()), "dm_trace_mark")

    def mark_reset(self, mask=None):
        """``reset`` of the engine: the mark of the fresh state; with ``clear_on_reset`` (a single env's log) the log starts over."""
        if self.clear_on_reset:
            self.clear()
        self.mark(mask=mask)

    # ---- reading back (each call synchronises)
    def _decode(self, rows, env):
        d = decode(rows, self.nq, self.nv, self.na)
        d["env"] = int(env) + self.env_offset
        return d

    def read(self, env):
        """Env ``env``'s ring in time order, oldest entry first, as a dict of numpy arrays (``FIELDS`` and ``env``)."""
        head = int(self.head[env].item()) & 0xFFFFFFFF
        n = min(head, self.K)
        ring = self.ring[env].cpu().numpy()
        return self._decode(ring[[(head - n + r) % self.K for r in range(n)]], env)

    def counts(self):
        """(copies filed, triggers seen)"""
        c = self.cap_count.cpu().numpy()
        return int(c[0]), int(c[1])

    def captures(self):
        """The filed copies in slot order: a list of ``read``-style dicts with ``meta`` = {env, entries, head, reason}."""
        filed = self.counts()[0]
        meta, cap = self.cap_meta[:filed].cpu().numpy(), self.cap[:filed].cpu().numpy()
        out = []
        for s in range(filed):
            d = self._decode(cap[s, :meta[s, 1]], meta[s, 0])
            d["meta"] = dict(env=int(meta[s, 0]) + self.env_offset, entries=int(meta[s, 1]), head=int(meta[s, 2]), reason=int(meta[s, 3]))
            out.append(d)
        return out

    def clear_captures(self):
        for x in (self.cap, self.cap_meta, self.cap_count):
            x.zero_()

    def clear(self):
        self.clear_captures()
        for x in (self.ring, self.head, self.trig):
            x.zero_()


# ------------------------------------------------------------------------------------------ the reference's dict and file
def _kinematics(model):
    from . import mjcf
    if isinstance(model, mjcf.GModel):
        return lambda q: mjcf.forward_kinematics_general(model, q)["xpos"]
    from .model import forward_kinematics
    return lambda q: forward_kinematics(model, q)["xpos"]


def to_episode_log(entries, motion, robot, model=None):
    """``read``-style ``entries`` -> the reference's ``episode_debug_log`` dict as ``json`` writes it (lists, floats, strings).

    ``action``, ``qpos``, ``qvel``, ``reward`` and ``body_xpos`` (host kinematics of ``model``; left out without one) hold one item per
    step entry of the last episode in the ring: what follows the last earlier step that reported done.  As in the reference the step
    that raised a sim error is not appended, its action is ``last_action``; an out-of-bounds step is.  ``full_traceback`` is set when
    the last step ended with reason 5 or 6.  ``body_xvelp`` is not written.  Everything else this build knows sits under
    ``entries``: the whole ring with marks, warm starts, done, reason, kind, step and env."""
    kind, done, reason = (np.asarray(entries[k]) for k in ("kind", "done", "reason"))
    steps = [i for i in range(len(kind)) if kind[i] == KIND_STEP]
    ended = [i for i in steps[:-1] if done[i] != 0]
    if ended:
        steps = [i for i in steps if i > ended[-1]]
    log = {}
    last = steps[-1] if steps else None
    sim_error = last is not None and done[last] != 0 and reason[last] == 5
    if sim_error:
        steps = steps[:-1]
    f64 = lambda a: np.asarray(a, np.float64).tolist()
    log["action"] = [f64(entries["action"][i]) for i in steps]
    if model is not None:
        fk = _kinematics(model)
        log["body_xpos"] = [f64(fk(np.asarray(entries["qpos"][i], np.float64))) for i in steps]
    log["qpos"] = [f64(entries["qpos"][i]) for i in steps]
    log["qvel"] = [f64(entries["qvel"][i]) for i in steps]
    log["reward"] = [float(entries["reward"][i]) for i in steps]
    if sim_error:
        log["last_action"] = f64(entries["action"][last])
        log["full_traceback"] = SIM_ERROR_TRACEBACK
    elif last is not None and done[last] != 0 and reason[last] == 6:
        log["full_traceback"] = OBS_BOUNDS_TRACEBACK
    log["motion"], log["robot"] = motion, robot
    ent = {k: (f64(entries[k]) if k in ("qpos", "qvel", "warm", "action", "reward") else np.asarray(entries[k]).astype(np.int64).tolist())
           for k in FIELDS}
    ent["env"] = int(entries.get("env", 0))
    log["entries"] = ent
    return log


def default_path(directory=None, env=None):
    """The reference's file name (src/deepmimic_env.py:369); a batch dump takes a directory and adds ``_env<i>``."""
    name = "deepmimic_episode_{}".format(time.strftime("%Y%m%d-%H%M_%S")) + ("" if env is None else "_env%d" % env) + ".json"
    return os.path.join("/tmp" if directory is None else directory, name)


def write(path, log):
    with open(path, "w") as f:
        f.write(json.dumps(log, indent=4))
    return path


def load(path):
    with open(path) as f:
        return json.load(f)


def entries_of(log):
    """The ``entries`` of a loaded file as numpy arrays again (a reference file without them: its steps, as step entries)."""
    ent = log.get("entries")
    if ent is None:
        n = len(log.get("qpos", []))
        z = np.zeros(n, np.int32)
        return dict(qpos=np.asarray(log["qpos"], np.float32), qvel=np.asarray(log["qvel"], np.float32), warm=None,
                    action=np.asarray(log["action"], np.float32), reward=np.asarray(log["reward"], np.float32), done=z, reason=z,
                    kind=z, step=np.arange(n, dtype=np.int32), env=0)
    out = {k: np.asarray(ent[k], np.float32 if k in ("qpos", "qvel", "warm", "action", "reward") else np.int32) for k in FIELDS}
    out["env"] = int(ent.get("env", 0))
    return out


# ------------------------------------------------------------------------------------------ surfaces
class BatchDebugLog:
    """What ``HipBatchEnv.enable_debug_log`` returns: one recorder per engine, env numbers offset by the sub-batch slice."""

    def __init__(self, env, steps=64, captures=16, reasons=("sim_error", "obs_out_of_bounds")):
        self.env = env
        self.recorders = [FlightRecorder(e, steps, captures, reasons, env_offset=sl.start) for e, sl in zip(env.engines, env.sub_slices)]
        self._dumped = [0, 0]          # captures, triggers of the dumps so far (a dump frees the slots)
        self.files = []

    def _motion(self, env_index):
        motions = getattr(self.env, "motions", None)
        return motions[env_index % len(motions)] if motions else "combined"

    def counts(self):
        """(captures filed, triggers seen) since ``enable_debug_log``."""
        c = [r.counts() for r in self.recorders]
        return self._dumped[0] + sum(x[0] for x in c), self._dumped[1] + sum(x[1] for x in c)

    def dump(self, directory):
        """Write the captures filed since the last dump, one file each, and free their slots; returns the paths."""
        paths = []
        robot = getattr(getattr(self.env, "robot_config", None), "robot", "humanoid3d")
        for r in self.recorders:
            filed, seen = r.counts()
            if seen == 0:
                continue
            os.makedirs(directory, exist_ok=True)
            for cap in r.captures():
                log = to_episode_log(cap, self._motion(cap["env"]), robot, self.env.model)
                log["capture"], log["auto_reset"] = cap["meta"], bool(self.env.auto_reset)
                path = default_path(directory, cap["env"])
                k = 1
                while os.path.exists(path):            # two captures of one env within the same second
                    path = default_path(directory, cap["env"])[:-5] + "_%d.json" % k
                    k += 1
                paths.append(write(path, log))
                print("Error in step, debug log written to {}".format(path) if cap["meta"]["reason"] == 5 else
                      "Observation out of bounds in step, debug log written to {}".format(path))
            self._dumped[0] += filed
            self._dumped[1] += seen
            r.clear_captures()
        self.files += paths
        return paths

    def close(self):
        for r in self.recorders:
            r.detach()


class SingleDebugLog:
    """``HipSingleEnv.enable_debug_log``: the whole episode of one env (``MAX_EP_LENGTH + 2`` entries), cleared on ``reset``."""

    def __init__(self, env):
        self.env = env
        self.recorder = FlightRecorder(env._eng, steps=env.ENV_CFG.MAX_EP_LENGTH + 2, captures=1)
        self.recorder.clear_on_reset = True
        self.files = []

    def _names(self):
        mcfg = getattr(self.env, "motion_config", None)
        return (mcfg.motion if mcfg is not None else "combined"), self.env.robot_config.robot

    def log(self):
        ent = self.recorder.read(0)
        if not (ent["kind"] == KIND_STEP).any():
            return {}
        return to_episode_log(ent, *self._names(), self.env.model)

    def on_step(self, reason):
        """After a step that ended with reason 5 or 6: the reference's file and message (src/deepmimic_env.py:366-378, :465-476)."""
        if reason not in (5, 6):
            return None
        path = write(default_path(), self.log() or to_episode_log(self.recorder.read(0), *self._names(), self.env.model))
        print("Error in step, debug log written to {}".format(path) if reason == 5 else
              "Observation out of bounds in step, debug log written to {}".format(path))
        self.files.append(path)
        return path


# ------------------------------------------------------------------------------------------ replay and re-simulation
def _engine_for(robot, motion, n, device=0):
    """An ``auto_reset=False`` engine of ``n`` envs of ``robot`` with ``motion`` loaded (the task layer needs a clip; the physics
    that ``resimulate`` compares does not depend on which)."""
    if robot == "unitree_g1":
        from . import g1
        eng = g1.G1HipEngine(n, device=device, auto_reset=False)
        mcfg, mc = g1._g1_mocap(None if motion == "combined" else motion)
        g1._load(eng, mcfg, mc)
        return eng
    from .config import MotionConfig, RobotConfig
    from .mocap import MocapDM
    from .model import load_model
    model = load_model(RobotConfig(robot).xml_path)
    mc = MocapDM(robot=robot, model=model)
    mc.load_mocap(MotionConfig(None if motion == "combined" else motion, robot).mocap_path)
    eng = _lib.HipEngine(model, n, device=device, auto_reset=False, low_z=RobotConfig(robot).low_z)
    eng.load_clip(0, mc)
    return eng


def resimulate(engine, rings):
    """One-step, teacher-forced replay.  ``rings``: ``engine.N`` ``read``-style dicts of equal length n (one per env).  For
    j = 0 .. n-2 every env is put at entry j's state with its warm start (``set_state``, no forward evaluation) and takes one step
    with entry j+1's action; where entry j+1 is a step entry the new state is compared with the logged one.  Returns
    ``dqpos``, ``dqvel`` float64 [n-1, N] (largest absolute difference; nan where entry j+1 is a mark), ``same`` bool [n-1, N]
    (every bit of qpos, qvel and warm start agrees), ``compared`` (entry j+1 is a step) and ``reason`` (its done reason, else 0).
    ``engine`` is built with ``auto_reset=False``; of a log made under auto-reset the done steps do not compare: the state logged
    after them is a fresh episode's, which no step from the previous state reproduces.  A step logged with a sim error does not
    either: the engine put qpos0 in place of the state."""
    t, N = engine.torch, engine.N
    assert len(rings) == N and len({len(r["kind"]) for r in rings}) == 1
    n = len(rings[0]["kind"])
    st = {k: np.stack([np.asarray(r[k], np.float32) for r in rings], 1) for k in ("qpos", "qvel", "warm", "action")}   # [n, N, .]
    kind = np.stack([np.asarray(r["kind"]) for r in rings], 1)
    dev = lambda a: t.as_tensor(np.ascontiguousarray(a), device=engine.device)
    out = engine.alloc_outputs()
    dq, dv, same = np.full((n - 1, N), np.nan), np.full((n - 1, N), np.nan), np.zeros((n - 1, N), bool)
    bits = lambda a: np.ascontiguousarray(a).view(np.int32)
    for j in range(n - 1):
        engine.set_state(dev(st["qpos"][j]), dev(st["qvel"][j]), warm=dev(st["warm"][j]), run_forward=False)
        engine.step(dev(st["action"][j + 1]), out)
        got = [x.cpu().numpy() for x in engine.get_state()[:3]]
        want = [st[k][j + 1] for k in ("qpos", "qvel", "warm")]
        stepped = kind[j + 1] == KIND_STEP
        with np.errstate(invalid="ignore"):
            a, b = np.abs(got[0].astype(np.float64) - want[0]).max(1), np.abs(got[1].astype(np.float64) - want[1]).max(1)
        dq[j], dv[j] = np.where(stepped, a, np.nan), np.where(stepped, b, np.nan)
        same[j] = stepped & np.all([(bits(g) == bits(w)).all(1) for g, w in zip(got, want)], 0)
    reason = np.stack([np.where(np.asarray(r["done"]) != 0, np.asarray(r["reason"]), 0) for r in rings], 1)
    return dict(dqpos=dq, dqvel=dv, same=same, compared=kind[1:] == KIND_STEP, reason=reason[1:])


def summary(log):
    """The lines the CLI prints: robot, motion, reason, number of steps and the largest |qvel| per step."""
    ent = entries_of(log)
    qvel = np.asarray(log.get("qvel", []), np.float64).reshape(len(log.get("qvel", [])), -1)
    tb = log.get("full_traceback")
    reason = "sim_error" if "last_action" in log else "obs_out_of_bounds" if tb == OBS_BOUNDS_TRACEBACK else "none"
    lines = ["robot   %s" % log.get("robot"), "motion  %s" % log.get("motion"), "reason  %s" % reason,
             "steps   %d (%d ring entries, %d marks)" % (len(qvel), len(ent["kind"]), int((ent["kind"] == KIND_MARK).sum()))]
    if tb:
        lines.append("traceback  %s" % tb.strip().splitlines()[-1])
    for i, v in enumerate(qvel):
        lines.append("step %4d  max|qvel| %.6g" % (i, np.abs(v).max() if v.size else 0.0))
    return lines


def render_frames(log, directory, renderer="stick", size=(320, 240), last=None, device=0):
    """check_debug_log.py's replay: every logged step state goes through ``set_state`` + ``render`` into ``frame_%04d.png``."""
    from PIL import Image
    from .deepmimic_env import DPEnv
    motion = None if log.get("motion") in (None, "combined") else log["motion"]
    env = DPEnv(motion, robot=log.get("robot", "humanoid3d"), device=device, renderer=renderer)
    os.makedirs(directory, exist_ok=True)
    qpos, qvel = np.asarray(log["qpos"], np.float64), np.asarray(log["qvel"], np.float64)
    idx = list(range(len(qpos)))[-last:] if last else list(range(len(qpos)))
    paths = []
    try:
        for i in idx:
            env.set_state(qpos[i], qvel[i])
            if renderer == "raycast":
                frame = env.render_batch([0], width=size[0], height=size[1])["rgb"][0].cpu().numpy()
            else:
                from .render import stick_figure
                frame = stick_figure(env._eng.body_xpos(), env.model.body_parent, size=size)
            paths.append(os.path.join(directory, "frame_%04d.png" % i))
            Image.fromarray(frame).save(paths[-1])
    finally:
        env.close()
    return paths


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m deepmimic_mujoco_amd.debug_log", description=__doc__.split("\n\n")[0])
    ap.add_argument("file")
    ap.add_argument("--frames", metavar="DIR", help="replay the logged states through set_state + render into PNGs")
    ap.add_argument("--renderer", default="stick", choices=["stick", "raycast"])
    ap.add_argument("--size", default="320x240", help="frame size WxH")
    ap.add_argument("--last", type=int, default=0, help="--frames: only the last N steps")
    ap.add_argument("--resimulate", action="store_true",
                    help="one engine step from every logged state with the next logged action, against the next logged state")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    log = load(args.file)
    if args.frames:
        w, h = (int(x) for x in args.size.lower().split("x"))
        paths = render_frames(log, args.frames, args.renderer, (w, h), args.last or None, args.device)
        print("%d frames written to %s" % (len(paths), args.frames))
    elif args.resimulate:
        ent = entries_of(log)
        if ent["warm"] is None:
            ap.error("--resimulate needs the warm starts under 'entries' (a file of this build)")
        eng = _engine_for(log.get("robot", "humanoid3d"), log.get("motion"), 1, args.device)
        try:
            r = resimulate(eng, [ent])
        finally:
            eng.close()
        for j in range(len(r["same"])):
            if r["compared"][j, 0] and ent["done"][j + 1] != 0 and (log.get("auto_reset") or ent["reason"][j + 1] == 5):
                print("entry %4d -> %4d  done (%s): the logged state is not this step's" % (j, j + 1, _lib.REASONS.get(int(ent["reason"][j + 1]))))
            elif r["compared"][j, 0]:
                print("entry %4d -> %4d  max|dqpos| %.3e  max|dqvel| %.3e  %s" % (j, j + 1, r["dqpos"][j, 0], r["dqvel"][j, 0],
                                                                                "all bits agree" if r["same"][j, 0] else "bits differ"))
            else:
                print("entry %4d -> %4d  mark: not a step" % (j, j + 1))
    else:
        print("\n".join(summary(log)))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
