"""One-step, teacher-forced comparison of an episode debug log (deepmimic_mujoco_amd/debug_log.py) against the fp64 oracle.

    python scripts/debug_log_vs_oracle.py /tmp/deepmimic_episode_<time>.json

Every logged state with its warm start goes into the oracle (oracle/oracle.py for humanoid3d, oracle/oracle_g1.py for unitree_g1),
which takes one physics step with the next logged action; the result is compared with the next logged state.  Prints, per step
entry, the largest |dqpos| and |dqvel| and the first step above the project's 1e-4 qpos gate: an engine step the oracle does not
reproduce from the same state is a kernel question, one it reproduces is physics.  CPU only.  Lives here, not in the package: the
package does not import the oracle.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GATE = 1e-4


def _oracle_step(robot):
    """step(qpos, qvel, warm, action) -> (qpos, qvel) after one fp64 physics step, or None when the oracle refuses the state."""
    if robot == "unitree_g1":
        from deepmimic_mujoco_amd.g1 import MAXCON, MAXROW, NU
        from oracle.oracle_g1 import G1Sim
        sim = G1Sim()
        sim.set_caps(MAXCON, MAXROW)                 # the engine's capacities
        nu, scale = NU, 20.0                         # src/deepmimic_env.py:348-351: hands zero, ACT_SCALE
    else:
        from deepmimic_mujoco_amd.model import load_model
        from oracle.oracle import OracleSim
        sim = OracleSim(load_model())
        sim.set_caps(32, 128)
        nu, scale = 28, 1.0

    def step(qpos, qvel, warm, action):
        ctrl = np.zeros(nu)
        ctrl[:len(action)] = np.asarray(action, np.float64) * scale
        for name, val in (("qpos", qpos), ("qvel", qvel), ("qacc_warmstart", warm), ("ctrl", ctrl)):
            sim.set(name, np.asarray(val, np.float64))
        if sim.step() != 0:
            return None
        return sim.get("qpos"), sim.get("qvel")
    return step


def compare(log):
    """Rows (entry, max|dqpos|, max|dqvel|) for every step entry that follows a finite logged state; None differences where
    the oracle refused the state (a sim error of its own)."""
    from deepmimic_mujoco_amd.debug_log import KIND_STEP, entries_of
    ent = entries_of(log)
    if ent["warm"] is None:
        raise SystemExit("this file has no 'entries' (warm starts): it was not written by this build")
    step = _oracle_step(log.get("robot", "humanoid3d"))
    rows = []
    for j in range(len(ent["kind"]) - 1):
        if ent["kind"][j + 1] != KIND_STEP:
            continue
        if ent["done"][j + 1] != 0 and ent["reason"][j + 1] == 5:
            rows.append((j + 1, None, None, "sim error in the log: the engine reset the state"))
            continue
        if ent["done"][j + 1] != 0 and log.get("auto_reset"):
            rows.append((j + 1, None, None, "done under auto-reset: the logged state is the next episode's"))
            continue
        got = step(ent["qpos"][j], ent["qvel"][j], ent["warm"][j], ent["action"][j + 1])
        if got is None:
            rows.append((j + 1, None, None, "the oracle refused the state"))
            continue
        dq = float(np.abs(got[0] - ent["qpos"][j + 1].astype(np.float64)).max())
        dv = float(np.abs(got[1] - ent["qvel"][j + 1].astype(np.float64)).max())
        rows.append((j + 1, dq, dv, ""))
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("file")
    args = ap.parse_args(argv)
    from deepmimic_mujoco_amd.debug_log import load
    rows = compare(load(args.file))
    first = None
    for j, dq, dv, note in rows:
        if dq is None:
            print("entry %4d  %s" % (j, note))
            continue
        print("entry %4d  max|dqpos| %.3e  max|dqvel| %.3e" % (j, dq, dv))
        if first is None and not dq <= GATE:
            first = j
    worst = max([r[1] for r in rows if r[1] is not None], default=0.0)
    print("steps compared %d  worst max|dqpos| %.3e  gate %.0e" % (sum(r[1] is not None for r in rows), worst, GATE))
    print("first step above the gate: %s" % ("none" if first is None else "entry %d" % first))
    return 0 if first is None else 1


if __name__ == "__main__":
    raise SystemExit(main())
