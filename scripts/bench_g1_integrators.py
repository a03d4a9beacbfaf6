#!/usr/bin/env python
"""Unitree G1 step throughput under RK4 and under Euler (DmG1Config.integrator), walk DPEnv and the combined task, one JSON line.

    python scripts/bench_g1_integrators.py [--envs 4096] [--steps 200] [--warmup 50] [--reps 3] [--legs RK4,Euler]

Per task one engine per integrator in the same process, auto-reset on, random actions in [-1, 1] as bench.py::g1_record.  After the
warm-up the timed windows alternate RK4, Euler, RK4, ... (--reps windows each, --steps steps, each window ends in a synchronise), so
clock and thermal drift fall on both alike.  Reported per leg: env-steps/s of every window, their median and spread (max - min) / median,
last_kernel_ms (HIP events around the launches of one step) and the share of envs that ended per step (those take one more
evaluation, at the reset state).  The RK4 leg passes no integrator argument, so the script also runs on a tree without the option;
there the Euler legs are reported as null.  `--legs RK4` times RK4 alone: the like-for-like run against such a tree (with the Euler
engine alive in the same process the RK4 windows of the combined task read 0.7 % lower)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def make_engine(task, n, integrator):
    from deepmimic_mujoco_amd import g1
    from deepmimic_mujoco_amd.config import MotionConfig
    from deepmimic_mujoco_amd.mocap import MocapDM
    kw = {} if integrator is None else {"integrator": integrator}
    if task == "combined":
        eng = g1.G1HipEngine(n, auto_reset=True, seed=3, task=g1.TASK_COMBINED, max_ep_length=2000, **kw)
        motions = g1.COMBINED_CLIPS
    else:
        eng = g1.G1HipEngine(n, auto_reset=True, seed=3, **kw)
        motions = ("walk",)
    for cid, m in enumerate(motions):
        mc = MocapDM(robot="unitree_g1")
        mc.load_mocap(MotionConfig(m, robot="unitree_g1").mocap_path)
        eng.load_clip(mc, clip_id=cid)
    return eng


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default="RK4,Euler", help="comma list of the integrators to time")
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from deepmimic_mujoco_amd.g1 import NACT
    n = args.envs
    rec = {"workload": "g1_integrators", "envs": n, "steps_per_window": args.steps, "warmup": args.warmup, "reps": args.reps, "tasks": {}}
    for task in ("walk", "combined"):
        legs = {}
        for name, integ in (("RK4", None), ("Euler", "Euler")):
            if name not in args.legs.split(","):
                continue
            try:
                eng = make_engine(task, n, integ)
            except TypeError:           # a tree without the option
                legs[name] = None
                continue
            out = eng.alloc_outputs()
            eng.reset(out["obs"])
            g = torch.Generator(device=eng.device).manual_seed(0)
            acts = [torch.rand(n, NACT, device=eng.device, generator=g) * 2 - 1 for _ in range(8)]
            for t in range(args.warmup):
                eng.step(acts[t % 8], out)
            torch.cuda.synchronize()
            legs[name] = {"eng": eng, "out": out, "acts": acts, "rates": []}
        for r in range(args.reps):
            for name in ("RK4", "Euler"):
                leg = legs.get(name)
                if leg is None:
                    continue
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for t in range(args.steps):
                    leg["eng"].step(leg["acts"][t % 8], leg["out"])
                torch.cuda.synchronize()
                leg["rates"].append(n * args.steps / (time.perf_counter() - t0))
        res = {}
        for name, leg in legs.items():
            if leg is None:
                res[name] = None
                continue
            kms, done = [], []
            for t in range(20):         # outside the timed windows: a host read per step
                leg["eng"].step(leg["acts"][t % 8], leg["out"])
                torch.cuda.synchronize()
                kms.append(leg["eng"].last_kernel_ms())
                done.append(float(leg["out"]["done"].float().mean()))
            med = float(np.median(leg["rates"]))
            res[name] = {"env_steps_per_s": leg["rates"], "median": med, "spread": (max(leg["rates"]) - min(leg["rates"])) / med,
                         "last_kernel_ms": float(np.median(kms)), "done_fraction_per_step": float(np.mean(done)),
                         "pipeline": "split" if leg["eng"].split else "monolithic"}
            leg["eng"].close()
        if res.get("RK4") and res.get("Euler"):
            res["euler_over_rk4"] = res["Euler"]["median"] / res["RK4"]["median"]
        rec["tasks"][task] = res
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
