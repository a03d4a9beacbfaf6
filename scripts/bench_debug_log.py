"""Cost of the episode debug log (debug_log.FlightRecorder, steps=64): milliseconds per batch step with and without a recorder.

Engine workloads (the humanoid at 4 096 envs with random actions and auto-reset; the Unitree G1 at 4 096 envs on the walk clip):
one env object, the two arms alternate in this process (recorder detached / attached), `--runs` timed windows each after a warm-up
window; a window is a host clock around `--steps` steps that ends in a device synchronise.  End to end: `train.py --json` on the
humanoid defaults, `--train-runs` alternating child processes per arm, with and without `--debug-log`.  The yardstick is the arm
without a recorder of the same run.  Writes profiles/debug_log_bench.json and prints it; the numbers are recorded, not gated.

    python scripts/bench_debug_log.py [--envs 4096] [--steps 400] [--g1-steps 60] [--runs 3] [--train-runs 3] [--train-total 2000000]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window(env, actions, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(steps):
        env.step_tensor(actions[t % len(actions)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def engine_case(env, actions, steps, runs):
    """ms per batch step, arms alternating: [(without, with), ...]."""
    dlog = env.enable_debug_log(steps=64)
    recs = [e._recorder for e in env.engines]

    def arm(on):
        for e, r in zip(env.engines, recs):
            e._recorder = r if on else None
    env.reset_tensor()
    out = {"without": [], "with": []}
    for on in (False, True):                 # warm-up window of either arm
        arm(on)
        window(env, actions, max(10, steps // 4))
    for _ in range(runs):
        for on in (False, True):
            arm(on)
            out["with" if on else "without"].append(window(env, actions, steps))
    arm(True)
    w, wo = statistics.median(out["with"]), statistics.median(out["without"])
    return {"ms_per_step_without": [round(x, 5) for x in out["without"]], "ms_per_step_with": [round(x, 5) for x in out["with"]],
            "median_without": round(wo, 5), "median_with": round(w, 5), "cost_ms": round(w - wo, 5), "cost_percent": round(100 * (w - wo) / wo, 2),
            "spread_without_percent": round(100 * (max(out["without"]) - min(out["without"])) / wo, 2),
            "spread_with_percent": round(100 * (max(out["with"]) - min(out["with"])) / w, 2),
            "triggers": dlog.counts()[1], "steps_per_window": steps}


def train_case(total, runs):
    rows = {"without": [], "with": []}
    tmp = tempfile.mkdtemp(prefix="debug_log_bench_")
    for _ in range(runs):
        for on in (False, True):
            cmd = [sys.executable, "-m", "deepmimic_mujoco_amd.train", "--json", "--total", str(total)] + (["--debug-log", tmp] if on else [])
            r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
            if r.returncode != 0:
                raise SystemExit("train.py failed:\n" + r.stderr[-2000:])
            line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            print("train.py %s recorder: %.0f env-steps/s overall" % ("with" if on else "without", line["overall_env_steps_per_s"]), file=sys.stderr, flush=True)
            rows["with" if on else "without"].append({k: line[k] for k in ("rollout_env_steps_per_s", "overall_env_steps_per_s", "rollout_path")}
                                                     | ({"debug_log": {k: line["debug_log"][k] for k in ("captures", "triggers")}} if on else {}))
    med = lambda arm, k: statistics.median(r[k] for r in rows[arm])
    return {"total": total, "runs": rows,
            "rollout_env_steps_per_s": {"without": round(med("without", "rollout_env_steps_per_s")), "with": round(med("with", "rollout_env_steps_per_s"))},
            "overall_env_steps_per_s": {"without": round(med("without", "overall_env_steps_per_s")), "with": round(med("with", "overall_env_steps_per_s"))}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--g1-steps", type=int, default=60)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--train-runs", type=int, default=3)
    ap.add_argument("--train-total", type=int, default=2_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "debug_log_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_debug_log.py measures on the GPU; none is visible")
    from deepmimic_mujoco_amd.deepmimic_env import HipDeepMimicVecEnv
    res = {"workload": "debug_log_cost", "recorder_steps": 64, "envs": args.envs, "timer": "host clock around a window of steps ending in a synchronise",
           "cases": {}}
    env = HipDeepMimicVecEnv(args.envs, motion="walk")
    bank = []
    for t in range(16):
        a = torch.zeros(args.envs, 28, device=env.device)
        env.engine.fill_random_actions(a, t)
        bank.append(a)
    res["cases"]["humanoid_random_auto_reset"] = engine_case(env, bank, args.steps, args.runs)
    env.close()
    env = HipDeepMimicVecEnv(args.envs, motion="walk", robot="unitree_g1")
    g = torch.Generator(device="cpu").manual_seed(0)
    hi = torch.as_tensor(env.action_space.high)
    bank = [((torch.rand(args.envs, 23, generator=g) * 2 - 1) * 0.3 * hi).to(env.device).contiguous() for _ in range(16)]
    res["cases"]["g1_walk"] = engine_case(env, bank, args.g1_steps, args.runs)
    env.close()
    if args.train_runs > 0:
        res["cases"]["train_humanoid_defaults"] = train_case(args.train_total, args.train_runs)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
