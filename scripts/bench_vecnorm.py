"""Cost of HipVecNormalize (vec_normalize.py, csrc/dm_vecnorm.hip) at 4 096 envs, on the humanoid walk task and the G1 combined task.

Per task: env-steps/s through `step_tensor`, the unwrapped env against the same env object behind the wrapper, arms alternating
window by window in this process (`--runs` timed windows each after a warm-up window; a window is a host clock around `--steps`
steps that ends in a device synchronise).  Per-launch times of the normaliser's three kernels: a child process under
`rocprofv3 --kernel-trace --stats` that only calls `dm_vecnorm_step` on buffers of the task's shape (`--kernel-loop`, internal).
End to end: `train.py --json` (the policy_forward route) with and without `--normalize`, `--train-runs` alternating child
processes per arm.  The yardstick is the arm without the wrapper of the same run.  Writes profiles/vecnorm_bench.json and prints it;
the numbers are recorded, not gated.

    python scripts/bench_vecnorm.py [--envs 4096] [--steps 400] [--g1-steps 60] [--runs 3] [--train-runs 3] [--train-total 2000000]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TASKS = {"humanoid_walk": dict(train=[], obs=67), "g1_combined": dict(train=["--env", "dp_combined_env", "--robot", "unitree_g1"], obs=98)}


def make_env(task, envs):
    if task == "g1_combined":
        from deepmimic_mujoco_amd.combined_env import HipCombinedVecEnv
        return HipCombinedVecEnv(envs, robot="unitree_g1")
    from deepmimic_mujoco_amd.deepmimic_env import HipDeepMimicVecEnv
    return HipDeepMimicVecEnv(envs, motion="walk")


def window(env, actions, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(steps):
        env.step_tensor(actions[t % len(actions)])
    torch.cuda.synchronize()
    return env.num_envs * steps / (time.perf_counter() - t0)


def step_case(task, envs, steps, runs):
    from deepmimic_mujoco_amd.vec_normalize import HipVecNormalize
    env = make_env(task, envs)
    vn = HipVecNormalize(env)
    g = torch.Generator(device="cpu").manual_seed(0)
    hi = torch.as_tensor(env.action_space.high)
    bank = [((torch.rand(envs, hi.numel(), generator=g) * 2 - 1) * 0.3 * hi).to(env.device).contiguous() for _ in range(16)]
    vn.reset_tensor()
    arms = {"unwrapped": env, "wrapped": vn}
    out = {k: [] for k in arms}
    for k, e in arms.items():
        window(e, bank, max(10, steps // 4))
    for _ in range(runs):
        for k, e in arms.items():
            out[k].append(window(e, bank, steps))
    env.close()
    med = {k: statistics.median(v) for k, v in out.items()}
    return {"env_steps_per_s": {k: [round(x) for x in v] for k, v in out.items()}, "median": {k: round(v) for k, v in med.items()},
            "cost_percent": round(100 * (med["unwrapped"] - med["wrapped"]) / med["unwrapped"], 2),
            "us_per_step_added": round(1e6 * envs * (1 / med["wrapped"] - 1 / med["unwrapped"]), 2),
            "spread_percent": {k: round(100 * (max(v) - min(v)) / med[k], 2) for k, v in out.items()}, "steps_per_window": steps}


def kernel_loop(envs, obs_dim, calls=200):
    """What the profiled child runs: `calls` training steps of the normaliser alone on random buffers."""
    from deepmimic_mujoco_amd.vec_env import Box

    class Shape:
        num_envs, device = envs, torch.device("cuda", 0)
        observation_space, action_space = Box(-1, 1, (obs_dim,)), Box(-1, 1, (1,))
    from deepmimic_mujoco_amd.vec_normalize import HipVecNormalize
    vn = HipVecNormalize(Shape())
    obs, rew = torch.randn(envs, obs_dim, device=vn.device), torch.rand(envs, device=vn.device)
    done = (torch.rand(envs, device=vn.device) < 0.02).to(torch.uint8)
    tobs, o, r, tb = torch.randn_like(obs), torch.empty_like(obs), torch.empty_like(rew), torch.empty_like(obs)
    for _ in range(calls):
        vn.normalize_step_(obs, rew, done, tobs, o, r, tb)
    torch.cuda.synchronize()


def kernel_case(envs, obs_dim):
    """Average ns per launch of the three kernels, from rocprofv3's kernel statistics of a child process."""
    if shutil.which("rocprofv3") is None:
        return {"unavailable": "rocprofv3 is not on PATH"}
    tmp = tempfile.mkdtemp(prefix="vecnorm_bench_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "run", "--", sys.executable,
           os.path.abspath(__file__), "--kernel-loop", "--envs", str(envs), "--obs", str(obs_dim)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
    files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
    if r.returncode != 0 or not files:
        return {"unavailable": "rocprofv3 run failed (%d): %s" % (r.returncode, r.stderr[-300:])}
    res = {}
    with open(files[0]) as f:
        for row in csv.DictReader(f):
            for k in ("moments", "update", "normalize"):
                if "vecnorm_%s_kernel" % k in row["Name"]:
                    res[k] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2),
                              "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    shutil.rmtree(tmp, ignore_errors=True)
    res["sum_average_us"] = round(sum(v["average_us"] for v in res.values()), 2)
    return res


def train_case(task, envs, total, runs):
    rows = {"without": [], "with": []}
    for _ in range(runs):
        for on in (False, True):
            cmd = ([sys.executable, "-m", "deepmimic_mujoco_amd.train", "--json", "--envs", str(envs), "--total", str(total)] + TASKS[task]["train"]
                   + (["--normalize"] if on else []))
            r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=900)
            if r.returncode != 0:
                raise SystemExit("train.py failed:\n" + r.stderr[-2000:])
            line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            print("%s train.py %s --normalize: %.0f env-steps/s overall" % (task, "with" if on else "without", line["overall_env_steps_per_s"]),
                  file=sys.stderr, flush=True)
            rows["with" if on else "without"].append({k: line[k] for k in ("rollout_env_steps_per_s", "overall_env_steps_per_s", "rollout_path", "normalize")})
    med = lambda arm, k: statistics.median(r[k] for r in rows[arm])
    res = {"total": total, "runs": rows}
    for k in ("rollout_env_steps_per_s", "overall_env_steps_per_s"):
        wo, w = med("without", k), med("with", k)
        res[k] = {"without": round(wo), "with": round(w), "cost_percent": round(100 * (wo - w) / wo, 2)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--g1-steps", type=int, default=60)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--train-runs", type=int, default=3)
    ap.add_argument("--train-total", type=int, default=2_000_000)
    ap.add_argument("--g1-train-total", type=int, default=400_000)
    ap.add_argument("--tasks", default=",".join(TASKS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vecnorm_bench.json"))
    ap.add_argument("--kernel-loop", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--obs", type=int, default=67, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vecnorm.py measures on the GPU; none is visible")
    if args.kernel_loop:
        return kernel_loop(args.envs, args.obs)
    res = {"workload": "vec_normalize_cost", "envs": args.envs, "timer": "host clock around a window of steps ending in a synchronise; "
           "kernels: rocprofv3 --kernel-trace --stats of a child that calls dm_vecnorm_step alone", "cases": {}}
    for task in args.tasks.split(","):
        g1 = task.startswith("g1")
        case = {"step_tensor": step_case(task, args.envs, args.g1_steps if g1 else args.steps, args.runs),
                "kernels": kernel_case(args.envs, TASKS[task]["obs"])}
        if args.train_runs > 0:
            case["train"] = train_case(task, args.envs, args.g1_train_total if g1 else args.train_total, args.train_runs)
        res["cases"][task] = case
        print(task, json.dumps(case), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
