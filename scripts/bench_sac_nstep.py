"""Cost of SAC(env, n_steps=n) (sac.py; dm_sac_gather_nstep of csrc/dm_sac.hip in the place of dm_sac_gather).

The method of DESIGN §24 / §25: the arms n_steps = 1, 3, 5 in this process, alternating window by window, `--runs` timed windows each
after a warm-up window, medians, spread stated.  The yardstick is the n_steps = 1 arm: its gradient step is the launch sequence it
always was (tests/test_sac_nstep_gpu.py holds that name for name), so no other build is needed and the code under test is never
measured against itself.
  * gradient step: microseconds per REPLAYED gradient step (the captured hipGraph) at B = 256, arch (1024, 512), for the humanoid
    (D, A) = (67, 28) and the G1 (98, 23), over a ring of 64 stored steps of a 32-env stub whose episodes end every fifth step (so
    chains of every length up to n occur).  A window is a pair of device events around `--replays` replays.
  * the gather kernels' own times come from a child process under `rocprofv3 --kernel-trace --stats` that runs eager gradient steps
    of all arms (`--kernel-loop`, internal).
Criterion: an n-step arm may exceed the yardstick by at most the larger of the windows' own spread and 2.6 %, the cost §25
accepted for the normaliser; `within_criterion` states it per arm.  Writes profiles/sac_nstep_bench.json and prints it.

    python scripts/bench_sac_nstep.py [--runs 3] [--replays 400]
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"humanoid_67_28": (67, 28), "g1_98_23": (98, 23)}
ARMS = (1, 3, 5)
ACCEPTED_PERCENT = 2.6           # the normaliser's cost per replayed gradient step at the G1 shape
KERNELS = ("sac_gather_kernel", "sac_gather_nstep_kernel")


class StubEnv:
    """step_tensor surface over random observations: only there to fill a ring; every env finishes on every fifth step."""

    def __init__(self, n, D, A, device):
        from deepmimic_mujoco_amd.vec_env import Box
        self.num_envs, self.device, self.D = n, torch.device(device), D
        self.observation_space, self.action_space = Box(-1, 1, (D,)), Box(-1, 1, (A,))
        self._g = torch.Generator(device=self.device).manual_seed(0)
        self._t = 0

    def _obs(self):
        return torch.randn(self.num_envs, self.D, device=self.device, generator=self._g).contiguous()

    def reset_tensor(self):
        return self._obs()

    def step_tensor(self, actions):
        self._t += 1
        done = torch.full((self.num_envs,), 1 if self._t % 5 == 0 else 0, dtype=torch.uint8, device=self.device)
        return dict(obs=self._obs(), rew=-(actions ** 2).mean(1).contiguous(), done=done, terminal_obs=self._obs())


def filled_learner(D, A, n_steps):
    from deepmimic_mujoco_amd.sac import SAC
    sac = SAC(StubEnv(32, D, A, "cuda"), net_arch=(1024, 512), batch_size=256, buffer_size=32 * 4096, learning_starts=10 ** 9, seed=0,
              n_steps=n_steps)
    for _ in range(64):
        sac.env_step()
    return sac


def gradient_case(D, A, runs, replays):
    arms = {}
    for n in ARMS:
        arms["n%d" % n] = filled_learner(D, A, n)
        arms["n%d" % n].train(1)                           # captures

    def window(sac, count):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(count):
            sac._graph.replay()
        b.record()
        torch.cuda.synchronize()
        return 1e3 * a.elapsed_time(b) / count

    out = {k: [] for k in arms}
    for sac in arms.values():
        window(sac, max(20, replays // 4))
    for _ in range(runs):
        for k, sac in arms.items():
            out[k].append(window(sac, replays))
    med = {k: statistics.median(v) for k, v in out.items()}
    spread = {k: 100 * (max(v) - min(v)) / med[k] for k, v in out.items()}
    allowed = max(ACCEPTED_PERCENT, max(spread.values()))
    cost = {k: 100 * (med[k] - med["n1"]) / med["n1"] for k in arms if k != "n1"}
    mean_k = {k: round(float(sac._fb["k"].float().mean()), 3) for k, sac in arms.items() if k != "n1"}
    return {"us_per_gradient_step": {k: [round(x, 2) for x in v] for k, v in out.items()}, "median": {k: round(v, 2) for k, v in med.items()},
            "spread_percent": {k: round(v, 2) for k, v in spread.items()}, "us_added": {k: round(med[k] - med["n1"], 2) for k in cost},
            "cost_percent": {k: round(v, 2) for k, v in cost.items()}, "allowed_percent": round(allowed, 2),
            "within_criterion": {k: bool(v <= allowed) for k, v in cost.items()}, "mean_chain_length_last_batch": mean_k,
            "replays_per_window": replays}


def kernel_loop(D, A, steps=200):
    """What the profiled child runs: eager gradient steps of every arm."""
    for n in ARMS:
        sac = filled_learner(D, A, n)
        for _ in range(steps):
            sac.gradient_step_fused()
    torch.cuda.synchronize()


def kernel_case(D, A):
    """Average microseconds per launch of the gather kernels, from rocprofv3's kernel statistics of a child process."""
    if shutil.which("rocprofv3") is None:
        return {"unavailable": "rocprofv3 is not on PATH"}
    tmp = tempfile.mkdtemp(prefix="sac_nstep_bench_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "run", "--", sys.executable,
           os.path.abspath(__file__), "--kernel-loop", "--obs", str(D), "--act", str(A)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=400)
    files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
    if r.returncode != 0 or not files:
        return {"unavailable": "rocprofv3 run failed (%d): %s" % (r.returncode, r.stderr[-300:])}
    res = {}
    with open(files[0]) as f:
        for row in csv.DictReader(f):
            for k in KERNELS:
                m = re.search(r"\b%s(<[^>]*>)?(\(|$)" % k, row["Name"])
                if m:                                      # the key carries the template argument: <false> without, <true> with a normaliser
                    res[k + (m.group(1) or "")] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2),
                              "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    shutil.rmtree(tmp, ignore_errors=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--replays", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sac_nstep_bench.json"))
    ap.add_argument("--no-kernels", action="store_true", help="skip the rocprofv3 child")
    ap.add_argument("--bench-line", metavar="FILE", help="a file whose last line starting with { is `bench.py --gpus 1`'s result on this "
                                                         "build: its value and ms_per_step are recorded next to the costs")
    ap.add_argument("--kernel-loop", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--obs", type=int, default=67, help=argparse.SUPPRESS)
    ap.add_argument("--act", type=int, default=28, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sac_nstep.py measures on the GPU; none is visible")
    if args.kernel_loop:
        return kernel_loop(args.obs, args.act)
    res = {"workload": "sac_nstep_cost", "batch": 256, "arch": [1024, 512], "arms_n_steps": list(ARMS),
           "timer": "device events around a window of graph replays; arms alternate window by window; the n_steps = 1 arm is the yardstick",
           "gradient_step": {}}
    for name, (D, A) in SHAPES.items():
        res["gradient_step"][name] = gradient_case(D, A, args.runs, args.replays)
        if not args.no_kernels:
            res["gradient_step"][name]["kernels"] = kernel_case(D, A)
        print(name, json.dumps(res["gradient_step"][name]), file=sys.stderr, flush=True)
    if args.bench_line:
        line = json.loads([x for x in open(args.bench_line).read().splitlines() if x.startswith("{")][-1])
        res["bench_py_gpus_1"] = {k: line[k] for k in ("value", "unit", "ms_per_step", "steps", "warmup")}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
