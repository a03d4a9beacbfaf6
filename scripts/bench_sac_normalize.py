"""Cost of SAC(env, normalizer=HipVecNormalize(env)) (sac.py; dm_sac_gather_norm of csrc/dm_sac.hip in the place of dm_sac_gather).

Two measurements, the method of DESIGN §24: both arms in this process, alternating window by window, `--runs` timed windows each
after a warm-up window, medians, spread stated.  The yardstick is the arm without the normaliser: its gradient step is the launch
sequence it always was (tests/test_sac_vecnorm_gpu.py holds that), so no other build is needed.
  * gradient step: microseconds per REPLAYED gradient step (the captured hipGraph) at B = 256, arch (1024, 512), for the humanoid
    (D, A) = (67, 28) and the G1 (98, 23), over a ring filled by a stub env of 32 envs.  A window is a pair of device events around
    `--replays` replays.  A third arm has the normaliser with both transforms switched off (the same launch, copying): it separates
    the cost of the launch from the cost of the arithmetic.  The two gather kernels' own times come from a child process under
    `rocprofv3 --kernel-trace --stats` that runs eager gradient steps of both arms (`--kernel-loop`, internal).
  * learn loop: env-steps/s of `SAC.learn` (env step + store + one gradient step per vec-env step, with the normaliser also its three
    statistics launches) on the humanoid walk env at 32 and 4 096 envs.  A window is a host clock around `--loop-steps` vec-env steps
    that ends in a device synchronise.
Writes profiles/sac_vecnorm_bench.json and prints it; the numbers are recorded, not gated.

    python scripts/bench_sac_normalize.py [--runs 3] [--replays 400] [--loop-steps 300] [--envs 32,4096]
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

SHAPES = {"humanoid_67_28": (67, 28), "g1_98_23": (98, 23)}


class StubEnv:
    """step_tensor surface over random observations of badly mixed scale: only there to fill a ring and the statistics."""

    def __init__(self, n, D, A, device):
        from deepmimic_mujoco_amd.vec_env import Box
        self.num_envs, self.device = n, torch.device(device)
        self.observation_space, self.action_space = Box(-1, 1, (D,)), Box(-1, 1, (A,))
        self._g = torch.Generator(device=self.device).manual_seed(0)
        self._scale = (10.0 ** torch.linspace(-3, 3, D)).to(self.device)
        self._t = 0

    def _obs(self):
        return (torch.randn(self.num_envs, self._scale.numel(), device=self.device, generator=self._g) * self._scale).contiguous()

    def reset_tensor(self):
        return self._obs()

    def step_tensor(self, actions):
        self._t += 1
        done = torch.full((self.num_envs,), 1 if self._t % 5 == 0 else 0, dtype=torch.uint8, device=self.device)
        return dict(obs=self._obs(), rew=-(actions ** 2).mean(1).contiguous(), done=done, terminal_obs=self._obs())


def summary(out, unit, digits):
    med = {k: statistics.median(v) for k, v in out.items()}
    return {unit: {k: [round(x, digits) for x in v] for k, v in out.items()}, "median": {k: round(v, digits) for k, v in med.items()},
            "spread_percent": {k: round(100 * (max(v) - min(v)) / med[k], 2) for k, v in out.items()}}, med


def filled_learner(D, A, name):
    """A learner over 64 stored steps of a 32-env stub; name: plain, normalizer, or normalizer_off (both transforms switched off)."""
    from deepmimic_mujoco_amd.sac import SAC
    from deepmimic_mujoco_amd.vec_normalize import HipVecNormalize
    env = StubEnv(32, D, A, "cuda")
    sac = SAC(env, net_arch=(1024, 512), batch_size=256, buffer_size=32 * 4096, learning_starts=10 ** 9, seed=0,
              normalizer=HipVecNormalize(env) if name != "plain" else None)
    for _ in range(64):
        sac.env_step()
    if name == "normalizer_off":
        sac.normalizer.norm_obs = sac.normalizer.norm_reward = False
    return sac


def gradient_case(D, A, runs, replays):
    arms = {}
    for name in ("plain", "normalizer", "normalizer_off"):
        arms[name] = filled_learner(D, A, name)
        arms[name].train(1)                                # captures

    def window(sac, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            sac._graph.replay()
        b.record()
        torch.cuda.synchronize()
        return 1e3 * a.elapsed_time(b) / n

    out = {k: [] for k in arms}
    for sac in arms.values():
        window(sac, max(20, replays // 4))
    for _ in range(runs):
        for k, sac in arms.items():
            out[k].append(window(sac, replays))
    res, med = summary(out, "us_per_gradient_step", 2)
    res.update(us_added=round(med["normalizer"] - med["plain"], 2), us_added_transforms_off=round(med["normalizer_off"] - med["plain"], 2),
               cost_percent=round(100 * (med["normalizer"] - med["plain"]) / med["plain"], 2), replays_per_window=replays)
    return res


def kernel_loop(D, A, steps=200):
    """What the profiled child runs: eager gradient steps of the plain and the normalised learner."""
    for name in ("plain", "normalizer"):
        sac = filled_learner(D, A, name)
        for _ in range(steps):
            sac.gradient_step_fused()
    torch.cuda.synchronize()


def kernel_case(D, A):
    """Average microseconds per launch of the two gather kernels, from rocprofv3's kernel statistics of a child process."""
    if shutil.which("rocprofv3") is None:
        return {"unavailable": "rocprofv3 is not on PATH"}
    tmp = tempfile.mkdtemp(prefix="sac_norm_bench_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "run", "--", sys.executable,
           os.path.abspath(__file__), "--kernel-loop", "--obs", str(D), "--act", str(A)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=400)
    files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
    if r.returncode != 0 or not files:
        return {"unavailable": "rocprofv3 run failed (%d): %s" % (r.returncode, r.stderr[-300:])}
    res = {}
    with open(files[0]) as f:
        for row in csv.DictReader(f):
            for k in ("sac_gather_kernel", "sac_gather_norm_kernel"):
                if k + "(" in row["Name"] or row["Name"].endswith(k):
                    res[k] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2),
                              "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    shutil.rmtree(tmp, ignore_errors=True)
    return res


def loop_case(envs, runs, steps):
    from deepmimic_mujoco_amd.deepmimic_env import HipDeepMimicVecEnv
    from deepmimic_mujoco_amd.sac import SAC
    from deepmimic_mujoco_amd.vec_normalize import HipVecNormalize
    arms = {}
    for name in ("plain", "normalizer"):
        env = HipDeepMimicVecEnv(envs, motion="walk")
        arms[name] = SAC(env, net_arch=(1024, 512), buffer_size=1_000_000, seed=0, normalizer=HipVecNormalize(env) if name == "normalizer" else None)

    def window(sac, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sac.learn(sac.num_timesteps + n * envs, log_interval=0)
        torch.cuda.synchronize()
        return n * envs / (time.perf_counter() - t0)

    out = {k: [] for k in arms}
    for sac in arms.values():
        window(sac, max(20, steps // 4))                   # past learning_starts: the graph is captured here
    for _ in range(runs):
        for k, sac in arms.items():
            out[k].append(window(sac, steps))
    for sac in arms.values():
        sac.env.close()
    res, med = summary(out, "env_steps_per_s", 0)
    res.update(cost_percent=round(100 * (med["plain"] - med["normalizer"]) / med["plain"], 2),
               us_per_vec_env_step_added=round(1e6 * envs * (1 / med["normalizer"] - 1 / med["plain"]), 2), steps_per_window=steps)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--replays", type=int, default=400)
    ap.add_argument("--loop-steps", type=int, default=300)
    ap.add_argument("--envs", default="32,4096")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sac_vecnorm_bench.json"))
    ap.add_argument("--kernel-loop", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--obs", type=int, default=67, help=argparse.SUPPRESS)
    ap.add_argument("--act", type=int, default=28, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sac_normalize.py measures on the GPU; none is visible")
    if args.kernel_loop:
        return kernel_loop(args.obs, args.act)
    res = {"workload": "sac_vecnormalize_cost", "batch": 256, "arch": [1024, 512],
           "timer": "gradient step: device events around a window of graph replays; learn loop: host clock around a window of vec-env "
                    "steps ending in a synchronise; arms alternate window by window",
           "gradient_step": {}, "learn_loop_humanoid_walk": {}}
    for name, (D, A) in SHAPES.items():
        res["gradient_step"][name] = gradient_case(D, A, args.runs, args.replays)
        res["gradient_step"][name]["kernels"] = kernel_case(D, A)
        print(name, json.dumps(res["gradient_step"][name]), file=sys.stderr, flush=True)
    for envs in (int(x) for x in args.envs.split(",")):
        res["learn_loop_humanoid_walk"][str(envs)] = loop_case(envs, args.runs, args.loop_steps)
        print(envs, json.dumps(res["learn_loop_humanoid_walk"][str(envs)]), file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
