"""The rollout's tail: microseconds per call of `compute_gae` (the PyTorch loop over T, eager and captured as a hipGraph) and of
`dm_rollout_finish` (GAE + episode monitor + statistics, three launches) at (T, N) = (32, 4096), (4096, 32) and (32, 16384).
Timed with HIP events around `--reps` back-to-back calls after `--warmup` calls, the three arms alternating over `--rounds`
rounds (the minimum and the median over rounds are printed).  Prints one JSON line.

    python scripts/bench_gae.py [--reps 20] [--rounds 5] [--shapes 32x4096,4096x32,32x16384]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="32x4096,4096x32,32x16384")
    args = ap.parse_args()
    from deepmimic_mujoco_amd.ppo import RolloutFinish, compute_gae
    if not torch.cuda.is_available():
        raise SystemExit("bench_gae.py measures on the GPU; none is visible")
    dev = torch.device("cuda", 0)
    out = {"workload": "gae_tail", "unit": "us_per_call", "reps": args.reps, "rounds": args.rounds, "shapes": {}}
    for shape in args.shapes.split(","):
        T, N = (int(x) for x in shape.split("x"))
        g = torch.Generator(device=dev).manual_seed(T + N)
        rew, val = torch.rand(T, N, device=dev, generator=g), torch.randn(T, N, device=dev, generator=g)
        done_u8 = (torch.rand(T, N, device=dev, generator=g) < 0.02).to(torch.uint8)
        done = done_u8.float()
        lv = torch.randn(N, device=dev, generator=g)
        fin = RolloutFinish(T, N, dev, 0.99, 0.95)
        adv, ret = torch.empty_like(rew), torch.empty_like(rew)
        eager = lambda: compute_gae(rew, val, done, lv, 0.99, 0.95)
        kernel = lambda: fin(rew, done_u8, val, lv, adv, ret)
        ref = eager()
        kernel()
        assert torch.equal(ref[0], adv) and torch.equal(ref[1], ret), "dm_rollout_finish differs from compute_gae"
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            eager()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            cap = eager()
        arms = {"compute_gae_eager": eager, "compute_gae_captured": graph.replay, "dm_rollout_finish": kernel}
        reps = {k: (max(2, args.reps // 4) if (k != "dm_rollout_finish" and T > 1000) else args.reps) for k in arms}
        for fn in arms.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        assert torch.equal(cap[0], adv)
        t = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, fn in arms.items():
                t[k].append(timed(fn, reps[k]))
        rec = {k: {"min": round(min(v), 2), "median": round(statistics.median(v), 2)} for k, v in t.items()}
        rec["launches_compute_gae"] = 6 * T + 1
        rec["speedup_vs_eager"] = round(rec["compute_gae_eager"]["median"] / rec["dm_rollout_finish"]["median"], 1)
        rec["speedup_vs_captured"] = round(rec["compute_gae_captured"]["median"] / rec["dm_rollout_finish"]["median"], 1)
        out["shapes"]["%dx%d" % (T, N)] = rec
        print("# %dx%d %s" % (T, N, json.dumps(rec)), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
