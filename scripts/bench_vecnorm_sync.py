"""Cost of the synchronised VecNormalize step and of sync() (vec_normalize.py, csrc/dm_vecnorm.hip) at 4 096 envs.

The normaliser alone on random buffers of D = 67 (humanoid) and D = 98 (G1 combined) columns, no env: `dm_vecnorm_step` (a plain
`HipVecNormalize`) against `dm_vecnorm_step_sync` (`sync_group="world"`, here a world of one), arms alternating window by window in
this process, `--runs` timed windows each after a warm-up window.  Two timers per arm: a host clock around `--calls` eager calls
ending in a device synchronise (what a host-driven rollout pays), and device events around one replay of a hipGraph of `--calls`
captured calls (what the kernels themselves take).  sync(): the same host clock around `--syncs` calls, in this process (pack +
merge, no collective) and in two child ranks over gloo on this one GPU (pack + one all-reduce of 2 x (2 D + 4) doubles + merge: a
rehearsal of the code path, the all-reduce goes through the host there).  Writes profiles/vecnorm_sync_bench.json and prints it; the
numbers are recorded, not gated.

    python scripts/bench_vecnorm_sync.py [--envs 4096] [--calls 500] [--runs 5] [--syncs 200]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make(envs, obs_dim, sync_group):
    from deepmimic_mujoco_amd.vec_env import Box
    from deepmimic_mujoco_amd.vec_normalize import HipVecNormalize

    class Shape:
        num_envs, device = envs, torch.device("cuda", 0)
        observation_space, action_space = Box(-1, 1, (obs_dim,)), Box(-1, 1, (1,))
    return HipVecNormalize(Shape(), sync_group=sync_group)


def buffers(vn, envs, obs_dim):
    g = torch.Generator(device="cpu").manual_seed(0)
    obs, rew = torch.randn(envs, obs_dim, generator=g).to(vn.device), torch.rand(envs, generator=g).to(vn.device)
    done = (torch.rand(envs, generator=g) < 0.02).to(torch.uint8).to(vn.device)
    tobs = torch.randn(envs, obs_dim, generator=g).to(vn.device)
    return obs, rew, done, tobs, torch.empty_like(obs), torch.empty_like(rew), torch.empty_like(tobs)


def eager_window(vn, bufs, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        vn.normalize_step_(*bufs)
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / calls


def graph_of(vn, bufs, calls):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        vn.normalize_step_(*bufs)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(calls):
            vn.normalize_step_(*bufs)
    return graph


def graph_window(graph, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    graph.replay()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / calls


def summary(v):
    med = statistics.median(v)
    return {"us": [round(x, 2) for x in v], "median_us": round(med, 2), "spread_percent": round(100 * (max(v) - min(v)) / med, 2)}


def step_case(envs, obs_dim, calls, runs):
    arms = {"step": make(envs, obs_dim, None), "step_sync": make(envs, obs_dim, "world")}
    bufs = {k: buffers(vn, envs, obs_dim) for k, vn in arms.items()}
    graphs = {k: graph_of(vn, bufs[k], calls) for k, vn in arms.items()}
    eager, replay = {k: [] for k in arms}, {k: [] for k in arms}
    for k, vn in arms.items():
        eager_window(vn, bufs[k], max(20, calls // 4))
        graph_window(graphs[k], calls)
    for _ in range(runs):
        for k, vn in arms.items():
            eager[k].append(eager_window(vn, bufs[k], calls))
        for k in arms:
            replay[k].append(graph_window(graphs[k], calls))
    res = {"eager_host_clock": {k: summary(v) for k, v in eager.items()}, "graph_replay_device_events": {k: summary(v) for k, v in replay.items()}}
    for r in res.values():
        r["step_sync_minus_step_us"] = round(r["step_sync"]["median_us"] - r["step"]["median_us"], 2)
        r["step_sync_minus_step_percent"] = round(100 * (r["step_sync"]["median_us"] - r["step"]["median_us"]) / r["step"]["median_us"], 2)
    return res


def sync_windows(vn, bufs, syncs, runs):
    out = []
    for i in range(runs + 1):
        vn.normalize_step_(*bufs)                        # something in acc
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(syncs):
            vn.sync()
        torch.cuda.synchronize()
        if i:                                            # the first window warms up
            out.append(1e6 * (time.perf_counter() - t0) / syncs)
    return out


def rank_main(args):
    """A child rank (started by torch.distributed.run): sync() over gloo, both ranks on this GPU; rank 0 prints its windows."""
    import torch.distributed as dist
    dist.init_process_group("gloo")
    torch.cuda.set_device(0)
    res = {}
    for obs_dim in (67, 98):
        vn = make(args.envs, obs_dim, "world")
        res[str(obs_dim)] = sync_windows(vn, buffers(vn, args.envs, obs_dim), args.syncs, args.runs)
    if dist.get_rank() == 0:
        print("SYNC_RANKS " + json.dumps(res), flush=True)
    dist.barrier()
    dist.destroy_process_group()


def two_rank_case(args):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
           "29561", os.path.abspath(__file__), "--envs", str(args.envs), "--syncs", str(args.syncs), "--runs", str(args.runs)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("SYNC_RANKS ")]
    if r.returncode != 0 or not lines:
        return {"unavailable": "the two-rank child failed (%d): %s" % (r.returncode, r.stderr[-300:])}
    return {k: summary(v) for k, v in json.loads(lines[-1][len("SYNC_RANKS "):]).items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--syncs", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vecnorm_sync_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vecnorm_sync.py measures on the GPU; none is visible")
    if "RANK" in os.environ:
        return rank_main(args)
    res = {"workload": "vec_normalize_sync_cost", "envs": args.envs, "calls_per_window": args.calls, "syncs_per_window": args.syncs,
           "timer": "eager: host clock around a window of calls ending in a synchronise; graph: device events around one replay of the "
                    "captured calls; arms alternate window by window", "step": {}, "sync_one_process": {}}
    for obs_dim in (67, 98):
        res["step"][str(obs_dim)] = step_case(args.envs, obs_dim, args.calls, args.runs)
        vn = make(args.envs, obs_dim, "world")
        res["sync_one_process"][str(obs_dim)] = summary(sync_windows(vn, buffers(vn, args.envs, obs_dim), args.syncs, args.runs))
        print(obs_dim, json.dumps(res["step"][str(obs_dim)]), file=sys.stderr, flush=True)
    res["sync_two_gloo_ranks_one_gpu"] = two_rank_case(args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
