"""Ray-cast renderer: milliseconds per `dm_render` call (kinematics + cast, rgb output) for both robots at a walk frame, 1 env at
320 x 240 and 256 envs at 64 x 64 with the default camera, and the host time of the stick figure per frame for comparison.
Each figure is the median of `--reps` calls, every call between its own pair of HIP events, after `--warmup` calls.  Prints one JSON
line (committed as profiles/render_bench.json); the numbers are recorded, not gated.

    python scripts/bench_render.py [--reps 20] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def event_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_render.py measures on the GPU; none is visible")
    from deepmimic_mujoco_amd import g1, raycast
    from deepmimic_mujoco_amd.config import MotionConfig
    from deepmimic_mujoco_amd.mocap import MocapDM
    from deepmimic_mujoco_amd.model import forward_kinematics, load_model
    from deepmimic_mujoco_amd.render import stick_figure
    hm, gm = load_model(), g1.load_g1_model()[0]
    out = {"workload": "raycast_render", "unit": "ms_per_call", "timer": "hip_events_per_call", "reps": args.reps, "warmup": args.warmup,
           "cases": {}}
    for robot, model in (("humanoid3d", hm), ("unitree_g1", gm)):
        mc = MocapDM(model=model) if robot == "humanoid3d" else MocapDM(robot=robot)
        mc.load_mocap(MotionConfig("walk", robot=robot).mocap_path)
        frames = np.asarray(mc.data_config, np.float32)
        r = raycast.RayRenderer(model)
        cam = raycast.Camera()
        for n, W, H in ((1, 320, 240), (256, 64, 64)):
            qpos = torch.tensor(frames[np.arange(n) % len(frames)], device=r.device).contiguous()
            rows = r.camera_rows(cam, qpos, None, W, H)
            work, o = torch.empty(n * r.G * 12, device=r.device), r.outputs(n, W, H)
            med, lo, hi = event_ms(lambda: r.render(qpos, width=W, height=H, cam=rows, workspace=work, out=o), args.reps, args.warmup)
            hit = float((o["rgb"].float().std() > 0).item())
            out["cases"]["%s_%denv_%dx%d" % (robot, n, W, H)] = {"median": round(med, 4), "min": round(lo, 4), "max": round(hi, 4),
                                                                 "geoms": r.G, "planes": r.scene.nplane, "frame_not_constant": hit}
        r.close()
    kin = forward_kinematics(hm, hm.qpos0)      # drawing only: the debug-buffer read and forward evaluation of render() come on top
    t = []
    for _ in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        stick_figure(kin["xpos"], hm.body_parent)
        t.append((time.perf_counter() - t0) * 1e3)
    out["stick_figure_host_ms_per_frame"] = round(statistics.median(t[args.warmup:]), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
