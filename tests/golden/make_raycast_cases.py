#!/usr/bin/env python
"""Writes tests/golden/raycast_cases.npz: frames of the fp64 ray-cast reference (tests/render_ref.py) for both robots.

    python tests/golden/make_raycast_cases.py            # writes tests/golden/raycast_cases.npz (CPU only, a few minutes)
    python tests/golden/make_raycast_cases.py --check    # regenerates and compares with the committed file

Per case NAME the file holds NAME/robot, NAME/wh (W, H), NAME/qpos float32 [N, nq], NAME/env_ids int32 [n] (rows of qpos; empty =
rows 0..N-1), NAME/cam float32 [n, 12] (eye, forward, right, up: what dm_render_cast takes), NAME/kin_xpos, NAME/kin_xmat float64
[n, G, 3 / 9] (the host kinematics at qpos), NAME/seg5 int8 [5, n, H, W] (model geom id of the five casts of every pixel, -1 =
miss; seg5[0] is the centre ray), NAME/depth float64 [n, H, W], NAME/rgb uint8 [n, H, W, 3], NAME/stable bool [n, H, W], and
NAME/err32: the worst relative depth error on stable pixels of the same reference run with every intermediate in float32.  The
frames are cast from float32(kin_xpos), float32(kin_xmat) and the float32 camera, promoted back to fp64: the geometry the kernel is
given.  The generator fails if more than 2 % of a frame is unstable (then the camera is moved, never the cap), if the float32 run
disagrees with the fp64 one in the geom id of a stable pixel, or if the file would exceed 500 KB.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "raycast_cases.npz")

import render_ref  # noqa: E402
from deepmimic_mujoco_amd import g1, raycast  # noqa: E402
from deepmimic_mujoco_amd.config import MotionConfig  # noqa: E402
from deepmimic_mujoco_amd.mocap import MocapDM  # noqa: E402
from deepmimic_mujoco_amd.model import load_model  # noqa: E402

Camera = raycast.Camera


def robots():
    hm, gm = load_model(), g1.load_g1_model()[0]
    return {"humanoid3d": (hm, raycast.build_scene(hm)), "unitree_g1": (gm, raycast.build_scene(gm))}


def frame(robot, motion, idx, model):
    mc = MocapDM(model=model) if robot == "humanoid3d" else MocapDM(robot=robot)
    mc.load_mocap(MotionConfig(motion, robot=robot).mocap_path)
    return np.asarray(mc.data_config[idx], np.float32)


def cases(R):
    """name -> (robot, W, H, qpos [N, nq], env_ids or None, cameras (one per rendered env))"""
    hm, gm = R["humanoid3d"][0], R["unitree_g1"][0]
    H3, G1 = "humanoid3d", "unitree_g1"
    gs = R[G1][1]
    c = {}
    # Cameras: a frame keeps its unstable pixels under the cap only if (a) no floor pixel is seen at a grazing angle (the depth of a
    # floor pixel moves by cot(angle below the horizon) * its angular size per pixel, so 1/32 pixel must stay under 1e-3 of it:
    # steep elevations and narrow fields of view) and (b) the image axes are not parallel to the checker (an axis-aligned camera
    # puts a whole pixel row within 1/64 pixel of a cell boundary).
    c["h_qpos0"] = (H3, 64, 48, hm.qpos0[None], None, [Camera(distance=6.0, azimuth=80, elevation=-45, fovy=30)])
    c["h_walk"] = (H3, 64, 48, frame(H3, "walk", 20, hm)[None], None, [Camera(distance=6.0, azimuth=120, elevation=-50, fovy=30)])
    c["h_lying"] = (H3, 64, 48, frame(H3, "getup_facedown", 0, hm)[None], None, [Camera(lookat=(0, 0, 0.3), azimuth=60, elevation=-55, distance=3.5, fovy=40)])
    c["g_walk"] = (G1, 64, 48, frame(G1, "walk", 10, gm)[None], None, [Camera(lookat=(0, 0, 0.7), distance=4.0, azimuth=75, elevation=-45, fovy=30)])
    c["g_getup"] = (G1, 64, 48, frame(G1, "getup_facedown", 40, gm)[None], None,
                    [Camera(lookat=(0, 0, 0.3), distance=4.5, azimuth=135, elevation=-50, fovy=30)])
    c["h_odd"] = (H3, 37, 29, frame(H3, "walk", 5, hm)[None], None, [Camera(distance=6.0, azimuth=70, elevation=-60, fovy=30)])
    c["g_odd"] = (G1, 37, 29, frame(G1, "walk", 30, gm)[None], None, [Camera(lookat=(0, 0, 0.7), distance=4.5, azimuth=100, elevation=-60, fovy=30)])
    c["h_sky"] = (H3, 64, 48, hm.qpos0[None], None, [Camera(lookat=(0, 0, 10.0), elevation=60, track_root=False)])
    q = frame(G1, "walk", 10, gm)
    c["g_top"] = (G1, 64, 48, q[None], None, [Camera(lookat=(float(q[0]), float(q[1]), float(q[2])), distance=1.5, azimuth=33, elevation=-89, fovy=70, track_root=False)])
    xpos = render_ref.kinematics(gm, gs, q)[0]
    torso = xpos[gs.geom_index(_mesh_geom(gm, "torso_link"))]
    # the close-up looks along the line from torso_link to the left ankle link, so that both hulls are candidates of the centre
    # tiles; at 0.6 m a 45 degree view puts several 7 mm facets into every pixel and a tenth of the frame is unstable, 8 degrees does not
    v = xpos[gs.geom_index(_mesh_geom(gm, "left_ankle_pitch_link"))] - torso
    az, el = np.degrees(np.arctan2(v[1], v[0])), np.degrees(np.arcsin(v[2] / np.linalg.norm(v)))
    c["g_torso"] = (G1, 64, 48, q[None], None, [Camera(lookat=tuple(float(v) for v in torso), distance=0.6, azimuth=float(az), elevation=float(el), fovy=8, track_root=False)])
    q8 = np.stack([frame(G1, "walk", 7 * k, gm) for k in range(8)])
    c["g_batch"] = (G1, 40, 30, q8, [2, 0, 5], [Camera(lookat=(0, 0, 0.7), distance=7.0, azimuth=100, elevation=-55, fovy=24),
                                               Camera(lookat=(0, 0, 0.7), distance=8.5, azimuth=40, elevation=-60, fovy=24),
                                               Camera(lookat=(0, 0, 0.6), distance=7.5, azimuth=150, elevation=-65, fovy=24)])
    return c


def _mesh_geom(gm, mesh):
    """model geom id of the collision geom that uses ``mesh``"""
    return [g for g in range(gm.ngeom) if gm.geom_mesh[g] == mesh and gm.geom_contype[g] != 0][0]


def one_case(name):
    """the arrays of one case, and its report line"""
    R = robots()
    out = {}
    robot, W, H, qpos, ids, cams = cases(R)[name]
    t0 = time.time()
    model, scene = R[robot]
    qpos = np.ascontiguousarray(qpos, np.float32)
    rows = list(range(len(qpos))) if ids is None else ids
    cam = np.stack([cm.rows(W, H, root_x=[qpos[r, 0]])[0] for cm, r in zip(cams, rows)]).astype(np.float32)
    kin = [render_ref.kinematics(model, scene, qpos[r]) for r in rows]
    kx, km = np.stack([k[0] for k in kin]), np.stack([k[1] for k in kin])
    seg5, dep, rgb, stable, err32 = [], [], [], [], 0.0
    for e in range(len(rows)):
        x32, m32, c32 = kx[e].astype(np.float32), km[e].astype(np.float32), cam[e]
        s5, d5, r5, st = render_ref.render5(scene, x32.astype(np.float64), m32.astype(np.float64), c32.astype(np.float64), W, H)
        bad = 1.0 - st.mean()
        assert bad <= render_ref.MAX_UNSTABLE, "%s env %d: %.2f %% of the frame is unstable: move the camera" % (name, e, 100 * bad)
        sf, df, _ = render_ref.render(scene, x32, m32, c32, W, H, np.float32)
        hit = st & (s5[0] >= 0)
        assert (sf == s5[0])[st].all(), "%s: the float32 reference changes the geom of a stable pixel" % name
        if hit.any():
            err32 = max(err32, float((np.abs(df.astype(np.float64) - d5[0]) / d5[0])[hit].max()))
        seg5.append(s5), dep.append(d5[0]), rgb.append(r5[0]), stable.append(st)
    assert np.abs(np.stack(seg5)).max() < 127
    out[name + "/robot"], out[name + "/wh"] = np.array(robot), np.array([W, H], np.int32)
    out[name + "/qpos"], out[name + "/cam"] = qpos, cam
    out[name + "/env_ids"] = np.array([] if ids is None else ids, np.int32)
    out[name + "/kin_xpos"], out[name + "/kin_xmat"] = kx, km
    out[name + "/seg5"] = np.stack(seg5, 1).astype(np.int8)
    out[name + "/depth"], out[name + "/rgb"], out[name + "/stable"] = np.stack(dep), np.stack(rgb), np.stack(stable)
    out[name + "/err32"] = np.array(err32)
    st = np.stack(stable)
    line = "%-8s %-11s %dx%d n=%d  unstable %.2f %% (worst env %.2f %%)  geoms seen %d  miss %.0f %%  err32 %.3g  (%.0f s)" % (
        name, robot, W, H, len(rows), 100 * (1 - st.mean()), 100 * max(1 - s.mean() for s in st), int((np.unique(out[name + "/seg5"][0]) >= 0).sum()),
        100 * (out[name + "/seg5"][0] < 0).mean(), err32, time.time() - t0)
    return out, line


def generate(jobs=8):
    """Every case, ``jobs`` at a time in worker processes (the cases are independent)."""
    import multiprocessing as mp
    R = robots()
    names = list(cases(R))
    out = {}
    with mp.Pool(min(jobs, len(names))) as pool:
        for part, line in pool.imap(one_case, names):
            out.update(part)
            print(line, flush=True)
    out["names"] = np.array(names)
    # what the cases are there for
    assert (out["h_sky/seg5"] < 0).all()
    gm, gs = R["unitree_g1"]
    seen = set(np.unique(out["g_torso/seg5"][0]).tolist())
    assert _mesh_geom(gm, "torso_link") in seen, "the close-up does not show torso_link"
    cam = out["g_torso/cam"][0].astype(np.float64)
    ankle = out["g_torso/kin_xpos"][0][gs.geom_index(_mesh_geom(gm, "left_ankle_pitch_link"))] - cam[0:3]
    z = ankle @ cam[3:6]
    assert z > 0 and abs(ankle @ cam[6:9]) / (cam[6:9] @ cam[6:9]) < z and abs(ankle @ cam[9:12]) / (cam[9:12] @ cam[9:12]) < z, \
        "the ankle link is outside the close-up's frame"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    out = generate()
    if args.check:
        old = np.load(OUT)
        assert set(old.files) == set(out), set(old.files) ^ set(out)
        for k in out:
            assert np.array_equal(old[k], out[k]), k
        print("matches", OUT)
        return
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 500 * 1000, size
    print("wrote %s (%d bytes); worst err32 %.3g" % (OUT, size, max(float(out[n + "/err32"]) for n in out["names"])))


if __name__ == "__main__":
    main()
