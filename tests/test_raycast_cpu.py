"""Ray-cast renderer, host side (no GPU): scene tables, hull half-spaces, the fp64 reference against its fixture, the C ABI
list, and the ``renderer`` keyword's default."""
import copy
import inspect
import os
import re

import numpy as np
import pytest

import render_ref
from deepmimic_mujoco_amd import g1, mjcf, raycast
from deepmimic_mujoco_amd.model import load_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "raycast_cases.npz")


@pytest.fixture(scope="module")
def cases():
    return np.load(FIXTURE)


@pytest.fixture(scope="module")
def scenes():
    hm, gm = load_model(), g1.load_g1_model()[0]
    return {"humanoid3d": (hm, raycast.build_scene(hm)), "unitree_g1": (gm, raycast.build_scene(gm))}


def test_hull_planes_contain_their_vertices_and_counts():
    """After orienting every normal away from mesh_center the 32 hulls are the intersection of their face half-spaces."""
    gm = g1.load_g1_model()[0]
    hulls = mjcf.load_g1_hulls()
    counts, worst, nearest = {}, 0.0, np.inf
    for mid, name in enumerate(gm.mesh_names):
        p = raycast.hull_planes(hulls[name], hulls[name + "__faces"], gm.mesh_center[mid])
        v = np.asarray(hulls[name], np.float64)
        worst = max(worst, float((v @ p[:, :3].T - p[:, 3]).max()))
        nearest = min(nearest, float((p[:, 3] - p[:, :3] @ gm.mesh_center[mid]).min()))
        assert np.allclose(np.linalg.norm(p[:, :3], axis=1), 1.0, atol=1e-12)
        counts[name] = len(p)
    assert len(counts) == 32 and sum(counts.values()) == 78350
    assert worst <= 1e-12 and nearest > 2e-3, (worst, nearest)
    assert max(counts, key=counts.get) == "torso_link" and counts["torso_link"] == 10726
    assert min(counts.values()) == 254 and "ankle" in min(counts, key=counts.get)


def test_build_scene_geoms(scenes):
    hm, hs = scenes["humanoid3d"]
    gm, gs = scenes["unitree_g1"]
    assert hs.ngeom == 16 and sorted(set(hs.geom_type.tolist())) == [0, 2, 3, 6] and hs.nplane == 0
    assert hs.geom_id.tolist() == list(range(16)) and (hs.nq, hs.nbody, hs.njnt) == (35, 14, 29)
    assert gs.ngeom == 47 and np.bincount(gs.geom_type, minlength=8).tolist() == [1, 0, 8, 0, 0, 4, 2, 32]
    assert all(gm.geom_contype[g] != 0 for g in gs.geom_id) and gs.nplane == 78350 == int(gs.geom_planenum.sum())
    assert (gs.nq, gs.nbody, gs.njnt) == (44, 39, 38)
    hull = gs.geom_type == raycast.GEOM_MESH
    assert (gs.geom_planenum[~hull] == 0).all() and (np.diff(gs.geom_planeadr[hull]) == gs.geom_planenum[hull][:-1]).all()
    for s in (hs, gs):
        for name, v in vars(s).items():
            if isinstance(v, np.ndarray):
                assert v.dtype in (np.float32, np.int32) and v.flags.c_contiguous, name
    # colours come from the MJCF: the humanoid's default-class rgba, MuJoCo's built-in grey for the G1's collision geoms,
    # the two `grid` texture colours and the top of the skybox gradient
    assert np.allclose(hs.geom_rgba[1], [0.7, 0.5, 0.3, 1]) and np.allclose(gs.geom_rgba[1], [0.5, 0.5, 0.5, 1])
    assert np.allclose(hs.checker, [[0.1, 0.2, 0.3], [0.2, 0.3, 0.4]]) and np.allclose(gs.sky, [0.4, 0.5, 0.6])
    assert np.allclose(raycast._xml_colours(gm.xml_path)[0][gm.geom_mesh.index("pelvis_contour_link")], [0.2, 0.2, 0.2, 1])   # material only


def test_unsupported_joint_type_raises():
    m = copy.copy(load_model())
    m.jnt_type = m.jnt_type.copy()
    m.jnt_type[3] = 1          # mjJNT_BALL
    with pytest.raises(NotImplementedError):
        raycast.build_scene(m)


def test_camera_convention():
    off, fwd, right, up = raycast.Camera(azimuth=90, elevation=0, distance=2.0, fovy=90).basis(320, 240)
    assert np.allclose(fwd, [0, 1, 0]) and np.allclose(right, [4 / 3, 0, 0]) and np.allclose(up, [0, 0, 1]) and np.allclose(off, [0, -2, 0])
    off, fwd, right, up = raycast.Camera(azimuth=0, elevation=-30).basis(100, 100)
    assert np.allclose(fwd, [np.cos(np.pi / 6), 0, -0.5]) and np.allclose(np.cross(fwd, up), right)   # W = H: both carry tan(fovy / 2)
    cam = raycast.Camera().rows(320, 240, root_x=[0.0, 2.5])
    assert cam.shape == (2, 12) and np.isclose(cam[1, 0] - cam[0, 0], 2.5) and np.allclose(cam[0, 1:], cam[1, 1:])
    assert np.allclose(raycast.Camera(track_root=False).rows(8, 8, root_x=[3.0]), raycast.Camera().rows(8, 8))
    for e in (89.9, -89.9, 120):
        with pytest.raises(ValueError):
            raycast.Camera(elevation=e)


@pytest.mark.parametrize("name", ["h_walk", "g_odd"])
def test_live_reference_reproduces_the_fixture(cases, scenes, name):
    model, scene = scenes[str(cases[name + "/robot"])]
    W, H = cases[name + "/wh"]
    qpos = cases[name + "/qpos"]
    kx, km = render_ref.kinematics(model, scene, qpos[0])
    assert np.array_equal(kx, cases[name + "/kin_xpos"][0]) and np.array_equal(km, cases[name + "/kin_xmat"][0])
    seg, depth, rgb = render_ref.render(scene, kx.astype(np.float32).astype(np.float64), km.astype(np.float32).astype(np.float64),
                                        cases[name + "/cam"][0].astype(np.float64), W, H)
    assert np.array_equal(seg, cases[name + "/seg5"][0, 0])
    hit = seg >= 0
    assert hit.any() and np.abs(depth[hit] - cases[name + "/depth"][0][hit]).max() <= 1e-12 and np.isinf(depth[~hit]).all()
    assert np.array_equal(rgb, cases[name + "/rgb"][0])


def test_fixture_cases_and_unstable_cap(cases):
    names = [str(n) for n in cases["names"]]
    assert set(names) == {"h_qpos0", "h_walk", "h_lying", "g_walk", "g_getup", "h_odd", "g_odd", "h_sky", "g_top", "g_torso", "g_batch"}
    for n in names:
        st = cases[n + "/stable"]
        for e in range(len(st)):
            assert 1.0 - st[e].mean() <= render_ref.MAX_UNSTABLE, (n, e, 1.0 - st[e].mean())
        same = (cases[n + "/seg5"] == cases[n + "/seg5"][0]).all(0)
        assert same[st].all()
    assert (cases["h_sky/seg5"] < 0).all() and cases["h_sky/stable"].all()
    assert tuple(cases["h_odd/wh"]) == (37, 29) == tuple(cases["g_odd/wh"]) and tuple(cases["g_batch/wh"]) == (40, 30)
    assert cases["g_batch/env_ids"].tolist() == [2, 0, 5] and cases["g_batch/qpos"].shape == (8, 44)
    gm = g1.load_g1_model()[0]
    torso = [g for g in range(gm.ngeom) if gm.geom_mesh[g] == "torso_link" and gm.geom_contype[g]][0]
    assert (cases["g_torso/seg5"][0] == torso).mean() > 0.2 and len(np.unique(cases["g_torso/seg5"][0])) >= 2
    assert os.path.getsize(FIXTURE) < 500 * 1000


def test_header_exports_and_library_agree():
    from deepmimic_mujoco_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "deepmimic_render.h")).read()
    declared = set(re.findall(r"\b(dm_render[a-z_0-9]*)\s*\(", hdr))
    assert declared == set(_lib.RENDER_EXPORTS), declared ^ set(_lib.RENDER_EXPORTS)
    L = _lib.load_library()
    for name in declared:
        assert getattr(L, name).argtypes is not None, name
    for k in ("MAX_BODIES", "MAX_GEOMS", "TILE"):
        assert int(re.search(r"#define DM_RENDER_%s (\d+)" % k, hdr).group(1)) == getattr(raycast, k)
    # the ctypes mirror has the header's fields, in its order
    body = re.search(r"typedef struct DmRenderSceneDesc \{(.*?)\} DmRenderSceneDesc;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip(" *") for decl in body.split(";") for f in re.sub(r"^\s*(const\s+)?\w+\s", "", decl.strip()).split(",") if f.strip()]
    fields = [re.sub(r"\[\d+\]", "", f) for f in fields]
    assert fields == [n for n, _ in raycast.DmRenderSceneDesc._fields_]


def test_stick_is_the_default_renderer():
    from deepmimic_mujoco_amd import combined_env, deepmimic_env, vec_env
    classes = [deepmimic_env.DPEnv, deepmimic_env.HipDeepMimicVecEnv, combined_env.DPCombinedEnv, combined_env.HipCombinedVecEnv,
               g1.G1DPEnv, g1.HipG1VecEnv, g1.G1CombinedEnv, g1.HipG1CombinedVecEnv]
    for c in classes:
        assert inspect.signature(c.__init__).parameters["renderer"].default == "stick", c
    assert vec_env.HipBatchEnv.renderer == "stick" and vec_env.HipSingleEnv.renderer == "stick"
    assert vec_env._check_renderer("raycast") == "raycast"
    with pytest.raises(ValueError):
        vec_env._check_renderer("opengl")
    from deepmimic_mujoco_amd.train import build_parser
    assert build_parser().parse_args([]).renderer == "stick" and build_parser().parse_args(["--renderer", "raycast"]).renderer == "raycast"
