"""Ray-cast renderer: rgb, depth and segmentation frames of either robot, computed on the device (csrc/dm_render.hip).

The reference renders through mujoco-py's OpenGL viewer (``render(mode="rgb_array")``, src/deepmimic_env.py:527,
src/combined_env.py:507-517).  Here a frame is cast from ``qpos`` alone: :func:`build_scene` flattens a compiled model
(``model.compile_mjcf`` humanoid3d or ``mjcf.compile_mjcf_general`` G1) into engine-independent float32 / int32 tables —
body tree, the collision geoms with their colours, one half-space per hull triangle — and :class:`RayRenderer` uploads
them once and runs the two kernels (own forward kinematics, then one workgroup per 16 x 16 pixel tile).  What is drawn is
the collision geometry (the G1's visual meshes have no triangles in the model), Lambert-shaded by one directional light,
over a 1 m checker floor and a flat sky.  DESIGN §20.
"""
from __future__ import annotations

import ctypes as C
import os
import xml.etree.ElementTree as ET

import numpy as np

from .model import ASSET_DIR, quat_to_mat

GEOM_PLANE, GEOM_SPHERE, GEOM_CAPSULE, GEOM_CYLINDER, GEOM_BOX, GEOM_MESH = 0, 2, 3, 5, 6, 7
JNT_FREE, JNT_HINGE = 0, 3
MAX_BODIES, MAX_GEOMS = 64, 256          # DM_RENDER_MAX_BODIES / DM_RENDER_MAX_GEOMS (include/deepmimic_render.h)
TILE = 16
LIGHT_DIR = np.array([0.2, -0.6, 0.75]) / np.linalg.norm([0.2, -0.6, 0.75])     # towards the light, world frame
AMBIENT, DIFFUSE = 0.35, 0.65
_DEFAULT_RGBA = (0.5, 0.5, 0.5, 1.0)     # MuJoCo's built-in geom rgba [EXT]


class Scene:
    """Flat tables of one model; every array is C-contiguous float32 or int32 (attribute names as DmRenderSceneDesc)."""

    def geom_index(self, model_geom_id):
        return int(np.nonzero(self.geom_id == model_geom_id)[0][0])


def _xml_colours(xml_path):
    """(rgba per <geom> in document order of the body tree, checker colours [2, 3], sky colour [3]) of an MJCF file."""
    root = ET.parse(xml_path).getroot()
    classes = {"main": None}

    def visit(node, parent):
        name = node.get("class", "main")
        g = node.find("geom")
        own = {k: g.get(k) for k in ("rgba", "material") if g is not None and g.get(k) is not None}
        merged = dict(classes.get(parent) or {})
        merged.update(own)
        classes[name] = merged
        for child in node.findall("default"):
            visit(child, name)
    for d in root.findall("default"):
        visit(d, "main")
    classes["main"] = classes["main"] or {}
    materials, textures, sky = {}, {}, None
    for a in root.findall("asset"):
        for t in a.findall("texture"):
            textures[t.get("name", "")] = t
            if t.get("type") == "skybox":
                sky = [float(v) for v in t.get("rgb1", "0 0 0").split()]
        for m in a.findall("material"):
            materials[m.get("name")] = m
    grid = textures.get("grid")
    checker = [[float(v) for v in grid.get(k).split()] for k in ("rgb1", "rgb2")] if grid is not None else [[0.2] * 3, [0.3] * 3]
    out = []

    def walk(e, cls):
        cls = e.get("childclass", cls)
        for g in e.findall("geom"):
            a = dict(classes[g.get("class", cls)])
            a.update({k: g.get(k) for k in ("rgba", "material") if g.get(k) is not None})
            if "rgba" in a:
                rgba = [float(v) for v in a["rgba"].split()]
            elif a.get("material") in materials and materials[a["material"]].get("rgba") is not None:
                rgba = [float(v) for v in materials[a["material"]].get("rgba").split()]
            else:
                rgba = list(_DEFAULT_RGBA)
            out.append(rgba)
        for c in e.findall("body"):
            walk(c, cls)
    walk(root.find("worldbody"), "main")
    return np.array(out, float), np.array(checker, float), np.array(sky if sky is not None else [0.4, 0.5, 0.6], float)


def hull_planes(verts, faces, center):
    """[F, 4] float64 (nx, ny, nz, d): one half-space n.x <= d per triangle, each normal oriented away from ``center`` (the
    asset's winding is not consistent, so the vertex order is not trusted)."""
    v = np.asarray(verts, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    n = np.cross(b - a, c - a)
    ln = np.linalg.norm(n, axis=1)
    if not np.all(ln > 0):
        raise ValueError("degenerate hull triangle")
    n /= ln[:, None]
    d = np.einsum("ij,ij->i", n, a)
    flip = n @ np.asarray(center, np.float64) > d
    n[flip], d[flip] = -n[flip], -d[flip]
    return np.concatenate([n, d[:, None]], axis=1)


def build_scene(model, hulls=None):
    """Compiled model (humanoid3d ``CompiledModel`` or G1 ``GModel``) -> :class:`Scene`.  Rendered geoms: the floor plane and
    every geom with ``contype != 0``; a geom's ``geom_id`` is the model's own geom index (the segmentation value)."""
    f32, i32 = np.float32, np.int32
    general = hasattr(model, "geom_contype")
    nbody, njnt, ngeom_model = len(model.body_parent), len(model.jnt_type), len(model.geom_type)
    jt = np.asarray(model.jnt_type)
    if not np.all((jt == JNT_FREE) | (jt == JNT_HINGE)):
        raise NotImplementedError("the renderer's kinematics know free and hinge joints only (got types %s)" % sorted(set(jt.tolist())))
    if nbody > MAX_BODIES:
        raise ValueError("more than %d bodies" % MAX_BODIES)
    xml_path = getattr(model, "xml_path", None) or os.path.join(
        ASSET_DIR, "deepmimic_unitree_g1.xml" if general else "deepmimic_humanoid3d.xml")
    rgba_all, checker, sky = _xml_colours(xml_path)
    if len(rgba_all) != ngeom_model:
        raise ValueError("%s has %d geoms, the model %d" % (xml_path, len(rgba_all), ngeom_model))
    contype = np.asarray(model.geom_contype) if general else np.ones(ngeom_model, int)
    sel = [g for g in range(ngeom_model) if contype[g] != 0 or model.geom_type[g] == GEOM_PLANE]
    if len(sel) > MAX_GEOMS:
        raise ValueError("more than %d rendered geoms" % MAX_GEOMS)

    s = Scene()
    s.nq, s.nbody, s.njnt, s.ngeom = len(model.qpos0), nbody, njnt, len(sel)
    s.body_parent = np.ascontiguousarray(model.body_parent, i32)
    s.body_jntadr = np.ascontiguousarray(model.body_jntadr, i32)
    s.body_jntnum = np.ascontiguousarray(model.body_jntnum, i32)
    s.body_pos = np.ascontiguousarray(model.body_pos, f32)
    s.body_quat = np.ascontiguousarray(model.body_quat, f32)
    s.jnt_type = np.ascontiguousarray(jt, i32)
    s.jnt_qposadr = np.ascontiguousarray(model.jnt_qposadr, i32)
    s.jnt_axis = np.ascontiguousarray(model.jnt_axis, f32)
    s.jnt_pos = np.ascontiguousarray(model.jnt_pos, f32)                        # the anchor, body frame
    s.jnt_ref = np.ascontiguousarray(np.asarray(model.qpos0)[s.jnt_qposadr], f32)   # a hinge turns by qpos - ref
    s.geom_id = np.array(sel, i32)
    s.geom_body = np.ascontiguousarray(np.asarray(model.geom_body)[sel], i32)
    s.geom_type = np.ascontiguousarray(np.asarray(model.geom_type)[sel], i32)
    s.geom_pos = np.ascontiguousarray(np.asarray(model.geom_pos)[sel], f32)
    s.geom_quat = np.ascontiguousarray(np.asarray(model.geom_quat)[sel], f32)
    s.geom_size = np.ascontiguousarray(np.asarray(model.geom_size)[sel], f32)
    s.geom_rbound = np.ascontiguousarray(np.asarray(model.geom_rbound)[sel], f32)
    s.geom_rgba = np.ascontiguousarray(rgba_all[sel], f32)
    s.geom_planeadr, s.geom_planenum = np.zeros(len(sel), i32), np.zeros(len(sel), i32)
    planes, adr = [], 0
    if np.any(s.geom_type == GEOM_MESH):
        if hulls is None:
            from .mjcf import load_g1_hulls
            hulls = load_g1_hulls()
        for k, g in enumerate(sel):
            if model.geom_type[g] != GEOM_MESH:
                continue
            mid = int(model.geom_meshid[g])
            name = model.mesh_names[mid]
            p = hull_planes(hulls[name], hulls[name + "__faces"], model.mesh_center[mid])
            s.geom_planeadr[k], s.geom_planenum[k] = adr, len(p)
            planes.append(p)
            adr += len(p)
    s.nplane = adr
    s.planes = np.ascontiguousarray(np.concatenate(planes) if planes else np.zeros((0, 4)), f32)
    s.checker = np.ascontiguousarray(checker, f32)
    s.sky = np.ascontiguousarray(sky, f32)
    s.light = np.ascontiguousarray(LIGHT_DIR, f32)
    return s


class Camera:
    """MuJoCo's free-camera convention [EXT mjv_updateCamera]: the camera looks at ``lookat`` from ``distance`` away, ``azimuth``
    degrees about +z from +x, ``elevation`` degrees above the horizontal (negative looks down).  ``track_root`` adds ``qpos[:, 0]``
    to ``lookat[0]`` (src/combined_env.py:517).  The defaults are this project's: ``mjModel.stat.extent`` is not computed here,
    so the reference's ``distance = extent * 0.3`` is not reproduced."""

    def __init__(self, lookat=(0.0, 0.0, 0.9), distance=4.0, azimuth=90.0, elevation=-20.0, fovy=45.0, track_root=True):
        if abs(float(elevation)) >= 89.9:
            raise ValueError("|elevation| must be below 89.9 degrees")
        self.lookat, self.distance, self.azimuth, self.elevation = tuple(float(v) for v in lookat), float(distance), float(azimuth), float(elevation)
        self.fovy, self.track_root = float(fovy), bool(track_root)

    def basis(self, width, height):
        """float64 (offset [3], forward [3], right [3], up [3]): eye = lookat + offset; right and up carry the tan(fovy / 2) scale."""
        a, e = np.deg2rad(self.azimuth), np.deg2rad(self.elevation)
        fwd = np.array([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)])
        up = np.array([-np.sin(e) * np.cos(a), -np.sin(e) * np.sin(a), np.cos(e)])
        right = np.array([np.sin(a), -np.cos(a), 0.0])
        th = np.tan(np.deg2rad(self.fovy) / 2)
        return -self.distance * fwd, fwd, right * th * width / height, up * th

    def rows(self, width, height, root_x=None):
        """float64 [n, 12] camera rows (eye, forward, right, up) for ``root_x`` [n] (or one row without it)."""
        off, fwd, right, up = self.basis(width, height)
        root_x = np.zeros(1) if root_x is None else np.asarray(root_x, float)
        cam = np.tile(np.concatenate([np.asarray(self.lookat) + off, fwd, right, up]), (len(root_x), 1))
        if self.track_root:
            cam[:, 0] += root_x
        return cam


class DmRenderSceneDesc(C.Structure):
    """include/deepmimic_render.h: DmRenderSceneDesc (host pointers, copied by dm_render_create)"""
    _fields_ = [("nq", C.c_int32), ("nbody", C.c_int32), ("njnt", C.c_int32), ("ngeom", C.c_int32), ("nplane", C.c_int32),
                ("device", C.c_int32)] + [(n, C.c_void_p) for n in (
                    "body_parent", "body_jntadr", "body_jntnum", "body_pos", "body_quat",
                    "jnt_type", "jnt_qposadr", "jnt_axis", "jnt_pos", "jnt_ref",
                    "geom_id", "geom_body", "geom_type", "geom_planeadr", "geom_planenum",
                    "geom_pos", "geom_quat", "geom_size", "geom_rbound", "geom_rgba", "planes")] + [
                    ("checker", C.c_float * 6), ("sky", C.c_float * 3), ("light", C.c_float * 3),
                    ("ambient", C.c_float), ("diffuse", C.c_float)]


def scene_desc(scene, device=0):
    """DmRenderSceneDesc pointing into ``scene``'s arrays (the scene must outlive the call that reads it)."""
    d = DmRenderSceneDesc()
    d.nq, d.nbody, d.njnt, d.ngeom, d.nplane, d.device = scene.nq, scene.nbody, scene.njnt, scene.ngeom, scene.nplane, device
    for name, ctype in DmRenderSceneDesc._fields_:
        if ctype is C.c_void_p:
            setattr(d, name, getattr(scene, name).ctypes.data)
    d.checker[:] = scene.checker.reshape(-1).tolist()
    d.sky[:] = scene.sky.tolist()
    d.light[:] = scene.light.tolist()
    d.ambient, d.diffuse = AMBIENT, DIFFUSE
    return d


class RayRenderer:
    """Device renderer of one model.  No CPU fallback: without the HIP library or a GPU the constructor raises."""

    def __init__(self, model, device=0):
        import torch
        from ._lib import load_library
        if not torch.cuda.is_available():
            raise RuntimeError("RayRenderer needs an MI355X (torch.cuda.is_available() is False); there is no CPU fallback")
        self.torch, self.L = torch, load_library()
        self.scene = build_scene(model)
        self.device = torch.device("cuda", device)
        self.h = C.c_void_p()
        rc = self.L.dm_render_create(C.byref(scene_desc(self.scene, device)), C.byref(self.h))
        if rc != 0:
            raise RuntimeError("dm_render_create failed (%d): %s" % (rc, (self.L.dm_render_last_error(None) or b"").decode()))
        self.G = self.scene.ngeom

    def close(self):
        if getattr(self, "h", None):
            self.L.dm_render_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, name, *args):
        t = self.torch
        args = [None if a is None else C.c_void_p(a.data_ptr()) if isinstance(a, t.Tensor) else a for a in args]
        rc = getattr(self.L, name)(self.h, *args, C.c_void_p(t.cuda.current_stream(self.device).cuda_stream))
        if rc != 0:
            raise RuntimeError("%s failed (%d): %s" % (name, rc, (self.L.dm_render_last_error(self.h) or b"").decode()))

    def _ids(self, env_ids, qpos):
        t = self.torch
        assert qpos.dtype == t.float32 and qpos.is_contiguous() and qpos.dim() == 2 and qpos.shape[1] == self.scene.nq
        if env_ids is None:
            return None, qpos.shape[0]
        ids = t.as_tensor(env_ids, device=self.device).to(t.int32).contiguous()
        return ids, ids.numel()

    def outputs(self, n, width, height, rgb=True, depth=False, segmentation=False):
        t, d = self.torch, self.device
        return dict(rgb=t.empty(n, height, width, 3, dtype=t.uint8, device=d) if rgb else None,
                    depth=t.empty(n, height, width, dtype=t.float32, device=d) if depth else None,
                    segmentation=t.empty(n, height, width, dtype=t.int32, device=d) if segmentation else None)

    def kinematics(self, qpos, env_ids=None):
        """dm_render_kinematics: (geom_xpos [n, G, 3], geom_xmat [n, G, 9]) of the listed rows of ``qpos`` (all without a list)."""
        ids, n = self._ids(env_ids, qpos)
        xpos, xmat = (self.torch.empty(n, self.G, k, device=self.device) for k in (3, 9))
        self._call("dm_render_kinematics", qpos, ids, n, xpos, xmat)
        return xpos, xmat

    def cast(self, geom_xpos, geom_xmat, cam, width, height, rgb=True, depth=False, segmentation=False):
        """dm_render_cast on given geom poses; ``cam`` float32 [n, 12] device tensor."""
        n = geom_xpos.shape[0]
        assert geom_xpos.shape == (n, self.G, 3) and geom_xmat.shape == (n, self.G, 9) and cam.shape == (n, 12)
        assert all(x.dtype == self.torch.float32 and x.is_contiguous() for x in (geom_xpos, geom_xmat, cam))
        out = self.outputs(n, width, height, rgb, depth, segmentation)
        self._call("dm_render_cast", geom_xpos, geom_xmat, n, cam, int(width), int(height), out["rgb"], out["depth"], out["segmentation"])
        return {k: v for k, v in out.items() if v is not None}

    def camera_rows(self, camera, qpos, ids, width, height):
        """float32 [n, 12] device tensor of ``camera`` for the listed envs, made with torch ops (no host sync)."""
        t = self.torch
        base = t.tensor(camera.rows(width, height)[0], dtype=t.float32, device=self.device)
        n = qpos.shape[0] if ids is None else ids.numel()
        cam = base.repeat(n, 1)
        if camera.track_root:
            cam[:, 0] += qpos[:, 0] if ids is None else qpos[ids.long(), 0]
        return cam

    def render(self, qpos, camera=None, width=320, height=240, env_ids=None, rgb=True, depth=False, segmentation=False,
               workspace=None, out=None, cam=None):
        """dm_render: kinematics and cast in one call -> dict of device tensors (``rgb`` uint8 [n, H, W, 3], ``depth`` float32
        [n, H, W], ``segmentation`` int32 [n, H, W]); nothing is synchronised.  ``workspace`` (float32, n * G * 12), ``out``
        (from :meth:`outputs`) and ``cam`` may be passed in, which makes the call capturable into a hipGraph."""
        ids, n = self._ids(env_ids, qpos)
        if cam is None:
            cam = self.camera_rows(camera or Camera(), qpos, ids, width, height)
        if workspace is None:
            workspace = self.torch.empty(n * self.G * 12, device=self.device)
        assert workspace.numel() >= n * self.G * 12 and workspace.dtype == self.torch.float32
        out = out or self.outputs(n, width, height, rgb, depth, segmentation)
        self._call("dm_render", qpos, ids, n, cam, int(width), int(height), out.get("rgb"), out.get("depth"), out.get("segmentation"),
                   workspace)
        return {k: v for k, v in out.items() if v is not None}
