"""Numpy reference of the ray-cast renderer (deepmimic_mujoco_amd/raycast.py, csrc/dm_render.hip), written from the
definitions in include/deepmimic_render.h and DESIGN §20, not from the kernel: brute force over every geom and every hull
plane, no bounding spheres, no tiles.  ``dtype=np.float64`` is the reference; ``dtype=np.float32`` runs the same formulas
with every intermediate in float32, which is what the kernel's depth tolerance is derived from.

A pixel is cast five times (centre, and the image-plane offset moved by +-1/64 pixel along each axis); it is *stable* if
the five casts agree in geom id, in depth to 1e-3 relative, and in rgb to 2 levels.
"""
import numpy as np

from deepmimic_mujoco_amd import mjcf, model as hmodel, raycast

SHIFTS = ((0.0, 0.0), (1 / 64, 0.0), (-1 / 64, 0.0), (0.0, 1 / 64), (0.0, -1 / 64))     # (columns, rows), in pixels
PLANE, SPHERE, CAPSULE, CYLINDER, BOX, HULL = 0, 2, 3, 5, 6, 7
PARALLEL2 = 1e-12
MAX_UNSTABLE = 0.02


def kinematics(model, scene, qpos):
    """fp64 (geom_xpos [G, 3], geom_xmat [G, 9]) of the scene's geoms by the project's host kinematics."""
    fk = mjcf.forward_kinematics_general if hasattr(model, "geom_contype") else hmodel.forward_kinematics
    kin = fk(model, np.asarray(qpos, np.float64))
    return kin["geom_xpos"][scene.geom_id], kin["geom_xmat"][scene.geom_id].reshape(-1, 9)


def rays(cam, W, H, dtype, shift=(0.0, 0.0)):
    """unit directions [H * W, 3] of one camera row (eye, forward, right, up)."""
    T = dtype
    cam = np.asarray(cam, T)
    fwd, right, up = cam[3:6], cam[6:9], cam[9:12]
    j, i = np.meshgrid(np.arange(W), np.arange(H))
    u = (T(2) * (j.reshape(-1).astype(T) + T(0.5) + T(shift[0])) / T(W) - T(1))
    v = (T(1) - T(2) * (i.reshape(-1).astype(T) + T(0.5) + T(shift[1])) / T(H))
    d = fwd[None] + u[:, None] * right[None] + v[:, None] * up[None]
    return d / np.sqrt((d * d).sum(1, keepdims=True))


def _sphere(o, d, r):
    b = (o * d).sum(1)
    p = o - b[:, None] * d
    disc = r * r - (p * p).sum(1)
    ok = disc >= 0
    sq = np.sqrt(np.where(ok, disc, 0))
    return ok, -b - sq, -b + sq


def _tube(o, d, r, T):
    a = d[:, 0] ** 2 + d[:, 1] ** 2
    par = a < T(PARALLEL2)
    a_ = np.where(par, T(1), a)
    b = (o[:, 0] * d[:, 0] + o[:, 1] * d[:, 1]) / a_
    px, py = o[:, 0] - b * d[:, 0], o[:, 1] - b * d[:, 1]
    disc = r * r - (px * px + py * py)
    ok = disc >= 0
    sq = np.sqrt(np.where(ok, disc, 0) / a_)
    inside = o[:, 0] ** 2 + o[:, 1] ** 2 <= r * r
    inf = T(np.inf)
    return np.where(par, inside, ok), np.where(par, -inf, -b - sq), np.where(par, inf, -b + sq)


def _slab(o, d, h, T):
    par = d == 0
    d_ = np.where(par, T(1), d)
    a, b = (-h - o) / d_, (h - o) / d_
    inf = T(np.inf)
    return np.where(par, np.abs(o) <= h, True), np.where(par, -inf, np.minimum(a, b)), np.where(par, inf, np.maximum(a, b))


def _primitive(gtype, size, o, d, T):
    """(hit-interval exists [R], t_in, t_out, entry normal [R, 3]) in the geom frame."""
    R = len(o)
    inf = T(np.inf)
    n = np.zeros((R, 3), T)
    if gtype == PLANE:
        ok = (d[:, 2] < 0) & (o[:, 2] > 0)
        n[:, 2] = 1
        return ok, -o[:, 2] / np.where(ok, d[:, 2], T(-1)), np.full(R, inf), n
    if gtype == SPHERE:
        ok, t0, t1 = _sphere(o, d, size[0])
        return ok, t0, t1, (o + t0[:, None] * d) / size[0]
    if gtype == CAPSULE:
        r, hl = size[0], size[1]
        lo, hi = np.full(R, inf), np.full(R, -inf)
        okt, a0, a1 = _tube(o, d, r, T)
        oks, z0, z1 = _slab(o[:, 2], d[:, 2], hl, T)
        a0, a1 = np.maximum(a0, z0), np.minimum(a1, z1)
        use = okt & oks & (a0 <= a1)
        lo, hi = np.where(use, a0, lo), np.where(use, a1, hi)
        for sgn in (T(1), T(-1)):
            c = o.copy()
            c[:, 2] -= sgn * hl
            ok, s0, s1 = _sphere(c, d, r)
            lo, hi = np.where(ok, np.minimum(lo, s0), lo), np.where(ok, np.maximum(hi, s1), hi)
        ok = lo <= hi
        p = o + np.where(ok, lo, T(0))[:, None] * d
        p[:, 2] -= np.clip(p[:, 2], -hl, hl)
        return ok, lo, hi, p / r
    if gtype == CYLINDER:
        okt, a0, a1 = _tube(o, d, size[0], T)
        oks, z0, z1 = _slab(o[:, 2], d[:, 2], size[1], T)
        cap = z0 > a0
        a0f = np.where(np.isfinite(a0), a0, T(0))
        n[:, 0], n[:, 1] = (o[:, 0] + a0f * d[:, 0]) / size[0], (o[:, 1] + a0f * d[:, 1]) / size[0]
        n[cap] = 0
        n[cap, 2] = np.where(d[cap, 2] > 0, T(-1), T(1))
        tin, tout = np.maximum(a0, z0), np.minimum(a1, z1)
        return okt & oks & (tin <= tout), tin, tout, n
    if gtype == BOX:
        ok, tin, tout = np.ones(R, bool), np.full(R, -inf), np.full(R, inf)
        for k in range(3):
            okk, t0, t1 = _slab(o[:, k], d[:, k], size[k], T)
            ok &= okk
            new = t0 > tin if k else np.ones(R, bool)
            tin = np.where(new, t0, tin)
            n[new] = 0
            n[new, k] = np.where(d[new, k] > 0, T(-1), T(1))
            tout = np.minimum(tout, t1)
        return ok & (tin <= tout), tin, tout, n
    raise ValueError(gtype)


def _hull(planes, o, d, T, chunk=2048):
    """Half-space clipping over ALL planes of the hull: t_in = max over n.d < 0, t_out = min over n.d > 0, a plane with
    n.d == 0 and n.o > d_p rejects; the entry normal is the first plane that gave t_in."""
    R = len(o)
    inf = T(np.inf)
    tin, tout, n = np.full(R, -inf), np.full(R, inf), -d.copy()
    rows = np.arange(R)
    for c0 in range(0, len(planes), chunk):
        P = planes[c0:c0 + chunk]
        den = d[:, 0:1] * P[None, :, 0] + d[:, 1:2] * P[None, :, 1] + d[:, 2:3] * P[None, :, 2]
        num = P[None, :, 3] - (o[:, 0:1] * P[None, :, 0] + o[:, 1:2] * P[None, :, 1] + o[:, 2:3] * P[None, :, 2])
        with np.errstate(divide="ignore", invalid="ignore"):
            t = num / den
        cin = np.where(den < 0, t, -inf)
        k = cin.argmax(1)
        val = cin[rows, k]
        new = val > tin
        tin = np.where(new, val, tin)
        n[new] = P[k[new], :3]
        tout = np.minimum(tout, np.where(den > 0, t, inf).min(1))
        tout = np.where(((den == 0) & (num < 0)).any(1), -inf, tout)
    return tin <= tout, tin, tout, n


def cast_rays(scene, geom_xpos, geom_xmat, cam, dirs, dtype=np.float64, ray_chunk=4096):
    """Nearest hit of every ray -> (scene geom index [R] (-1 miss), t [R], world normal [R, 3])."""
    T = dtype
    cam = np.asarray(cam, T)
    eye = cam[0:3]
    planes = scene.planes.astype(T)
    R = len(dirs)
    best, best_g, best_n = np.full(R, T(np.inf)), np.full(R, -1), np.zeros((R, 3), T)
    for g in range(scene.ngeom):
        pos, M = np.asarray(geom_xpos[g], T), np.asarray(geom_xmat[g], T).reshape(3, 3)
        o = np.broadcast_to((eye - pos) @ M, (R, 3)).astype(T)      # M^T (eye - pos)
        d = dirs @ M
        gt = int(scene.geom_type[g])
        if gt == HULL:
            P = planes[scene.geom_planeadr[g]:scene.geom_planeadr[g] + scene.geom_planenum[g]]
            parts = [_hull(P, o[a:a + ray_chunk], d[a:a + ray_chunk], T) for a in range(0, R, ray_chunk)]
            ok, tin, tout, n = (np.concatenate([p[k] for p in parts]) for k in range(4))
        else:
            ok, tin, tout, n = _primitive(gt, scene.geom_size[g].astype(T), o, d, T)
        t = np.maximum(tin, T(0))
        new = ok & (tout > 0) & (t < best)                          # strict: equal t stays with the lower geom
        best, best_g = np.where(new, t, best), np.where(new, g, best_g)
        best_n[new] = n[new] @ M.T
    return best_g, best, best_n


def shade(scene, cam, dirs, g, t, n, dtype=np.float64):
    """(model geom id [R] int, depth along forward [R], rgb [R, 3] uint8)."""
    T = dtype
    cam = np.asarray(cam, T)
    eye, fwd = cam[0:3], cam[3:6]
    hit = g >= 0
    gi = np.where(hit, g, 0)
    col = scene.geom_rgba.astype(T)[gi, :3]
    floor = hit & (scene.geom_type[gi] == PLANE)
    with np.errstate(invalid="ignore"):
        p = eye[None] + np.where(hit, t, T(0))[:, None] * dirs
    par = (np.floor(p[:, 0]).astype(np.int64) + np.floor(p[:, 1]).astype(np.int64)) & 1
    col = np.where(floor[:, None], scene.checker.astype(T)[par], col)
    lam = np.maximum(T(0), n @ scene.light.astype(T))
    c = col * (T(raycast.AMBIENT) + T(raycast.DIFFUSE) * lam)[:, None]
    c = np.where(hit[:, None], c, scene.sky.astype(T)[None])
    rgb = np.floor(np.clip(c, 0, 1) * T(255) + T(0.5)).astype(np.uint8)
    depth = np.where(hit, t * (dirs @ fwd), T(np.inf))
    return np.where(hit, scene.geom_id[gi], -1), depth, rgb


def render(scene, geom_xpos, geom_xmat, cam, W, H, dtype=np.float64, shift=(0.0, 0.0)):
    """One frame -> (segmentation [H, W] int32, depth [H, W] dtype, rgb [H, W, 3] uint8)."""
    dirs = rays(cam, W, H, dtype, shift)
    g, t, n = cast_rays(scene, geom_xpos, geom_xmat, cam, dirs, dtype)
    seg, depth, rgb = shade(scene, cam, dirs, g, t, n, dtype)
    return seg.reshape(H, W).astype(np.int32), depth.reshape(H, W), rgb.reshape(H, W, 3)


def render5(scene, geom_xpos, geom_xmat, cam, W, H):
    """The five fp64 casts of a frame -> (seg5 [5, H, W], depth5, rgb5, stable [H, W] bool)."""
    outs = [render(scene, geom_xpos, geom_xmat, cam, W, H, np.float64, s) for s in SHIFTS]
    seg5, dep5, rgb5 = (np.stack([o[k] for o in outs]) for k in range(3))
    same = (seg5 == seg5[0]).all(0)
    miss = seg5[0] < 0
    with np.errstate(invalid="ignore"):
        dep_ok = miss | (dep5.max(0) - dep5.min(0) <= 1e-3 * dep5.min(0))
    rgb_ok = (rgb5.max(0).astype(int) - rgb5.min(0).astype(int)).max(-1) <= 2
    return seg5, dep5, rgb5, same & dep_ok & rgb_ok
