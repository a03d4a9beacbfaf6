#!/usr/bin/env python
"""Writes tests/golden/g1_pair_cover.npz: Unitree G1 poses that between them put (nearly) every collision pair of the model into
contact, with the fp64 oracle's answer for each.  tests/test_g1_pair_cover_cpu.py re-derives every stored number on the oracle;
tests/test_g1_pair_cover_gpu.py holds the HIP narrowphase (csrc/dm_g1_narrow.h) to them.  CPU only, seeded, about ten minutes on one
core:

    python tests/golden/make_g1_pair_cover.py            # writes tests/golden/g1_pair_cover.npz
    python tests/golden/make_g1_pair_cover.py --check    # regenerates and compares with the committed file

Search.  (1) Blind: free flight at z = 1.5 m and poses over the floor (base at 0.2 .. 0.8 m), joints uniform over jnt_range, the
floor poses over a random fraction of it.  (2) For every pair that (1) touched fewer than twice, a descent on the distance of the
two geom centres (geom_xpos; the bounding radii only shift that number, they give the reported gap), moving only the joints that
lie on one of the two kinematic chains and not on both, with a step that shrinks from 0.4 to 0.004 rad.  The first touching pose
is the shallow state; the descent then goes on in the pair's own contact distance for a deep one.  The accepted poses form the
path: the near-miss twin of an MPR pair is the touching pose backed off along the last segment of that path until the oracle
reports no contact for the pair, the centres still inside the bounding-sphere filter.

A state is kept only if it is float32-exact, has fewer than 48 contacts and 256 rows (by count, on a sim whose caps are 200 / 500),
keeps every limited joint 1e-4 rad inside its range, and leaves the ordered (geom1, geom2) contact list unchanged under 8 seeded
perturbations of qpos by +-1e-6 per coordinate (quaternion re-normalised); and if the oracle's contact geometry is well defined
there: under 6 perturbations of 1e-12 no contact moves by more than a tenth of the GPU test's bounds (conditioned() says why
MPR's answer sometimes is not).

Selection.  Greedy weighted set cover: a state's worth is the number of pairs it touches that are still wanted, per byte it costs
in the file; a state that is the shallowest or the deepest the search has for a pair counts half a unit more for it.  Level 1
takes every reached pair once (a descent's first touching pose for the pairs only a descent reached: it carries the twin).
Level 2 wants every pair in a second state and spends what is left of BYTE_BUDGET on it: first the deepest pose of every pair of
the ten small classes, then the cheapest second states per pair.  (Taking the shallowest and the deepest state of every pair
outright would need some 1400 states; the fixture has to stay under the largest one already in tests/golden/.)

Arrays.  qpos [n, 44] float32; kind [n] (0 blind free flight, 1 blind over the floor, 2 descent, 3 near-miss twin); the oracle's
ncon, nefc, nlimit, xpos [n, 39, 3] and qacc (float32, for information); its contacts of all states in a row, state i owning
con_start[i] : con_start[i + 1] of con_geom [.., 2], con_dist, con_pos, con_normal (float64); covered / uncovered [.., 2] pair
lists and uncovered_gap (the smallest centre distance minus bounding radii the search saw, for a floor pair height minus
bounding radius); twins [.., 4] = (twin state, touching partner state, geom1, geom2); ill_qpos [.., 44]: the candidates that
conditioned() refused (stable contact list, but the oracle's own contact geometry moves under 1e-12); seed.
"""
import argparse, os, sys, time
import ctypes as C

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "g1_pair_cover.npz")
SEED = 7
MAXCON, MAXROW = 48, 256            # the HIP engine's caps (deepmimic_mujoco_amd.g1.MAXCON / MAXROW)
LIMIT_MARGIN, NPERT, PERT = 1e-4, 8, 1e-6
NCOND, COND_PERT, COND_TOL = 6, 1e-12, (1e-7, 1e-6, 1e-6)     # distance, position, normal: a tenth of the GPU test's bounds
MIN_PAIRS, MIN_TWINS, MAX_TWINS = 740, 32, 40
MAX_BYTES = 789005                  # tests/golden/step_paths_bits.npz, the largest fixture before this one
BYTE_BUDGET = 880000                # what the selection spends: STATE_BYTES per state, CON_BYTES per contact, as stored (the file compresses to about 0.86 of it)
STATE_BYTES, CON_BYTES = 44 * 4 + 117 * 8 + 43 * 4 + 17, 2 * 2 + 7 * 8
TYPE_NAME = {0: "plane", 2: "sphere", 5: "cylinder", 6: "box", 7: "mesh"}
CLASSES = ["plane-mesh", "plane-cylinder", "plane-sphere", "plane-box", "mesh-mesh", "cylinder-mesh", "sphere-mesh", "box-mesh",
           "sphere-cylinder", "cylinder-cylinder", "cylinder-box", "sphere-sphere", "sphere-box", "box-box"]


def type_class(g, g1, g2):
    """Name of the geom-type class of a pair, one of CLASSES (the two type names in the model's order of types)."""
    return "%s-%s" % (TYPE_NAME[int(g.geom_type[g1])], TYPE_NAME[int(g.geom_type[g2])])


def is_mpr(g, g1, g2):
    """pair_class(t1, t2) == 2 of csrc/dm_g1_narrow.h: everything that is neither plane-x, sphere-sphere, sphere-box nor box-box."""
    t1, t2 = int(g.geom_type[g1]), int(g.geom_type[g2])
    return not (t1 == 0 or (t1 == 2 and t2 in (2, 6)) or (t1 == 6 and t2 == 6))


def perturbation(k):
    """The k-th of the NPERT seeded perturbations: +-PERT on every coordinate of qpos."""
    return np.random.default_rng([SEED, 1000 + k]).choice([-PERT, PERT], 44)


def perturbed(q32, k):
    q = np.asarray(q32, np.float32).astype(np.float64) + perturbation(k)
    q[3:7] /= np.linalg.norm(q[3:7])
    return q


class Oracle:
    """One G1Sim at the oracle's own caps (200 contacts, 500 rows), so that ncon and nefc are true counts."""

    def __init__(self):
        from oracle import oracle_g1 as og
        self.og = og
        self.g, _ = og.g1_model()
        self.s = og.G1Sim()
        self.buf = np.zeros(200 * 17)
        self.gx = np.zeros(94 * 3)
        self.zero = np.zeros(43)
        self.nev = 0

    def __call__(self, q, want_xpos=False):
        """(contacts [ncon, 17], nefc, geom_xpos or None) of qpos q (zero velocity, zero warm start)."""
        s, L = self.s, self.s.L
        self.nev += 1
        s.set("qacc_warmstart", self.zero)
        rc = s.set_state(np.asarray(q, np.float64), self.zero)
        assert rc == 0, rc
        n = L.dmo_get(s.d, b"contact", self.buf.ctypes.data_as(C.c_void_p), self.buf.size)
        assert n >= 0
        c = self.buf[:n].reshape(-1, 17).copy()
        gx = None
        if want_xpos:
            L.dmo_get(s.d, b"geom_xpos", self.gx.ctypes.data_as(C.c_void_p), self.gx.size)
            gx = self.gx.reshape(94, 3).copy()
        return c, s.geti("nefc"), gx


def pair_list(c):
    return [(int(r[13]), int(r[14])) for r in c]


def limits_ok(g, q):
    lo, hi = g.jnt_range[1:, 0], g.jnt_range[1:, 1]
    lim = np.asarray(g.jnt_limited[1:], bool)
    x = np.asarray(q, np.float64)[7:]
    return bool(np.all(~lim | ((x - lo >= LIMIT_MARGIN) & (hi - x >= LIMIT_MARGIN))))


def uncut(c, nefc):
    return len(c) < MAXCON and nefc < MAXROW


def stable(ora, q32):
    """The ordered contact pair list survives the NPERT perturbations, and every perturbed pose is uncut too."""
    c0, nefc, _ = ora(q32.astype(np.float64))
    if not uncut(c0, nefc):
        return False
    p0 = pair_list(c0)
    for k in range(NPERT):
        c, nefc, _ = ora(perturbed(q32, k))
        if pair_list(c) != p0 or not uncut(c, nefc):
            return False
    return True


def conditioned(ora, q32):
    """The oracle's own answer is well defined here: under NCOND seeded perturbations of qpos at rounding level (+-COND_PERT per
    coordinate) no contact moves by more than a tenth of what the GPU test allows the engine.  MPR stops when the portal is
    within 1e-6 of the surface; where a curved side of radius r (a 15 mm cylinder) carries the contact that leaves the normal
    free by sqrt(2e-6 / r) ~ 1e-2, and which of the admissible portals it stops on can hang on the last bit of the input."""
    q = np.asarray(q32, np.float32).astype(np.float64)
    c0, _, _ = ora(q)
    for k in range(NCOND):
        c, _, _ = ora(q + np.random.default_rng([SEED, 2000 + k]).choice([-COND_PERT, COND_PERT], 44))
        if pair_list(c) != pair_list(c0):
            return False
        if len(c0) and (np.abs(c[:, 0] - c0[:, 0]).max() > COND_TOL[0] or np.abs(c[:, 1:4] - c0[:, 1:4]).max() > COND_TOL[1]
                        or np.abs(c[:, 4:7] - c0[:, 4:7]).max() > COND_TOL[2]):
            return False
    return True


def chain(g, body):
    """Hinge joints between `body` and the root body."""
    js = set()
    while body > 0:
        a, n = int(g.body_jntadr[body]), int(g.body_jntnum[body])
        js.update(j for j in range(a, a + n) if int(g.jnt_type[j]) == 3)
        body = int(g.body_parent[body])
    return js


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-o", "--out", default=OUT)
    ap.add_argument("--check", action="store_true", help="write nothing; compare the regenerated arrays with --out")
    ap.add_argument("--blind", type=int, default=12000)
    ap.add_argument("--tries", type=int, default=250)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    t0 = time.time()
    ora = Oracle()
    g = ora.g
    rng = np.random.default_rng(SEED)
    pairs = [(int(p[0]), int(p[1])) for p in g.pairs]
    pid = {p: i for i, p in enumerate(pairs)}
    npair = len(pairs)
    lo, hi = np.array(g.jnt_range[1:, 0]), np.array(g.jnt_range[1:, 1])
    assert np.all(np.asarray(g.jnt_limited[1:]) == 1) and np.all(np.asarray(g.jnt_type[1:]) == 3)
    m = 1e-3                                    # sampled joints stay this far inside the range (float32 rounding included)
    rad = np.where(np.asarray(g.geom_type) == 2, np.asarray(g.geom_size)[:, 0], np.asarray(g.geom_rbound))

    def search():
        # ------------------------------------------------------------------------------------------------ pool of candidate states
        index = {}
        Q, KIND, PAIRS, DEPTH, NCON = [], [], [], [], []       # per candidate: qpos f32, kind, pair ids (set), {pair id: min dist}, ncon

        def add(q32, c, kind):
            key = q32.tobytes()
            if key in index:            # a descent that starts on a touching pose, or a step clipped back onto its start
                return index[key]
            index[key] = len(Q)
            dep = {}
            for r in c:
                p = pid[(int(r[13]), int(r[14]))]
                dep[p] = min(dep.get(p, 0.0), r[0])
            Q.append(q32); KIND.append(kind); PAIRS.append(set(dep)); DEPTH.append(dep); NCON.append(len(c))
            return len(Q) - 1

        def quat():
            x = rng.normal(size=4)
            return x / np.linalg.norm(x)

        # ------------------------------------------------------------------------------------------------ (1) blind sampling
        best_gap = np.full(npair, np.inf)
        plane_pairs = [p for p in range(npair) if int(g.geom_type[pairs[p][0]]) == 0]
        GX = []                 # geom_xpos of the free-flight samples: where the descents start
        GXI = []
        for i in range(a.blind):
            q = np.zeros(44)
            floor = i % 5 >= 3
            q[3:7] = quat()
            if floor:
                q[2] = rng.uniform(0.2, 0.8)
                f = rng.uniform(0.2, 1.0)
                mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo) - m
                q[7:] = mid + f * half * rng.uniform(-1, 1, 37)
            else:
                q[2] = 1.5
                q[7:] = rng.uniform(lo + m, hi - m)
            q32 = q.astype(np.float32)
            c, nefc, gx = ora(q32.astype(np.float64), want_xpos=True)
            if floor:                                       # the floor is the plane z = 0: what the pairs with it came down to
                for p in plane_pairs:
                    best_gap[p] = min(best_gap[p], gx[pairs[p][1], 2] - rad[pairs[p][1]])
            if not uncut(c, nefc) or not limits_ok(g, q32):
                continue
            k = add(q32, c, 1 if floor else 0)
            if not floor:
                GX.append(gx.astype(np.float32)); GXI.append(k)
        GX = np.array(GX)
        hits = np.zeros(npair, int)
        for ps in PAIRS:
            for p in ps:
                hits[p] += 1
        print("blind: %d samples, %d usable, %d pairs touched, %d at least twice (%.0f s)" % (
            a.blind, len(Q), (hits > 0).sum(), (hits > 1).sum(), time.time() - t0), flush=True)

        # ------------------------------------------------------------------------------------------------ (2) descent per missing pair
        descent = {}            # pair id -> (shallow candidate, deep candidate, previous pose on the path)
        for p in np.nonzero(hits < 2)[0]:
            g1, g2 = pairs[p]
            t1 = int(g.geom_type[g1])
            b1, b2 = int(g.geom_body[g1]), int(g.geom_body[g2])
            J = sorted(chain(g, b1) ^ chain(g, b2))
            if t1 == 0 or not J:
                continue        # plane pairs are the blind floor samples' business
            qa = np.array([int(g.jnt_qposadr[j]) for j in J])
            jl, jh = lo[qa - 7] + m, hi[qa - 7] - m
            rsum = rad[g1] + rad[g2]
            tries = a.tries * (6 if rsum < 0.01 else 1)
            cd = np.linalg.norm(GX[:, g1] - GX[:, g2], axis=1)
            order = np.argsort(cd)
            found = None
            for start in order[:2]:
                q = Q[GXI[start]].astype(np.float64)
                d = np.inf
                for t in range(tries):
                    step = 0.4 * (0.01 ** (t / tries))
                    qn = q.copy()
                    if t:
                        mask = rng.random(len(qa)) < 0.6
                        if not mask.any():
                            mask[rng.integers(len(qa))] = True
                        qn[qa] = np.clip(qn[qa] + step * rng.normal(size=len(qa)) * mask, jl, jh)
                    q32 = qn.astype(np.float32)
                    c, nefc, gx = ora(q32.astype(np.float64), want_xpos=True)
                    dn = np.linalg.norm(gx[g1] - gx[g2])
                    best_gap[p] = min(best_gap[p], dn - rsum)
                    touch = [r[0] for r in c if (int(r[13]), int(r[14])) == (g1, g2)]
                    if touch and uncut(c, nefc) and limits_ok(g, q32):
                        found = (q32, c, min(touch), q.astype(np.float32) if t else None)
                        break
                    if dn < d and not touch:
                        q, d = q32.astype(np.float64), dn
                if found:
                    break
            if not found:
                continue
            q32, c, dist0, prev = found
            shallow = add(q32, c, 2)
            # go on in the pair's own contact distance: the deep state
            q, dbest, deep = q32.astype(np.float64), dist0, shallow
            for t in range(40):
                step = min(0.05, rsum) * (0.1 ** (t / 40))           # 1 mm spheres: a millimetre at arm's length
                qn = q.copy()
                qn[qa] = np.clip(qn[qa] + step * rng.normal(size=len(qa)), jl, jh)
                q32 = qn.astype(np.float32)
                c, nefc, _ = ora(q32.astype(np.float64))
                touch = [r[0] for r in c if (int(r[13]), int(r[14])) == (g1, g2)]
                if touch and uncut(c, nefc) and limits_ok(g, q32):          # every touching pose is a candidate, the deeper ones move on
                    k = add(q32, c, 2)
                    if min(touch) < dbest:
                        q, dbest, deep = q32.astype(np.float64), min(touch), k
            best_gap[p] = dbest
            descent[p] = (shallow, deep, prev)
        hits[:] = 0
        for ps in PAIRS:
            for p in ps:
                hits[p] += 1
        print("descent: %d pairs reached, pool %d states, %d pairs touched (%.0f s, %d evaluations)" % (
            len(descent), len(Q), (hits > 0).sum(), time.time() - t0, ora.nev), flush=True)
        return Q, KIND, PAIRS, DEPTH, NCON, GX, hits, best_gap, descent

    Q, KIND, PAIRS, DEPTH, NCON, GX, hits, best_gap, descent = search()

    # ------------------------------------------------------------------------------------------------ selection
    ncand = len(Q)
    alive = np.ones(ncand, bool)
    inv = [[] for _ in range(npair)]
    for k, ps in enumerate(PAIRS):
        for p in ps:
            inv[p].append(k)
    extreme = [set() for _ in range(ncand)]     # pairs for which the candidate is the shallowest or the deepest of the pool
    for p in range(npair):
        if inv[p]:
            ds = [DEPTH[k][p] for k in inv[p]]
            extreme[inv[p][int(np.argmax(ds))]].add(p)
            extreme[inv[p][int(np.argmin(ds))]].add(p)
    have = np.zeros(npair, int)
    size = {}
    for p in range(npair):
        size[type_class(g, *pairs[p])] = size.get(type_class(g, *pairs[p]), 0) + 1
    rare = np.array([size[type_class(g, *pairs[p])] <= 32 for p in range(npair)])     # every class but the four x-mesh ones
    level = 1
    kept, checked, ill = [], {}, []
    nbytes = 0
    budget = BYTE_BUDGET - MAX_TWINS * (STATE_BYTES + 8 * CON_BYTES)

    def is_stable(k):
        if k not in checked:
            checked[k] = stable(ora, Q[k])
            if checked[k] and not conditioned(ora, Q[k]):
                checked[k] = False
                ill.append(Q[k])            # kept in the fixture: the record of what conditioned() refuses
        return checked[k]

    def cost(k):
        return STATE_BYTES + CON_BYTES * NCON[k]

    def keep(k):
        nonlocal nbytes
        kept.append(k)
        alive[k] = False
        nbytes += cost(k)
        for p in PAIRS[k]:
            have[p] += 1

    def gain(k):
        """Pairs still wanted at this level that state k touches, per byte it costs."""
        if not alive[k]:
            return 0.0
        return sum((1.0 + 0.5 * (p in extreme[k])) for p in PAIRS[k] if have[p] < level) / cost(k)

    # level 1: every reached pair once, whatever it costs; level 2: second states while the bytes last, first for the pairs of the
    # small classes (each its own routine or MPR shape pairing), then the cheapest per pair
    for level in (1, 2):
        if level == 1:
            for p, (sh, dp, _) in sorted(descent.items()):          # a descent's first touching pose carries its twin
                if have[p] < 1 and alive[sh] and is_stable(sh):
                    keep(sh)
        else:
            for p in np.nonzero(rare & (have == 1))[0]:              # pairs of the small classes: their deepest pose outright
                for k in sorted((k for k in inv[p] if alive[k]), key=lambda k: DEPTH[k][p]):
                    if is_stable(k):
                        keep(k)
                        break
        gains = np.array([gain(k) for k in range(ncand)])
        while True:
            k = int(np.argmax(gains))
            if gains[k] <= 0:
                break
            if (level == 2 and nbytes + cost(k) > budget) or not is_stable(k):
                if level == 1 or nbytes + cost(k) <= budget:
                    alive[k] = False
                gains[k] = 0
                continue
            touched = set(PAIRS[k])
            keep(k)
            for j in {j for p in touched for j in inv[p]}:
                gains[j] = gain(j)
        print("selection, level %d: %d states kept, about %d bytes" % (level, len(kept), nbytes), flush=True)
    print("selection: %d states kept, %d stability checks, %d failed (%.0f s)" % (
        len(kept), len(checked), sum(1 for v in checked.values() if not v), time.time() - t0), flush=True)

    # ------------------------------------------------------------------------------------------------ near-miss twins
    states = [Q[k] for k in kept]
    kinds = [KIND[k] for k in kept]
    where = {k: i for i, k in enumerate(kept)}
    twins = []
    for p, (sh, dp, prev) in sorted(descent.items()):
        g1, g2 = pairs[p]
        if len(twins) >= MAX_TWINS:
            break
        if sh not in where or not is_mpr(g, g1, g2) or prev is None:
            continue
        h, b = Q[sh].astype(np.float64), prev.astype(np.float64)
        for f in (0.9, 0.75, 0.5, 0.25, 0.0):
            q32 = (b + f * (h - b)).astype(np.float32)
            c, nefc, gx = ora(q32.astype(np.float64), want_xpos=True)
            if (g1, g2) in pair_list(c):
                continue
            inside = np.linalg.norm(gx[g1] - gx[g2]) <= g.geom_rbound[g1] + g.geom_rbound[g2]
            new = all(not np.array_equal(q32, s) for s in states)
            if new and inside and uncut(c, nefc) and limits_ok(g, q32) and stable(ora, q32) and conditioned(ora, q32):
                twins.append((len(states), where[sh], g1, g2))
                states.append(q32)
                kinds.append(3)
            break
    print("twins: %d (%.0f s)" % (len(twins), time.time() - t0), flush=True)

    # ------------------------------------------------------------------------------------------------ the oracle's answers
    n = len(states)
    qpos = np.array(states, np.float32)
    og = ora.og
    ncon, nefc, nlimit = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    xpos, qacc = np.zeros((n, 39, 3)), np.zeros((n, 43), np.float32)
    cg, cd, cp, cn = [], [], [], []
    for i in range(n):
        s = og.G1Sim()
        s.set_caps(MAXCON, MAXROW)
        assert s.set_state(qpos[i].astype(np.float64), np.zeros(43)) == 0
        assert s.geti("overflow_con") == 0 and s.geti("overflow_row") == 0
        cons = s.contacts()
        ncon[i], nefc[i], nlimit[i] = len(cons), s.geti("nefc"), s.geti("nlimit")
        xpos[i] = s.get("xpos").reshape(39, 3)
        qacc[i] = s.get("qacc")
        for k in cons:
            cg.append((k["geom1"], k["geom2"])); cd.append(k["dist"]); cp.append(k["pos"]); cn.append(k["frame"][0])
    con_start = np.concatenate([[0], np.cumsum(ncon)]).astype(np.int32)
    cg = np.array(cg, np.int16).reshape(-1, 2)
    count = np.zeros(npair, int)
    for i in range(n):
        if kinds[i] != 3:
            for p in {pid[(int(x[0]), int(x[1]))] for x in cg[con_start[i]:con_start[i + 1]]}:
                count[p] += 1
    covered = np.array([pairs[p] for p in range(npair) if count[p] > 0], np.int16).reshape(-1, 2)
    unc = [p for p in range(npair) if count[p] == 0]
    # a pair the blind samples or another pair's descent came near without a descent of its own: the gap of the nearest free pose
    for p in unc:
        if not np.isfinite(best_gap[p]):
            g1, g2 = pairs[p]
            if int(g.geom_type[g1]) != 0:
                best_gap[p] = float(np.linalg.norm(GX[:, g1] - GX[:, g2], axis=1).min()) - (rad[g1] + rad[g2])
    out = dict(qpos=qpos, kind=np.array(kinds, np.int8), ncon=ncon, nefc=nefc, nlimit=nlimit, xpos=xpos, qacc=qacc,
               con_start=con_start, con_geom=cg, con_dist=np.array(cd), con_pos=np.array(cp).reshape(-1, 3),
               con_normal=np.array(cn).reshape(-1, 3), covered=covered,
               uncovered=np.array([pairs[p] for p in unc], np.int16).reshape(-1, 2), uncovered_gap=best_gap[unc],
               twins=np.array(twins, np.int32).reshape(-1, 4), ill_qpos=np.array(ill, np.float32).reshape(-1, 44), seed=np.array(SEED))

    # ------------------------------------------------------------------------------------------------ coverage conditions
    classes = {}
    for p in range(npair):
        cl = type_class(g, *pairs[p])
        t = classes.setdefault(cl, [0, 0, 0])
        t[0] += 1; t[1] += count[p] > 0; t[2] += count[p] > 1
    print("class               pairs covered  in two states")
    for cl in CLASSES:
        print("%-18s %6d %7d %7d" % (cl, *classes[cl]))
    print("total              %6d %7d %7d; %d states, %d twins, %d contacts" % (
        npair, (count > 0).sum(), (count > 1).sum(), n, len(twins), len(cd)))
    assert sorted(classes) == sorted(CLASSES)
    assert all(classes[cl][1] > 0 for cl in CLASSES), "a geom-type class is not covered"
    assert (count > 0).sum() >= MIN_PAIRS, (count > 0).sum()
    assert len(twins) >= MIN_TWINS, len(twins)
    assert ncon.max() < MAXCON and nefc.max() < MAXROW

    if a.check:
        with np.load(a.out) as z:
            diff = [k for k in sorted(set(z.files) | set(out)) if k not in out or k not in z.files or not np.array_equal(out[k], z[k], equal_nan=True)]
        print("%s: %s" % (a.out, "differ: %s" % diff if diff else "all %d arrays equal" % len(out)))
        return 1 if diff else 0
    np.savez_compressed(a.out, **out)
    size = os.path.getsize(a.out)
    print("wrote %s, %d bytes (%.0f s)" % (a.out, size, time.time() - t0))
    assert size < MAX_BYTES, size
    return 0


if __name__ == "__main__":
    sys.exit(main())
