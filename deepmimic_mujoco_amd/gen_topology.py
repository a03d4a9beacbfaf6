"""Generate csrc/dm_topology.h: the dof tree of the compiled model as constexpr tables.

The HIP kernels are specialised to the humanoid3d dimensions (include/dm_model.h) and to its dof
tree: with the tree known at compile time the triangular solves on constraint rows touch only the
276 ancestor pairs with static register and LDS indices.  dm_create() rejects a DmModel whose
dof_parent differs from this header.  Run: python -m deepmimic_mujoco_amd.gen_topology
"""
import os

from .model import NV, NBODY, load_model

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "dm_topology.h")

# Emission order of the column L^T D L elimination (fwd_smooth): a list of (op, k, i, slot).
#   FS_DIAG  d[slot] = readlane(C[k], k)          FS_RCP  rk[k] = rcp(d[slot])          FS_SCALE  Cs[k] = C[k] * rk[k]
#   FS_BCAST m[slot] = readlane(Cs[k], i)         FS_FMA  C[i] = fma(-m[slot], C[k], C[i])   FS_FENCE / FS_DFENCE  m[0..slot) / d[0..slot) are formed here
FS_DIAG, FS_RCP, FS_SCALE, FS_BCAST, FS_FMA, FS_FENCE, FS_DFENCE = range(7)
FS_SLOTS = 8        # scalars of one batch of broadcasts (they live in SGPRs: more of them and the kernels spill)


def factor_schedule(parent, slots=FS_SLOTS):
    """A topological order of the elimination's dependency DAG that keeps every bit of the descending-k loop.

    The loop `for k = nv-1 .. 1: Cs = C[k] / C[k][k]; for every ancestor i of k: C[i] -= Cs[i] * C[k]` fixes, per register
    C[i], the sequence of its updates (descending k), and a pivot reads C[k] after the last of them.  Any order that keeps
    these two rules computes the same bits.  The trunk (dofs with a branching dof in their subtree) is a serial chain; the
    limbs (chains of the other dofs) are independent of each other but for their updates into the trunk.  So: (1) the limbs
    are eliminated side by side, round by round, each pivot updating its limb only (the first limb, which holds the highest
    dofs, its trunk ancestors too); (2) the updates of the other limbs' pivots into the trunk follow in descending k, Cs kept;
    (3) the trunk.  Broadcasts go out in batches of `slots` scalars in front of their FMAs, which then cover the two wait
    states between a VALU write of an SGPR and its VALU read; the update that feeds the next pivot leads its batch.
    """
    nv = len(parent)
    anc, trunk, limbs = _tree(parent)
    ops = []

    def heads(ks, stages):
        for op in stages:
            for s, k in enumerate(ks):
                ops.append((op, k, k, s))
            if op == FS_DIAG and ks:
                ops.append((FS_DFENCE, 0, 0, len(ks)))

    def batches(pairs):
        return [pairs[b:b + slots] for b in range(0, len(pairs), slots)]

    def updates(batch):
        for s, (k, i) in enumerate(batch):
            ops.append((FS_BCAST, k, i, s))
        ops.append((FS_FENCE, 0, 0, len(batch)))
        for s, (k, i) in enumerate(batch):
            ops.append((FS_FMA, k, i, s))

    first = limbs[0] if limbs and all(min(limbs[0]) > max(l) for l in limbs[1:]) else None
    assert len(limbs) <= slots      # one round's pivots share one batch of diagonal scalars
    rounds = [[l[r] for l in limbs if len(l) > r] for r in range(max((len(l) for l in limbs), default=0))]
    for r, piv in enumerate(rounds):
        nxt = rounds[r + 1] if r + 1 < len(rounds) else []
        if r == 0:
            heads(piv, (FS_DIAG, FS_RCP, FS_SCALE))
        own = {k: [i for i in anc[k] if i not in trunk or k in (first or ())] for k in piv}
        todo = batches([(k, own[k][0]) for k in piv if own[k]] + [(k, i) for k in piv for i in own[k][1:]])
        # the next round's pivots start as soon as the leading batch has updated their registers; the other batches of
        # this round issue while their readlane -> rcp -> mul chain is in flight
        for n, batch in enumerate(todo):
            updates(batch)
            if n == 0:
                heads(nxt, (FS_DIAG,))
            if n == min(1, len(todo) - 1):
                heads(nxt, (FS_RCP, FS_SCALE))
    later = sorted((k for l in limbs if l is not first for k in l), reverse=True)
    for batch in batches([(k, i) for k in later for i in anc[k] if i in trunk]):
        updates(batch)
    for k in sorted(trunk, reverse=True):
        if k >= 1:
            heads([k], (FS_DIAG, FS_RCP, FS_SCALE))
            for batch in batches([(k, i) for i in anc[k]]):
                updates(batch)
    check_factor_schedule(parent, ops)
    return ops


def check_factor_schedule(parent, ops):
    """The three rules of factor_schedule(); raises AssertionError with the offending op."""
    nv = len(parent)
    anc = {k: [] for k in range(nv)}
    for k in range(nv):
        a = parent[k]
        while a >= 0:
            anc[k].append(a)
            a = parent[a]
    pairs = [(k, i) for k in range(nv) for i in anc[k]]
    fmas = [(k, i) for op, k, i, s in ops if op == FS_FMA]
    assert sorted(fmas) == sorted(pairs), "the updates are not a permutation of the (dof, ancestor) pairs"
    for op in (FS_DIAG, FS_RCP, FS_SCALE):
        assert sorted(k for o, k, i, s in ops if o == op) == list(range(1, nv)), "every dof 1.. has one pivot"
    last = {i: nv for i in range(nv)}           # the k of the last update into C[i]
    left = {i: sum(1 for p in pairs if p[1] == i) for i in range(nv)}
    slot, dslot, have = {}, {}, {k: set() for k in range(nv)}
    for n, (op, k, i, s) in enumerate(ops):
        if op == FS_DIAG:
            assert left[k] == 0, "op %d: pivot %d before the last update into C[%d]" % (n, k, k)
            dslot[s] = (k, False)
        elif op == FS_RCP:
            assert dslot.get(s) == (k, True), "op %d: rcp of dof %d reads slot %d, which does not hold its fenced diagonal" % (n, k, s)
            have[k].add(FS_RCP)
        elif op == FS_SCALE:
            assert FS_RCP in have[k], "op %d: scale of dof %d before its rcp" % (n, k)
            have[k].add(FS_SCALE)
        elif op == FS_BCAST:
            assert FS_SCALE in have[k] and i in anc[k], "op %d: broadcast (%d, %d)" % (n, k, i)
            slot[s] = (k, i, False)
        elif op == FS_FENCE:
            for t in range(s):
                slot[t] = slot[t][:2] + (True,)
        elif op == FS_DFENCE:
            for t in range(s):
                dslot[t] = (dslot[t][0], True)
        elif op == FS_FMA:
            assert slot.get(s) == (k, i, True), "op %d: update (%d, %d) reads slot %d, which does not hold its fenced multiplier" % (n, k, i, s)
            assert k < last[i], "op %d: update (%d, %d) after the update of dof %d into C[%d]" % (n, k, i, last[i], i)
            last[i] = k
            left[i] -= 1
    return True


# Emission order of the triangular solves (solve_LT / solve_L): a list of (op, k, slot, lslot, kind).
#   SS_LOAD  ld[lslot] = the lane's factor entry of row k (solve_LT) / of depth k (solve_L: one entry serves a whole level)
#   SS_SCALE xs = x * dv          SS_BCAST s[slot] = readlane(xs, k)          SS_FENCE s[0..slot) are formed here
#   SS_FMA   r = fma(-sel<mask(kind, k)>(ld[lslot], 0), s[slot], r), r = xt for SM_TRUNK and x otherwise; lslot SS_NOLOAD: the
#            mask is empty and the multiplier is the constant 0
#   SS_MERGE x = sel<trunk lanes>(xt, x)
SS_LOAD, SS_SCALE, SS_BCAST, SS_FENCE, SS_FMA, SS_MERGE = range(6)
# lanes of an FMA from dof k: its descendants (solve_L); its ancestors outside the trunk, inside it, all of them (solve_LT)
SM_DESC, SM_LIMB, SM_TRUNK, SM_ANC = range(4)
SS_NOLOAD = 255
SS_AHEAD = 2        # serial rounds (one level, one trunk dof): entries are requested in pairs, this many rounds ahead
SS_BATCH_AHEAD = 1  # limb rounds and trunk batches (up to FS_SLOTS entries each): requested this many rounds ahead


def _tree(parent):
    """anc (nearest first), trunk (dofs with a branching dof in their subtree), limbs (each from its leaf down), highest first."""
    nv = len(parent)
    kids = [[c for c in range(nv) if parent[c] == k] for k in range(nv)]
    anc = []
    for k in range(nv):
        a, l = parent[k], []
        while a >= 0:
            l.append(a)
            a = parent[a]
        anc.append(l)
    trunk = [k for k in range(nv) if any(len(kids[j]) > 1 for j in range(nv) if j == k or k in anc[j])]
    limbs = []
    for k in reversed(range(nv)):
        if k not in trunk and not kids[k]:
            limb = [k]
            while parent[limb[-1]] not in trunk and parent[limb[-1]] >= 0:
                limb.append(parent[limb[-1]])
            limbs.append(limb)
    return anc, trunk, limbs


def solve_mask(parent, kind, k):
    """The lanes (dofs) an SS_FMA of this kind from dof k updates."""
    anc, trunk, _ = _tree(parent)
    if kind == SM_DESC:
        return [i for i in range(len(parent)) if k in anc[i]]
    return [j for j in anc[k] if kind == SM_ANC or (j in trunk) == (kind == SM_TRUNK)]


def _emit_rounds(rounds, slots):
    """rounds: [(request_at, [load keys], body)] with body a list of (op, k, slot, load key or None, kind) -> ops.  The loads of
    a round are emitted at the head of round `request_at`; a load slot is free again after the last FMA that reads it."""
    ops, held, free, top = [], {}, [], 0
    for r, (_, _, body) in enumerate(rounds):
        for at, keys, _ in rounds:
            if at == r:
                for key in keys:
                    if free:
                        held[key] = free.pop(0)
                    else:
                        held[key], top = top, top + 1
                    ops.append((SS_LOAD, key[1], 0, held[key], 0))
        last = {key: n for n, (op, k, s, key, kind) in enumerate(body) if key is not None}
        for n, (op, k, s, key, kind) in enumerate(body):
            ops.append((op, k, s, SS_NOLOAD if key is None else held[key], kind))
            if key is not None and last[key] == n:
                free.append(held.pop(key))
                free.sort()
    assert not held and all(0 <= o[2] <= slots for o in ops)
    return ops


def _serial_request(first, r):
    """Serial rounds first, first+1, ...: the entries of rounds 2m, 2m+1 go out together, SS_AHEAD rounds before round 2m (the
    first ones at the head of the round before the serial part, if there is one)."""
    return max(first - 1, 0, first + 2 * ((r - first) // 2) - SS_AHEAD)


def solve_schedule(parent, slots=FS_SLOTS):
    """-> (ops of solve_L, ops of solve_LT): orders that keep every bit of the serial loops.

    Both loops are `for k: s = (x * dv)[k]; x[lanes(k)] -= M[..] * s`, each step a wave-wide FMA whose multiplier is 0 outside
    lanes(k).  A lane's value is fixed by the sequence of the FMAs that update it and by the x_k each of them reads; the FMAs
    with multiplier 0 only add a signed zero (or spread a NaN), they commute with every other step, and each lane must see each
    of them exactly once.  solve_L (k ascending, lanes = descendants of k): a lane is updated by its ancestors only, which lie on
    one path, so the dofs of one depth go together: one scale, their broadcasts as a batch, their FMAs; the factor entry
    M[lane][ancestor at depth d] is the same load for the whole level.  solve_LT (k descending, lanes = ancestors of k): (a) the
    limbs side by side from their leaves down, each FMA on the limb's own lanes; (b) the limb dofs' updates into the trunk in
    descending k, on a copy xt of the incoming x (so that a trunk lane sees one step per limb dof, as in the loop, and not the
    zero step of (a) besides), the scalars broadcast again from the finished limb lanes in batches of `slots`; x takes the trunk
    lanes of xt; (c) the trunk dofs serially.  Factor entries are requested ahead of the round that uses them: a limb round or a
    batch one round ahead, serial rounds in pairs SS_AHEAD rounds ahead.  (The kernels walk the solve_L table; the solve_LT
    table is compiled in only with -DDMK_SOLVE_LT_SCHED=1, see csrc/dm_kernels.hip.)
    """
    nv = len(parent)
    anc, trunk, limbs = _tree(parent)
    depth = [len(a) for a in anc]
    desc = [[i for i in range(nv) if k in anc[i]] for k in range(nv)]

    def round_of(ks, kind, masks, key_of, scale=True):
        body = [(SS_SCALE, 0, 0, None, 0)] if scale else []
        body += [(SS_BCAST, k, s, None, 0) for s, k in enumerate(ks)] + [(SS_FENCE, 0, len(ks), None, 0)]
        body += [(SS_FMA, k, s, key_of(k) if masks[k] else None, kind) for s, k in enumerate(ks)]
        return sorted({key_of(k) for k in ks if masks[k]}), body

    # solve_L: dofs 0 .. nv-2 by depth
    levels = [[j for j in range(nv - 1) if depth[j] == d] for d in range(max(depth) + 1)]
    levels = [l for l in levels if l]
    assert all(len(l) <= slots for l in levels)
    rounds = []
    for r, ks in enumerate(levels):
        keys, body = round_of(ks, SM_DESC, desc, lambda k: ("d", depth[k]))
        rounds.append((_serial_request(0, r), keys, body))
    ops_l = _emit_rounds(rounds, slots)

    # solve_LT: dofs nv-1 .. 1
    rounds = []
    nlimb = max((len(l) for l in limbs), default=0)
    own = {k: [j for j in anc[k] if j not in trunk] for k in range(nv)}
    tr = {k: [j for j in anc[k] if j in trunk] for k in range(nv)}
    for r in range(nlimb):                                                      # (a)
        keys, body = round_of([l[r] for l in limbs if len(l) > r], SM_LIMB, own, lambda k: ("a", k))
        rounds.append((max(0, r - SS_BATCH_AHEAD), keys, body))
    later = sorted((k for l in limbs for k in l), reverse=True)
    for b in range(0, len(later), slots):                                       # (b)
        keys, body = round_of(later[b:b + slots], SM_TRUNK, tr, lambda k: ("b", k), scale=(b == 0))
        rounds.append((len(rounds) - SS_BATCH_AHEAD, keys, body))
    rounds[-1][2].append((SS_MERGE, 0, 0, None, 0))
    first_c = len(rounds)
    for k in sorted(trunk, reverse=True):                                       # (c)
        if k >= 1:
            keys, body = round_of([k], SM_ANC, anc, lambda k: ("c", k))
            rounds.append((_serial_request(first_c, len(rounds)), keys, body))
    ops_lt = _emit_rounds(rounds, slots)
    check_solve_schedule(parent, ops_l, ops_lt)
    return ops_l, ops_lt


def check_solve_schedule(parent, ops_l, ops_lt):
    """The rules of solve_schedule(), by symbolic execution of the op lists; raises AssertionError with the offending op.

    Every lane carries the list of the dofs whose FMA has updated it and the set of the dofs whose zero step it has seen.  A
    broadcast of dof k must read a lane whose list is the serial loop's complete one; at the end every dof lane holds that list
    and has seen every other broadcast dof's zero step exactly once; every FMA reads a fenced scalar of its own dof and a factor
    entry loaded for it that no other load has overwritten."""
    nv = len(parent)
    anc, trunk, _ = _tree(parent)
    depth = [len(a) for a in anc]
    for lt, ops in ((False, ops_l), (True, ops_lt)):
        srcs = list(range(nv - 1, 0, -1)) if lt else list(range(nv - 1))
        want = {i: [k for k in srcs if (i in anc[k] if lt else k in anc[i])] for i in range(nv)}
        real = {"x": {i: [] for i in range(nv)}, "xt": {i: [] for i in range(nv)}}
        zero = {"x": {i: [] for i in range(nv)}, "xt": {i: [] for i in range(nv)}}
        xs, s, ld = None, {}, {}
        for n, (op, k, slot, lslot, kind) in enumerate(ops):
            if op == SS_LOAD:
                ld[lslot] = k
            elif op == SS_SCALE:
                xs = {i: list(real["x"][i]) for i in range(nv)}
            elif op == SS_BCAST:
                assert xs is not None and xs[k] == want[k], "op %d: broadcast of dof %d before the last update into its lane" % (n, k)
                s[slot] = (k, False)
            elif op == SS_FENCE:
                for t in range(slot):
                    s[t] = (s[t][0], True)
            elif op == SS_FMA:
                assert s.get(slot) == (k, True), "op %d: FMA of dof %d reads slot %d, which does not hold its fenced scalar" % (n, k, slot)
                assert kind == SM_DESC if not lt else kind in (SM_LIMB, SM_TRUNK, SM_ANC), "op %d: mask kind %d" % (n, kind)
                lanes = solve_mask(parent, kind, k)
                if lanes:
                    assert ld.get(lslot) == (k if lt else depth[k]), "op %d: FMA of dof %d reads load slot %d, which does not hold its entry" % (n, k, lslot)
                else:
                    assert lslot == SS_NOLOAD, "op %d: an entry for an empty mask" % n
                reg = "xt" if kind == SM_TRUNK else "x"
                for i in range(nv):
                    (real if i in lanes else zero)[reg][i].append(k)
                    if i in lanes:
                        assert real[reg][i] == want[i][:len(real[reg][i])], "op %d: update of dof %d into lane %d out of order" % (n, k, i)
            elif op == SS_MERGE:
                for i in trunk:
                    assert not real["x"][i], "op %d: x's trunk lane %d was updated before the merge" % (n, i)
                    real["x"][i], zero["x"][i] = real["xt"][i], zero["xt"][i]
            else:
                raise AssertionError("op %d: unknown op %d" % (n, op))
        for i in range(nv):
            assert real["x"][i] == want[i], "lane %d ends with the updates %s" % (i, real["x"][i])
            assert sorted(real["x"][i] + zero["x"][i]) == sorted(srcs), "lane %d does not see every step once" % i
    return True


def render(model):
    parent = [int(x) for x in model.dof_parent]
    nanc = []
    for k in range(NV):
        n, a = 0, parent[k]
        while a >= 0:
            n += 1
            a = parent[a]
        nanc.append(n)
    madr = [int(x) for x in model.dof_Madr]
    bparent = [int(x) for x in model.body_parent]
    lines = [
        "// GENERATED by deepmimic_mujoco_amd/gen_topology.py from deepmimic_humanoid3d.xml — do not edit.",
        "// Dof tree of the model (reference: mjModel.dof_parentid / dof_Madr of the asset loaded at",
        "// src/deepmimic_env.py:301).  Sparse inertia layout: row i = M(i,i), M(i,parent), M(i,grandparent), ...",
        "#pragma once",
        "namespace topo {",
        "constexpr int NV = %d;" % NV,
        "constexpr int NM = %d;" % (madr[-1] + nanc[-1] + 1),
        "constexpr int PARENT[NV] = {%s};" % ", ".join(map(str, parent)),
        "constexpr int NANC[NV] = {%s};" % ", ".join(map(str, nanc)),
        "constexpr int MADR[NV] = {%s};" % ", ".join(map(str, madr)),
        "constexpr bool is_anc(int j, int i) {  // j is a strict ancestor of i",
        "  for (int a = PARENT[i]; a >= 0; a = PARENT[a]) if (a == j) return true;",
        "  return false;",
        "}",
        "constexpr int midx(int i, int j) { return MADR[i] + NANC[i] - NANC[j]; }  // j ancestor-or-self of i",
        "constexpr int NB = %d;" % NBODY,
        "constexpr int BPARENT[NB] = {%s};  // body tree (body 0 = world)" % ", ".join(map(str, bparent)),
        "constexpr unsigned long long body_ancself_mask(int c) {  // bit b: body b (>= 1) is c or an ancestor of c",
        "  unsigned long long m = 0;",
        "  for (int b = c; b >= 1; b = BPARENT[b]) m |= 1ull << b;",
        "  return m;",
        "}",
        "constexpr unsigned long long desc_mask(int j) {  // bit i: dof i is a strict descendant of j",
        "  unsigned long long m = 0;",
        "  for (int i = 0; i < NV; i++) if (is_anc(j, i)) m |= 1ull << i;",
        "  return m;",
        "}",
        "constexpr unsigned long long anc_mask(int i) {  // bit j: dof j is a strict ancestor of i (= the lanes that own M[i][j])",
        "  unsigned long long m = 0;",
        "  for (int a = PARENT[i]; a >= 0; a = PARENT[a]) m |= 1ull << a;",
        "  return m;",
        "}",
    ]
    sched = factor_schedule(parent)
    lines += [
        "// Emission order of the L^T D L elimination in fwd_smooth: a topological order of its dependency DAG in which the",
        "// limbs run side by side and the broadcasts of a batch precede their FMAs (gen_topology.factor_schedule).",
        "enum { FS_DIAG, FS_RCP, FS_SCALE, FS_BCAST, FS_FMA, FS_FENCE, FS_DFENCE };",
        "struct FactorOp { unsigned char op, k, i, slot; };",
        "constexpr int FS_SLOTS = %d;" % FS_SLOTS,
        "constexpr int FS_NOPS = %d;" % len(sched),
        "constexpr FactorOp FACTOR_SCHED[FS_NOPS] = {",
    ]
    names = ("FS_DIAG", "FS_RCP", "FS_SCALE", "FS_BCAST", "FS_FMA", "FS_FENCE", "FS_DFENCE")
    for b in range(0, len(sched), 6):
        lines.append("  " + " ".join("{%s, %d, %d, %d}," % (names[op], k, i, s) for op, k, i, s in sched[b:b + 6]))
    lines.append("};")
    ops_l, ops_lt = solve_schedule(parent)
    _, trunk, _ = _tree(parent)
    lines += [
        "// Emission order of the triangular solves solve_L (by depth level) and solve_LT (limbs side by side, their updates into the",
        "// trunk on the copy xt, the trunk serially), factor entries requested ahead of their round (gen_topology.solve_schedule).",
        "enum { SS_LOAD, SS_SCALE, SS_BCAST, SS_FENCE, SS_FMA, SS_MERGE };",
        "enum { SM_DESC, SM_LIMB, SM_TRUNK, SM_ANC };",
        "struct SolveOp { unsigned char op, k, slot, lslot, kind; };",
        "constexpr int SS_NOLOAD = %d;" % SS_NOLOAD,
        "constexpr int SS_LSLOTS = %d;" % (1 + max(o[3] for o in ops_l + ops_lt if o[3] != SS_NOLOAD)),
        "constexpr unsigned long long TRUNK_MASK = 0x%xull;" % sum(1 << k for k in trunk),
        "constexpr unsigned long long solve_mask(int kind, int k) {",
        "  return kind == SM_DESC ? desc_mask(k) : kind == SM_LIMB ? anc_mask(k) & ~TRUNK_MASK : kind == SM_TRUNK ? anc_mask(k) & TRUNK_MASK : anc_mask(k);",
        "}",
    ]
    snames = ("SS_LOAD", "SS_SCALE", "SS_BCAST", "SS_FENCE", "SS_FMA", "SS_MERGE")
    knames = ("SM_DESC", "SM_LIMB", "SM_TRUNK", "SM_ANC")
    for tag, ops in (("L", ops_l), ("LT", ops_lt)):
        lines += ["constexpr int SS_%s_NOPS = %d;" % (tag, len(ops)), "constexpr SolveOp SOLVE_%s_SCHED[SS_%s_NOPS] = {" % (tag, tag)]
        for b in range(0, len(ops), 5):
            lines.append("  " + " ".join("{%s, %d, %d, %d, %s}," % (snames[op], k, s, ls, knames[kind]) for op, k, s, ls, kind in ops[b:b + 5]))
        lines.append("};")
    lines += [
        "}  // namespace topo",
        "",
    ]
    return "\n".join(lines)


OUT_G1 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "dm_g1_topology.h")


def render_g1(g):
    """csrc/dm_g1_topology.h: the 43-dof tree of deepmimic_unitree_g1.xml (from the general MJCF compiler's GModel)."""
    parent = [int(x) for x in g.dof_parent]
    madr = [int(x) for x in g.dof_Madr]
    nanc = []
    for k in range(g.nv):
        n, a = 0, parent[k]
        while a >= 0:
            n, a = n + 1, parent[a]
        nanc.append(n)
    return "\n".join([
        "// GENERATED by deepmimic_mujoco_amd/gen_topology.py from deepmimic_unitree_g1.xml — do not edit.",
        "// Dof tree of the Unitree G1 model: with it known at compile time the constraint rows are solved against the sparse",
        "// factor in registers (static indices).  dmg1_create() rejects a model whose dof tree differs.",
        "#pragma once",
        "namespace g1topo {",
        "constexpr int NV = %d;" % g.nv,
        "constexpr int PARENT[NV] = {%s};" % ", ".join(map(str, parent)),
        "constexpr int NANC[NV] = {%s};" % ", ".join(map(str, nanc)),
        "constexpr int MADR[NV] = {%s};" % ", ".join(map(str, madr)),
        "}  // namespace g1topo",
        "",
    ])


def _write(path, txt):
    old = open(path).read() if os.path.exists(path) else None
    if old != txt:
        with open(path, "w") as f:
            f.write(txt)


def main():
    _write(OUT, render(load_model()))
    from . import mjcf
    from .model import ASSET_DIR
    _write(OUT_G1, render_g1(mjcf.compile_mjcf_general(os.path.join(ASSET_DIR, "deepmimic_unitree_g1.xml"))))
    return OUT


if __name__ == "__main__":
    print(main())
