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
    kids = [[c for c in range(nv) if parent[c] == k] for k in range(nv)]
    anc = []
    for k in range(nv):
        a, l = parent[k], []
        while a >= 0:
            l.append(a)
            a = parent[a]
        anc.append(l)                                       # nearest first
    trunk = [k for k in range(nv) if any(len(kids[j]) > 1 for j in range(nv) if j == k or k in anc[j])]
    limbs = []                                              # each from its leaf down to its first dof
    for k in reversed(range(nv)):
        if k not in trunk and not kids[k]:
            limb = [k]
            while parent[limb[-1]] not in trunk and parent[limb[-1]] >= 0:
                limb.append(parent[limb[-1]])
            limbs.append(limb)
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
    lines += [
        "};",
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
