"""topo::SOLVE_L_SCHED / SOLVE_LT_SCHED, the emission orders of the triangular solves (gen_topology.solve_schedule): each must give
every lane the FMAs of the serial loop in the loop's order, every broadcast must read a finished lane, and every lane must see
each step exactly once, as an update or as the `x + (-+0)` of a lane outside the step's mask.  The rules are restated here from
the op lists alone, apart from gen_topology.check_solve_schedule; then both orders are run in emulated fp32 against the serial
loops on random tree-sparse factors, bit for bit."""
import re

import numpy as np
import pytest

from deepmimic_mujoco_amd import gen_topology as G

NLANE = 64


@pytest.fixture(scope="module")
def parent(model):
    return [int(x) for x in model.dof_parent]


@pytest.fixture(scope="module")
def scheds(parent):
    return G.solve_schedule(parent)


def _anc(parent, k):
    out, a = [], parent[k]
    while a >= 0:
        out.append(a)
        a = parent[a]
    return out


def _trunk(parent):
    nv = len(parent)
    branching = [k for k in range(nv) if sum(p == k for p in parent) > 1]
    return sorted({j for b in branching for j in [b] + _anc(parent, b)})


def _lanes(parent, lt, kind, k):
    """The lanes an FMA of dof k updates, from the mask kind."""
    nv, trunk = len(parent), _trunk(parent)
    if not lt:
        assert kind == G.SM_DESC
        return [i for i in range(nv) if k in _anc(parent, i)]
    assert kind in (G.SM_LIMB, G.SM_TRUNK, G.SM_ANC)
    return [j for j in _anc(parent, k) if kind == G.SM_ANC or (j in trunk) == (kind == G.SM_TRUNK)]


def _serial_sources(parent, lt):
    nv = len(parent)
    return list(range(nv - 1, 0, -1)) if lt else list(range(nv - 1))


def _rules(parent, lt, ops):
    """-> None, or the first broken rule as text."""
    nv, trunk = len(parent), _trunk(parent)
    srcs = _serial_sources(parent, lt)
    pairs = sorted((k, i) for k in srcs for i in range(nv) if (i in _anc(parent, k) if lt else k in _anc(parent, i)))
    fmas = [(n, k, kind) for n, (op, k, s, ls, kind) in enumerate(ops) if op == G.SS_FMA]
    got = sorted((k, i) for n, k, kind in fmas for i in _lanes(parent, lt, kind, k))
    if got != pairs:
        return "the FMAs are not the (dof, ancestor) pairs once each"
    # per lane: the sequence of source dofs, in the register the lane's value lives in
    seq = {i: [] for i in range(nv)}
    last_into = {i: -1 for i in range(nv)}
    for n, k, kind in fmas:
        for i in _lanes(parent, lt, kind, k):
            seq[i].append(k)
            last_into[i] = n
    for i in range(nv):
        want = [k for k in srcs if (k, i) in set(pairs)]
        if seq[i] != want:
            return "lane %d is updated in the order %s, the loop's is %s" % (i, seq[i], want)
    merge = [n for n, o in enumerate(ops) if o[0] == G.SS_MERGE]
    if len(merge) != (1 if lt else 0):
        return "solve_LT needs exactly one merge, solve_L none"
    # a broadcast reads the scale before it; that scale must follow the last FMA into the dof's lane, and, for a trunk lane
    # of solve_LT (whose updates from the limbs live in xt), the merge too
    scale_at = -1
    seen = set()
    for n, (op, k, s, ls, kind) in enumerate(ops):
        if op == G.SS_SCALE:
            scale_at = n
        elif op == G.SS_BCAST:
            if scale_at < last_into[k]:
                return "dof %d is broadcast before the last update into its lane" % k
            if lt and k in trunk and scale_at < merge[0]:
                return "trunk dof %d is broadcast before the merge" % k
            seen.add(k)
    if sorted(seen) != sorted(srcs):
        return "not every dof of the loop is broadcast"
    # in solve_LT no FMA may touch x's trunk lanes before the merge, nor xt after it
    if lt:
        for n, k, kind in fmas:
            if (kind == G.SM_ANC and n < merge[0]) or (kind == G.SM_TRUNK and n > merge[0]):
                return "FMA of dof %d on the wrong side of the merge" % k
    return None


def test_counts(parent, scheds):
    """33 broadcast dofs per solve; solve_L has one FMA per dof, solve_LT two per limb dof (limb lanes, trunk lanes) and one per
    trunk dof; 13 scales (levels) in solve_L, 7 limb rounds + 1 + 8 in solve_LT; batches hold at most FS_SLOTS scalars."""
    ops_l, ops_lt = scheds
    assert len(parent) == 34
    cnt = lambda ops, op: sum(o[0] == op for o in ops)
    assert cnt(ops_l, G.SS_BCAST) == 33 and cnt(ops_l, G.SS_FMA) == 33 and cnt(ops_l, G.SS_SCALE) == 13 and cnt(ops_l, G.SS_MERGE) == 0
    assert cnt(ops_lt, G.SS_BCAST) == 25 + 25 + 8 and cnt(ops_lt, G.SS_FMA) == 25 + 25 + 8 and cnt(ops_lt, G.SS_SCALE) == 7 + 1 + 8
    for ops in scheds:
        assert all(0 <= s < G.FS_SLOTS for op, k, s, ls, kind in ops if op in (G.SS_BCAST, G.SS_FMA))
        assert all(1 <= s <= G.FS_SLOTS for op, k, s, ls, kind in ops if op == G.SS_FENCE)


def test_orders_keep_the_loops(parent, scheds):
    for lt, ops in zip((False, True), scheds):
        assert _rules(parent, lt, ops) is None
    assert G.check_solve_schedule(parent, *scheds)


def test_values_travel_through_their_slots(parent, scheds):
    """Every FMA reads the scalar slot its own broadcast wrote, with a fence and no other write in between, and the load slot
    that holds its own factor entry; no load is requested directly in front of the FMA that reads it (a round ahead at least)."""
    depth = [len(_anc(parent, k)) for k in range(len(parent))]
    for lt, ops in zip((False, True), scheds):
        s, ld = {}, {}
        for n, (op, k, slot, lslot, kind) in enumerate(ops):
            if op == G.SS_BCAST:
                s[slot] = [k, False]
            elif op == G.SS_FENCE:
                for t in range(slot):
                    s[t][1] = True
            elif op == G.SS_LOAD:
                ld[lslot] = (k, n)
            elif op == G.SS_FMA:
                assert s[slot] == [k, True], (n, k, slot, s[slot])
                if _lanes(parent, lt, kind, k):
                    key, at = ld[lslot]
                    assert key == (k if lt else depth[k]), (n, k, lslot, key)
                    between = [o[0] for o in ops[at:n]]
                    assert G.SS_FENCE in between and G.SS_BCAST in between, "load at %d is used at %d without a round between" % (at, n)
                else:
                    assert lslot == G.SS_NOLOAD


def _swap_trunk_updates(ops):
    """solve_LT with the updates of two limb dofs into the trunk (neighbours in one batch of part b) exchanged, each with its
    broadcast and its factor entry, so that only the order is wrong."""
    fm = [n for n, o in enumerate(ops) if o[0] == G.SS_FMA and o[4] == G.SM_TRUNK]
    a, b = fm[3], fm[4]
    bad = list(ops)
    for n, other in ((a, ops[b][1]), (b, ops[a][1])):
        bc = max(m for m in range(n) if ops[m][0] == G.SS_BCAST and ops[m][2] == ops[n][2])
        ld = max(m for m in range(n) if ops[m][0] == G.SS_LOAD and ops[m][3] == ops[n][3])
        assert ops[bc][1] == ops[n][1] and ops[ld][1] == ops[n][1]
        for m in (n, bc, ld):
            bad[m] = (ops[m][0], other) + tuple(ops[m][2:])
    return bad


def test_broken_orders_are_refused(parent, scheds):
    """Two trunk updates of one lane swapped, and a child broadcast before its parent's update: both checkers refuse."""
    ops_l, ops_lt = scheds
    bad = _swap_trunk_updates(ops_lt)
    assert "order" in (_rules(parent, True, bad) or "")
    with pytest.raises(AssertionError):
        G.check_solve_schedule(parent, ops_l, bad)
    # solve_L: move the broadcast of a depth-2 dof in front of the level-1 FMA (its parent's update into its lane)
    bc = [n for n, o in enumerate(ops_l) if o[0] == G.SS_BCAST and o[1] == 2][0]
    fm = [n for n, o in enumerate(ops_l) if o[0] == G.SS_FMA and o[1] == 1][0]
    assert fm < bc
    bad = list(ops_l)
    bad.insert(fm, bad.pop(bc))
    assert "before the last update" in (_rules(parent, False, bad) or "")
    with pytest.raises(AssertionError):
        G.check_solve_schedule(parent, bad, ops_lt)


def _fma32(a, b, c):
    """fp32 fma emulated: fp64 product-sum, rounded once to fp32 (the same helper for both orders)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _serial(parent, lt, x, dv, Mf):
    """The loops of csrc/dm_kernels.hip as they were: Mf[k] is the per-lane multiplier of step k (0 outside the mask)."""
    x = x.copy()
    for k in _serial_sources(parent, lt):
        xk = (x * dv)[k]
        x = _fma32(-Mf[k], np.full(NLANE, xk, np.float32), x)
    return x


def _scheduled(parent, lt, ops, x, dv, Mf):
    x, xt = x.copy(), x.copy()
    xs, s = None, {}
    trunk = _trunk(parent)
    for op, k, slot, lslot, kind in ops:
        if op == G.SS_SCALE:
            xs = x * dv
        elif op == G.SS_BCAST:
            s[slot] = xs[k]
        elif op == G.SS_FMA:
            l = np.zeros(NLANE, np.float32)
            lanes = _lanes(parent, lt, kind, k)
            l[lanes] = Mf[k][lanes]
            if kind == G.SM_TRUNK:
                xt = _fma32(-l, np.full(NLANE, s[slot], np.float32), xt)
            else:
                x = _fma32(-l, np.full(NLANE, s[slot], np.float32), x)
        elif op == G.SS_MERGE:
            x[trunk] = xt[trunk]
    return x


@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e3])
def test_emulated_fp32_bits(parent, scheds, scale):
    """200 seeded tree-sparse factors and right-hand sides (some entries exactly +-0) per scale: the table orders give the serial
    loops' bit patterns in all 64 lanes.  At 1e3 a solve can overflow, which puts the spread of an Inf / NaN broadcast under the
    same comparison."""
    nv = len(parent)
    rng = np.random.default_rng(int(scale * 1000) + 7)
    for draw in range(200):
        x0 = np.zeros(NLANE, np.float32)
        x0[:nv] = (rng.normal(0, scale, nv)).astype(np.float32)
        x0[rng.integers(0, nv, 3)] = rng.choice(np.array([0.0, -0.0], np.float32), 3)
        dv = np.zeros(NLANE, np.float32)
        dv[:nv] = rng.uniform(0.2, 5.0, nv).astype(np.float32)
        for lt, ops in zip((False, True), scheds):
            Mf = np.zeros((nv, NLANE), np.float32)
            for k in _serial_sources(parent, lt):
                lanes = [i for i in range(nv) if (i in _anc(parent, k) if lt else k in _anc(parent, i))]
                Mf[k][lanes] = rng.normal(0, 0.3 * scale, len(lanes)).astype(np.float32)
            with np.errstate(over="ignore", invalid="ignore"):
                a, b = _serial(parent, lt, x0, dv, Mf), _scheduled(parent, lt, ops, x0, dv, Mf)
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), (scale, draw, lt)


def test_header_holds_these_orders(model, scheds):
    """csrc/dm_topology.h carries exactly these ops, and gen_topology.render() reproduces the committed header byte for byte."""
    text = open(G.OUT).read()
    assert text == G.render(model)
    snames = ("SS_LOAD", "SS_SCALE", "SS_BCAST", "SS_FENCE", "SS_FMA", "SS_MERGE")
    knames = ("SM_DESC", "SM_LIMB", "SM_TRUNK", "SM_ANC")
    for tag, ops in zip(("L", "LT"), scheds):
        body = text[text.index("SOLVE_%s_SCHED[SS_%s_NOPS] = {" % (tag, tag)):]
        body = body[:body.index("};")]
        got = [(snames.index(a), int(b), int(c), int(d), knames.index(e)) for a, b, c, d, e in re.findall(r"\{(SS_\w+), (\d+), (\d+), (\d+), (SM_\w+)\}", body)]
        assert got == list(ops) and "SS_%s_NOPS = %d;" % (tag, len(ops)) in text
