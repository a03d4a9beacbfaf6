"""topo::FACTOR_SCHED, the emission order of fwd_smooth's column elimination (gen_topology.factor_schedule): it must be a
topological order of the descending-k loop's dependency DAG, since only then are the factor's bits those of the loop.  The rules
are restated here from the op list alone, apart from gen_topology.check_factor_schedule."""
import re

import pytest

from deepmimic_mujoco_amd import gen_topology as G


@pytest.fixture(scope="module")
def parent(model):
    return [int(x) for x in model.dof_parent]


@pytest.fixture(scope="module")
def ops(parent):
    return G.factor_schedule(parent)


def _anc(parent, k):
    out, a = [], parent[k]
    while a >= 0:
        out.append(a)
        a = parent[a]
    return out


def _rules(parent, ops):
    """-> None, or the first broken rule as text."""
    nv = len(parent)
    pairs = sorted((k, i) for k in range(nv) for i in _anc(parent, k))
    fmas = [(k, i) for op, k, i, s in ops if op == G.FS_FMA]
    pivots = [k for op, k, i, s in ops if op == G.FS_DIAG]
    if sorted(fmas) != pairs or sorted(pivots) != list(range(1, nv)):
        return "not a permutation of the pairs and the pivots"
    at = {("f", k, i): n for n, (op, k, i, s) in enumerate(ops) if op == G.FS_FMA}
    at.update({("p", k): n for n, (op, k, i, s) in enumerate(ops) if op == G.FS_DIAG})
    for k, i in pairs:
        if at[("f", k, i)] < at[("p", k)]:
            return "update (%d, %d) before pivot %d" % (k, i, k)
        if i >= 1 and at[("p", i)] < at[("f", k, i)]:
            return "pivot %d before the update (%d, %d) into its register" % (i, k, i)
    for i in range(nv):
        ks = [k for k, j in fmas if j == i]
        if ks != sorted(ks, reverse=True):
            return "updates into C[%d] not in descending k: %s" % (i, ks)
    return None


def test_counts(parent, ops):
    """276 (dof, ancestor) pairs and 33 pivots for the humanoid3d tree; every batch holds at most FS_SLOTS scalars."""
    assert len(parent) == 34
    assert sum(op == G.FS_FMA for op, *_ in ops) == 276 and sum(op == G.FS_BCAST for op, *_ in ops) == 276
    for kind in (G.FS_DIAG, G.FS_RCP, G.FS_SCALE):
        assert sum(op == kind for op, *_ in ops) == 33
    assert all(0 <= s < G.FS_SLOTS for op, k, i, s in ops if op not in (G.FS_FENCE, G.FS_DFENCE))
    assert all(1 <= s <= G.FS_SLOTS for op, k, i, s in ops if op in (G.FS_FENCE, G.FS_DFENCE))


def test_order_is_topological(parent, ops):
    """A permutation of the pairs plus the pivots; each pivot after every update into its register and before its own updates;
    the updates into each register in descending k."""
    assert _rules(parent, ops) is None
    assert G.check_factor_schedule(parent, ops)


def test_values_travel_through_their_slots(parent, ops):
    """Every FMA reads the slot its own broadcast wrote, with a fence and no other write of the slot in between; every rcp reads
    the slot of its own diagonal; a scale follows its rcp and precedes the dof's broadcasts."""
    m, d, scaled, rcp = {}, {}, set(), set()
    for op, k, i, s in ops:
        if op == G.FS_BCAST:
            assert k in scaled
            m[s] = [k, i, False]
        elif op == G.FS_DIAG:
            d[s] = [k, False]
        elif op == G.FS_FENCE:
            for t in range(s):
                m[t][2] = True
        elif op == G.FS_DFENCE:
            for t in range(s):
                d[t][1] = True
        elif op == G.FS_FMA:
            assert m[s] == [k, i, True], (k, i, s, m[s])
        elif op == G.FS_RCP:
            assert d[s] == [k, True], (k, s, d[s])
            rcp.add(k)
        elif op == G.FS_SCALE:
            assert k in rcp
            scaled.add(k)


def test_swapped_updates_are_caught(parent, ops):
    """Two updates of one register exchanged (slots and broadcasts with them): both checkers refuse the order."""
    fm = [n for n, (op, k, i, s) in enumerate(ops) if op == G.FS_FMA and i == 0]
    bc = {(k, i): n for n, (op, k, i, s) in enumerate(ops) if op == G.FS_BCAST}
    a, b = fm[3], fm[4]
    bad = list(ops)
    (ka, sa), (kb, sb) = (ops[a][1], ops[a][3]), (ops[b][1], ops[b][3])
    bad[a], bad[b] = (G.FS_FMA, kb, 0, sa), (G.FS_FMA, ka, 0, sb)
    bad[bc[(ka, 0)]], bad[bc[(kb, 0)]] = (G.FS_BCAST, kb, 0, sa), (G.FS_BCAST, ka, 0, sb)
    assert "descending" in (_rules(parent, bad) or "")
    with pytest.raises(AssertionError):
        G.check_factor_schedule(parent, bad)


def test_header_holds_this_order(model, ops):
    """csrc/dm_topology.h carries exactly these ops (the header as a whole is compared with render() in test_mocap_and_abi.py)."""
    text = open(G.OUT).read()
    body = text[text.index("FACTOR_SCHED[FS_NOPS] = {"):]
    names = ("FS_DIAG", "FS_RCP", "FS_SCALE", "FS_BCAST", "FS_FMA", "FS_FENCE", "FS_DFENCE")
    got = [(names.index(a), int(b), int(c), int(e)) for a, b, c, e in re.findall(r"\{(FS_\w+), (\d+), (\d+), (\d+)\}", body)]
    assert got == list(ops) and "FS_NOPS = %d;" % len(ops) in text
