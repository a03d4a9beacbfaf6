"""The G1 collision path (csrc/dm_g1_narrow.h: broadphase with its oriented-box and box-above-plane filters, the eight analytic
routines, MPR with the cluster-culled mesh support map and the separating-direction cache) on the states of
tests/golden/g1_pair_cover.npz, which between them touch every collision pair the search could reach, plus near-miss twins.  The
fp64 oracle's answers come from the fixture (tests/test_g1_pair_cover_cpu.py ties them to the live oracle); no state is left out
and no difference in a contact set is allowed.

Which kernel runs: dmg1_set_state's forward evaluation is ALWAYS the monolithic g1_step_kernel (shared 16-entry cache per env),
whatever `pipeline` says; g1_env_kernel / g1_pair_kernel (narrow_pair<true>, one cache entry per (env, pair)) run only in
dmg1_step of a split engine.  So:

  a. set_state: the monolithic kernel against the oracle: contact list in order, counts, flag, body / contact geometry
  b. one step from every state, monolithic engine and split engine: stage 0 of the step is the fixture state, so its contact
     count, contact-list hash and row count are the fixture's in BOTH; everything the step leaves (debug rows with the last
     stage's contact geometry, state, observation, reward) is bit-identical between the two, so the pair kernel's geometry is the
     monolithic kernel's, which (a) holds to the oracle; the split engine's ticket counters show the pair kernel ran
  c. the separating-direction caches filled by ANOTHER pose, and by the near-miss twin, change no bit: set_state sequences on
     the monolithic kernel, step sequences on the split pipeline; each cache is shown to hold entries
  d. the monolithic kernel with a null cache (dmg1_set_null_cache) leaves the same bits, and its cache stays empty
"""
import numpy as np
import pytest

import constraint_path_states as cps
from test_g1_pair_cover_cpu import FIXTURE, contact_pairs, load_generator

pytestmark = pytest.mark.gpu

TOL_XPOS, TOL_DIST, TOL_POS, TOL_NRM = 2e-6, 1e-6, 1e-5, 1e-5      # _forward_parity, test_g1_forward_evaluation_at_the_caps
NBITS = 900                                                       # debug slots 900.. hold per-kernel timing marks


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def cover():
    gen = load_generator()
    with np.load(FIXTURE) as z:
        F = {k: z[k] for k in z.files}
    from deepmimic_mujoco_amd.g1 import load_g1_model
    return gen, F, load_g1_model()[0]


def _engine(n, pipeline, torch=None):
    """Engine with the debug rows on; with `torch` also reset to frame 0 of the clip, ready to step."""
    from deepmimic_mujoco_amd.g1 import G1HipEngine
    eng = G1HipEngine(n, auto_reset=False, pipeline=pipeline)
    eng.load_clip(cps.g1_mocap("walk"))
    if torch is not None:
        eng.out = eng.alloc_outputs()
        eng.reset(eng.out["obs"], idx_init=torch.zeros(n, dtype=torch.int32, device=eng.device))
    return eng, eng.enable_debug()


def _evaluate(eng, buf, torch, qpos):
    """set_state(qpos, 0, 0) with its forward evaluation (g1_step_kernel): the debug rows [n, DEBUG_STRIDE]."""
    n = len(qpos)
    eng.set_state(torch.tensor(qpos, dtype=torch.float32, device=eng.device).contiguous(),
                  torch.zeros(n, 43, device=eng.device), torch.zeros(n, 43, device=eng.device))
    torch.cuda.synchronize()
    return buf.cpu().numpy().copy()


def _step(eng, buf, torch, qpos):
    """set_state(qpos, 0, 0) without a forward pass, then one dmg1_step of zero action: debug rows, state and outputs."""
    n = len(qpos)
    eng.set_state(torch.tensor(qpos, dtype=torch.float32, device=eng.device).contiguous(),
                  torch.zeros(n, 43, device=eng.device), torch.zeros(n, 43, device=eng.device), run_forward=False)
    eng.step(torch.zeros(n, 23, device=eng.device), eng.out)
    torch.cuda.synchronize()
    q, v, w = [x.cpu().numpy() for x in eng.get_state()]
    return dict(rows=buf.cpu().numpy().copy(), state=np.concatenate([q, v, w], axis=1),
                outs=np.concatenate([eng.out["obs"].cpu().numpy(), eng.out["rew"].cpu().numpy()[:, None],
                                     eng.out["done"].cpu().numpy()[:, None].astype(np.float32)], axis=1))


def _fresh_rows(torch, qpos, pipeline=1, null_cache=False):
    eng, buf = _engine(len(qpos), pipeline)
    if null_cache:
        eng.set_null_cache(True)
    d = _evaluate(eng, buf, torch, qpos)
    entries = eng.sep_cache_entries()
    eng.close()
    return d, entries


@pytest.fixture(scope="module")
def fresh(torch_mod, cover):
    """Debug rows of every state after set_state on a fresh engine (empty cache): the monolithic kernel."""
    return _fresh_rows(torch_mod, cover[1]["qpos"])[0]


@pytest.fixture(scope="module")
def stepped(torch_mod, cover):
    """One step from every state on a fresh monolithic (1) and a fresh split (2) engine, and the split engine's ticket counters."""
    res = {}
    for pl in (1, 2):
        eng, buf = _engine(len(cover[1]["qpos"]), pl, torch_mod)
        res[pl] = _step(eng, buf, torch_mod, cover[1]["qpos"])
        res[pl]["split"], res[pl]["tickets"] = eng.split, eng.queue_counters()
        eng.close()
    return res


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same_bits(a, b):
    return np.array_equal(_bits(a[..., :NBITS]), _bits(b[..., :NBITS]))


def _orders(F):
    """The three evaluations of the cache tests: env -> state.  The batch; every env another state (order reversed and shifted
    by one); the batch again.  After the batch, one env per twin running twin -> touching -> twin and one running touching ->
    twin -> touching."""
    n, tw = len(F["qpos"]), F["twins"]
    perm = np.roll(np.arange(n)[::-1], 1)
    for f in np.nonzero(perm == np.arange(n))[0]:           # a reversal of an odd count keeps one env in place: move it on
        perm[[f, (f + 1) % n]] = perm[[(f + 1) % n, f]]
    assert np.all(perm != np.arange(n))
    t, p = tw[:, 0], tw[:, 1]
    return [np.concatenate([np.arange(n), t, p]), np.concatenate([perm, p, t]), np.concatenate([np.arange(n), t, p])]


def _contact_hash(pairs):
    h = 0
    for g1, g2 in pairs:                # include/deepmimic_g1_hip.h, dmg1_set_debug: the stage's contact list in order
        h = (h * 131 + g1 * 97 + g2 + 1) & 0xFFFFFF
    return h


def _no_twin_touches(F, idx, rows, what):
    tw = F["twins"]
    for e, i in enumerate(idx):
        for row in tw[tw[:, 0] == i]:
            got = [(int(r[1]), int(r[2])) for r in rows[e, 208:208 + 9 * int(rows[e, 203])].reshape(-1, 9)]
            assert (int(row[2]), int(row[3])) not in got, ("twin carries a contact for its pair", what, e, i)


def test_g1_pair_cover_matches_the_oracle(cover, fresh):
    """set_state on every state (g1_step_kernel): ncon, the ordered geom pairs, nefc and nlimit equal, the overflow flag clear,
    the broadphase's survivor count the sum of its three class counts and no smaller than the number of touching pairs; body
    positions to 2e-6, contact distance 1e-6, position 1e-5, normal 1e-5.  (Measured on an MI355X: DESIGN.md 10-r4.)"""
    gen, F, g = cover
    dbg = fresh
    worst = {cl: [0, 0.0, 0.0, 0.0] for cl in gen.CLASSES}
    wx = wq = 0.0
    touched = set()
    for i in range(len(F["qpos"])):
        d, name = dbg[i], "state %d (kind %d)" % (i, F["kind"][i])
        want = contact_pairs(F, i)
        ncon = int(d[203])
        c = d[208:208 + 9 * ncon].reshape(-1, 9)
        assert ncon == F["ncon"][i], (name, ncon, F["ncon"][i])
        assert [(int(r[1]), int(r[2])) for r in c] == want, name
        assert (int(d[204]), int(d[206])) == (F["nefc"][i], F["nlimit"][i]), (name, d[204], d[206])
        assert d[207] == 0, (name, d[207])
        assert d[1009] + d[1010] + d[1011] == d[1008], (name, d[1008:1012])
        assert d[1008] >= len(set(want)), (name, d[1008])
        wx = max(wx, np.abs(d[:117] - F["xpos"][i].ravel()).max())
        assert wx < TOL_XPOS, (name, wx)
        a = F["con_start"][i]
        for k, (r, p) in enumerate(zip(c, want)):
            w = worst[gen.type_class(g, *p)]
            w[0] += 1
            w[1] = max(w[1], abs(r[0] - F["con_dist"][a + k]))
            w[2] = max(w[2], np.abs(r[3:6] - F["con_pos"][a + k]).max())
            w[3] = max(w[3], np.abs(r[6:9] - F["con_normal"][a + k]).max())
            assert w[1] < TOL_DIST and w[2] < TOL_POS and w[3] < TOL_NRM, (name, p, r, F["con_dist"][a + k], w)
        if F["kind"][i] != 3:
            touched |= set(want)
        qa = F["qacc"][i].astype(np.float64)
        wq = max(wq, np.abs(d[160:203] - qa).max() / max(1.0, np.abs(qa).max()))
    print("   G1 pair cover, monolithic kernel: %d states, %d of %d pairs touched; body positions %.2e; qacc (not asserted) %.2e" % (
        len(F["qpos"]), len(touched), len(g.pairs), wx, wq))
    print("   class              contacts  distance  position  normal")
    for cl in gen.CLASSES:
        print("   %-18s %7d  %.2e  %.2e  %.2e" % (cl, *worst[cl]))
        assert worst[cl][0] > 0, cl
    assert len(touched) == len(F["covered"]) >= 740
    _no_twin_touches(F, np.arange(len(F["qpos"])), dbg, "fresh")


def test_g1_pair_kernel_equals_the_monolithic_kernel_on_every_state(cover, stepped):
    """One dmg1_step of zero action from every state (zero velocity, zero warm start), on a monolithic and on a split engine.
    The split engine's pair kernel pulled tickets.  RK stage 0 is evaluated at the fixture state: its contact count, the hash of
    its ordered contact list and its row count are the fixture's on both engines, so g1_pair_kernel finds exactly the oracle's
    contact set on every state.  All the step leaves is bit-identical between the two engines: debug slots [:900] (the last
    stage's contact geometry out of the pair kernel included), qpos / qvel / warm start, observation, reward and done."""
    gen, F, g = cover
    a, b = stepped[1], stepped[2]
    assert not a["split"] and b["split"]
    assert all(t[2] == 0 for t in a["tickets"])
    assert all(b["tickets"][r][2] > 0 for r in range(4)), b["tickets"]      # the four RK stages went through g1_pair_kernel
    last = set()
    for i in range(len(F["qpos"])):
        want, name = contact_pairs(F, i), "state %d (kind %d)" % (i, F["kind"][i])
        for pl, r in ((1, a["rows"][i]), (2, b["rows"][i])):
            assert (int(r[1000]), int(r[1012])) == (len(want), _contact_hash(want)), ("stage 0 contact list", name, pl, r[1000], r[1012])
            assert int(r[1004]) == (int(F["nefc"][i]) & 0xFF), ("stage 0 rows", name, pl, r[1004])
        assert _same_bits(a["rows"][i], b["rows"][i]), (name, np.nonzero(_bits(a["rows"][i, :NBITS]) != _bits(b["rows"][i, :NBITS]))[0][:8])
        assert np.array_equal(_bits(a["state"][i]), _bits(b["state"][i])), name
        assert np.array_equal(_bits(a["outs"][i]), _bits(b["outs"][i])), name
        r = b["rows"][i]
        last |= {(int(x[1]), int(x[2])) for x in r[208:208 + 9 * int(r[203])].reshape(-1, 9)}
    print("   split pipeline, one step from %d states: tickets per round %s; %d distinct pairs in the last stage's contact lists, %d states ended" % (
        len(F["qpos"]), [t[2] for t in b["tickets"]], len(last), int(b["outs"][:, -1].sum())))


def test_g1_monolithic_cache_is_result_neutral(cover, fresh, torch_mod):
    """One engine, three set_state evaluations (_orders): every env's 16-entry cache holds entries of a different pose, the twin
    envs the stale hint of a near miss.  The cache does hold entries, and every row of every evaluation equals the fresh
    engine's row of the state the env holds, bit for bit; no twin carries a contact for its pair."""
    gen, F, g = cover
    order = _orders(F)
    eng, buf = _engine(len(order[0]), 1)
    for k, idx in enumerate(order):
        d = _evaluate(eng, buf, torch_mod, F["qpos"][idx])
        assert eng.sep_cache_entries()[0] > len(F["twins"]), eng.sep_cache_entries()
        for e, i in enumerate(idx):
            assert _same_bits(d[e], fresh[i]), ("evaluation %d, env %d, state %d" % (k, e, i),
                                                np.nonzero(_bits(d[e, :NBITS]) != _bits(fresh[i, :NBITS]))[0][:8])
        _no_twin_touches(F, idx, d, k)
    print("   monolithic cache entries alive after the three evaluations:", eng.sep_cache_entries()[0])
    eng.close()


def test_g1_pair_kernel_cache_is_result_neutral(cover, stepped, torch_mod):
    """The same three orders as steps of ONE split engine: the per-(env, pair) cache of g1_pair_kernel holds what the four stages
    of another pose's step (or of the near-miss twin's) left.  The cache does hold entries; debug slots [:900] and the state after
    each step equal those of the fresh split engine's step from the same state, bit for bit."""
    gen, F, g = cover
    order = _orders(F)
    ref = stepped[2]
    eng, buf = _engine(len(order[0]), 2, torch_mod)
    assert eng.split
    for k, idx in enumerate(order):
        r = _step(eng, buf, torch_mod, F["qpos"][idx])
        assert eng.sep_cache_entries()[1] > len(F["twins"]), eng.sep_cache_entries()
        assert eng.queue_counters()[0][2] > 0
        for e, i in enumerate(idx):
            assert _same_bits(r["rows"][e], ref["rows"][i]), ("step %d, env %d, state %d" % (k, e, i),
                                                              np.nonzero(_bits(r["rows"][e, :NBITS]) != _bits(ref["rows"][i, :NBITS]))[0][:8])
            assert np.array_equal(_bits(r["state"][e]), _bits(ref["state"][i])), ("step %d, env %d, state %d" % (k, e, i))
    print("   pair-kernel cache entries alive after the three steps:", eng.sep_cache_entries()[1])
    eng.close()


def test_g1_null_cache_leaves_the_same_bits(cover, fresh, torch_mod):
    """dmg1_set_null_cache hands np_convex of the monolithic kernel a null cache: the same bits as with it on every state, twice
    over (the second evaluation gives every env another state), and the switch took effect: the cache has no live entry
    afterwards, where the default engine of the test above has some after one evaluation."""
    gen, F, g = cover
    order = _orders(F)
    eng, buf = _engine(len(order[0]), 1)
    eng.set_null_cache(True)
    for idx in order[:2]:
        d = _evaluate(eng, buf, torch_mod, F["qpos"][idx])
        for e, i in enumerate(idx):
            assert _same_bits(d[e], fresh[i]), "env %d, state %d" % (e, i)
    assert eng.sep_cache_entries() == (0, 0)
    eng.set_null_cache(False)
    _evaluate(eng, buf, torch_mod, F["qpos"][order[0]])
    assert eng.sep_cache_entries()[0] > 0
    eng.close()
