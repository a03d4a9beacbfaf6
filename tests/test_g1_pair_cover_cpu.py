"""tests/golden/g1_pair_cover.npz (tests/golden/make_g1_pair_cover.py) against the live fp64 G1 oracle, without a GPU: every stored
answer is the oracle's, every state is float32-exact, uncut, clear of the joint limits and keeps its contact pair list under the
generator's perturbations; the cover reaches all 14 geom-type classes and at least 740 of the model's collision pairs; every
near-miss twin misses its pair inside the bounding-sphere filter while its partner touches.  tests/test_g1_pair_cover_gpu.py
holds the HIP narrowphase to the same file."""
import importlib.util
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "g1_pair_cover.npz")


def load_generator():
    spec = importlib.util.spec_from_file_location("make_g1_pair_cover", os.path.join(GOLDEN, "make_g1_pair_cover.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def contact_pairs(F, i):
    return [(int(a), int(b)) for a, b in F["con_geom"][F["con_start"][i]:F["con_start"][i + 1]]]


@pytest.fixture(scope="module")
def cover():
    gen = load_generator()
    with np.load(FIXTURE) as z:
        F = {k: z[k] for k in z.files}
    return gen, F, gen.Oracle()


def test_fixture_layout_and_size(cover):
    gen, F, ora = cover
    n = len(F["qpos"])
    assert os.path.getsize(FIXTURE) < gen.MAX_BYTES
    assert F["qpos"].dtype == np.float32 and F["qpos"].shape == (n, 44)
    for k in ("con_dist", "con_pos", "con_normal", "xpos"):
        assert F[k].dtype == np.float64, k
    assert F["xpos"].shape == (n, 39, 3)
    assert F["con_start"].shape == (n + 1,) and F["con_start"][0] == 0 and F["con_start"][-1] == len(F["con_dist"])
    assert np.array_equal(np.diff(F["con_start"]), F["ncon"])
    assert len(F["con_geom"]) == len(F["con_pos"]) == len(F["con_normal"]) == len(F["con_dist"])
    assert int(F["seed"]) == gen.SEED
    assert np.abs(np.linalg.norm(F["qpos"][:, 3:7].astype(np.float64), axis=1) - 1).max() < 1e-6
    assert len(np.unique(F["qpos"], axis=0)) == n, "a state is stored twice"


def test_every_stored_answer_is_the_live_oracle_s(cover):
    """A fresh sim per state at the engine's caps, fed the stored float32 values with zero velocity and warm start: contact list
    identical, distance / position / normal / body positions to 1e-12, counts equal, nothing cut."""
    gen, F, ora = cover
    og = ora.og
    worst = 0.0
    for i, q in enumerate(F["qpos"]):
        s = og.G1Sim()
        s.set_caps(gen.MAXCON, gen.MAXROW)
        assert s.set_state(q.astype(np.float64), np.zeros(43)) == 0
        assert s.geti("overflow_con") == 0 and s.geti("overflow_row") == 0, i
        cons = s.contacts()
        assert [(c["geom1"], c["geom2"]) for c in cons] == contact_pairs(F, i), i
        assert (len(cons), s.geti("nefc"), s.geti("nlimit")) == (F["ncon"][i], F["nefc"][i], F["nlimit"][i]), i
        a, b = F["con_start"][i], F["con_start"][i + 1]
        if cons:
            worst = max(worst, np.abs(np.array([c["dist"] for c in cons]) - F["con_dist"][a:b]).max(),
                        np.abs(np.array([c["pos"] for c in cons]) - F["con_pos"][a:b]).max(),
                        np.abs(np.array([c["frame"][0] for c in cons]) - F["con_normal"][a:b]).max())
        worst = max(worst, np.abs(s.get("xpos").reshape(39, 3) - F["xpos"][i]).max())
        assert worst <= 1e-12, (i, worst)
        qa = s.get("qacc")
        assert np.abs(qa - F["qacc"][i]).max() <= 1e-5 * max(1.0, np.abs(qa).max()), i      # stored in float32, for information
    print("   %d states, %d contacts: worst |stored - live| %.3g" % (len(F["qpos"]), len(F["con_dist"]), worst))


def test_every_state_is_uncut_inside_the_limits_and_stable(cover):
    """By count on a sim whose caps are 200 / 500 (the oracle's overflow counters are cumulative): fewer than 48 contacts and 256
    rows; every limited joint 1e-4 rad inside its range; the ordered contact pair list unchanged under the 8 seeded perturbations
    of 1e-6 per coordinate; and no contact's distance, position or normal moves by more than 1e-7 / 1e-6 / 1e-6 (a tenth of the
    GPU test's bounds) under 6 perturbations of 1e-12: the reference is well defined where the engine is held to it."""
    gen, F, ora = cover
    for i, q in enumerate(F["qpos"]):
        c, nefc, _ = ora(q.astype(np.float64))
        assert len(c) == F["ncon"][i] < gen.MAXCON and nefc == F["nefc"][i] < gen.MAXROW, i
        assert gen.pair_list(c) == contact_pairs(F, i), i
        assert gen.limits_ok(ora.g, q), i
        assert F["nlimit"][i] == 0, i
        assert gen.stable(ora, q), "state %d changes its contact list under a 1e-6 perturbation" % i
        assert gen.conditioned(ora, q), "state %d: the oracle's own contact geometry moves under a 1e-12 perturbation" % i
    assert gen.NPERT == 8 and gen.PERT == 1e-6 and gen.LIMIT_MARGIN == 1e-4
    assert gen.COND_TOL == (1e-7, 1e-6, 1e-6) and gen.COND_PERT == 1e-12
    assert np.abs(gen.perturbation(0)).min() == 1e-6


def test_the_cover_reaches_every_class_and_740_pairs(cover):
    gen, F, ora = cover
    g = ora.g
    pairs = [(int(a), int(b)) for a, b in g.pairs]
    seen = {}
    for i in range(len(F["qpos"])):
        if F["kind"][i] != 3:
            for p in set(contact_pairs(F, i)):
                seen[p] = seen.get(p, 0) + 1
    covered = [tuple(int(x) for x in p) for p in F["covered"]]
    uncovered = [tuple(int(x) for x in p) for p in F["uncovered"]]
    assert sorted(seen) == sorted(covered)
    assert not set(covered) & set(uncovered)
    assert sorted(covered + uncovered) == sorted(pairs) and len(set(pairs)) == len(pairs) == 1013
    assert len(F["uncovered_gap"]) == len(uncovered)
    assert not np.any(np.isinf(F["uncovered_gap"]))
    per = {cl: [0, 0, 0] for cl in gen.CLASSES}
    for p in pairs:
        t = per[gen.type_class(g, *p)]
        t[0] += 1; t[1] += p in seen; t[2] += seen.get(p, 0) > 1
    print("   class               pairs covered  in two states")
    for cl in gen.CLASSES:
        print("   %-18s %6d %7d %7d" % (cl, *per[cl]))
        assert per[cl][0] > 0 and per[cl][1] > 0, cl
    print("   total              %6d %7d %7d" % (len(pairs), len(seen), sum(1 for v in seen.values() if v > 1)))
    assert len(gen.CLASSES) == 14
    assert len(seen) >= 740


def test_every_twin_misses_its_pair_inside_the_sphere_filter(cover):
    gen, F, ora = cover
    g = ora.g
    tw = F["twins"]
    assert len(tw) >= 32 and len({(int(t[2]), int(t[3])) for t in tw}) == len(tw)
    assert sorted(int(t[0]) for t in tw) == [i for i in range(len(F["qpos"])) if F["kind"][i] == 3]
    for t, partner, g1, g2 in (tuple(int(x) for x in r) for r in tw):
        assert gen.is_mpr(g, g1, g2), (g1, g2)
        assert F["kind"][partner] == 2, partner
        assert (g1, g2) in contact_pairs(F, partner) and (g1, g2) not in contact_pairs(F, t), (t, partner, g1, g2)
        c, nefc, gx = ora(F["qpos"][t].astype(np.float64), want_xpos=True)
        assert (g1, g2) not in gen.pair_list(c)
        assert np.linalg.norm(gx[g1] - gx[g2]) <= g.geom_rbound[g1] + g.geom_rbound[g2], (t, g1, g2)


def test_the_refused_states_are_ill_conditioned_in_the_oracle_alone(cover):
    """ill_qpos holds the candidates conditioned() refused: uncut, stable contact list, yet the ORACLE's own contact geometry moves
    under 1e-12 perturbations of qpos by more than the GPU test allows the engine (distance 1e-6, position 1e-5 or normal 1e-5),
    on a cylinder-mesh pair: MPR's stop tolerance on a curved side.  No GPU is involved."""
    gen, F, ora = cover
    ill = F["ill_qpos"]
    assert ill.dtype == np.float32 and ill.shape[1:] == (44,) and len(ill) >= 1
    for q32 in ill:
        assert gen.stable(ora, q32) and gen.limits_ok(ora.g, q32) and not gen.conditioned(ora, q32)
        q = q32.astype(np.float64)
        c0, _, _ = ora(q)
        move = np.zeros((len(c0), 3))
        for k in range(20):
            c, _, _ = ora(q + np.random.default_rng([gen.SEED, 3000 + k]).choice([-1e-12, 1e-12], 44))
            assert gen.pair_list(c) == gen.pair_list(c0)
            move = np.maximum(move, np.stack([np.abs(c[:, 0] - c0[:, 0]), np.abs(c[:, 1:4] - c0[:, 1:4]).max(1),
                                              np.abs(c[:, 4:7] - c0[:, 4:7]).max(1)], axis=1))
        bad = np.nonzero((move[:, 0] > 1e-6) | (move[:, 1] > 1e-5) | (move[:, 2] > 1e-5))[0]
        assert len(bad) >= 1
        for j in bad:
            g1, g2 = int(c0[j, 13]), int(c0[j, 14])
            print("   pair (%d, %d) %s, depth %.4f: under 1e-12 the oracle's distance moves %.1e, position %.1e, normal %.1e" % (
                g1, g2, gen.type_class(ora.g, g1, g2), -c0[j, 0], *move[j]))
            assert gen.is_mpr(ora.g, g1, g2)
