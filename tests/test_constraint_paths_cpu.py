"""The state generator of tests/constraint_path_states.py, checked by the oracle alone (no GPU): every path of the constraint
stage, every boundary between two paths and both caps are in the set that tests/test_constraint_paths_gpu.py runs."""
import time

import numpy as np
import pytest

import constraint_path_states as cps


@pytest.fixture(scope="module")
def states(model):
    t0 = time.time()
    H = cps.humanoid_states(model)
    print("humanoid search: %d draws, %d states, %.1f s" % (H["draws"], len(H["labels"]), time.time() - t0))
    return H


def test_humanoid_states_fill_every_quota(states):
    """At least 4 states at each nefc of 0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65 and 2 at 127 and 128 uncut; 8 inside each path's
    range; 6 on either side of the 20-active-rows transpose; 8 warm starts kept and 8 discarded; 8 PGS runs leaving early and 8
    going to `iterations`; 12 with limit rows, every limited joint beyond its low and its high bound; 6 contact-cut, 6 row-cut
    (3 of them where row 128 falls inside a pyramid, which then gets no row: nefc 125..127; 2 where it falls between two
    contacts: nefc 128) and 2 cut both ways.  Warm-started repeats of a pose count for the warm-start quotas only."""
    counts, quotas = states["counts"], states["quotas"]
    joints = [k for k in quotas if k.startswith("joint")]
    for k in quotas:
        if k not in joints:
            print("  %-36s %3d (wanted %d)" % (k, counts[k], quotas[k]))
    print("  joints beyond a bound, low / high side: %d / %d of 28" % (sum(counts[k] > 0 for k in joints if k.endswith("low")),
                                                                     sum(counts[k] > 0 for k in joints if k.endswith("high"))))
    short = {k: (counts[k], quotas[k]) for k in quotas if counts[k] < quotas[k]}
    assert not short, short
    # the counts are what the labels say, and the labels are the oracle's: spot-check the set from scratch
    L = states["labels"]
    assert len(L) == len(states["qpos"]) <= 160
    for n in cps.BOUNDARY_NEFC:
        assert sum(1 for x in L if x["nefc"] == n and not x["warm_nonzero"] and not (x["cut_con"] or x["cut_row"])) >= 4, n
    assert all(x["ncon"] == cps.MAXCON for x in L if x["cut_con"]) and all(cps.MAXROW - 4 < x["nefc"] <= cps.MAXROW for x in L if x["cut_row"])
    assert all(x["straddle"] == (x["nefc"] < cps.MAXROW) for x in L if x["cut_row"])
    assert all(x["ncon"] <= cps.MAXCON and x["nefc"] <= cps.MAXROW for x in L)
    f32 = lambda a: np.array_equal(a, a.astype(np.float32).astype(np.float64))
    assert f32(states["qpos"]) and f32(states["qvel"]) and f32(states["warm"])


def test_humanoid_labels_are_the_oracles(model, states):
    """A fresh oracle environment, given each state, reports the labelled counts and cuts; the dense mass matrix and the rows
    exported for the force check reproduce the oracle's own constraint acceleration (qacc - qacc_smooth = M^-1 J^T f)."""
    from oracle.oracle import OracleSim
    s = OracleSim(model)
    s.set_caps(cps.MAXCON, cps.MAXROW)
    worst = 0.0
    for q, v, w, lab in zip(states["qpos"], states["qvel"], states["warm"], states["labels"]):
        oc, orow = s.geti("overflow_con"), s.geti("overflow_row")          # the two counters accumulate
        s.set("qacc_warmstart", w)
        assert s.set_state(q, v) == 0
        got = (s.nefc, s.ncon, s.geti("nlimit"), s.geti("overflow_con") > oc, s.geti("overflow_row") > orow, s.geti("solver_iter"))
        assert got == (lab["nefc"], lab["ncon"], lab["nlimit"], lab["cut_con"], lab["cut_row"], lab["sweeps"]), cps.describe(lab)
        ref = lab["ref"]
        assert np.array_equal(ref["qacc"], s.get("qacc"))
        if "M" in ref:
            dq = np.linalg.solve(ref["M"], ref["J"].T @ ref["force"])
            worst = max(worst, np.abs(dq - (ref["qacc"] - ref["qacc_smooth"])).max() / max(1.0, np.abs(ref["qacc"]).max()))
    print("M^-1 J^T f against the oracle's qacc - qacc_smooth: worst relative difference %.2e" % worst)
    assert worst < 1e-9


def test_generators_are_reproducible(model, states):
    cps._CACHE.clear()
    try:
        again = cps.humanoid_states(model)
    finally:
        cps._CACHE.clear()
    for k in ("qpos", "qvel", "warm"):
        assert np.array_equal(states[k], again[k]), k
    assert [cps.describe(a) for a in states["labels"]] == [cps.describe(b) for b in again["labels"]]
    g1, g2 = cps.g1_states(), None
    cps._CACHE.pop(("g1", 7, 400, 0))
    g2 = cps.g1_states()
    assert np.array_equal(g1["qpos"], g2["qpos"]) and np.array_equal(g1["qvel"], g2["qvel"])


def test_sweep_counts_are_stable_on_most_states(model, states):
    """The GPU test compares sweep counts where the oracle's count survives its tolerance scaled by 0.9 and by 1.1, and skips
    the rest: the share it can compare must stay at least 80 % of the constrained states."""
    tol = model.cstruct.tolerance
    con = [x for x in states["labels"] if x["nefc"] > 0]
    share = np.mean([x["stable"] for x in con])
    print("sweep count stable under tolerance x 0.9 / x 1.1: %d of %d constrained states (%.1f %%)" %
          (sum(x["stable"] for x in con), len(con), 100 * share))
    assert share >= 0.8
    assert model.cstruct.tolerance == tol == 1e-8, "the generator must put the solver tolerance back"


def test_g1_states_reach_the_contact_cap():
    """Getup frames pressed 2..9 cm into the floor, joints +-0.5 rad off the clip: at least 8 states cut by the 48-contact cap
    and 8 uncut controls of 40..48 contacts.  Row-cut states (more than 256 rows) are searched for with every joint beyond a
    bound with probability 0.9, at most 200 draws; the pressed family alone peaks below 256 rows."""
    t0 = time.time()
    G = cps.g1_states(row_cut_draws=200)
    kinds = [x["kind"] for x in G["labels"]]
    print("G1 search: %d + %d draws, %.1f s; contact-cut %d, controls %d, row-cut %d; rows %s" %
          (G["draws"], G["row_cut_draws"], time.time() - t0, kinds.count("cut"), kinds.count("control"), kinds.count("row-cut"),
           [x["nefc"] for x in G["labels"]]))
    assert kinds.count("cut") >= 8 and kinds.count("control") >= 8
    for x in G["labels"]:
        assert x["ncon"] <= cps.G1_MAXCON and x["nefc"] <= cps.G1_MAXROW
        if x["kind"] == "cut":
            assert x["ncon"] == cps.G1_MAXCON and x["cut_con"] and not x["cut_row"]
        elif x["kind"] == "control":
            assert 40 <= x["ncon"] <= cps.G1_MAXCON and not x["cut_con"] and not x["cut_row"]
        else:
            assert cps.G1_MAXROW - 4 < x["nefc"] <= cps.G1_MAXROW and x["cut_row"]
    assert kinds.count("row-cut") >= 1, "the joints-beyond-bounds family no longer reaches the 256-row cap"
