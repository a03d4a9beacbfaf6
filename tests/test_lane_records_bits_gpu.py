"""Kinematics, velocities, contacts and accelerations of dm_step_kernel and dm_step_kernel_w3, bit for bit against a recording:
the step kernels may read their model constants from the lane-major records (csrc/dm_tables.h) and request them a phase ahead,
what they compute from them may not change.  The other two recordings hold qacc and the state; this one holds the debug-row slots
xpos, geom_xpos, cvel, qacc, qacc_smooth, the contact list (geom1, geom2, dist), ncon / nefc / solver_iter / nlimit / overflow
after a forward evaluation and after one RK4 step (the step's last evaluation), on the 16 airborne states of
test_factor_bits_gpu.py followed by the 108 constraint-path states of tests/constraint_path_states.py.
tests/golden/lane_records_bits.npz was recorded on an MI355X by tests/golden/make_lane_records_bits.py from the library as it was
before the records.  One array set per kernel variant: 124 envs run the two-wave kernel, the same states tiled to >= 3072 envs
the three-wave kernel; the two need not equal each other."""
import os

import numpy as np
import pytest

import constraint_path_states as cps
import test_factor_bits_gpu as fb

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lane_records_bits.npz")
NSTATES = fb.NSTATES + 108
VARIANTS = {"w2": 1, "w3": None}        # variant -> tile count (None: the smallest that reaches 3072 envs)
RUNS = ("fwd", "rk4")
# debug row slots (include/deepmimic_hip.h)
SLOTS = dict(xpos=slice(0, 42), gpos=slice(42, 90), cvel=slice(90, 174), qacc=slice(174, 208), qacc_smooth=slice(208, 242),
             counts=slice(242, 247), contacts=slice(256, 352))
NCON, NEFC, NLIMIT, OVERFLOW = 0, 1, 3, 4   # within counts


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def all_states(model, clips):
    """qpos [124, 35], qvel [124, 34], warm [124, 34], act [124, 28] as fp32: the airborne states (their own actions, no warm
    start), then the constraint-path states (their own warm start, zero actions)."""
    A, C = fb.airborne_states(model, clips), cps.humanoid_states(model)
    na, nc = len(A["qpos"]), len(C["qpos"])
    cat = lambda a, b: np.concatenate([np.asarray(a, np.float32), np.asarray(b, np.float32)])
    return dict(qpos=cat(A["qpos"], C["qpos"]), qvel=cat(A["qvel"], C["qvel"]), warm=cat(np.zeros((na, 34)), C["warm"]),
                act=cat(A["act"], np.zeros((nc, 28))))


def _tiles_equal(a, what):
    for k in range(1, a.shape[0]):
        assert np.array_equal(_bits(a[0]), _bits(a[k])), "%s: tile %d differs from tile 0" % (what, k)
    return a[0]


def compute(model, clips, torch, H):
    """What the fixture holds, from the library under test: name -> int32 array (fp32 bit patterns), one set per variant and run."""
    from deepmimic_mujoco_amd._lib import HipEngine
    n = len(H["qpos"])
    out = {k + "_in": _bits(H[k]) for k in ("qpos", "qvel", "warm", "act")}
    for v, tile in VARIANTS.items():
        tile = tile or -(-3072 // n)
        assert (n * tile >= 3072) == (v == "w3")
        t = lambda a: torch.tensor(np.tile(a, (tile, 1)), dtype=torch.float32, device="cuda:0").contiguous()
        for run in RUNS:
            eng = HipEngine(model, n * tile, auto_reset=False)
            eng.load_clip(0, clips["walk"])
            act = t(H["act"])
            eng.set_state(t(H["qpos"]), t(H["qvel"]), t(H["warm"]), act)
            dbg = eng.enable_debug()
            if run == "fwd":
                eng.forward()
            else:
                eng.step(act, eng.alloc_outputs())
            torch.cuda.synchronize()
            d = _tiles_equal(dbg.cpu().numpy().reshape(tile, n, -1), "%s %s debug rows" % (v, run))
            eng.close()
            out.update({"%s_%s_%s" % (v, run, k): _bits(d[:, s]) for k, s in SLOTS.items()})
    return out


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def states(model, clips):
    return all_states(model, clips)


@pytest.fixture(scope="module")
def golden():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def got(model, clips, torch_mod, states):
    return compute(model, clips, torch_mod, states)


def test_fixture_covers_every_geom_and_hinge(model, states, golden):
    """On the fixture alone: it was taken at the 124 states the generators give today; every geom of the candidate-pair table is in
    at least one recorded contact (so every contact-row record is read), and every hinge is beyond a bound, i.e. owns a limit
    row, in at least one state (so every limit-row record is read); the recorded limit-row count of a forward evaluation is the
    number of hinges beyond a bound wherever the rows were not cut."""
    for k in ("qpos", "qvel", "warm", "act"):
        assert golden[k + "_in"].shape[0] == NSTATES and np.array_equal(_bits(states[k]), golden[k + "_in"]), k
    npair = int(model.npair)
    can_collide = set(int(g) for g in model.pair_geom1[:npair]) | set(int(g) for g in model.pair_geom2[:npair])
    q = golden["qpos_in"].view(np.float32)[:, 7:]
    lo, hi = (model.jnt_range[1:, i].astype(np.float32) for i in (0, 1))
    beyond = (q < lo) | (q > hi)
    assert beyond.any(axis=0).all(), "hinges never beyond a bound: %s" % np.nonzero(~beyond.any(axis=0))[0]
    for v in VARIANTS:
        seen = set()
        for run in RUNS:
            counts = golden["%s_%s_counts" % (v, run)].view(np.float32)
            con = golden["%s_%s_contacts" % (v, run)].view(np.float32).reshape(NSTATES, 32, 3)
            for s in range(NSTATES):
                seen |= set(int(g) for g in con[s, :int(counts[s, NCON]), :2].ravel())
            for k in ("xpos", "gpos", "cvel", "qacc", "qacc_smooth"):
                assert np.isfinite(golden["%s_%s_%s" % (v, run, k)].view(np.float32)).all(), (v, run, k)
        assert can_collide <= seen, "%s: geoms never in a recorded contact: %s" % (v, sorted(can_collide - seen))
        counts = golden[v + "_fwd_counts"].view(np.float32)
        uncut = (counts[:, OVERFLOW].astype(np.int64) & 2) == 0
        assert np.array_equal(counts[uncut, NLIMIT].astype(np.int64), beyond[uncut].sum(axis=1)), v
        assert (counts[:, NLIMIT] > 0).sum() >= 12


def _compare(got, golden, keys):
    for k in keys:
        bad = np.nonzero((got[k] != golden[k]).any(axis=1))[0]
        assert bad.size == 0, "%s differs on %d of %d states, first: state %d" % (k, bad.size, len(got[k]), bad[0])


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_forward_bits(got, golden, variant):
    """set_state + forward(): body and geom positions, body velocities, the contact list and counts, both accelerations."""
    _compare(got, golden, ["%s_fwd_%s" % (variant, k) for k in SLOTS])


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_rk4_step_bits(got, golden, variant):
    """One dm_step: the same slots as the step's last evaluation left them."""
    _compare(got, golden, ["%s_rk4_%s" % (variant, k) for k in SLOTS])
