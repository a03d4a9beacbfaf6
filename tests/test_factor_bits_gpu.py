"""M, its L^T D L factorisation and the triangular solves of fwd_smooth (csrc/dm_kernels.hip), bit for bit against a recording:
the column elimination may be emitted in any topological order of its dependency DAG (topo::FACTOR_SCHED), its arithmetic may not
change.  16 airborne states (clip frames of walk and spinkick with seeded joint-angle and velocity edits, the root lifted 2 m, no
contact and no joint at a limit, so qacc_smooth and qacc hold nothing but M, the factor and the solves) go through a forward
evaluation, one RK4 step with fixed non-zero actions and one step of integrator="Euler", whose implicit damping runs the second
instantiation of the factorisation (M + h B).  qacc, qacc_smooth and the final qpos / qvel must have the bits of
tests/golden/factor_bits.npz, recorded on an MI355X by tests/golden/make_factor_bits.py from the library as it was before the
elimination was rescheduled.  One array set per kernel variant: 16 envs run the two-wave kernel, the same states tiled to 3072
envs the three-wave kernel; the two need not equal each other."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "factor_bits.npz")
NSTATES = 16
LIFT = 2.0
HORIZON = 0.04      # seconds over which a joint moving at its start velocity stays inside the margins (timestep 0.0166)
VARIANTS = {"w2": 1, "w3": None}        # variant -> tile count (None: the smallest that reaches 3072 envs)
# debug row slots (include/deepmimic_hip.h)
QACC, QACC_SMOOTH, NCON, NEFC = slice(174, 208), slice(208, 242), 242, 243


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def airborne_states(model, clips):
    """qpos [16, 35], qvel [16, 34], actions [16, 28], fp32-rounded: 8 frames each of walk and spinkick, joint angles and
    velocities perturbed (seeded), angles kept a quarter of their range (at most 0.3 rad) inside it, the root 2 m above its clip height.  A draw in
    which the fp64 oracle finds a contact between two bodies or a constraint row is drawn again."""
    from oracle.oracle import OracleSim
    sim = OracleSim(model)
    sim.set_caps(32, 128)
    rng = np.random.default_rng(20240611)
    span = model.jnt_range[1:, 1] - model.jnt_range[1:, 0]
    lo, hi = model.jnt_range[1:, 0] + np.minimum(0.3, 0.25 * span), model.jnt_range[1:, 1] - np.minimum(0.3, 0.25 * span)
    qs, vs = [], []
    for name in ("walk", "spinkick"):
        q_all, v_all = clips[name].tables()[:2]
        for f in np.linspace(0, len(q_all) - 1, NSTATES // 2).astype(int):
            for attempt in range(20):
                q, v = np.array(q_all[f], np.float64), np.array(v_all[f], np.float64)
                q[2] += LIFT
                q[7:] = np.clip(q[7:] + rng.normal(0.0, 0.2, 28), lo, hi)
                v += rng.normal(0.0, 1.0, 34) * rng.choice([0.1, 1.0, 5.0])
                v[6:] = np.clip(v[6:], (lo - q[7:]) / HORIZON, (hi - q[7:]) / HORIZON)     # no limit row within the step either
                q, v = q.astype(np.float32), v.astype(np.float32)
                sim.set("ctrl", np.zeros(28))
                sim.set("qacc_warmstart", np.zeros(34))
                if sim.set_state(q.astype(np.float64), v.astype(np.float64)) == 0 and sim.nefc == 0 and len(sim.get("contact")) == 0:
                    break
            else:
                raise AssertionError("no contact-free draw at %s frame %d" % (name, f))
            qs.append(q)
            vs.append(v)
    act = rng.uniform(-0.8, 0.8, (NSTATES, 28))
    return {k: np.asarray(a, np.float32) for k, a in (("qpos", qs), ("qvel", vs), ("act", act))}


def _tiles_equal(a, what):
    for k in range(1, a.shape[0]):
        assert np.array_equal(_bits(a[0]), _bits(a[k])), "%s: tile %d differs from tile 0" % (what, k)
    return a[0]


def compute(model, clips, torch, H):
    """What the fixture holds, from the library under test: name -> int32 array (fp32 bit patterns), one set per variant."""
    from deepmimic_mujoco_amd._lib import HipEngine
    n = len(H["qpos"])
    out = dict(qpos_in=_bits(H["qpos"]), qvel_in=_bits(H["qvel"]), act_in=_bits(H["act"]))
    for v, tile in VARIANTS.items():
        tile = tile or -(-3072 // n)
        assert (n * tile >= 3072) == (v == "w3")
        t = lambda a: torch.tensor(np.tile(a, (tile, 1)), dtype=torch.float32, device="cuda:0").contiguous()
        for run, integrator in (("fwd", None), ("rk4", None), ("euler", "Euler")):
            eng = HipEngine(model, n * tile, auto_reset=False, integrator=integrator)
            eng.load_clip(0, clips["walk"])
            act = t(H["act"])
            eng.set_state(t(H["qpos"]), t(H["qvel"]), torch.zeros(n * tile, 34, device=eng.device), act)
            dbg = eng.enable_debug()
            if run == "fwd":
                eng.forward()
            else:
                eng.step(act, eng.alloc_outputs())
            torch.cuda.synchronize()
            d = _tiles_equal(dbg.cpu().numpy().reshape(tile, n, -1), "%s %s debug rows" % (v, run))
            q, qv = (_tiles_equal(x.cpu().numpy().reshape(tile, n, -1), "%s %s state" % (v, run)) for x in eng.get_state()[:2])
            eng.close()
            out.update({"%s_%s_qacc" % (v, run): _bits(d[:, QACC]), "%s_%s_qacc_smooth" % (v, run): _bits(d[:, QACC_SMOOTH]),
                        "%s_%s_rows" % (v, run): _bits(d[:, [NCON, NEFC]])})
            if run != "fwd":
                out.update({"%s_%s_qpos" % (v, run): _bits(q), "%s_%s_qvel" % (v, run): _bits(qv)})
    return out


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def states(model, clips):
    return airborne_states(model, clips)


@pytest.fixture(scope="module")
def golden():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def got(model, clips, torch_mod, states):
    return compute(model, clips, torch_mod, states)


def test_fixture_is_of_these_states(states, golden):
    """16 states, the inputs the generator gives today, none with a contact or a limit row in any recorded run, and the
    accelerations finite and not all alike (the states vary the magnitudes)."""
    for k in ("qpos", "qvel", "act"):
        assert golden[k + "_in"].shape[0] == NSTATES and np.array_equal(_bits(states[k]), golden[k + "_in"]), k
    for v in VARIANTS:
        for run in ("fwd", "rk4", "euler"):
            assert not golden["%s_%s_rows" % (v, run)].any(), (v, run)
            for k in ("qacc", "qacc_smooth"):
                a = golden["%s_%s_%s" % (v, run, k)].view(np.float32)
                assert a.shape == (NSTATES, 34) and np.isfinite(a).all() and np.unique(np.abs(a).max(axis=1)).size == NSTATES
        assert golden[v + "_rk4_qpos"].shape == (NSTATES, 35) and golden[v + "_euler_qvel"].shape == (NSTATES, 34)


def _compare(got, golden, keys):
    for k in keys:
        bad = np.nonzero((got[k] != golden[k]).any(axis=1))[0]
        assert bad.size == 0, "%s differs on %d of %d states, first: state %d" % (k, bad.size, len(got[k]), bad[0])


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_forward_bits(got, golden, variant):
    """set_state + forward(): qacc_smooth and qacc (equal without rows) carry the recorded bits."""
    _compare(got, golden, [variant + "_fwd_" + k for k in ("rows", "qacc_smooth", "qacc")])


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_rk4_step_bits(got, golden, variant):
    """One dm_step with fixed non-zero actions: four forward evaluations, then qpos and qvel, bit for bit."""
    _compare(got, golden, [variant + "_rk4_" + k for k in ("rows", "qacc_smooth", "qacc", "qpos", "qvel")])


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_euler_step_bits(got, golden, variant):
    """One step of integrator="Euler": the second factorisation (M + h B) of the implicit joint damping."""
    _compare(got, golden, [variant + "_euler_" + k for k in ("rows", "qacc_smooth", "qacc", "qpos", "qvel")])
