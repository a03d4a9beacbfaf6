"""The triangular solves of the step kernels (solve_LT / solve_L in csrc/dm_kernels.hip), bit for bit against a recording: they may
be emitted in any order that keeps, per lane, the sequence of its FMAs (topo::SOLVE_L_SCHED / SOLVE_LT_SCHED), their arithmetic
may not change.  24 airborne states go through a forward evaluation, one RK4 step and one step of integrator="Euler" (whose
implicit damping runs the solves on the second factor, M + h B): the 16 of test_factor_bits_gpu.airborne_states, and 8 chosen for
exact zeros in the right-hand sides, where the order of the `x + (-0 * x_k)` operations of the lanes outside a step's mask could
show in the sign of a zero: the root lifted 2 m, qvel = 0 and zero action (walk frame 0), then the same with one non-zero joint
velocity in one limb (each of the five limbs, signs alternating) and with one in every limb (all positive, all negative).  No
state has a contact or a joint at a limit, by the same fp64 oracle check, so qacc_smooth and qacc hold nothing but M, the factor
and the solves.  qacc, qacc_smooth and the final qpos / qvel must have the bits of tests/golden/solve_bits.npz, recorded on an
MI355X by tests/golden/make_solve_bits.py from the library as it was before the solves were rescheduled.  One array set per kernel
variant: 24 envs run the two-wave kernel, the same states tiled to 3072 envs the three-wave kernel (all tiles equal)."""
import os

import numpy as np
import pytest

import test_factor_bits_gpu as fb

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solve_bits.npz")
NZERO = 8
NSTATES = fb.NSTATES + NZERO
LIMB_DOF = (10, 13, 17, 23, 30)      # one dof inside each of the five limbs (dofs 9..11, 12..15, 16..19, 20..26, 27..33)
RUNS = ("fwd", "rk4", "euler")


def zero_states(model, clips):
    """qpos [8, 35], qvel [8, 34], act [8, 28] (all zero), fp32: walk frame 0 lifted 2 m, joint angles kept inside their ranges as
    airborne_states() keeps them; qvel zero but for +-1 rad/s on the dofs named in the module docstring.  Each state is checked
    contact- and limit-free with the fp64 oracle."""
    from oracle.oracle import OracleSim
    sim = OracleSim(model)
    sim.set_caps(32, 128)
    span = model.jnt_range[1:, 1] - model.jnt_range[1:, 0]
    lo, hi = model.jnt_range[1:, 0] + np.minimum(0.3, 0.25 * span), model.jnt_range[1:, 1] - np.minimum(0.3, 0.25 * span)
    q = np.array(clips["walk"].tables()[0][0], np.float64)
    q[2] += fb.LIFT
    q[7:] = np.clip(q[7:], lo, hi)
    q = q.astype(np.float32)
    vels = [{}] + [{d: (1.0 if n % 2 == 0 else -1.0)} for n, d in enumerate(LIMB_DOF)]
    vels += [{d: 1.0 for d in LIMB_DOF}, {d: -1.0 for d in LIMB_DOF}]
    assert len(vels) == NZERO
    qs, vs = [], []
    for spec in vels:
        v = np.zeros(34, np.float32)
        for d, s in spec.items():
            v[d] = s
        assert np.all(v[6:] >= (lo - q[7:]) / fb.HORIZON) and np.all(v[6:] <= (hi - q[7:]) / fb.HORIZON)
        sim.set("ctrl", np.zeros(28))
        sim.set("qacc_warmstart", np.zeros(34))
        assert sim.set_state(q.astype(np.float64), v.astype(np.float64)) == 0 and sim.nefc == 0 and len(sim.get("contact")) == 0
        qs.append(q)
        vs.append(v)
    return {"qpos": np.asarray(qs, np.float32), "qvel": np.asarray(vs, np.float32), "act": np.zeros((NZERO, 28), np.float32)}


def solve_states(model, clips):
    A, Z = fb.airborne_states(model, clips), zero_states(model, clips)
    return {k: np.concatenate([A[k], Z[k]]) for k in ("qpos", "qvel", "act")}


def compute(model, clips, torch, H):
    """What the fixture holds, from the library under test (the recorder of test_factor_bits_gpu at these 24 states)."""
    return fb.compute(model, clips, torch, H)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def states(model, clips):
    return solve_states(model, clips)


@pytest.fixture(scope="module")
def golden():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def got(model, clips, torch_mod, states):
    return compute(model, clips, torch_mod, states)


def test_fixture_is_of_these_states(states, golden):
    """24 states, the inputs the generators give today, none with a contact or a limit row in any recorded run, every recorded
    value finite; the zero-velocity state's smooth acceleration is not all zero (gravity), so the solves ran on it."""
    for k in ("qpos", "qvel", "act"):
        assert golden[k + "_in"].shape[0] == NSTATES and np.array_equal(fb._bits(states[k]), golden[k + "_in"]), k
    assert not states["qvel"][fb.NSTATES].any() and not states["act"][fb.NSTATES:].any()
    for v in fb.VARIANTS:
        for run in RUNS:
            assert not golden["%s_%s_rows" % (v, run)].any(), (v, run)
            for k in ("qacc", "qacc_smooth"):
                a = golden["%s_%s_%s" % (v, run, k)].view(np.float32)
                assert a.shape == (NSTATES, 34) and np.isfinite(a).all() and a[fb.NSTATES].any()
        assert golden[v + "_rk4_qpos"].shape == (NSTATES, 35) and golden[v + "_euler_qvel"].shape == (NSTATES, 34)


def _compare(got, golden, keys):
    for k in keys:
        bad = np.nonzero((got[k] != golden[k]).any(axis=1))[0]
        assert bad.size == 0, "%s differs on %d of %d states, first: state %d" % (k, bad.size, len(got[k]), bad[0])


@pytest.mark.parametrize("variant", list(fb.VARIANTS))
def test_forward_bits(got, golden, variant):
    """set_state + forward(): qacc_smooth and qacc (equal without rows) carry the recorded bits."""
    _compare(got, golden, [variant + "_fwd_" + k for k in ("rows", "qacc_smooth", "qacc")])


@pytest.mark.parametrize("variant", list(fb.VARIANTS))
def test_rk4_step_bits(got, golden, variant):
    """One dm_step: four forward evaluations, then qpos and qvel, bit for bit."""
    _compare(got, golden, [variant + "_rk4_" + k for k in ("rows", "qacc_smooth", "qacc", "qpos", "qvel")])


@pytest.mark.parametrize("variant", list(fb.VARIANTS))
def test_euler_step_bits(got, golden, variant):
    """One step of integrator="Euler": solve_LT and solve_L on the factor of M + h B (euler_damped_solve)."""
    _compare(got, golden, [variant + "_euler_" + k for k in ("rows", "qacc_smooth", "qacc", "qpos", "qvel")])
