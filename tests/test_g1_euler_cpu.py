"""Euler integrator option of the Unitree G1 engine, the parts that need no GPU: the C ABI field, the command-line flag, and what
the fp64 oracle's mj_Euler branch (oracle/dm_oracle.c::dmo_step) does on the G1, which the GPU tests hold the engine to."""
import ctypes as C

import numpy as np
import pytest

from deepmimic_mujoco_amd.config import MotionConfig
from deepmimic_mujoco_amd.mocap import MocapDM


def test_g1_config_ends_with_the_integrator_and_defaults_to_the_models():
    from deepmimic_mujoco_amd import _lib, g1
    assert g1.DmG1Config._fields_[-1][0] == "integrator" and g1.DmG1Config._fields_[-2][0] == "pipeline"
    L = _lib.load_library()
    L.dmg1_default_config.argtypes = [C.POINTER(g1.DmG1Config)]
    L.dmg1_default_config.restype = None
    cfg = g1.DmG1Config()
    cfg.integrator = 5
    L.dmg1_default_config(C.byref(cfg))
    assert cfg.integrator == 0 == _lib.INTEGRATORS[None] == _lib.INTEGRATORS["model"]
    assert (_lib.INTEGRATORS["Euler"], _lib.INTEGRATORS["RK4"]) == (1, 2)
    assert cfg.pipeline == 0 and cfg.max_ep_length == 1000        # the fields in front of it are where they were


def test_train_parser_takes_the_integrator():
    from deepmimic_mujoco_amd import train
    ap = train.build_parser()
    assert ap.parse_args([]).integrator == "model"
    assert ap.parse_args(["--integrator", "Euler"]).integrator == "Euler"
    assert ap.parse_args(["--integrator", "RK4"]).integrator == "RK4"
    for word in ("euler", "implicit", "RK2"):
        with pytest.raises(SystemExit):
            ap.parse_args(["--integrator", word])


def _euler_model():
    from deepmimic_mujoco_amd.g1 import DmModelG1
    from oracle import oracle_g1 as og
    g, cm = og.g1_model()
    ce = DmModelG1.from_buffer_copy(cm)
    ce.integrator = 0
    assert cm.integrator == 1, "the cached model struct stays RK4"
    return og, g, ce


def test_g1_oracle_euler_step_is_finite_and_its_damping_is_implicit():
    """Eight walk frames lifted off the floor with noisy joint velocities, one mj_Euler step each: finite, and far from the explicit
    update qvel + h qacc (0.09 .. 0.74 relative in qvel on these states, max |dv| / max(1, max |v|); every hinge has damping 0.5) —
    an engine without the (M + h B) solve cannot meet the parity gates of tests/test_g1_euler_gpu.py."""
    og, g, ce = _euler_model()
    mc = MocapDM(robot="unitree_g1")
    mc.load_mocap(MotionConfig("walk", robot="unitree_g1").mocap_path)
    rng = np.random.default_rng(5)
    h = ce.timestep
    rels = []
    for fr in range(0, 40, 5):
        q, v = np.array(mc.data_config[fr], np.float64), np.array(mc.data_vel[fr], np.float64)
        q[2] += 0.3
        v = v + rng.normal(0.0, 0.5, 43)
        s = og.G1Sim(g, ce)
        s.set_caps(48, 256)
        assert s.set_state(q, v) == 0
        assert s.step(np.zeros(37)) == 0
        q1, v1, qacc = s.get("qpos"), s.get("qvel"), s.get("qacc")
        assert np.isfinite(q1).all() and np.isfinite(v1).all() and np.isfinite(qacc).all()
        explicit = v + h * qacc
        rels.append(float(np.abs(v1 - explicit).max() / max(1.0, np.abs(v1).max())))
        # position: integrated with the NEW velocity (semi-implicit)
        assert np.abs(q1[7:] - (q[7:] + h * v1[6:])).max() < 1e-12
    print("G1 oracle, Euler: implicit against explicit velocity update, relative:", ["%.3f" % r for r in rels])
    assert min(rels) > 0.05
