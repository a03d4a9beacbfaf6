"""``dmg1_step_active`` and the evaluator's ``compact`` rule without a GPU: the header declares the entry point, the library exports
it, the ctypes table and ``G1HipEngine`` bind it, and ``evaluation.resolve_compact`` follows its table."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_dmg1_step_active_with_ten_arguments():
    hdr = open(os.path.join(ROOT, "include", "deepmimic_g1_hip.h")).read()
    m = re.search(r"\bint\s+dmg1_step_active\s*\(([^)]*)\)\s*;", hdr)
    assert m, "include/deepmimic_g1_hip.h does not declare dmg1_step_active"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 10
    assert args[0].startswith("DmG1Handle") and "int32_t *env_ids" in args[2] and args[3] == "int nslots" and args[-1] == "void *stream"


def test_library_exports_and_binds_dmg1_step_active():
    import ctypes as C
    from deepmimic_mujoco_amd import _lib, g1
    assert "dmg1_step_active" in g1.EXPORTS
    L = g1._lib()
    assert getattr(_lib.load_library(), "dmg1_step_active") is not None
    argtypes = L.dmg1_step_active.argtypes
    assert len(argtypes) == 10
    assert argtypes[3] is C.c_int and all(a is C.c_void_p for i, a in enumerate(argtypes) if i != 3)


def test_engine_classes_have_step_active():
    from deepmimic_mujoco_amd._lib import EngineBase, HipEngine
    from deepmimic_mujoco_amd.g1 import G1HipEngine
    assert callable(getattr(G1HipEngine, "step_active", None))
    assert callable(getattr(HipEngine, "step_active", None))
    assert G1HipEngine.PREFIX == "dmg1_" and issubclass(G1HipEngine, EngineBase)


def test_resolve_compact_table():
    from deepmimic_mujoco_amd.evaluation import resolve_compact
    humanoid, g1 = True, False
    assert resolve_compact(True, humanoid) is True
    assert resolve_compact(True, g1) is False
    assert resolve_compact("all", humanoid) is True and resolve_compact("all", g1) is True
    assert resolve_compact(False, humanoid) is False and resolve_compact(False, g1) is False
    for bad in ("ALL", "yes", "", None, 1, 0, 2, "true", [True]):
        for h in (humanoid, g1):
            with pytest.raises(ValueError):
                resolve_compact(bad, h)


def test_evaluate_policy_and_run_episodes_take_compact():
    import inspect
    from deepmimic_mujoco_amd import evaluation
    for fn in (evaluation.run_episodes, evaluation.evaluate_policy, evaluation.evaluation_record):
        assert "compact" in inspect.signature(fn).parameters, fn.__name__
    assert inspect.signature(evaluation.BatchEvaluator.__init__).parameters["compact"].default is True
