"""The constraint rows of dm_step_kernel and dm_step_kernel_w3, bit for bit against a recording: build_row's back-substitution
(csrc/dm_kernels.hip) may be rescheduled, its arithmetic may not change.  On the 108 humanoid states of
tests/constraint_path_states.py (nefc 0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127 / 128, contact-cut, row-cut: build_row<true>,
build_row<false> and both rows per lane of the wide path) a forward evaluation and one RK4 step with zero actions must leave the
bits of tests/golden/constraint_rows_bits.npz, recorded on an MI355X by tests/golden/make_constraint_rows_bits.py from the
library as it was before the factor-row prefetch.  One array set per kernel variant: 108 envs run the two-wave kernel, the same
states tiled to >= 3072 envs the three-wave kernel; the two need not equal each other."""
import os

import numpy as np
import pytest

import constraint_path_states as cps

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "constraint_rows_bits.npz")
NSTATES = 108
VARIANTS = {"w2": 1, "w3": None}        # variant -> tile count (None: the smallest that reaches 3072 envs)
PATHS = ("0", "1..7", "8..32", "33..64", "65..128", "cut")
# debug row slots (include/deepmimic_hip.h)
QACC, QACC_SMOOTH, COUNTS, STAGES, FORCE = slice(174, 208), slice(208, 242), slice(242, 247), slice(247, 249), slice(352, 416)


def _engine(model, clips, n):
    from deepmimic_mujoco_amd._lib import HipEngine
    eng = HipEngine(model, n, auto_reset=False)
    eng.load_clip(0, clips["walk"])
    return eng


def _put(eng, torch, H, tile):
    t = lambda a: torch.tensor(np.tile(a, (tile, 1)), dtype=torch.float32, device=eng.device).contiguous()
    eng.set_state(t(H["qpos"]), t(H["qvel"]), t(H["warm"]), torch.zeros(len(H["qpos"]) * tile, 28, device=eng.device))


def _path(lab):
    if lab["cut_con"] or lab["cut_row"]:
        return "cut"
    n = lab["nefc"]
    return "0" if n == 0 else "1..7" if n < 8 else "8..32" if n <= 32 else "33..64" if n <= 64 else "65..128"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _tiles_equal(a, what):
    """[tile, states, k] -> tile 0, after every other tile was seen to hold the same bits."""
    for k in range(1, a.shape[0]):
        assert np.array_equal(_bits(a[0]), _bits(a[k])), "%s: tile %d differs from tile 0" % (what, k)
    return a[0]


def compute(model, clips, torch, H):
    """What the fixture holds, from the library under test: name -> int32 array (fp32 bit patterns), one set per variant."""
    n = len(H["qpos"])
    out = dict(qpos_in=_bits(H["qpos"]), qvel_in=_bits(H["qvel"]), warm_in=_bits(H["warm"]),
               path=np.array([_path(lab) for lab in H["labels"]]))
    for v, tile in VARIANTS.items():
        tile = tile or -(-3072 // n)
        assert (n * tile >= 3072) == (v == "w3")
        # ---- set_state + forward(), debug rows on
        eng = _engine(model, clips, n * tile)
        _put(eng, torch, H, tile)
        dbg = eng.enable_debug()
        eng.forward()
        torch.cuda.synchronize()
        d = _tiles_equal(dbg.cpu().numpy().reshape(tile, n, -1), v + " forward")
        eng.close()
        nefc = d[:, 243].astype(np.int64)
        force = np.where(((nefc > 0) & (nefc <= 64))[:, None], d[:, FORCE], 0)      # not written without rows / on the wide path
        out.update({v + "_fwd_qacc": _bits(d[:, QACC]), v + "_fwd_qacc_smooth": _bits(d[:, QACC_SMOOTH]),
                    v + "_fwd_force": _bits(force), v + "_fwd_counts": _bits(d[:, COUNTS]), v + "_fwd_stages": _bits(d[:, STAGES])})
        # ---- one dm_step, zero actions
        eng = _engine(model, clips, n * tile)
        _put(eng, torch, H, tile)
        dbg = eng.enable_debug()
        eng.step(torch.zeros(n * tile, 28, device=eng.device), eng.alloc_outputs())
        torch.cuda.synchronize()
        q, qv, w, _ = (x.cpu().numpy().reshape(tile, n, -1) for x in eng.get_state())
        st = dbg.cpu().numpy().reshape(tile, n, -1)[:, :, STAGES]
        eng.close()
        out.update({v + "_step_qpos": _bits(_tiles_equal(q, v + " step qpos")), v + "_step_qvel": _bits(_tiles_equal(qv, v + " step qvel")),
                    v + "_step_warm": _bits(_tiles_equal(w, v + " step qacc_warmstart")),
                    v + "_step_stages": _bits(_tiles_equal(st, v + " step stage bytes"))})
    return out


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def states(model):
    return cps.humanoid_states(model)


@pytest.fixture(scope="module")
def golden():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def got(model, clips, torch_mod, states):
    return compute(model, clips, torch_mod, states)


def test_fixture_is_of_these_states(states, golden):
    """Taken at 108 states, every path label among them, and at exactly the inputs the generator gives today."""
    assert len(states["labels"]) == NSTATES and golden["path"].shape == (NSTATES,)
    assert set(golden["path"]) == set(PATHS)
    assert [_path(lab) for lab in states["labels"]] == list(golden["path"])
    for k in ("qpos", "qvel", "warm"):
        assert np.array_equal(_bits(states[k]), golden[k + "_in"]), k
    for v in VARIANTS:
        assert golden[v + "_fwd_qacc"].shape == (NSTATES, 34) and golden[v + "_step_qpos"].shape == (NSTATES, 35)
        nefc = golden[v + "_fwd_counts"].view(np.float32)[:, 1]
        assert {0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128} <= set(int(x) for x in nefc)


def _compare(got, golden, keys, states):
    for k in keys:
        bad = np.nonzero((got[k] != golden[k]).any(axis=1))[0]
        assert bad.size == 0, "%s differs on %d states, first: state %d, %s" % (
            k, bad.size, bad[0], cps.describe(states["labels"][bad[0]]))


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_forward_bits(got, golden, states, variant):
    """set_state + forward(): qacc, qacc_smooth, the exported row forces, ncon / nefc / solver_iter / nlimit / overflow and the
    stage bytes equal the recording bit for bit on all 108 states."""
    _compare(got, golden, [variant + "_fwd_" + k for k in ("counts", "stages", "qacc_smooth", "force", "qacc")], states)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_step_bits(got, golden, states, variant):
    """One dm_step with zero actions from the same states: qpos, qvel, qacc_warmstart and the stage bytes, bit for bit."""
    _compare(got, golden, [variant + "_step_" + k for k in ("stages", "qpos", "qvel", "warm")], states)
