"""Lifetime of the two engines' device memory (csrc/dm_host.h: one owner per engine) seen from outside, at 4 envs.

* reload: a clip slot loaded twice (second time with a motion of another length) behaves bit for bit like a fresh engine that was
  given the second motion only;
* create / destroy does not accumulate: after one warm cycle, 8 further cycles lose less free device memory than ONE engine occupies
  (a leaked engine costs one such footprint per cycle); the footprint is what K engines alive together take, divided by K;
* messages: a step before any load_clip and a model with an index out of range are refused on the host with DM_EINVAL and a text
  that says why.

G1 with pipeline=2 and integrator="Euler" allocates the split-pipeline and Euler buffers at any batch size, so 4 envs reach them.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 4
IDX = [0, 3, 7, 11]
KINDS = {"humanoid": {}, "g1_mono": dict(pipeline=1), "g1_split_euler": dict(pipeline=2, integrator="Euler")}


def _mocap(kind, motion, model):
    if kind == "humanoid":
        from deepmimic_mujoco_amd.config import MotionConfig
        from deepmimic_mujoco_amd.mocap import MocapDM
        mc = MocapDM(model=model)
        mc.load_mocap(MotionConfig(motion).mocap_path)
        return mc
    from deepmimic_mujoco_amd.g1 import _g1_mocap
    return _g1_mocap(motion)[1]


@pytest.fixture(scope="module")
def mocaps(model):
    return {(k, m): _mocap(k, m, model) for k in ("humanoid", "g1") for m in ("walk", "run")}


def _create(kind, model):
    if kind == "humanoid":
        from deepmimic_mujoco_amd._lib import HipEngine
        return HipEngine(model, N, auto_reset=False)
    from deepmimic_mujoco_amd.g1 import G1HipEngine
    return G1HipEngine(N, auto_reset=False, **KINDS[kind])


def _load(eng, kind, mc):
    eng.load_clip(0, mc) if kind == "humanoid" else eng.load_clip(mc, clip_id=0)


def _actions(eng, kind):
    from deepmimic_mujoco_amd import g1, model as hm
    g = torch.Generator().manual_seed(5)
    return (torch.rand(3, N, hm.NU if kind == "humanoid" else g1.NACT, generator=g) - 0.5).to(eng.device)


def _rollout(eng, kind):
    """Reset at fixed frames, three steps: every output of every step and the final state, as host arrays."""
    out = eng.alloc_outputs()
    eng.reset(out["obs"], idx_init=torch.tensor(IDX, dtype=torch.int32, device=eng.device))
    got = [out["obs"].cpu().numpy().copy()]
    for a in _actions(eng, kind):
        eng.step(a.contiguous(), out)
        got += [out[k].cpu().numpy().copy() for k in ("obs", "rew", "done", "terms", "reason")]
    got += [t.cpu().numpy() for t in eng.get_state()]
    return got


@pytest.mark.parametrize("kind", ["humanoid", "g1_mono"])
def test_a_reloaded_clip_slot_equals_a_fresh_one(kind, model, mocaps):
    robot = "humanoid" if kind == "humanoid" else "g1"
    first, second = mocaps[(robot, "run")], mocaps[(robot, "walk")]
    assert first.get_length() != second.get_length() and max(IDX) < second.get_length()
    a = _create(kind, model)
    _load(a, kind, first)
    _load(a, kind, second)
    got = _rollout(a, kind)
    a.close()
    b = _create(kind, model)
    _load(b, kind, second)
    want = _rollout(b, kind)
    b.close()
    assert len(got) == len(want) == 1 + 3 * 5 + (4 if kind == "humanoid" else 3)
    for x, y in zip(got, want):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
    assert np.isfinite(got[1]).all() and np.abs(got[1]).max() > 0      # observations of a live step, not an untouched buffer


def _free():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def _footprint(kind, model):
    """Bytes of device memory one engine occupies.  The runtime carves buffers of this size out of blocks that it keeps, so free
    memory moves a block at a time and the create of ONE 4-env engine after a warm cycle moves it by nothing (measured: 0 bytes).
    So K engines are held alive together, K doubling from 8 until free memory drops, and the drop is divided by K."""
    k = 8
    while True:
        before = _free()
        engines = [_create(kind, model) for _ in range(k)]
        held = before - _free()
        for e in engines:
            e.close()
        if held > 0 or k >= 64:
            return held // k
        k *= 2


@pytest.mark.parametrize("kind", list(KINDS))
def test_create_destroy_does_not_accumulate(kind, model, mocaps):
    mc = mocaps[("humanoid" if kind == "humanoid" else "g1", "walk")]

    def cycle():
        eng = _create(kind, model)
        _load(eng, kind, mc)
        out = eng.alloc_outputs()
        eng.reset(out["obs"], idx_init=torch.tensor(IDX, dtype=torch.int32, device=eng.device))
        eng.step(_actions(eng, kind)[0].contiguous(), out)
        torch.cuda.synchronize()
        eng.close()

    cycle()                       # warm: the runtime's and torch's own pools are grown here
    start = _free()
    for _ in range(8):
        cycle()
    lost = start - _free()
    footprint = _footprint(kind, model)      # after the cycles: the blocks it makes the runtime keep could hide a leak
    print("%s: one engine occupies %d bytes, 8 cycles lost %d bytes" % (kind, footprint, lost))
    assert lost < footprint


@pytest.mark.parametrize("kind", ["humanoid", "g1_mono"])
def test_a_step_before_any_clip_is_refused_with_the_reason(kind, model):
    eng = _create(kind, model)
    out = eng.alloc_outputs()
    with pytest.raises(RuntimeError, match=r"step failed \(-22\): no clip loaded"):
        eng.step(_actions(eng, kind)[0].contiguous(), out)
    assert b"no clip loaded" in getattr(eng.L, eng.PREFIX + "last_error")(eng.h)
    eng.close()


def test_a_pair_geom_out_of_range_is_refused_by_name():
    from deepmimic_mujoco_amd import g1
    cmodel = g1.DmModelG1.from_buffer_copy(bytes(g1.load_g1_model()[1]))
    cmodel.pair_geom1[0] = g1.NGEOM
    with pytest.raises(RuntimeError, match=r"dmg1_create failed \(-22\)"):
        g1.G1HipEngine(N, cmodel=cmodel)
    assert b"pair_geom1" in g1._lib().dmg1_last_error(None)
    assert g1.load_g1_model()[1].pair_geom1[0] != g1.NGEOM       # the packaged model was not touched
