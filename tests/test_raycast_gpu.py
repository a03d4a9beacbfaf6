"""Ray-cast renderer on the device (csrc/dm_render.hip) against the fp64 reference frames of tests/golden/raycast_cases.npz.

Depth tolerance.  It is not tuned to the kernel: tests/render_ref.py run with every intermediate in float32 differs from its fp64
run by at most ``DEPTH_ERR32_REF`` (relative, worst stable pixel of all fixture cases; the generator measures it and the fixture
stores it per case, which the ``cases`` fixture below holds the constant to).  The kernel is allowed ``8 x`` that: it differs from the float32 reference in FMA
contraction and in the order of operations over at most 11 plane chunks.  Measured on an MI355X, the kernel's own worst relative
depth error over the same pixels is ``KERNEL_WORST_SEEN`` (for the record; nothing depends on it).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH_ERR32_REF = 7.3392e-07    # tests/golden/make_raycast_cases.py: worst case g_torso
DEPTH_TOL = 8 * DEPTH_ERR32_REF
KERNEL_WORST_SEEN = 5.03e-07      # g_torso; 1.9e-07 .. 3.3e-07 on the other cases
XPOS_TOL, XMAT_TOL = 2e-5, 1e-5     # <= 10 chained fp32 transforms, each a few ulp of values under 4 m


@pytest.fixture(scope="module")
def cases():
    z = np.load(os.path.join(ROOT, "tests", "golden", "raycast_cases.npz"))
    assert DEPTH_ERR32_REF == pytest.approx(max(float(z[str(n) + "/err32"]) for n in z["names"]), rel=1e-3)
    return z


@pytest.fixture(scope="module")
def renderers():
    from deepmimic_mujoco_amd import g1, raycast
    from deepmimic_mujoco_amd.model import load_model
    r = {"humanoid3d": raycast.RayRenderer(load_model()), "unitree_g1": raycast.RayRenderer(g1.load_g1_model()[0])}
    yield r
    for v in r.values():
        v.close()


NAMES = ["h_qpos0", "h_walk", "h_lying", "g_walk", "g_getup", "h_odd", "g_odd", "h_sky", "g_top", "g_torso", "g_batch"]


def _inputs(cases, renderers, name):
    import torch
    r = renderers[str(cases[name + "/robot"])]
    dev = r.device
    W, H = (int(v) for v in cases[name + "/wh"])
    ids = cases[name + "/env_ids"]
    return dict(r=r, W=W, H=H, qpos=torch.tensor(cases[name + "/qpos"], device=dev), ids=ids.tolist() if len(ids) else None,
                cam=torch.tensor(cases[name + "/cam"], device=dev),
                xpos=torch.tensor(cases[name + "/kin_xpos"].astype(np.float32), device=dev),
                xmat=torch.tensor(cases[name + "/kin_xmat"].astype(np.float32), device=dev))


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("name", NAMES)
def test_kinematics_match_the_fp64_host_kinematics(cases, renderers, name):
    i = _inputs(cases, renderers, name)
    xpos, xmat = i["r"].kinematics(i["qpos"], i["ids"])
    ex, em = np.abs(xpos.cpu().numpy() - cases[name + "/kin_xpos"]).max(), np.abs(xmat.cpu().numpy() - cases[name + "/kin_xmat"]).max()
    print("%s: geom_xpos error %.3g m, geom_xmat error %.3g" % (name, ex, em))
    assert ex <= XPOS_TOL and em <= XMAT_TOL


@pytest.mark.parametrize("name", NAMES)
def test_cast_matches_the_reference_on_stable_pixels(cases, renderers, name):
    i = _inputs(cases, renderers, name)
    out = _np(i["r"].cast(i["xpos"], i["xmat"], i["cam"], i["W"], i["H"], rgb=True, depth=True, segmentation=True))
    seg5, st = cases[name + "/seg5"].astype(np.int32), cases[name + "/stable"]
    assert out["segmentation"].shape == st.shape and out["rgb"].dtype == np.uint8 and out["depth"].dtype == np.float32
    hit = st & (seg5[0] >= 0)
    ref_d = cases[name + "/depth"]
    derr = float((np.abs(out["depth"].astype(np.float64) - ref_d) / ref_d)[hit].max()) if hit.any() else 0.0
    rerr = int(np.abs(out["rgb"].astype(int) - cases[name + "/rgb"].astype(int))[st].max())
    print("%s: worst relative depth error %.3g (allowed %.3g), worst rgb difference %d, %d unstable pixels" % (
        name, derr, DEPTH_TOL, rerr, (~st).sum()))
    assert np.array_equal(out["segmentation"][st], seg5[0][st])
    assert rerr <= 1
    assert derr <= DEPTH_TOL
    assert np.isposinf(out["depth"][st & (seg5[0] < 0)]).all()
    assert (out["segmentation"][None] == seg5).any(0)[~st].all()       # an unstable pixel still carries one of the five casts' geoms


def _same_on_stable(a, b, st):
    for k in a:
        assert np.array_equal(a[k][st], b[k][st]), k


@pytest.mark.parametrize("name", ["h_lying", "g_batch"])
def test_dm_render_equals_the_two_calls_and_any_subset_of_outputs(cases, renderers, name):
    i = _inputs(cases, renderers, name)
    r, st = i["r"], cases[name + "/stable"]
    full = _np(r.render(i["qpos"], width=i["W"], height=i["H"], env_ids=i["ids"], cam=i["cam"], rgb=True, depth=True, segmentation=True))
    xpos, xmat = r.kinematics(i["qpos"], i["ids"])
    _same_on_stable(full, _np(r.cast(xpos, xmat, i["cam"], i["W"], i["H"], True, True, True)), st)
    assert np.array_equal(full["segmentation"][st], cases[name + "/seg5"][0][st])
    for mask in range(1, 7):
        flags = dict(rgb=bool(mask & 1), depth=bool(mask & 2), segmentation=bool(mask & 4))
        part = _np(r.render(i["qpos"], width=i["W"], height=i["H"], env_ids=i["ids"], cam=i["cam"], **flags))
        assert set(part) == {k for k, v in flags.items() if v}
        _same_on_stable(part, full, st)


def test_env_ids_equal_the_reordered_batch(cases, renderers):
    i = _inputs(cases, renderers, "g_batch")
    r, st = i["r"], cases["g_batch/stable"]
    a = _np(r.render(i["qpos"], width=i["W"], height=i["H"], env_ids=i["ids"], cam=i["cam"], rgb=True, depth=True, segmentation=True))
    b = _np(r.render(i["qpos"][i["ids"]].contiguous(), width=i["W"], height=i["H"], cam=i["cam"], rgb=True, depth=True, segmentation=True))
    _same_on_stable(a, b, st)
    # the Camera path: track_root follows the listed rows of qpos
    from deepmimic_mujoco_amd.raycast import Camera
    c = r.camera_rows(Camera(), i["qpos"], r._ids(i["ids"], i["qpos"])[0], 32, 24).cpu().numpy()
    assert np.allclose(c[:, 0], cases["g_batch/qpos"][i["ids"], 0]) and np.allclose(c[:, 1:], Camera().rows(32, 24)[0, 1:], atol=1e-6)


def test_graph_replay_is_bit_identical_to_the_eager_call(cases, renderers):
    import torch
    i = _inputs(cases, renderers, "g_odd")
    r = i["r"]
    eager = r.render(i["qpos"], width=i["W"], height=i["H"], cam=i["cam"], rgb=True, depth=True, segmentation=True)
    work = torch.empty(r.G * 12, device=r.device)
    out = r.outputs(1, i["W"], i["H"], True, True, True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r.render(i["qpos"], width=i["W"], height=i["H"], cam=i["cam"], workspace=work, out=out)
    for v in out.values():
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k in eager:
        assert torch.equal(eager[k].view(torch.uint8), out[k].view(torch.uint8)), k


def _frames_ok(rgb, depth):
    assert rgb.shape == (240, 320, 3) and rgb.dtype == np.uint8 and depth.shape == (240, 320) and depth.dtype == np.float32
    assert len(np.unique(rgb.reshape(-1, 3), axis=0)) > 4 and np.isfinite(depth).any() and depth[np.isfinite(depth)].min() > 0.5


def test_dpenv_raycast_frames_leave_the_next_step_alone():
    from deepmimic_mujoco_amd.deepmimic_env import DPEnv
    from deepmimic_mujoco_amd.render import stick_figure
    a, b = DPEnv("walk", renderer="raycast"), DPEnv("walk")
    act = np.linspace(-0.3, 0.3, 28)
    obs = []
    for env, draw in ((a, True), (b, False)):
        env.reset_model(idx_init=5)
        o1 = env.step(act)[0]
        if draw:
            _frames_ok(env.render(mode="rgb_array"), env.render(mode="depth_array"))
            assert np.array_equal(env.render(), env.render(mode="rgb_array"))
        obs.append((o1, env.step(act)[0], env.step(-act)[0]))
    for x, y in zip(*obs):
        assert np.array_equal(x, y)
    assert b.renderer == "stick"
    assert np.array_equal(b.render(mode="rgb_array"), stick_figure(b._eng.body_xpos(), b.model.body_parent))
    with pytest.raises(RuntimeError):
        b.render_batch([0])
    a.close(), b.close()


def test_g1_vec_env_raycast_frames_leave_the_next_step_alone():
    import torch
    from deepmimic_mujoco_amd.g1 import HipG1VecEnv
    from deepmimic_mujoco_amd.raycast import Camera
    a, b = HipG1VecEnv(4, motion="walk", seed=7, renderer="raycast"), HipG1VecEnv(4, motion="walk", seed=7)
    act = torch.linspace(-0.2, 0.2, 4 * 23, device=a.device).reshape(4, 23).contiguous()
    outs = []
    for env, draw in ((a, True), (b, False)):
        env.reset_tensor(torch.arange(4, dtype=torch.int32, device=env.device) * 9)
        o1 = env.step_tensor(act)["obs"].clone()
        if draw:
            _frames_ok(env.render(mode="rgb_array"), env.render(mode="depth_array"))
            fr = env.render_batch([3, 1], 64, 48, camera=Camera(distance=3.0, elevation=-30), depth=True, segmentation=True)
            assert fr["rgb"].shape == (2, 48, 64, 3) and fr["rgb"].dtype == torch.uint8 and fr["rgb"].is_cuda
            assert fr["depth"].shape == (2, 48, 64) and fr["depth"].dtype == torch.float32
            assert fr["segmentation"].shape == (2, 48, 64) and fr["segmentation"].dtype == torch.int32
            assert fr["segmentation"].max().item() > 0 and env.render_batch(width=32, height=24)["rgb"].shape == (4, 24, 32, 3)
        o2 = env.step_tensor(act)
        outs.append((o1, o2["obs"].clone(), o2["rew"].clone()))
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    assert b.render().shape == (240, 320, 3)          # the stick figure, as before
    a.close(), b.close()
