"""The six layer entry points of the fp32 library-path learner (csrc/dm_ppo.hip: dm_linear_tanh, dm_tanh_linear_wgrad,
dm_tanh_bwd_colsum, dm_colsum, dm_linear_wgrad, dm_ppo_loss — what every optimizer step of MLP(1024, 512) runs through) called
directly on the MI355X and held, element by element, to the fp64 restatements and derived bounds of tests/ppo_layer_ref64.py,
at the smallest shapes that reach each path of each kernel: every NT instantiation of the fused weight gradient at its first
and last column, the 16-byte staging with groups that straddle two rows, its second round trip, the scalar fill behind an
offset pointer, I = 1, 2, 3, lone ragged tiles, both branches of lt_tanh and where it saturates, wave row ranges that end
inside a load group, both tanh-backward kernels and their tails, the column sum's unrolled loop and tail, split-K and its cuts,
the loss kernel's grid-stride wrap, full half-waves and exact clip edges; then the whole path, PPO.train against the fp64 PPO.

Every output lives in a NaN-fenced buffer (kernel_helpers.guarded); outputs a kernel accumulates into are zeroed first, as the
ABI asks, outputs it writes per row start as NaN.  No flat tolerance, no element left out; each comparison prints its worst
error / bound (pytest -s; DESIGN section 22 quotes them).  The shape lists and inputs come from ppo_layer_ref64, where
tests/test_ppo_layer_ref64.py holds each of them to the drop-one-row / drop-one-column sensitivity condition."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import ppo_layer_ref64 as ref
import ppo_ref64 as R
from kernel_helpers import DEV, check_out8, checked, guard_ok, guarded, lib, note, offset, ptr, stream, within

pytestmark = pytest.mark.gpu

EINVAL = -22


def call(name, *args):
    from deepmimic_mujoco_amd import _lib
    _lib.call(name, *args, device=DEV)


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32).cpu()


def put(x, off=0):
    """The fp32 array on the device, 16-byte aligned, or `off` floats past alignment."""
    return offset(dev(x), off) if off else dev(x)


def synced_ok(*pairs):
    torch.cuda.synchronize()
    for buf, view in pairs:
        assert guard_ok(buf, view)


# ------------------------------------------------------------------------------------------------------------- dm_linear_tanh
@functools.lru_cache(maxsize=None)
def _lt_ref(B, O, I):
    X, W, b = ref.in_linear_tanh(B, O, I)
    return (X, W, b) + ref.linear_tanh(X, W, b)


def _linear_tanh(B, O, I, offx, offw):
    X, W, b, val, bnd = _lt_ref(B, O, I)
    ybuf, y = guarded(B, O)
    call("dm_linear_tanh", put(X, offx), put(W, offw), dev(b), y, B, O, I)
    synced_ok((ybuf, y))
    within("linear_tanh Y  B %d O %d I %d%s" % (B, O, I, " off x%d w%d" % (offx, offw) if offx or offw else ""), y, val, bnd)
    assert bool((y.abs() <= 1).all())
    return y


@pytest.mark.parametrize("I", ref.LT_I)
@pytest.mark.parametrize("B,O", ref.LT_BO)
@checked
def test_linear_tanh(B, O, I):
    """A lone ragged tile (scalar fill), one full 64 x 128 tile (16-byte staging where I >= 4: odd I copies flat, even I splits
    groups that straddle two rows from I = 6 on, the second round trip begins at I = 86), a full tile beside ragged ones and
    3 x 3 tiles, for I = 1 (odd-K tail only), 2, 3 (no 8-wide loop) up to 128."""
    _linear_tanh(B, O, I, 0, 0)


@pytest.mark.parametrize("offx,offw", [(1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("B,O,I", ref.LT_OFFSET)
@checked
def test_linear_tanh_unaligned(B, O, I, offx, offw):
    """X, W or both one float past 16-byte alignment: the full tile takes the scalar fill as well (vec = 0); same values, same
    bounds, and the same bits as the aligned call (the fill only changes how the tile reaches LDS)."""
    y = _linear_tanh(B, O, I, offx, offw)
    X, W, b, _, _ = _lt_ref(B, O, I)
    ybuf, y0 = guarded(B, O)
    call("dm_linear_tanh", dev(X), dev(W), dev(b), y0, B, O, I)
    synced_ok((ybuf, y0))
    assert torch.equal(bits(y), bits(y0))


@checked
def test_lt_tanh_alone():
    """I = 1, W = 1, b = 0: the pre-activation is the input bit for bit (one product by 1 added to a +0 accumulator, which also
    turns -0 into +0, in the kernel as in the restatement), one row per value of ref.tanh_table: zeros, tiny arguments, 0.25 and
    its neighbours (the branch), moderate values, and where exp2 overflows or underflows.  Each output within T_TANH of fp64 tanh,
    |y| <= 1, exactly +-1 where fp64 tanh rounds to +-1 in fp32, zero for zero with the reference's sign, odd within 2 T_TANH."""
    x = ref.tanh_table()
    n = x.size
    val, _ = ref.linear_tanh(x[:, None], np.ones((1, 1), np.float32), np.zeros(1, np.float32))
    assert np.array_equal(val[:, 0], np.tanh(x.astype(np.float64) + 0.0))       # the pre-activation's own allowance is not granted: T_TANH alone
    ybuf, y = guarded(n, 1)
    call("dm_linear_tanh", dev(x[:, None]), torch.ones(1, 1, device=DEV), torch.zeros(1, device=DEV), y, n, 1, 1)
    synced_ok((ybuf, y))
    got = y.cpu().numpy()[:, 0]
    for xi, gi, vi in zip(x, got, val[:, 0]):
        print("lt_tanh(%-14.9g) = %-14.9g  err %6.3f U" % (xi, gi, abs(float(gi) - vi) / ref.U))
    within("lt_tanh table", y, val, ref.T_TANH)
    assert np.all(np.abs(got) <= 1)
    one = np.abs(val[:, 0]).astype(np.float32) == 1
    assert one.sum() >= 10 and np.array_equal(got[one], np.sign(val[one, 0]).astype(np.float32))
    zero = val[:, 0] == 0
    assert zero.sum() == 2 and np.all(got[zero] == 0) and np.array_equal(np.signbit(got[zero]), np.signbit(val[zero, 0]))
    within("lt_tanh odd symmetry", got[0::2].astype(np.float64) + got[1::2].astype(np.float64), np.zeros(n // 2), 2 * ref.T_TANH)


def test_linear_tanh_and_its_wgrad_refuse_wide_inputs():
    """I = 129 is beyond the LDS tile: both entry points return DM_EINVAL and write nothing."""
    L = lib()
    x, w, b = torch.zeros(8, 129, device=DEV), torch.zeros(8, 129, device=DEV), torch.zeros(8, device=DEV)
    ybuf, y = guarded(8, 8)
    assert L.dm_linear_tanh(ptr(x), ptr(w), ptr(b), ptr(y), 8, 8, 129, stream()) == EINVAL
    wbuf, dw = guarded(8, 129)
    assert L.dm_tanh_linear_wgrad(ptr(y), ptr(y), ptr(x), ptr(dw), ptr(b), 8, 8, 129, stream()) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(ybuf).all()) and bool(torch.isnan(wbuf).all())


# ------------------------------------------------------------------------------------------------------- dm_tanh_linear_wgrad
@pytest.mark.parametrize("I", ref.TW_I)
@pytest.mark.parametrize("B,O", ref.TW_BO)
@checked
def test_tanh_linear_wgrad(B, O, I):
    """All four NT instantiations at their first and last column (I = 1 | 31, 32 | 33, 64 | 65, 96 | 97, 128), one to three
    32-output tiles, and batches whose per-wave row ranges end inside a 32-row load group: B < 8 (waves with no rows), 31, 257
    (one group of rows, the fifth wave gets one row), 513 (two groups of 257 and 256), 1000 (two groups of 500).  Rows of Y
    hold exactly +-1 and 0 (a = g 0 and a = g)."""
    gy, y, x = ref.in_tanh_wgrad(B, O, I)
    val, bnd = ref.tanh_wgrad(gy, y, x)
    wbuf, dw = guarded(O, I, fill=0.0)
    bbuf, db = guarded(O, fill=0.0)
    call("dm_tanh_linear_wgrad", dev(gy), dev(y), dev(x), dw, db, B, O, I)
    synced_ok((wbuf, dw), (bbuf, db))
    within("tanh_wgrad dW  B %d O %d I %d" % (B, O, I), dw, val["dw"], bnd["dw"])
    within("tanh_wgrad db  B %d O %d I %d" % (B, O, I), db, val["db"], bnd["db"])


# --------------------------------------------------------------------------------------------------------- dm_tanh_bwd_colsum
def _tanh_bwd(B, O, off=(0, 0, 0), tag=""):
    gy, y = ref.in_tanh_bwd(B, O)
    val, bnd = ref.tanh_bwd(gy, y)
    dgy, dy = put(gy, off[0]), put(y, off[1])
    zraw, z = guarded(B * O + 1)
    dz = zraw[off[2]:off[2] + B * O].view(B, O)
    bbuf, db = guarded(O, fill=0.0)
    call("dm_tanh_bwd_colsum", dgy, dy, dz, db, B, O)
    torch.cuda.synchronize()
    assert guard_ok(bbuf, db) and bool(torch.isnan(zraw[off[2] + B * O:]).all()) and bool(torch.isnan(zraw[:off[2]]).all())
    within("tanh_bwd dZ  B %d O %d%s" % (B, O, tag), dz, val["dz"], bnd["dz"])
    within("tanh_bwd db  B %d O %d%s" % (B, O, tag), db, val["db"], bnd["db"])
    # in place: dZ aliases dY; the same bits as out of place
    io = max(off[0], off[2])                       # the same kernel as out of place: an offset dY or dZ is an offset dY = dZ
    ibuf, iz = guarded(B * O + 1)
    ig = ibuf[io:io + B * O].view(B, O)
    ig.copy_(dev(gy))
    b2buf, db2 = guarded(O, fill=0.0)
    call("dm_tanh_bwd_colsum", ig, dy, ig, db2, B, O)
    torch.cuda.synchronize()
    assert guard_ok(b2buf, db2) and bool(torch.isnan(ibuf[io + B * O:]).all()) and bool(torch.isnan(ibuf[:io]).all())
    assert torch.equal(bits(ig), bits(dz)), "in place differs"
    within("tanh_bwd db  B %d O %d%s in place" % (B, O, tag), db2, val["db"], bnd["db"])


@pytest.mark.parametrize("O", ref.TB_O_SCALAR)
@checked
def test_tanh_bwd_colsum_scalar_kernel(O):
    """O % 4 != 0: ppo_tanh_bwd_colsum_kernel.  One column, a ragged single column block, one block and one column, O = 77; B on
    both sides of the 16-row unrolled group and of the 32-row slice split, where the 4-row tail loop carries what is left."""
    for B in ref.TB_B:
        _tanh_bwd(B, O)


@pytest.mark.parametrize("which", [0, 1, 2])
@checked
def test_tanh_bwd_colsum_scalar_kernel_by_offset(which):
    """O = 64 would take the 16-byte kernel; dY, Y or dZ one float past alignment sends it to the scalar one."""
    off = tuple(1 if k == which else 0 for k in range(3))
    for B in ref.TB_B:
        _tanh_bwd(B, ref.TB_O_OFFSET, off, " off %s" % ("dY", "Y", "dZ")[which])


@pytest.mark.parametrize("O", ref.TB_O_VEC)
@checked
def test_tanh_bwd_colsum_float4_kernel(O):
    """O % 4 == 0, aligned: ppo_tanh_bwd_colsum4_kernel.  One 16-byte group, a full 64-column block, O = 68 ((O % 64) no multiple
    of 16: the last block has one live group), O = 300; B around the 16-row step of the unrolled loads and the 64-row block."""
    for B in ref.TB_B:
        _tanh_bwd(B, O)


# ------------------------------------------------------------------------------------------------------------------ dm_colsum
@pytest.mark.parametrize("O", ref.CS_O)
@checked
def test_colsum(O):
    """Direct calls: O below, at and past the 64-column block; B = 1, 3 (fewer rows than the four row groups), 16 | 17, 127 | 128 |
    129 (the slice split begins at 128) and 1001 (eight slices of 126 rows: the 16-row loop and the 4-row tail split them
    unevenly).  Into a zeroed `out`, and accumulated into a non-zero one."""
    for B in ref.CS_B:
        y, out0 = ref.in_colsum(B, O)
        for o0, tag in ((None, ""), (out0, " into out")):
            val, bnd = ref.colsum(y, o0)
            obuf, out = guarded(O, fill=0.0)
            if o0 is not None:
                out.copy_(dev(o0))
            call("dm_colsum", dev(y), B, O, out)
            synced_ok((obuf, out))
            within("colsum  B %d O %d%s" % (B, O, tag), out, val, bnd)


# ------------------------------------------------------------------------------------------------------------ dm_linear_wgrad
@pytest.mark.parametrize("B", ref.LW_B)
@pytest.mark.parametrize("O,I", ref.LW_OI)
@checked
def test_linear_wgrad(B, O, I):
    """B = 64 (one unrolled group, no split), 128, 192 (kchunk = 192: 192 % 128 != 0 blocks the split), 320 (likewise, five
    groups), 1024 (split 16 ways, or cut short by splitk x 2 x tiles <= 1024: (300, 300) has 100 tiles and splits 8 ways); one
    ragged tile, one full tile, O and I just past a tile, and the skinny head shapes."""
    gy, x = ref.in_linear_wgrad(B, O, I)
    val, bnd = ref.linear_wgrad(gy, x)
    wbuf, dw = guarded(O, I, fill=0.0)
    bbuf, db = guarded(O, fill=0.0)
    call("dm_linear_wgrad", dev(gy), dev(x), dw, db, B, O, I)
    synced_ok((wbuf, dw), (bbuf, db))
    within("linear_wgrad dW  B %d O %d I %d" % (B, O, I), dw, val["dw"], bnd["dw"])
    within("linear_wgrad db  B %d O %d I %d" % (B, O, I), db, val["db"], bnd["db"])


def test_linear_wgrad_refuses_ragged_batches():
    """B = 0, 63, 65: no multiple of the 64-row unrolled group; DM_EINVAL, nothing written."""
    L = lib()
    gy, x = torch.zeros(128, 8, device=DEV), torch.zeros(128, 8, device=DEV)
    wbuf, dw = guarded(8, 8)
    bbuf, db = guarded(8)
    for B in (0, 63, 65):
        assert L.dm_linear_wgrad(ptr(gy), ptr(x), ptr(dw), ptr(db), B, 8, 8, stream()) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(wbuf).all()) and bool(torch.isnan(bbuf).all())


# ---------------------------------------------------------------------------------------------------------------- dm_ppo_loss
def _ppo_loss(args, B, A, clip, ent, normalize, tag, tie_rows=None, listed=None):
    """One call: out8 by kernel_helpers.check_out8, grad_mean / grad_value (NaN before the call) and grad_log_std against their
    bounds.  On an ambiguous row (ref.ppo_loss) grad_mean may be either branch's value; `listed`, when given, must hold them."""
    val, bnd, info = ref.ppo_loss(*args, clip, 0.5, ent, normalize, tie_rows=tie_rows)
    amb = info["amb"]
    if listed is not None:
        assert set(amb) <= set(listed)
    mbuf, gm = guarded(B, A)
    vbuf, gv = guarded(B)
    lbuf, gl = guarded(A)
    obuf, out8 = guarded(8)
    sbuf, scratch = guarded(2)
    call("dm_ppo_loss", *[dev(a) for a in args], B, A, float(clip), 0.5, float(ent), 1 if normalize else 0, gm, gl, gv, out8, scratch)
    synced_ok((mbuf, gm), (vbuf, gv), (lbuf, gl), (obuf, out8), (sbuf, scratch))
    assert not bool(torch.isnan(gm).any()) and not bool(torch.isnan(gv).any())
    ratio = torch.tensor(info["ratio"])
    if tie_rows is None:
        check_out8(out8.cpu(), val["out8"], ratio, float(np.float32(clip)), B, width=46)
    got = gm.cpu().numpy().astype(np.float64)
    ref_gm = val["gm"] if tie_rows is None else info["gm_rows"]
    if amb.size:                                   # either branch: compare each ambiguous row with the nearer one
        ref_gm = ref_gm.copy()
        alt = info["gm_alt"][amb]
        nearer = np.abs(got[amb] - alt).sum(1) < np.abs(got[amb] - ref_gm[amb]).sum(1)
        ref_gm[amb[nearer]] = alt[nearer]
    within("ppo_loss grad_mean  %s" % tag, got, ref_gm, bnd["gm"])
    within("ppo_loss grad_value  %s" % tag, gv, val["gv"], bnd["gv"])
    within("ppo_loss grad_log_std  %s" % tag, gl, val["gl"] if tie_rows is None else info["gl_rows"], bnd["gl"])
    return got, info


@pytest.mark.parametrize("normalize,ent", ref.PPO_LOSS_MODES)
@pytest.mark.parametrize("B,A", ref.PPO_LOSS)
@checked
def test_ppo_loss(B, A, normalize, ent):
    """B = 1 (no normalisation whatever the flag), A = 1 and A = 32 = PPO_MAXA (every lane of the half-wave live), B = 7 (one
    block, one half-wave idle), 64 and 257 (the grid is sized for eight rows per half-wave: the grid-stride loop wraps seven
    times from B = 64 on), 2049 (33 blocks) and 16 449 rows (past 16 384 the grid is capped at 256 blocks x 8 half-waves: a ninth
    pass begins at row 16 384)."""
    _ppo_loss(ref.in_ppo_loss(B, A), B, A, 0.2, ent, normalize, "B %d A %d norm %d ent %g" % (B, A, normalize, ent))


@checked
def test_ppo_loss_near_the_clip_edges():
    """old_logp rebuilt from the fp64 logp so that every other pair of rows has its fp64 ratio within 1e-6 of 1 + clip or 1 - clip:
    on those listed rows grad_mean may take either branch's value (a_n's or 0), every other row and grad_value are held to their
    bounds; grad_log_std's bound carries the listed rows' whole contribution."""
    args, edge = ref.in_ppo_loss_edge()
    B, A = ref.EDGE_SHAPE
    _ppo_loss(args, B, A, 0.2, 0.0, True, "near edge B %d A %d" % (B, A), listed=edge)


@checked
def test_ppo_loss_exactly_on_the_clip_edge():
    """clip_range = 0, where both edges are 1, and even rows whose fp32 log-ratio is exactly 0 (ref.in_ppo_loss_tie): the ratio is
    exactly on the edge, `inside` holds with `>=` and `<=`, and the row carries a_n's gradient, as autograd's evenly split tie of
    two equal branches does.  Odd rows are clipped.  out8 is left to the other tests: its fp64 clip fraction counts the tie rows,
    whose fp64 ratio is 1 +- 1e-7, as clipped."""
    args, ties = ref.in_ppo_loss_tie()
    B, A = ref.TIE_SHAPE
    got, info = _ppo_loss(args, B, A, 0.0, 0.0, True, "exact edge B %d A %d" % (B, A), tie_rows=ties)
    assert np.all(np.any(got[ties] != 0, 1))


def test_ppo_loss_refuses_wide_actions():
    L = lib()
    import ctypes as C
    z = torch.zeros(64, 33, device=DEV)
    v = torch.zeros(64, device=DEV)
    mbuf, gm = guarded(64, 33)
    rc = L.dm_ppo_loss(ptr(z), ptr(v), ptr(v), ptr(z), ptr(v), ptr(v), ptr(v), 64, 33, C.c_float(0.2), C.c_float(0.5), C.c_float(0.0), 1,
                       ptr(gm), ptr(v), ptr(v), ptr(v), ptr(v), stream())
    torch.cuda.synchronize()
    assert rc == EINVAL and bool(torch.isnan(mbuf).all())


# ------------------------------------------------------------------------------------------ the library path end to end
# net_arch (320, 288) reaches five of the six: behind a fused tanh trunk no layer of a two-hidden-layer net is a PLAIN linear layer
# beyond 256 x 128, the one place dm_colsum is called from.  A third hidden layer of 200 units is (out <= 256, so the trunk
# leaves it to HipLinear; 200 x 288 is beyond 256 x 128, so HipLinear takes the library GEMM + dm_colsum).
ARCH, D_E2E, A_E2E, MB = (320, 288, 200), 98, 23, 1024
SIX = ("dm_linear_tanh", "dm_tanh_linear_wgrad", "dm_tanh_bwd_colsum", "dm_colsum", "dm_linear_wgrad", "dm_ppo_loss")


def _plain_fp32(pol, flat, perms, B, lr):
    """Plain fp32 PyTorch: F.linear trunks (ppo_ref64 in float32), clip_grad_norm_ + torch.optim.Adam."""
    P = R.params64(pol, DEV, dtype=torch.float32)
    opt = torch.optim.Adam(list(P.values()), lr=lr, eps=1e-5)
    for perm in perms:
        for s in range(0, perm.numel(), B):
            i = perm[s:s + B]
            loss, _ = R.loss(P, flat["obs"][i], flat["act"][i], flat["adv"][i], flat["ret"][i], flat["logp"][i])
            opt.zero_grad()
            loss.backward()
            nn.utils.clip_grad_norm_(list(P.values()), 0.5)
            opt.step()
    return P


def test_library_path_runs_all_six_kernels(monkeypatch):
    """One eager minibatch step of MlpPolicy(98, 23, (320, 288, 200)) at B = 1024 with _lib.call counted: the first layer goes
    through dm_linear_tanh + dm_tanh_linear_wgrad, the 288 x 320 layer through dm_tanh_bwd_colsum + the library GEMM, the
    200 x 288 layer through the library GEMM + dm_colsum, the heads through dm_linear_wgrad, the loss through dm_ppo_loss."""
    from deepmimic_mujoco_amd import _lib
    from deepmimic_mujoco_amd.ppo import PPO, MlpPolicy
    torch.manual_seed(3)
    ppo = PPO(None, policy=MlpPolicy(obs_dim=D_E2E, act_dim=A_E2E, net_arch=ARCH), device=DEV, batch_size=MB, use_hip_graph=False)
    assert ppo.learner_path() == "library_fp32"
    seen = {}
    real = _lib.call

    def counted(name, *a, **kw):
        seen[name] = seen.get(name, 0) + 1
        return real(name, *a, **kw)

    monkeypatch.setattr(_lib, "call", counted)
    g = torch.Generator(device=DEV); g.manual_seed(1)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    ppo._minibatch_step(rn(MB, D_E2E), rn(MB, A_E2E), rn(MB), rn(MB), rn(MB) - 30)
    torch.cuda.synchronize()
    print("entry points called:", seen)
    for name in SIX:
        assert seen.get(name, 0) > 0, (name, seen)


@pytest.mark.parametrize("graph", [False, None])
def test_library_path_train_matches_the_fp64_reference(graph):
    """PPO.train on the fp32 library path, MlpPolicy(98, 23, (320, 288, 200)), minibatch 1024, called twice on a synthetic 4 x 512
    buffer, eager (use_hip_graph=False) and with the default (captured), against ppo_ref64.train on the same permutations.  The
    product's parameter error (max and L2) is at most 4x that of plain fp32 PyTorch on the same run, and the update is far larger
    than either error."""
    from deepmimic_mujoco_amd.ppo import PPO, MlpPolicy
    lr, T, N, E = 4e-4, 4, 512, 2
    torch.manual_seed(12)
    kw = {} if graph is None else {"use_hip_graph": graph}
    ppo = PPO(None, policy=MlpPolicy(obs_dim=D_E2E, act_dim=A_E2E, net_arch=ARCH), device=DEV, batch_size=MB, learning_rate=lr, n_epochs=E, **kw)
    assert ppo.learner_path() == "library_fp32" and ppo.flat_adam and ppo.use_hip_graph == (graph is None)
    pol = ppo.policy
    P64 = R.params64(pol, DEV)
    p0 = R.flat(P64).clone()
    g = torch.Generator(device=DEV); g.manual_seed(5)
    with torch.no_grad():
        obs = torch.randn(T, N, D_E2E, device=DEV, generator=g) * 0.7
        mean, _ = R.heads(P64, obs)
        act = (mean + P64["log_std"].exp() * torch.randn(T, N, A_E2E, device=DEV, generator=g, dtype=torch.float64)).float()
        logp = (R.logp(act, mean, P64["log_std"]) + 0.1 * torch.randn(T, N, device=DEV, generator=g, dtype=torch.float64)).float()
    buf = dict(obs=obs, act=act, adv=torch.randn(T, N, device=DEV, generator=g) + 0.2, ret=torch.randn(T, N, device=DEV, generator=g),
               logp=logp, val=torch.zeros(T, N, device=DEV), rew=torch.zeros(T, N, device=DEV), done=torch.zeros(T, N, device=DEV))
    pol32 = MlpPolicy(obs_dim=D_E2E, act_dim=A_E2E, net_arch=ARCH).to(DEV)
    pol32.load_state_dict(pol.state_dict())
    gen = torch.Generator(device=DEV); gen.manual_seed(77)
    ppo.train(buf, generator=gen)
    ppo.train(buf, generator=gen)
    torch.cuda.synchronize()
    gen = torch.Generator(device=DEV); gen.manual_seed(77)
    perm = torch.empty(T * N, dtype=torch.int64, device=DEV)
    perms = []
    for _ in range(2 * E):
        torch.randperm(T * N, device=DEV, generator=gen, out=perm)
        perms.append(perm.clone())
    flat = {k: v.reshape(-1, *v.shape[2:]) for k, v in buf.items() if k in ("obs", "act", "adv", "ret", "logp")}
    R.train(P64, flat, perms, MB, R.Adam64(p0.numel(), lr, device=DEV))
    P32 = _plain_fp32(pol32, flat, perms, MB, lr)
    want, prod, f32 = R.flat(P64), torch.cat([p.detach().double().reshape(-1) for p in pol.parameters()]), R.flat(P32).double()
    e_prod, e_32 = (prod - want).abs(), (f32 - want).abs()
    tag = "eager" if graph is False else "graph"
    print("library path %s: max|err| product %.3g, plain fp32 %.3g; L2 product %.3g, plain fp32 %.3g; update L2 %.3g"
          % (tag, float(e_prod.max()), float(e_32.max()), float(e_prod.norm()), float(e_32.norm()), float((want - p0).norm())))
    note("library train %s max|err| / fp32 torch's" % tag, float(e_prod.max()) / float(e_32.max()), 4.0, width=46)
    note("library train %s L2 err / fp32 torch's" % tag, float(e_prod.norm()) / float(e_32.norm()), 4.0, width=46)
    assert float(e_prod.max()) <= 4 * float(e_32.max()), (float(e_prod.max()), float(e_32.max()))
    assert float(e_prod.norm()) <= 4 * float(e_32.norm()), (float(e_prod.norm()), float(e_32.norm()))
    assert float((want - p0).norm()) > 50 * float(e_prod.norm())
