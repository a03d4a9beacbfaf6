"""tests/ppo_layer_ref64.py on the CPU: every restatement pinned to torch fp64 autograd of tanh(F.linear(...)) and of the PPO head
loss, every bound positive and finite, the lt_tanh error budget evaluated on a dense grid, and the SENSITIVITY CONDITION for
every (entry point, shape) pair that tests/test_ppo_layer_kernels_gpu.py runs (both files take the lists from ppo_layer_ref64):

  the fp64 reference recomputed with the last batch row left out differs from the full one by more than the bound, on at least
  one element of each reduction output of that shape; the same with the last input column k = I - 1 left out, for the three GEMM
  kernels.

It is a condition on the inputs and bounds, not a measurement: a kernel that skipped the last row or column of any of these
shapes cannot pass the GPU file.  (A per-row output of a skipped row stays unwritten: the GPU file pre-fills those with NaN.)

The one exception, as stated and not loosened elsewhere: the batch sums of dm_ppo_loss at B > 16 384.  There
(B + 2) U sum|terms| is B^2 U = 16 times the mean term, more than one row contributes, so grad_log_std (and the scalar means of
out8) cannot see one row under a worst-case bound; at (16 449, 2) the rows are covered by grad_mean and grad_value, one element
per row and action, NaN before the call."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ppo_layer_ref64 as ref
import ppo_ref64

REL = 1e-12


def close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all(np.abs(a - b) <= REL * max(1.0, float(np.abs(b).max()))))


def good(bound):
    b = np.asarray(bound, np.float64)
    return bool(np.all(np.isfinite(b)) and np.all(b > 0))


def moved(full, part, bound):
    """Somewhere the two references differ by more than the bound."""
    return bool(np.any(np.abs(np.asarray(full) - np.asarray(part)) > np.asarray(bound)))


def last_out(B):
    k = np.ones(B, bool)
    k[B - 1] = False
    return k


T = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)


# ------------------------------------------------------------------------------------------------------------- pinned to autograd
@pytest.mark.parametrize("B,O,I", [(5, 3, 1), (7, 4, 6), (33, 9, 17)])
def test_layer_restatements_equal_fp64_autograd(B, O, I):
    X, W, b = ref.in_linear_tanh(B, O, I)
    gy = ref.in_linear_wgrad(B, O, I)[0]
    tw, tb = T(W).requires_grad_(True), T(b).requires_grad_(True)
    y = torch.tanh(F.linear(T(X), tw, tb))
    gw, gb = torch.autograd.grad(y, [tw, tb], T(gy))
    y64 = y.detach().numpy()
    assert close(ref.linear_tanh(X, W, b)[0], y64)
    v, _ = ref.tanh_wgrad(gy, y64, X)                         # fp64 activations taken as they are
    assert close(v["dw"], gw.numpy()) and close(v["db"], gb.numpy())
    v, _ = ref.tanh_bwd(gy, y64)
    assert close(v["dz"], T(gy).numpy() * (1 - y64 ** 2)) and close(v["db"], gb.numpy())
    z = F.linear(T(X), tw, tb)
    gw2, gb2 = torch.autograd.grad(z, [tw, tb], T(gy))
    v, _ = ref.linear_wgrad(gy, X)
    assert close(v["dw"], gw2.numpy()) and close(v["db"], gb2.numpy())
    out0 = ref.in_colsum(B, O)[1]
    assert close(ref.colsum(gy, out0)[0], T(out0).numpy() + T(gy).sum(0).numpy())
    assert close(ref.colsum(gy)[0], T(gy).sum(0).numpy())


@pytest.mark.parametrize("B,A", [(1, 1), (7, 32), (257, 3)])
@pytest.mark.parametrize("normalize,ent", ref.PPO_LOSS_MODES)
def test_ppo_loss_rows_equal_fp64_autograd(B, A, normalize, ent):
    """The per-row terms behind the bounds and the sensitivity condition (gm_rows, gv_rows, gl_rows) are the autograd gradients."""
    v, bnd, info = ref.ppo_loss(*ref.in_ppo_loss(B, A), 0.2, 0.5, ent, normalize)
    assert close(info["gm_rows"], v["gm"]) and close(info["gv_rows"], v["gv"]) and close(info["gl_rows"], v["gl"])
    assert all(good(bnd[k]) for k in ("gm", "gv", "gl"))
    args = ref.in_ppo_loss(B, A)
    m, ls, val = (T(args[i]).requires_grad_(True) for i in (0, 1, 2))
    total, out8 = ppo_ref64.head_loss(m, ls, val, T(args[3]), T(args[5]), T(args[6]), T(args[4]), clip_range=float(np.float32(0.2)),
                                      vf_coef=0.5, ent_coef=float(np.float32(ent)), normalize=normalize and B > 1)
    assert close(v["out8"], out8.numpy())


def test_the_exact_tie_batch_is_inside_by_construction():
    """in_ppo_loss_tie: the fp32 logp the kernel forms equals old_logp on the even rows (their fp64 ratio is within 1e-6 of 1, the
    restatement treats them as inside), the odd rows are clipped; no row is ambiguous."""
    args, ties = ref.in_ppo_loss_tie()
    v, bnd, info = ref.ppo_loss(*args, 0.0, 0.5, 0.0, True, tie_rows=ties)
    B = ref.TIE_SHAPE[0]
    odd = np.setdiff1d(np.arange(B), ties)
    assert info["amb"].size == 0 and np.all(np.abs(info["ratio"][ties] - 1) < 1e-6) and np.all(np.abs(info["ratio"][odd] - 1) > 0.2)
    assert np.all(np.any(info["gm_rows"][ties] != 0, 1))
    # a kernel with `>` in place of `>=` treats the even rows as clipped: p1 = p2 there, so their gradient is 0
    assert moved(info["gm_rows"][ties], 0.0, bnd["gm"][ties])


def test_the_clip_edge_batch():
    args, edge = ref.in_ppo_loss_edge()
    v, bnd, info = ref.ppo_loss(*args, 0.2, 0.5, 0.0, True)
    lo, hi = 1 - float(np.float32(0.2)), 1 + float(np.float32(0.2))
    r = info["ratio"]
    assert np.all(np.minimum(np.abs(r[edge] - lo), np.abs(r[edge] - hi)) < 1e-6)
    rest = np.setdiff1d(np.arange(r.size), edge)
    assert np.all(np.minimum(np.abs(r[rest] - lo), np.abs(r[rest] - hi)) > 0.04)
    assert set(info["amb"]) <= set(edge) and info["amb"].size > 0


# ------------------------------------------------------------------------------------------------------------------ lt_tanh
def test_tanh_budget_on_a_dense_grid():
    """T_TANH / U = 8 is above the first-order budget everywhere: 7.4 near x = -1.3, below 1 inside the polynomial's range."""
    x = np.concatenate([np.linspace(-50, 50, 2000001), np.linspace(-0.3, 0.3, 200001)])
    e = ref.tanh_error_units(x)
    assert 7.3 < e.max() <= ref.T_TANH / ref.U == 8.0
    assert e[np.abs(x) < 0.25].max() < 1.0
    assert -1.6 < x[np.argmax(e)] < -1.0


def test_tanh_table_holds_what_the_gpu_test_needs():
    t = ref.tanh_table().astype(np.float64)
    assert np.array_equal(np.sort(t[t > 0]), np.sort(-t[t < 0])) and np.sum(t == 0) == 2 and np.signbit(t[t == 0]).sum() == 1
    q = np.float32(0.25)
    assert {float(np.nextafter(q, np.float32(0))), 0.25, float(np.nextafter(q, np.float32(1)))} <= set(t)
    one = np.tanh(t).astype(np.float32) == 1                     # fp64 tanh rounds to 1 in fp32
    assert one.sum() >= 5 and t[one].min() == 20.0 and not one[t == 9.0].any()


# --------------------------------------------------------------------------------------------------------- sensitivity, by shape
@pytest.mark.parametrize("B,O,I", ref.LINEAR_TANH)
def test_linear_tanh_sees_the_last_column(B, O, I):
    X, W, b = ref.in_linear_tanh(B, O, I)
    y, bnd = ref.linear_tanh(X, W, b)
    assert good(bnd)
    assert moved(y, ref.linear_tanh(X, W, b, cols=I - 1)[0], bnd)
    frac = float(np.mean(np.abs(np.arctanh(np.clip(y, -1 + 1e-15, 1 - 1e-15))) < 0.25))
    assert B * O < 2000 or 0.05 < frac < 0.5                      # both branches of lt_tanh well populated


@pytest.mark.parametrize("B,O,I", ref.TANH_WGRAD)
def test_tanh_wgrad_sees_the_last_row_and_column(B, O, I):
    gy, y, x = ref.in_tanh_wgrad(B, O, I)
    v, bnd = ref.tanh_wgrad(gy, y, x)
    assert good(bnd["dw"]) and good(bnd["db"])
    part = ref.tanh_wgrad(gy, y, x, keep=last_out(B))[0]
    assert moved(v["dw"], part["dw"], bnd["dw"]) and moved(v["db"], part["db"], bnd["db"])
    assert moved(v["dw"][:, I - 1], ref.tanh_wgrad(gy, y, x, cols=I - 1)[0]["dw"][:, I - 1], bnd["dw"][:, I - 1])
    if B > 4:
        assert (y[1] == 1).all() and (y[2] == -1).all() and (y[3] == 0).all()


@pytest.mark.parametrize("B,O", ref.TANH_BWD + [(B, ref.TB_O_OFFSET) for B in ref.TB_B])
def test_tanh_bwd_sees_the_last_row(B, O):
    gy, y = ref.in_tanh_bwd(B, O)
    v, bnd = ref.tanh_bwd(gy, y)
    assert good(bnd["dz"]) and good(bnd["db"])
    assert moved(v["db"], ref.tanh_bwd(gy, y, keep=last_out(B))[0]["db"], bnd["db"])


@pytest.mark.parametrize("B,O", ref.COLSUM)
def test_colsum_sees_the_last_row(B, O):
    y, out0 = ref.in_colsum(B, O)
    for o in (None, out0):
        v, bnd = ref.colsum(y, o)
        assert good(bnd)
        assert moved(v, ref.colsum(y, o, keep=last_out(B))[0], bnd)
    assert moved(ref.colsum(y, out0)[0], ref.colsum(y)[0], ref.colsum(y, out0)[1])      # and the value already in `out`


@pytest.mark.parametrize("B,O,I", ref.LINEAR_WGRAD)
def test_linear_wgrad_sees_the_last_row_and_column(B, O, I):
    gy, x = ref.in_linear_wgrad(B, O, I)
    v, bnd = ref.linear_wgrad(gy, x)
    assert good(bnd["dw"]) and good(bnd["db"])
    part = ref.linear_wgrad(gy, x, keep=last_out(B))[0]
    assert moved(v["dw"], part["dw"], bnd["dw"]) and moved(v["db"], part["db"], bnd["db"])
    assert moved(v["dw"][:, I - 1], 0.0, bnd["dw"][:, I - 1])


@pytest.mark.parametrize("B,A", ref.PPO_LOSS)
@pytest.mark.parametrize("normalize,ent", ref.PPO_LOSS_MODES)
def test_ppo_loss_sees_the_last_row(B, A, normalize, ent):
    """grad_log_std moves by more than its bound when the last row leaves the sum (B <= 16 384; see the module docstring); at
    every shape that row's grad_mean and grad_value are further than their bounds from any other finite value only because
    they are NaN before the call, which the GPU file checks.  At most one row in a thousand is ambiguous (at B = 16 449 the
    worst-case error of the advantage mean, 1.6e-3, exceeds three rows' |a_n|), never the last one, and a good part of the rows
    is clipped."""
    v, bnd, info = ref.ppo_loss(*ref.in_ppo_loss(B, A), 0.2, 0.5, ent, normalize)
    assert all(good(bnd[k]) for k in ("gm", "gv", "gl"))
    assert info["amb"].size <= B // 1000 and B - 1 not in info["amb"]
    if B >= 64:
        assert 0.05 < float(v["out8"][5]) < 0.95
    if B <= ref.PPO_ROW_SENSITIVE_MAX_B:
        part = ref.ppo_loss(*ref.in_ppo_loss(B, A), 0.2, 0.5, ent, normalize, keep=last_out(B))[0]
        assert moved(v["gl"], part["gl"], bnd["gl"])
    else:
        assert np.all(info["gm_rows"][B - 1] != 0) and info["gv_rows"][B - 1] != 0
