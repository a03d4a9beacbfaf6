"""fp64 restatements of the layer kernels of the fp32 library-path learner (csrc/dm_ppo.hip: dm_linear_tanh,
dm_tanh_linear_wgrad, dm_tanh_bwd_colsum, dm_colsum, dm_linear_wgrad, dm_ppo_loss), each with a per-element error bound, the
inputs the tests feed them and the shape lists of the GPU tests (test helper, not a conftest; numpy and torch-on-CPU only, no
``deepmimic_mujoco_amd`` import and no ``dm_*`` call).

Every function takes the kernel's fp32 inputs as numpy arrays, widens them to fp64 and returns ``(value, bound)``: the fp64
value of every output element and the most an fp32 evaluation may differ from it.  Bounds are first-order propagation with
U = 2**-24, the unit roundoff of fp32 (a rounded operation is off by at most U relative, one ulp by at most 2 U relative), and
are derived from what the kernels do, never from what they give:

  * a dot product or a sum of n terms, IN ANY ORDER (split-K, partial sums met in LDS, float atomics): (n + 2) U sum|terms|.
    Each term passes through at most n - 1 additions and one multiplication; the 2 covers the bias added to a dot product
    or one more operation on the sum.
  * dZ = dY (1 - Y^2) as fl(g * fl(1 - fl(y y))): |g| U (y^2 + 2 (1 - y^2)) = U |dY| (2 - Y^2) — an absolute statement
    relative to |dY|, because 1 - y^2 cancels near |y| = 1 and no bound relative to dZ exists there.  With the product
    contracted into an FMA one of the three roundings disappears, so the bound holds either way.
  * lt_tanh, T_TANH = 8 U absolute (see `tanh_error_units`, which the CPU test evaluates on a dense grid):
      |x| >= 0.25:  y = 1 - 2 rcp(fl(t + 1)),  t = exp2(fl(x c)),  c = fp32(2 / ln 2).  fl(x c) and c's own rounding move the
      argument by 2 U relative, i.e. t by 4 |x| U relative; v_exp_f32 and v_rcp_f32 are 1 ulp each (AMD's ISA documentation:
      2 U relative), t + 1 rounds by U relative, the last subtraction (or the FMA that replaces it) by U |y|.  With
      p = 2 / (t + 1) = 1 - tanh x and q = t / (t + 1):  |err| <= (p (q (4 |x| + 2) + 3) + |y|) U, whose supremum over
      |x| >= 0.25 is 7.4 U near x = -1.3 (7 U as x -> -inf, where p -> 2: the negative side carries 1 - 2 r with r near 1).
      |x| < 0.25:  x (1 + s (c1 + s (c2 + s (c3 + s c4)))), s = x^2: the series cut after x^9 leaves 0.00886 x^11 <= 2.2e-9
      = 0.04 U; the coefficients' roundings and the Horner steps inside the bracket (values near 1, each step scaled by
      s <= 1 / 16) stay below 1.2 U relative to the bracket, the last product adds U: |err| <= 0.25 x 2.2 U + 0.04 U < U.
  * y = lt_tanh(fl(z)) with z the pre-activation, |fl(z) - z| <= dz = (I + 2) U (sum_k |x_k w_k| + |b|):
    (1 - y^2 + dz) dz + T_TANH.  |tanh''| <= 0.77, so the second-order term is below 0.4 dz^2 and `+ dz` covers it.
  * dm_ppo_loss: see `ppo_loss`.

`keep` (rows) and `cols` (input columns) recompute a VALUE with part of the input left out — what a kernel that skipped that
row or column would give.  The bound is always that of the full input.  tests/test_ppo_layer_ref64.py asserts that leaving
out the last row, or the last column, moves every shape's reference by more than its bound."""
import math

import numpy as np
import torch

import ppo_ref64

U = 2.0 ** -24
T_TANH = 8 * U
LOG_2PI = math.log(2.0 * math.pi)


def f64(x):
    """The fp32 values of an array, as fp64.  (An array that already is fp64 is taken as it is: the CPU test pins the backward
    restatements to autograd with the unrounded activations of an fp64 forward.)"""
    x = np.asarray(x)
    return x if x.dtype == np.float64 else x.astype(np.float32).astype(np.float64)


def tanh_error_units(x):
    """The first-order error of lt_tanh at x in units of U (module docstring).  T_TANH / U is its supremum rounded up."""
    x = np.asarray(x, np.float64)
    y = np.tanh(x)
    p, q = 1.0 - y, (1.0 + y) / 2.0
    big = p * (q * (4.0 * np.abs(x) + 2.0) + 3.0) + np.abs(y)
    poly = np.abs(x) * 2.2 + 0.00886 * np.abs(x) ** 11 / U
    return np.where(np.abs(x) < 0.25, poly, big)


# ---------------------------------------------------------------------------------------------------------------- the kernels
def linear_tanh(X, W, b, cols=None):
    """dm_linear_tanh: tanh(X W^T + b), [B x O]."""
    X, W, b = f64(X), f64(W), f64(b)
    I = X.shape[1]
    k = I if cols is None else cols
    z = X[:, :k] @ W[:, :k].T + b
    dz = (I + 2) * U * (np.abs(X) @ np.abs(W).T + np.abs(b))
    y = np.tanh(z)
    yf = np.tanh(X @ W.T + b)
    return y, (1.0 - yf * yf + dz) * dz + T_TANH


def _rows(B, keep):
    m = np.ones(B, bool) if keep is None else np.asarray(keep, bool)
    return m[:, None].astype(np.float64)


def tanh_bwd(dY, Y, keep=None):
    """dm_tanh_bwd_colsum: {"dz": dY (1 - Y^2) [B x O], "db": its column sums [O]}."""
    g, y = f64(dY), f64(Y)
    B = g.shape[0]
    dz = g * (1.0 - y * y)
    edz = U * np.abs(g) * (2.0 - y * y)
    val = {"dz": dz, "db": (dz * _rows(B, keep)).sum(0)}
    return val, {"dz": edz, "db": (B + 2) * U * np.abs(dz).sum(0) + edz.sum(0)}


def tanh_wgrad(dY, Y, X, keep=None, cols=None):
    """dm_tanh_linear_wgrad: {"dw": (dY (1 - Y^2))^T X [O x I], "db": column sums of dY (1 - Y^2) [O]}.  The kernel forms
    a = dY (1 - Y^2) in fp32 (off by U |dY| (2 - Y^2)) and sums a x over the batch."""
    g, y, x = f64(dY), f64(Y), f64(X)
    B, I = x.shape
    a = g * (1.0 - y * y)
    ea = U * np.abs(g) * (2.0 - y * y)
    am = a * _rows(B, keep)
    dw = am.T @ x
    if cols is not None:
        dw[:, cols:] = 0.0
    val = {"dw": dw, "db": am.sum(0)}
    return val, {"dw": (B + 2) * U * (np.abs(a).T @ np.abs(x)) + ea.T @ np.abs(x), "db": (B + 2) * U * np.abs(a).sum(0) + ea.sum(0)}


def linear_wgrad(dY, X, keep=None, cols=None):
    """dm_linear_wgrad: {"dw": dY^T X [O x I], "db": column sums of dY [O]}."""
    g, x = f64(dY), f64(X)
    B = x.shape[0]
    gm = g * _rows(B, keep)
    dw = gm.T @ x
    if cols is not None:
        dw[:, cols:] = 0.0
    return {"dw": dw, "db": gm.sum(0)}, {"dw": (B + 2) * U * (np.abs(g).T @ np.abs(x)), "db": (B + 2) * U * np.abs(g).sum(0)}


def colsum(Y, out0=None, keep=None):
    """dm_colsum: out0 + column sums of Y [O] (the kernel ACCUMULATES into its output; out0 = None is a zeroed one)."""
    y = f64(Y)
    B = y.shape[0]
    o = np.zeros(y.shape[1]) if out0 is None else f64(out0)
    return o + (y * _rows(B, keep)).sum(0), (B + 3) * U * (np.abs(y).sum(0) + np.abs(o))


def ppo_loss(mean, log_std, value, act, old_logp, adv, ret, clip, vf_coef, ent_coef, normalize, keep=None, tie_rows=None):
    """dm_ppo_loss.  Values: {"out8", "gm" [B x A], "gv" [B], "gl" [A]} from ppo_ref64.head_loss and autograd in fp64 (clip,
    vf_coef, ent_coef enter as the fp32 values the host passes).  Bounds for gm, gv, gl, following ppo_loss_kernel line by line
    (expf is 2 ulp = 4 U relative, HIP's documented class):
      d = act - mean: U |d|;  iv = expf(-2 log_std): 4 U;  z2 = d d iv: 8 U z2;  zs = sum_j z2 over a 5-step butterfly: 13 U zs;
      lconst = -sum log_std - fl(fl(0.5 log 2pi) A): 5 U sum|log_std| + 2 U 0.919 A + U |lconst|;
      logp = -0.5 zs + lconst: 6.5 U zs + e(lconst) + U |logp|;  lr = logp - old_logp: e(logp) + U |lr|;
      ratio = expf(lr): ratio (4 U + e(lr));
      the advantage statistics (ppo_prepare_body): e(mean) = (B + 2) U sum|adv| / B, the centred squares carry
      2 e(mean) sum|c| + 2 U q on q = sum c^2 besides (B + 2) U q for the sum, and 1 / (sqrt(q / (B - 1)) + 1e-8) adds the
      division, the root, the addition and the reciprocal: rel(ainv) = (rel(q) + U) / 2 + 3 U;
      a_n = (adv - amean) ainv: (e(mean) + U |c|) ainv + |a_n| (rel(ainv) + U)  (0 when the advantages are not normalised);
      dlogp = -(1 / B) dr ratio: (e(a_n) ratio + |a_n| e(ratio)) / B + 3 U |dlogp|;
      grad_mean = dlogp d iv: |d iv| e(dlogp) + 7 U |grad_mean|;  grad_value = vf_coef 2 (1 / B) (value - ret): 5 U |grad_value|;
      grad_log_std_j = sum_b dlogp (z2 - 1) - ent_coef: per term e(dlogp) |z2 - 1| + |dlogp| (8 U z2 + U |z2 - 1|) + U |term|,
      (B + 2) U sum|terms| for the sum in any order (block partials, float atomics), 2 U (|result| + ent_coef) for the last step.
    Which branch of the clipped surrogate a row takes is decided by comparisons of fp32 quantities: a row whose fp64 ratio lies
    within e(ratio) + 2 U of 1 - clip or 1 + clip, or whose |a_n| <= e(a_n) outside the clip range, may take either, and is
    listed in ``amb``; its grad_mean row may equal the a_n branch or 0 (``gm_alt`` holds the other one), and its whole
    contribution is added to the bound of grad_log_std.  ``tie_rows`` names rows built so that the fp32 ratio is EXACTLY 1 with
    clip = 0 (the `>=` / `<=` of `inside`): they are inside by construction and never ambiguous.
    ``keep`` leaves rows out of the grad_log_std SUM only (1 / B and the statistics stay those of the full batch: what a loop
    that skipped the row would give)."""
    clip, vf_coef, ent_coef = (float(np.float32(v)) for v in (clip, vf_coef, ent_coef))
    m, ls, v, a, olp, ad, rt = (f64(t) for t in (mean, log_std, value, act, old_logp, adv, ret))
    B, A = m.shape
    norm = bool(normalize) and B > 1
    T = lambda t: torch.tensor(t, dtype=torch.float64)
    tm, tl, tv = T(m).requires_grad_(True), T(ls).requires_grad_(True), T(v).requires_grad_(True)
    total, out8 = ppo_ref64.head_loss(tm, tl, tv, T(a), T(ad), T(rt), T(olp), clip_range=clip, vf_coef=vf_coef, ent_coef=ent_coef,
                                      normalize=norm)
    gm, gl, gv = (t.numpy() for t in torch.autograd.grad(total, [tm, tl, tv]))
    # the kernel's quantities in fp64, row by row
    d = a - m
    iv = np.exp(-2.0 * ls)[None, :]
    z2 = d * d * iv
    zs = z2.sum(1)
    lconst = -ls.sum() - 0.5 * LOG_2PI * A
    logp = -0.5 * zs + lconst
    lr = logp - olp
    ratio = np.exp(lr)
    e_lconst = 5 * U * np.abs(ls).sum() + 2 * U * 0.919 * A + U * abs(lconst)
    e_lr = 6.5 * U * zs + e_lconst + U * np.abs(logp) + U * np.abs(lr)
    e_ratio = ratio * (4 * U + e_lr)
    if norm:
        am = ad.mean()
        c = ad - am
        q = (c * c).sum()
        ainv = 1.0 / (math.sqrt(q / (B - 1)) + 1e-8)
        e_mean = (B + 2) * U * np.abs(ad).sum() / B
        rel_q = (B + 2) * U + 2 * U + 2 * e_mean * np.abs(c).sum() / q
        rel_ainv = (rel_q + U) / 2 + 3 * U
        a_n = c * ainv
        e_an = (e_mean + U * np.abs(c)) * ainv + np.abs(a_n) * (rel_ainv + U)
    else:
        a_n, e_an = ad.copy(), np.zeros(B)
    lo, hi = 1.0 - clip, 1.0 + clip
    inside = (ratio >= lo) & (ratio <= hi)
    near = np.minimum(np.abs(ratio - lo), np.abs(ratio - hi)) <= e_ratio + 2 * U
    if tie_rows is not None:
        inside[np.asarray(tie_rows)] = True
        near[np.asarray(tie_rows)] = False
    amb = near | (~inside & (np.abs(a_n) <= e_an))
    live = inside | (a_n * ratio < a_n * np.clip(ratio, lo, hi))
    dl_full = -(a_n * ratio) / B                                  # dlogp of the a_n branch
    dlogp = np.where(live, dl_full, 0.0)
    e_dl = (e_an * ratio + np.abs(a_n) * e_ratio) / B + 3 * U * np.abs(dl_full)
    gm_a = dl_full[:, None] * d * iv
    e_gm = np.abs(d * iv) * e_dl[:, None] + 7 * U * np.abs(gm_a)
    gm_alt = np.where(live[:, None], 0.0, gm_a)
    terms = dlogp[:, None] * (z2 - 1.0)
    terms_a = dl_full[:, None] * (z2 - 1.0)
    e_terms = e_dl[:, None] * np.abs(z2 - 1.0) + np.abs(dl_full)[:, None] * (8 * U * z2 + U * np.abs(z2 - 1.0)) + U * np.abs(terms_a)
    e_terms = np.where(live[:, None] | amb[:, None], e_terms, 0.0)
    gl_rows = terms.sum(0) - ent_coef
    e_gl = (e_terms.sum(0) + (B + 2) * U * np.abs(terms).sum(0) + 2 * U * (np.abs(gl_rows) + ent_coef)
            + (np.abs(terms_a) * amb[:, None]).sum(0))
    val = {"out8": out8.detach().numpy(), "gm": gm, "gv": gv, "gl": gl if keep is None else (terms * _rows(B, keep)).sum(0) - ent_coef}
    info = {"amb": np.nonzero(amb)[0], "gm_alt": gm_alt, "ratio": ratio, "gl_rows": gl_rows, "gm_rows": np.where(live[:, None], gm_a, 0.0),
            "gv_rows": vf_coef * 2.0 * (v - rt) / B}
    return val, {"gm": e_gm, "gv": 5 * U * np.abs(gv), "gl": e_gl}, info


# ------------------------------------------------------------------------------------------------------------------ the inputs
def _rng(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 12345) % (2 ** 31 - 1)
    return np.random.RandomState(seed)


def f32(x):
    return np.ascontiguousarray(x, np.float32)


def in_linear_tanh(B, O, I):
    """X ~ N(0, 1), W ~ 1.5 N(0, 1) / sqrt(I), b ~ 0.5 N(0, 1): pre-activations of spread 1.6, a fifth of them inside the
    polynomial's |z| < 0.25, a few percent beyond 3."""
    r = _rng(1, B, O, I)
    return f32(r.randn(B, I)), f32(1.5 * r.randn(O, I) / math.sqrt(I)), f32(0.5 * r.randn(O))


def activations(r, B, O):
    """[B x O] values of a tanh layer: tanh of N(0, 1.5^2) rounded to fp32, with rows b = 1, 2, 3 (mod 8) set to exactly +1, -1
    and 0 (never the last row: the sensitivity condition leaves that one out)."""
    y = np.tanh(1.5 * r.randn(B, O))
    for k, v in ((1, 1.0), (2, -1.0), (3, 0.0)):
        rows = np.arange(k, B - 1, 8)
        y[rows] = v
    return f32(y)


def in_tanh_wgrad(B, O, I):
    r = _rng(2, B, O, I)
    return f32(r.randn(B, O)), activations(r, B, O), f32(r.randn(B, I))


def in_tanh_bwd(B, O):
    r = _rng(3, B, O)
    return f32(r.randn(B, O)), activations(r, B, O)


def in_colsum(B, O):
    r = _rng(4, B, O)
    return f32(r.randn(B, O) + 0.25), f32(3.0 * r.randn(O))


def in_linear_wgrad(B, O, I):
    r = _rng(5, B, O, I)
    return f32(r.randn(B, O)), f32(r.randn(B, I))


def in_ppo_loss(B, A, noise=0.15):
    """(mean, log_std, value, act, old_logp, adv, ret): actions drawn from the policy, old_logp = the fp64 logp + N(0, noise^2), so
    that with clip 0.2 a fifth of the rows is clipped on either side."""
    r = _rng(6, B, A)
    mean = f32(2.0 * r.randn(B, A))
    log_std = f32(np.linspace(-0.7, 0.4, A))
    value, ret = f32(r.randn(B)), f32(r.randn(B))
    act = f32(mean + np.exp(log_std.astype(np.float64)) * r.randn(B, A))
    d = f64(act) - f64(mean)
    logp = (-0.5 * d * d * np.exp(-2.0 * f64(log_std)) - f64(log_std) - 0.5 * LOG_2PI).sum(1)
    eps = noise * r.randn(B)
    eps[B - 1] = 0.01                  # the last row inside the clip range with a large advantage: it carries a live gradient
    old_logp = f32(logp + eps)
    adv = f32(2.0 * r.randn(B) + 0.3)
    adv[B - 1] = 3.0
    return mean, log_std, value, act, old_logp, adv, ret


EDGE_SHAPE = (257, 2)


def in_ppo_loss_edge(clip=0.2):
    """The (257, 2) batch with old_logp rebuilt from the fp64 logp: rows b = 0, 1 (mod 4) sit on the upper and lower clip edge
    (old_logp = fp32(logp - log(1 +- clip)): the fp64 ratio of the ROUNDED old_logp is within 1e-6 of the edge, on either side of
    it as the rounding falls), rows 2, 3 (mod 4) well inside (ratio 1.05) and well outside (ratio 1.5 / 0.6).  Returns the batch
    and the list of near-edge rows."""
    B, A = EDGE_SHAPE
    mean, log_std, value, act, _, adv, ret = in_ppo_loss(B, A)
    d = f64(act) - f64(mean)
    logp = (-0.5 * d * d * np.exp(-2.0 * f64(log_std)) - f64(log_std) - 0.5 * LOG_2PI).sum(1)
    b = np.arange(B)
    target = np.select([b % 4 == 0, b % 4 == 1, b % 4 == 2, b % 8 == 3], [1.0 + float(np.float32(clip)), 1.0 - float(np.float32(clip)), 1.05, 1.5], 0.6)
    old_logp = f32(logp - np.log(target))
    return (mean, log_std, value, act, old_logp, adv, ret), np.nonzero(b % 4 < 2)[0]


TIE_SHAPE = (64, 2)


def in_ppo_loss_tie():
    """A (64, 2) batch for clip_range = 0, where 1 - clip = 1 + clip = 1: log_std = 0 (so expf(-2 log_std) = 1 exactly), act - mean
    in {-2, -1, 1, 2} on halves and quarters (d and the row's sum of squares are small integers, exact in fp32), so that
    logp = fl(-0.5 zs - fl(fl(0.5 log 2pi) A)) is ONE fp32 rounding that numpy reproduces.  Even rows get old_logp = that very
    value: lr = 0, expf(0) = 1, the ratio sits exactly on both clip edges and `inside` must hold (autograd: the tie of the min
    splits evenly over two branches that both carry a_n).  Odd rows get old_logp -+ 0.25: clipped.  Returns the batch and the
    even rows."""
    B, A = TIE_SHAPE
    r = _rng(7, B, A)
    mean = f32(np.round(r.randn(B, A) * 4) / 4)
    step = r.choice(np.array([-2.0, -1.0, 1.0, 2.0]), size=(B, A))
    act = f32(f64(mean) + step)
    assert np.array_equal(f64(act) - f64(mean), step)
    log_std = np.zeros(A, np.float32)
    c32 = np.float32(np.float32(0.5) * np.float32(1.8378770664093453)) * np.float32(A)
    zs = (step * step).sum(1)
    logp32 = (-0.5 * zs - np.float64(c32)).astype(np.float32)           # exact operands, one rounding
    b = np.arange(B)
    old_logp = f32(logp32 + np.where(b % 2 == 0, 0.0, np.where(b % 4 == 1, 0.25, -0.25)).astype(np.float32))
    value, ret, adv = f32(r.randn(B)), f32(r.randn(B)), f32(2.0 * r.randn(B) + 0.3)
    return (mean, log_std, value, act, old_logp, adv, ret), np.nonzero(b % 2 == 0)[0]


def tanh_table():
    """The arguments of the lt_tanh test, one row each (I = 1, W = 1, b = 0: the pre-activation is the input bit for bit)."""
    q = np.float32(0.25)
    up, dn = np.nextafter(q, np.float32(1)), np.nextafter(q, np.float32(0))
    pos = [0.0, 1e-30, 1e-8, dn, q, up, 0.375, 0.49, 0.5, 1.0, 4.0, 9.0, 20.0, 44.3, 44.4, 100.0, 3e38]
    return np.array([s * np.float32(v) for v in pos for s in (np.float32(1), np.float32(-1))], np.float32)


# ------------------------------------------------------------------------------------------------------------------ the shapes
# (tests/test_ppo_layer_kernels_gpu.py runs them, tests/test_ppo_layer_ref64.py holds every one to the sensitivity condition)
LT_BO = [(1, 1), (63, 127), (64, 128), (65, 129), (200, 300)]      # lone ragged tile, one full 64 x 128 tile, full next to ragged
LT_I = [1, 2, 3, 4, 5, 6, 8, 33, 64, 67, 85, 86, 98, 127, 128]
LT_OFFSET = [(65, 129, I) for I in (4, 5, 6, 8, 64, 85, 86, 128)]  # again with X, W, and both one float off 16-byte alignment
LINEAR_TANH = [(B, O, I) for (B, O) in LT_BO for I in LT_I]

TW_BO = [(1, 1), (7, 32), (31, 33), (257, 70), (513, 33), (1000, 70)]
TW_I = [1, 31, 32, 33, 64, 65, 96, 97, 128]
TANH_WGRAD = [(B, O, I) for (B, O) in TW_BO for I in TW_I]

TB_B = [1, 15, 16, 17, 63, 64, 65, 200]
TB_O_SCALAR = [1, 63, 65, 77]
TB_O_VEC = [4, 64, 68, 300]
TB_O_OFFSET = 64                                                   # the scalar kernel by an offset dY, Y or dZ
TANH_BWD = [(B, O) for O in TB_O_SCALAR + TB_O_VEC for B in TB_B]

CS_B = [1, 3, 16, 17, 127, 128, 129, 1001]
CS_O = [1, 63, 64, 65, 130]
COLSUM = [(B, O) for O in CS_O for B in CS_B]

LW_B = [64, 128, 192, 320, 1024]
LW_OI = [(1, 1), (1, 33), (33, 1), (32, 32), (33, 33), (23, 288), (288, 98), (300, 300)]
LINEAR_WGRAD = [(B, O, I) for (O, I) in LW_OI for B in LW_B]

PPO_LOSS = [(1, 1), (1, 32), (7, 32), (64, 1), (257, 32), (2049, 2), (16449, 2)]
PPO_LOSS_MODES = [(True, 0.0), (True, 0.01), (False, 0.0), (False, 0.01)]     # (normalize, ent_coef)
PPO_ROW_SENSITIVE_MAX_B = 16384       # beyond it (B + 2) U sum|terms| exceeds one row's term: see test_ppo_layer_ref64.py
