"""fp64 restatements of the entry points of csrc/dm_sac.hip, one function per kernel, each with a per-element error bound
(test helper, not a conftest; numpy only, no ``deepmimic_mujoco_amd`` import and no ``dm_*`` call).

Every function takes the kernel's fp32 inputs as numpy arrays and returns ``(values, bounds)``: two dicts with the same keys, the
fp64 value of every output and the most an fp32 evaluation may differ from it.  An output the kernel only moves (ring rows,
gathered rows, the ReLU-masked gradient) is returned in its own dtype with bound 0: the test compares bits.

Bounds, by first-order propagation with U = 2**-24 (the unit roundoff of fp32; one ulp is at most 2 U relative):
  * a dot product or a sequential / tree sum of n terms: (n + 2) U sum|terms| (any order of summation; the 2 covers one more
    operation on the result, e.g. the division of a mean);
  * expf, logf, tanhf: 2 ulp each (HIP's documented accuracy class); powf 2 ulp, sqrtf and the four operations U;
  * the action a = tanh(mu + std eps): A_TOL = 4 ulp of 1 = 2 ulp of tanhf + the rounding of mu + std eps carried through
    (1 - a^2) |u| <= 0.45.  That holds for a u rounded ONCE, relative to |u|: the kernels form the noise and u in fp64 and round
    u to fp32 (csrc/dm_sac.hip: sac_normal2, sac_squash_u);
  * everything downstream of a (log(1 - a^2 + 1e-6), 2 a om / (om + 1e-6)): |df/da| A_TOL on top of its own roundings.  Near
    saturation df/da reaches millions, and the bound is that large there on purpose;
  * the draws: the kernels evaluate dm_normal2's Box-Muller pair (csrc/dm_rng.h) in fp64 and round it to fp32 where log pi and the
    log_std gradient use it, so eps is off by U |eps| (`draws`); it enters log pi through eps^2 / 2 and the log_std gradient
    through g_u std eps.
Scalars the host passes as C floats (learning rate, betas, gamma, tau, target entropy) enter as their fp32 values."""
import math

import numpy as np

from kernel_helpers import hash32
from sac_helpers import gather_rows, uniforms

U = 2.0 ** -24
ULP = 2.0 ** -23
A_TOL = 4 * 2.0 ** -24 * 2
LOG_SQRT_2PI = 0.9189385332046727
SQ = 1e-6                       # SB3's epsilon inside the squash correction
EP_HIST = 100
SAC_THREADS = 256

# the values every head row of the kernel tests is built from
MU_SET = np.array([0.0, 0.1, -0.1, 3.0, -3.0, 9.0, -9.0, 12.0, -12.0, 30.0, -30.0], np.float32)
_m20, _p2 = np.float32(-20.0), np.float32(2.0)
LS_SET = np.array([-25.0, np.nextafter(_m20, np.float32(-np.inf)), _m20, np.nextafter(_m20, np.float32(0)), -5.0, 0.0,
                   np.nextafter(_p2, np.float32(0)), _p2, np.nextafter(_p2, np.float32(np.inf)), 5.0], np.float32)


def f32(x):
    """The fp32 value of a scalar or array, as fp64."""
    return np.asarray(x, np.float32).astype(np.float64)


def head_rows(R, A):
    """[R, 2A] fp32 head rows [mu | raw log_std]: element k = r A + c takes mu = MU_SET[k % 11] and log_std = LS_SET[(k // 11) % 10],
    so 110 consecutive elements hold every (mu, log_std) pair once."""
    k = np.arange(R * A).reshape(R, A)
    return np.concatenate([MU_SET[k % 11], LS_SET[(k // 11) % 10]], 1).astype(np.float32)


def draws(seed, rows, ctr, A):
    """(eps, deps) [rows, A]: kernel_helpers.normals (the same arithmetic, asserted equal by the CPU tests) and the bound on the
    kernel's value of it: fp64 Box-Muller rounded to fp32 once, U |eps| (the fp64 evaluation's own error is 2^-29 of that)."""
    r = np.arange(rows)[:, None]
    j = np.arange(0, A + 1, 2)[None, :]
    u1 = ((hash32(seed, r, ctr, j) >> np.uint64(8)).astype(np.float64) + 1.0) / 16777216.0
    u2 = (hash32(seed, r, ctr, j + 1) >> np.uint64(8)).astype(np.float64) / 16777216.0
    rad, th = np.sqrt(-2.0 * np.log(u1)), 2 * np.pi * u2
    cs, sn = np.cos(th), np.sin(th)
    eps = np.stack([rad * cs, rad * sn], -1).reshape(rows, -1)[:, :A]
    return eps, U * np.abs(eps)


def _squash(head, A, eps):
    """mu, raw and clamped log_std, std, u, a = tanh(u) and om = 1 - a^2 (as 1 / cosh^2: exact where a rounds to 1 in fp64)."""
    h = np.asarray(head, np.float32).astype(np.float64)
    mu, lsr = h[:, :A], h[:, A:2 * A]
    ls = np.clip(lsr, -20.0, 2.0)
    sd = np.exp(ls)
    u = mu + sd * eps
    return mu, lsr, ls, sd, u, np.tanh(u), 1.0 / np.cosh(u) ** 2


def log_term(a, om):
    """(log(1 - a^2 + 1e-6), its bound): |d/da| A_TOL = 2 |a| A_TOL / arg, the roundings of a a, 1 - . and . + 1e-6 over arg, and
    logf's 2 ulp."""
    arg = om + SQ
    t = np.log(arg)
    return t, 2 * ULP * np.abs(t) + (2 * np.abs(a) * A_TOL + U * (a * a + 2 * arg)) / arg


# ---- dm_sac_act
def act(head, N, A, ld, seed, ctr, warmup, deterministic, lo, hi):
    lo, hi = f32(lo)[None, :], f32(hi)[None, :]
    w = hi - lo
    if warmup:
        u = uniforms(seed, N, ctr, A)                       # exact in fp32
        ae = lo + u * w
        dae = U * (np.abs(ae) + 2 * np.abs(u * w))          # hi - lo, the product, the sum
        t = (ae - lo) / w
        dt = (dae + U * np.abs(ae - lo)) / np.abs(w) + 2 * U * np.abs(t)
        a = 2 * t - 1
        return dict(act=a, act_env=ae), dict(act=2 * dt + U * np.abs(a), act_env=dae)
    h = np.asarray(head, np.float32).reshape(N, ld)[:, :2 * A]
    eps = np.zeros((N, A)) if deterministic else draws(seed, N, ctr, A)[0]
    a = _squash(h, A, eps)[5]
    ae = lo + 0.5 * (a + 1) * w
    p = 0.5 * (a + 1) * w
    dae = 0.5 * np.abs(w) * (A_TOL + U * np.abs(a + 1)) + 3 * U * np.abs(p) + U * np.abs(ae)
    return dict(act=a, act_env=ae), dict(act=np.full_like(a, A_TOL), act_env=dae)


# ---- dm_sac_store
def new_store_state(N, D, A, cap, last_obs, ring=None, counter=0):
    z = lambda *s: np.zeros(s, np.float32)
    return dict(r_obs=z(cap * N, D), r_act=z(cap * N, A), r_rew=z(cap * N), r_done=z(cap * N), r_next=z(cap * N, D),
                last_obs=np.array(last_obs, np.float32), ring=np.array([0, 0, 0, 0] if ring is None else ring, np.int64),
                counter=int(counter), ep_acc=z(2 * N), ep_hist=z(2 * EP_HIST), episodes=[])


def store(S, N, D, A, cap, act, rew, done, obs, terminal_obs):
    """One vec-env step into the state S of new_store_state, in place; every value is moved or added in fp32, so all bounds
    are 0.  Finished episodes enter ep_hist in env order, which is ONE of the orders the kernel's atomics may produce: compare
    ep_hist as a multiset per step (S["episodes"] lists (step's episodes) in arrival order of this reference)."""
    pos = int(S["ring"][0])
    sl = slice(pos * N, (pos + 1) * N)
    d = np.asarray(done) != 0
    S["r_obs"][sl] = S["last_obs"]
    S["r_next"][sl] = np.where(d[:, None], terminal_obs, obs)
    S["r_act"][sl] = act
    S["r_rew"][sl] = rew
    S["r_done"][sl] = d.astype(np.float32)
    S["last_obs"] = np.array(obs, np.float32)
    ret = (S["ep_acc"][:N] + np.asarray(rew, np.float32)).astype(np.float32)
    ln = (S["ep_acc"][N:] + np.float32(1)).astype(np.float32)
    step_eps = []
    for e in np.nonzero(d)[0]:
        k = int(S["ring"][3]) % EP_HIST
        S["ep_hist"][k], S["ep_hist"][EP_HIST + k] = ret[e], ln[e]
        S["ring"][3] += 1
        step_eps.append((float(ret[e]), float(ln[e])))
    S["episodes"].append(step_eps)
    S["ep_acc"][:N] = np.where(d, np.float32(0), ret)
    S["ep_acc"][N:] = np.where(d, np.float32(0), ln)
    S["ring"][0] = (pos + 1) % cap
    S["ring"][1] = min(int(S["ring"][1]) + 1, cap)
    S["ring"][2] = 0
    S["counter"] += 1
    return S, {k: 0.0 for k in S if k != "episodes"}


# ---- dm_sac_gather
def gather(B, N, D, A, seed, ctr, fill, r_obs, r_act, r_rew, r_done, r_next):
    """Rows drawn over the fill * N stored transitions; xpi / xt hold their first D columns only (the head writes the rest)."""
    idx = gather_rows(seed, B, ctr, int(fill) * N).astype(np.int64)
    o, n = r_obs[idx], r_next[idx]
    v = dict(idx=idx, obs2=np.concatenate([o, n]), xq=np.concatenate([o, r_act[idx]], 1), xpi_obs=o, xt_obs=n, rew=r_rew[idx],
             done=r_done[idx])
    return v, {k: 0.0 for k in v}


# ---- the one-scalar Adam step of dm_sac_head_fwd (torch.optim.Adam, no weight decay)
def adam_scalar(p, m0, v0, t0, g, dg, lr, b1, b2, eps):
    """(p, m, v, t) after one step and their bounds; dg is the bound on the gradient.  bc1 = 1 - b1^t cancels (powf 2 ulp of b1^t
    over 1 - b1^t), likewise bc2."""
    t = t0 + 1.0
    m = b1 * m0 + (1 - b1) * g
    dm = (1 - b1) * dg + 3 * U * (abs(b1 * m0) + abs((1 - b1) * g))
    v = b2 * v0 + (1 - b2) * g * g
    dv = (1 - b2) * 2 * abs(g) * dg + 4 * U * (abs(b2 * v0) + (1 - b2) * g * g)
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    dbc1, dbc2 = 2 * ULP * b1 ** t + U * bc1, 2 * ULP * b2 ** t + U * bc2
    bc2s = math.sqrt(bc2)
    dbc2s = dbc2 / (2 * bc2s) + U * bc2s
    sv = math.sqrt(v)
    dsv = dv / (2 * sv) + U * sv
    den = sv / bc2s + eps
    dden = dsv / bc2s + sv * dbc2s / bc2s ** 2 + U * sv / bc2s + U * den
    step = (lr / bc1) * m / den
    dstep = abs(step) * (dbc1 / bc1 + dden / den + 3 * U) + abs(lr / bc1 / den) * dm
    pn = p - step
    return (pn, m, v, t), (dstep + U * abs(pn), dm, dv, 0.0)


# ---- dm_sac_head_fwd
def head_fwd(head, R, Rpi, A, seed, ctr, st, alpha_step, target_entropy, lr, b1=0.9, b2=0.999, eps_adam=1e-8):
    """a [R, A] (rows [0, Rpi) are a_pi, the rest a'), logp [R], st [16] (slots 4, 8, 5 and, with alpha_step, 0..3; the others
    as given).  `terms` / `dterms` are the per-action summands of log pi and their bounds (the saturated-action check)."""
    eps, deps = draws(seed, R, ctr, A)
    mu, lsr, ls, sd, u, a, om = _squash(np.asarray(head, np.float32).reshape(R, 2 * A), A, eps)
    lt, dlt = log_term(a, om)
    gauss = 0.5 * eps * eps + ls + LOG_SQRT_2PI
    mag = 0.5 * eps * eps + np.abs(ls) + LOG_SQRT_2PI
    lp = -(gauss + lt).sum(1)
    # 4A summands in sequence; eps^2 / 2 moves by |eps| deps, the log term by its own bound
    dlp = (4 * A + 2) * U * (mag + np.abs(lt)).sum(1) + (np.abs(eps) * deps + dlt).sum(1)
    st = np.asarray(st, np.float32).astype(np.float64).copy()
    dst = np.zeros(16)
    la = st[0]
    mean = lp[:Rpi].sum() / Rpi
    dmean = ((Rpi + 2) * U * np.abs(lp[:Rpi]).sum() + dlp[:Rpi].sum()) / Rpi
    te, lr = float(f32(target_entropy)), float(f32(lr))
    st[4], dst[4] = math.exp(la), 2 * ULP * math.exp(la)
    st[8], dst[8] = mean, dmean
    st[5] = -la * (mean + te)
    dst[5] = abs(la) * (dmean + U * abs(mean + te)) + U * abs(st[5])
    if alpha_step:
        g, dg = -(mean + te), dmean + U * abs(mean + te)
        (st[0], st[1], st[2], st[3]), (dst[0], dst[1], dst[2], dst[3]) = adam_scalar(
            la, st[1], st[2], st[3], g, dg, lr, float(f32(b1)), float(f32(b2)), float(f32(eps_adam)))
    vals = dict(a=a, logp=lp, st=st, terms=dict(gauss=gauss, mag=mag, log=lt, eps=eps, deps=deps))
    return vals, dict(a=np.full_like(a, A_TOL), logp=dlp, st=dst)


# ---- dm_sac_critic_loss
def critic_loss(q, qt, logp_next, rew, done, B, gamma, alpha):
    q, qt = f32(q).reshape(2, B), f32(qt).reshape(2, B)
    lpn, rew, done, gamma, alpha = f32(logp_next), f32(rew), f32(done), float(f32(gamma)), float(f32(alpha))
    nq = np.minimum(qt[0], qt[1]) - alpha * lpn
    dnq = U * np.abs(alpha * lpn) + U * np.abs(nq)
    k = (1 - done) * gamma
    y = rew + k * nq
    dy = k * (dnq + 2 * U * np.abs(nq)) + U * np.abs(y)
    e = q - y[None, :]
    de = dy[None, :] + U * np.abs(e)
    dq = e / B
    ddq = (de + 2 * U * np.abs(e)) / B
    db3 = dq.sum(1)
    ddb3 = (B + 2) * U * np.abs(dq).sum(1) + ddq.sum(1)
    loss = 0.5 * (e * e).sum() / B
    dloss = 0.5 * ((2 * B + 4) * U * (e * e).sum() + (2 * np.abs(e) * de).sum()) / B + 3 * U * abs(loss)
    return dict(dq=dq, db3=db3, loss=loss, y=y), dict(dq=ddq, db3=ddb3, loss=dloss)


# ---- dm_sac_actor_loss
def actor_loss(q, logp, B, alpha):
    """dq is exact: -fl(1 / B) on the smaller critic's row, the first on a tie (torch.min), 0 on the other."""
    q32 = np.asarray(q, np.float32).reshape(2, B)
    q, lp, alpha = q32.astype(np.float64), f32(logp), float(f32(alpha))
    first = q[0] <= q[1]
    inv = np.float32(1) / np.float32(B)
    dq = np.zeros((2, B), np.float32)
    dq[0, first], dq[1, ~first] = -inv, -inv
    qmin = np.where(first, q[0], q[1])
    mags = np.abs(alpha * lp) + np.abs(qmin)
    loss = (alpha * lp - qmin).sum() / B
    return dict(dq=dq, loss=loss), dict(dq=0.0, loss=(2 * B + 3) * U * mags.sum() / B + 3 * U * abs(loss))


# ---- dm_sac_head_bwd
def head_bwd(head, B, A, seed, ctr, dx, K, col, alpha):
    """dhead [B, 2A] = [dmu | dlog_std] and dbias [2A].  g_u = da om + w 2 a om / (om + 1e-6), w = alpha / B."""
    eps, deps = draws(seed, B, ctr, A)
    mu, lsr, ls, sd, u, a, om = _squash(np.asarray(head, np.float32).reshape(-1, 2 * A)[:B], A, eps)
    dx = f32(dx).reshape(2 * B, K)
    da = dx[:B, col:col + A] + dx[B:, col:col + A]
    w = float(f32(alpha)) / B
    c = float(np.float32(SQ))
    f1 = da * om
    f2 = w * 2 * a * om / (om + c)
    gu = f1 + f2
    dom = U * (a * a + om)                                                   # a a and 1 - . in fp32
    dgu_da = np.abs(-2 * a * da + w * (2 * om / (om + c) - 4 * a * a * c / (om + c) ** 2))
    dgu = (dgu_da * A_TOL + np.abs(da) * dom + 3 * U * np.abs(f1) + np.abs(w * 2 * a) * c / (om + c) ** 2 * dom
           + 7 * U * np.abs(f2) + U * np.abs(gu))
    se = sd * eps
    dse = sd * deps + (2 * ULP + U) * np.abs(se)                             # expf 2 ulp, the product
    inside = (lsr >= -20.0) & (lsr <= 2.0)
    dls = np.where(inside, gu * se - w, 0.0)
    ddls = np.where(inside, dgu * np.abs(se) + np.abs(gu) * dse + 2 * U * np.abs(gu * se) + 2 * U * w + U * np.abs(dls), 0.0)
    dhead, ddhead = np.concatenate([gu, dls], 1), np.concatenate([dgu, ddls], 1)
    dbias = dhead.sum(0)
    ddbias = (B + 2) * U * np.abs(dhead).sum(0) + ddhead.sum(0)
    return dict(dhead=dhead, dbias=dbias, inside=inside, a=a), dict(dhead=ddhead, dbias=ddbias)


# ---- dm_sac_linear_relu
def linear_relu(X, ldx, W, b, B, O, I, nets):
    """Y [nets, B, O / nets] = relu(X W^T + b) and (I + 2) U (sum_k |x_k| |w_k| + |b|)."""
    x = f32(X).reshape(B, ldx)[:, :I]
    W, b = f32(W).reshape(O, I), f32(b)
    On = O // nets
    y = np.maximum(x @ W.T + b, 0.0)
    d = (I + 2) * U * (np.abs(x) @ np.abs(W).T + np.abs(b))
    lay = lambda t: t.reshape(B, nets, On).transpose(1, 0, 2).copy()
    return dict(Y=lay(y)), dict(Y=lay(d))


# ---- dm_sac_relu_bwd_colsum
def relu_bwd_colsum(dY, Y, B, O, nets):
    """dZ (fp32, exact) = dY where Y > 0 (0.0 and -0.0 are not), db [nets, O] = its sums over the rows."""
    dY, Y = np.asarray(dY, np.float32).reshape(nets, B, O), np.asarray(Y, np.float32).reshape(nets, B, O)
    dZ = np.where(Y > 0, dY, np.float32(0)).astype(np.float32)
    z = dZ.astype(np.float64)
    return dict(dZ=dZ, db=z.sum(1)), dict(dZ=0.0, db=(B + 2) * U * np.abs(z).sum(1))


# ---- dm_sac_polyak
def polyak(p, t, tau):
    """t (1 - tau) + tau p; the bound of tests/test_sac_gpu.py: 1 - tau, two products and the sum, each rounded once."""
    p, t, tau = f32(p), f32(t), float(f32(tau))
    return dict(t=t * (1 - tau) + tau * p), dict(t=3 * U * (np.abs(t) + tau * np.abs(p)) + 1e-30)


# ---- inputs the CPU and GPU tests share (the CPU tests assert the conditions the GPU tests rely on)
def loss_inputs(B, flip=0, ties=True):
    """q, qt, q_pi [2, B], logp, logp_next, rew, done [B] in fp32: done alternates (starting with `flip`), every third row of
    q_pi is an exact tie q0 == q1 (ceil(B / 3) >= B // 4 rows); q and qt have no ties."""
    rng = np.random.default_rng(1000 + 2 * B + flip)
    n = lambda *s: rng.standard_normal(s).astype(np.float32)
    q, qt, qpi = 3 * n(2, B), 3 * n(2, B), 3 * n(2, B)
    if ties:
        qpi[1, ::3] = qpi[0, ::3]
    done = ((np.arange(B) + flip) % 2).astype(np.float32)
    return dict(q=q, qt=qt, qpi=qpi, logp=(10 * n(B) - 5).astype(np.float32), logp_next=(10 * n(B) - 5).astype(np.float32), rew=n(B),
                done=done)


TINY = np.float32(1.1754944e-38)


def relu_inputs(B, O, nets, shift=0):
    """(dY, Y) [nets, B, O] fp32: Y[n, r, c] is 0.0, -0.0, the smallest normal or a normal draw by (r + c + shift) % 4."""
    rng = np.random.default_rng(77 + B + O)
    dY = rng.standard_normal((nets, B, O)).astype(np.float32)
    Y = rng.standard_normal((nets, B, O)).astype(np.float32)
    kind = np.broadcast_to((np.arange(B)[:, None] + np.arange(O)[None, :] + shift) % 4, (nets, B, O))
    Y[kind == 0], Y[kind == 1], Y[kind == 2] = np.float32(0.0), np.float32(-0.0), TINY
    return dY, Y, kind


def store_inputs(N, D, A, step, all_done=False):
    """What one vec-env step hands dm_sac_store: act, rew, done (env e is done when (e + step) % 3 == 0), obs, terminal_obs."""
    rng = np.random.default_rng(5000 + 131 * step + N)
    n = lambda *s: rng.standard_normal(s).astype(np.float32)
    done = np.ones(N, np.uint8) if all_done else ((np.arange(N) + step) % 3 == 0).astype(np.uint8)
    return dict(act=np.tanh(n(N, A)), rew=n(N), done=done, obs=n(N, D), terminal_obs=n(N, D))
