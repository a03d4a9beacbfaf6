"""Every entry point of csrc/dm_sac.hip called directly on the MI355X and held, element by element, to the fp64 restatements and
derived bounds of tests/sac_kernels_ref64.py: ragged batch sizes around the 256-thread workgroup, tiles that straddle the twin
critics, clamp edges, saturated actions, exact ties, signed zeros, the ring's ticket and the history's wrap.  Every output lives
in a NaN-fenced buffer (kernel_helpers.guarded), so a write out of range shows in the fence; no flat tolerance, no element left
out.  Each comparison prints its worst error / bound ratio (pytest -s): DESIGN section 11 quotes them.

The bounds are the derived ones and are not fitted to what the kernels give.  The action's A_TOL = 4 ulp of 1 is met because the
kernels form the noise and u = mu + std eps in fp64 and round u once (csrc/dm_sac.hip: sac_normal2, sac_squash_u); an fp32 u misses
it by up to 13 x where std = e^2 or where std eps cancels mu."""
import collections
import functools
import math

import numpy as np
import pytest
import torch

import sac_kernels_ref64 as ref
from kernel_helpers import DEV, checked, guard_ok, guarded, within

pytestmark = pytest.mark.gpu

SEED = 0x5AC1EA12
ALPHA = np.float32(0.2)


def call(name, *args):
    from deepmimic_mujoco_amd import _lib
    _lib.call(name, *args, device=DEV)


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def ints(vals):
    """A guarded int32 array: the float buffer of `guarded` seen as integers (0.0 is 0; the NaN fence keeps its bits)."""
    buf, v = guarded(len(vals), fill=0.0)
    iv = v.view(torch.int32)
    iv.copy_(torch.tensor(vals, dtype=torch.int32))
    return buf, iv


def filled(x):
    """A guarded buffer that holds the fp32 array x."""
    x = np.asarray(x, np.float32)
    buf, v = guarded(*x.shape)
    v.copy_(dev(x))
    return buf, v


def ctr_of(c):
    return torch.tensor([c], dtype=torch.int32, device=DEV)


def bits(t):
    t = t if isinstance(t, torch.Tensor) else dev(np.asarray(t, np.float32))
    return t.contiguous().view(torch.int32).cpu()


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def untouched(t):
    return bool(torch.isnan(t).all())


# ---------------------------------------------------------------------------------------------------------------- head forward
@pytest.mark.parametrize("A", [1, 2, 23, 28])
@pytest.mark.parametrize("R,Rpi", [(1, 1), (255, 255), (257, 100), (600, 300), (513, 256)])
@checked
def test_head_fwd(R, Rpi, A):
    _head_fwd(R, Rpi, A, actions=False)


@pytest.mark.parametrize("A", [1, 2, 23, 28])
@pytest.mark.parametrize("R,Rpi", [(1, 1), (255, 255), (257, 100), (600, 300), (513, 256)])
@checked
def test_head_fwd_actions(R, Rpi, A):
    """a_pi and a' per element within A_TOL = 4 ulp of 1, the same calls as test_head_fwd: the rows hold std = e^2 next to
    mu = 0, +-0.1 (an error in eps is multiplied by 7.4 and not damped by the tanh) and std eps cancelling mu = +-9, +-12 down to
    |u| < 1 (half an ulp of an fp32 product of size 12 is A_TOL / 2)."""
    _head_fwd(R, Rpi, A, actions=True)


def _head_fwd(R, Rpi, A, actions):
    """a_pi / a' (into the action columns of a wider buffer, row stride lda), log pi, st[4], st[5], st[8] and the Adam step of
    log_ent_coef at steps 1 and 5 from nonzero moments; without the alpha step st[0..3] keep their bits.  Where the fp32 action is
    exactly +-1 (A = 1 isolates one action per row) log pi is the Gaussian term minus log(1e-6) to logf's 2 ulp and the rounding of
    the four summands: the |d/da| A_TOL term, which is of order 1 there, is not granted."""
    head_np = ref.head_rows(R, A)
    head, te, lr = dev(head_np), -float(A), 3e-4
    for lda, t0, alpha_step in ((A, 0, 1), (A + 5, 4, 1), (A + 5, 2, 0)):
        ctr, off = 3 + t0, lda - A
        st0 = np.full(16, 7.0, np.float32)
        st0[:4] = [math.log(0.2), 0.3, 0.7, t0]
        sbuf, st = filled(st0)
        pbuf, pi = guarded(Rpi, lda)
        nbuf, nx = guarded(max(R - Rpi, 1), lda)
        lbuf, logp = guarded(R)
        call("dm_sac_head_fwd", head, R, Rpi, A, SEED, ctr_of(ctr), pi[:, off:], nx[:, off:] if R > Rpi else None, lda, logp, st,
             alpha_step, te, lr)
        torch.cuda.synchronize()
        assert guard_ok(sbuf, st) and guard_ok(pbuf, pi) and guard_ok(nbuf, nx) and guard_ok(lbuf, logp)
        assert untouched(pi[:, :off]) and untouched(nx[:, :off] if R > Rpi else nx)
        v, d = ref.head_fwd(head_np, R, Rpi, A, SEED, ctr, st0, alpha_step, te, lr)
        tag = "head_fwd R%d/%d A%d lda%d t%d" % (R, Rpi, A, lda, t0 + 1)
        a_got = torch.cat([pi[:, off:], nx[:, off:]]) if R > Rpi else pi[:, off:]
        if actions:
            within(tag + " a", a_got, v["a"], d["a"])
            continue
        assert bool(torch.isfinite(a_got).all()) and float(a_got.abs().max()) <= 1.0
        within(tag + " logp", logp, v["logp"], d["logp"])
        s = host(st).astype(np.float64)
        for k in (4, 8, 5) + ((0, 1, 2, 3) if alpha_step else ()):
            within(tag + " st[%d]" % k, s[k], v["st"][k], d["st"][k])
        keep = [6, 7] + list(range(9, 16)) + ([] if alpha_step else [0, 1, 2, 3])
        assert same_bits(st[keep], st0[keep])
        a32, ls = host(a_got), head_np[:, A:]
        sat = np.abs(a32) == 1.0
        if R * A >= 255:
            assert int(sat.sum()) >= 8 and int((ls == np.float32(-20)).sum()) >= 8 and int((ls == np.float32(2)).sum()) >= 8
        if A == 1 and sat.any():
            t, rows, L = v["terms"], sat[:, 0], math.log(1e-6)
            bound = 2 * ref.ULP * abs(L) + 6 * ref.U * (t["mag"][:, 0] + abs(L)) + np.abs(t["eps"][:, 0]) * t["deps"][:, 0]
            within(tag + " saturated", host(logp)[rows], (-t["gauss"][:, 0] - L)[rows], bound[rows])


# --------------------------------------------------------------------------------------------------------------- head backward
BWD = [pytest.mark.parametrize("D", [5, 98]), pytest.mark.parametrize("A", [1, 23, 28]), pytest.mark.parametrize("B", [1, 100, 256, 300])]


@functools.lru_cache(maxsize=None)
def _head_bwd(B, A, D):
    """Three runs (with dbias twice, then dbias = NULL) of dm_sac_head_bwd on the head rows of the forward tests, K = D + A, col = D,
    and the reference: shared by the two tests below, nothing in it is changed."""
    K, col, ctr = D + A, D, 11
    head_np = ref.head_rows(B, A)
    dx_np = np.random.default_rng(B + A + D).standard_normal((2 * B, K)).astype(np.float32)
    st0 = np.zeros(16, np.float32)
    st0[4] = ALPHA
    head, dx, st, runs = dev(head_np), dev(dx_np), dev(st0), []
    for with_bias in (True, True, False):
        hbuf, dh = guarded(B, 2 * A)
        bbuf, db = guarded(2 * A)
        call("dm_sac_head_bwd", head, B, A, SEED, ctr_of(ctr), dx, K, col, st, dh, db if with_bias else None)
        torch.cuda.synchronize()
        assert guard_ok(hbuf, dh) and guard_ok(bbuf, db)
        runs.append((dh, db))
    return head_np, runs, ref.head_bwd(head_np, B, A, SEED, ctr, dx_np, K, col, ALPHA)


@BWD[0]
@BWD[1]
@BWD[2]
@checked
def test_head_bwd_rows_mask_and_order(B, A, D):
    """Every row of dhead and every dbias column is written (B = 300: a second pass of the 256 threads); the log_std half is exactly
    0.0 where the raw log_std lies outside [-20, 2] and nonzero at -20 and 2 themselves (SB3's clamp passes the gradient at its
    edges); the column sums add in a fixed order, so two runs give the same bits; dbias = NULL leaves its fenced buffer alone."""
    head_np, runs, (v, d) = _head_bwd(B, A, D)
    assert bool(torch.isfinite(runs[0][0]).all()) and bool(torch.isfinite(runs[0][1]).all())
    assert same_bits(runs[0][0], runs[1][0]) and same_bits(runs[0][1], runs[1][1])
    assert same_bits(runs[0][0], runs[2][0]) and untouched(runs[2][1])
    lsr, g = head_np[:, A:], host(runs[0][0])[:, A:]
    assert bool((g[(lsr < -20) | (lsr > 2)] == 0.0).all()) and bool((g[(lsr == -20) | (lsr == 2)] != 0.0).all())
    assert np.array_equal((lsr >= -20) & (lsr <= 2), v["inside"])
    if B * A >= 255:
        assert int((lsr == -20).sum()) >= 8 and int((lsr == 2).sum()) >= 8


@BWD[0]
@BWD[1]
@BWD[2]
@checked
def test_head_bwd(B, A, D):
    """dhead per element (its bound grants |dg_u / da| A_TOL for the action's error) and dbias within its sum bound."""
    head_np, runs, (v, d) = _head_bwd(B, A, D)
    tag = "head_bwd B%d A%d D%d" % (B, A, D)
    within(tag + " dhead", runs[0][0], v["dhead"], d["dhead"])
    within(tag + " dbias", runs[0][1], v["dbias"], d["dbias"])


# ------------------------------------------------------------------------------------------------------------------ loss heads
@pytest.mark.parametrize("B", [1, 7, 255, 256, 257, 1000])
@checked
def test_critic_loss(B):
    """dq per element, db3 and st[6] within their sum bounds, done = 0 and 1 both present, alpha read from st[4], db3 = NULL."""
    seen = set()
    for flip in (0, 1):
        I = ref.loss_inputs(B, flip)
        seen |= set(I["done"].tolist())
        assert B == 1 or set(I["done"].tolist()) == {0.0, 1.0}
        st0 = np.full(16, 7.0, np.float32)
        st0[4] = ALPHA
        v, d = ref.critic_loss(I["q"], I["qt"], I["logp_next"], I["rew"], I["done"], B, 0.99, ALPHA)
        for with_db3 in (True, False):
            sbuf, st = filled(st0)
            qbuf, dq = guarded(2, B)
            bbuf, db3 = guarded(2)
            call("dm_sac_critic_loss", dev(I["q"]), dev(I["qt"]), dev(I["logp_next"]), dev(I["rew"]), dev(I["done"]), B, 0.99, st, dq,
                 db3 if with_db3 else None)
            torch.cuda.synchronize()
            assert guard_ok(sbuf, st) and guard_ok(qbuf, dq) and guard_ok(bbuf, db3)
            tag = "critic_loss B%d flip%d" % (B, flip)
            within(tag + " dq", dq, v["dq"], d["dq"])
            within(tag + " st[6]", host(st)[6], v["loss"], d["loss"])
            if with_db3:
                within(tag + " db3", db3, v["db3"], d["db3"])
            else:
                assert untouched(db3)
            keep = [k for k in range(16) if k != 6]
            assert same_bits(st[keep], st0[keep])
    assert seen == {0.0, 1.0}


@pytest.mark.parametrize("B", [1, 7, 255, 256, 257, 1000])
@checked
def test_actor_loss(B):
    """dq bit-exact: -fl(1 / B) on the smaller critic, on the FIRST where q0 == q1 (every third row, placed on purpose); st[7]."""
    for flip in (0, 1):
        I = ref.loss_inputs(B, flip)
        tie = I["qpi"][0] == I["qpi"][1]
        assert int(tie.sum()) >= max(B // 4, 1)
        st0 = np.full(16, 7.0, np.float32)
        st0[4] = ALPHA
        sbuf, st = filled(st0)
        qbuf, dq = guarded(2, B)
        call("dm_sac_actor_loss", dev(I["qpi"]), dev(I["logp"]), B, st, dq)
        torch.cuda.synchronize()
        assert guard_ok(sbuf, st) and guard_ok(qbuf, dq)
        v, d = ref.actor_loss(I["qpi"], I["logp"], B, ALPHA)
        assert same_bits(dq, v["dq"])
        got = host(dq)
        assert bool((got[0, tie] == -(np.float32(1) / np.float32(B))).all()) and bool((got[1, tie] == 0).all())
        within("actor_loss B%d flip%d st[7]" % (B, flip), host(st)[7], v["loss"], d["loss"])
        keep = [k for k in range(16) if k != 7]
        assert same_bits(st[keep], st0[keep])


# ------------------------------------------------------------------------------------------------------------ ReLU first layer
@pytest.mark.parametrize("B,O,I,nets,ldx", [(1, 1, 1, 1, 1), (33, 70, 5, 1, 5), (100, 2 * 96, 8, 2, 11), (65, 2 * 300, 121, 2, 121),
                                            (31, 40, 128, 1, 128), (64, 64, 67, 1, 67)])
@checked
def test_linear_relu(B, O, I, nets, ldx):
    """Every element of Y [nets, B, O / nets] within (I + 2) U (sum |x| |w| + |b|) of relu(fp64); the nets have different weights,
    so a column filed under the wrong net is off by O(1); the padding of X behind column I is NaN and must not be read."""
    rng = np.random.default_rng(B + O + I)
    X = np.full((B, ldx), np.nan, np.float32)
    X[:, :I] = rng.standard_normal((B, I))
    W, b = rng.standard_normal((O, I)).astype(np.float32), rng.standard_normal(O).astype(np.float32)
    ybuf, Y = guarded(nets, B, O // nets)
    call("dm_sac_linear_relu", dev(X), ldx, dev(W), dev(b), Y, B, O, I, nets)
    torch.cuda.synchronize()
    assert guard_ok(ybuf, Y)
    v, d = ref.linear_relu(np.nan_to_num(X), ldx, W, b, B, O, I, nets)
    within("linear_relu B%d O%d I%d nets%d ldx%d" % (B, O, I, nets, ldx), Y, v["Y"], d["Y"])
    on = float((host(Y) > 0).mean())
    assert bool((host(Y) >= 0).all()) and (B * O < 8 or 0.2 < on < 0.8)          # both sides of the ReLU are exercised


# -------------------------------------------------------------------------------------------------- ReLU backward + bias sums
@pytest.mark.parametrize("B,O,nets", [(1, 1, 1), (3, 65, 2), (100, 96, 2), (257, 300, 1)])
@checked
def test_relu_bwd_colsum(B, O, nets):
    """dZ bit-exact in place and out of place (0.0 and -0.0 are off, the smallest normal is on), db within the sum bound and the
    same bits on every run, db = NULL allowed.  The single element of (1, 1, 1) takes each kind in turn."""
    for shift in (range(4) if B * O < 4 else (0,)):
        dY, Y, kind = ref.relu_inputs(B, O, nets, shift)
        if B * O >= 4:
            for c0 in range(0, O, 64):
                assert all(int((kind[:, :, c0:c0 + 64] == i).sum()) >= 1 for i in range(3))
        v, d = ref.relu_bwd_colsum(dY, Y, B, O, nets)
        Yd, dbs = dev(Y), []
        for inplace in (False, True):
            for with_db in (True, False):
                zbuf, z = filled(dY) if inplace else guarded(nets, B, O)
                bbuf, db = guarded(nets, O)
                call("dm_sac_relu_bwd_colsum", z if inplace else dev(dY), Yd, z, db if with_db else None, B, O, nets)
                torch.cuda.synchronize()
                assert guard_ok(zbuf, z) and guard_ok(bbuf, db)
                assert same_bits(z, v["dZ"])
                if with_db:
                    within("relu_bwd_colsum B%d O%d nets%d shift%d db" % (B, O, nets, shift), db, v["db"], d["db"])
                    dbs.append(db)
                else:
                    assert untouched(db)
        assert same_bits(dbs[0], dbs[1])


# ------------------------------------------------------------------------------------------------------------------ rollout head
@pytest.mark.parametrize("mode", ["warmup", "stochastic", "deterministic"])
@pytest.mark.parametrize("A", [1, 23])
@pytest.mark.parametrize("N", [1, 255, 257])
@checked
def test_act(N, A, mode):
    """Warm-up (uniform in [lo, hi), rescaled to [-1, 1)), stochastic and deterministic actions for per-column asymmetric boxes,
    head rows of stride 2A and 2A + 3 (the padding is NaN)."""
    lo = (-1.0 - 0.1 * np.arange(A)).astype(np.float32)
    hi = (2.0 + 0.3 * np.arange(A)).astype(np.float32)
    warm, det = int(mode == "warmup"), int(mode == "deterministic")
    for ctr, ld in enumerate((2 * A, 2 * A + 3), 20):
        head_np = np.full((N, ld), np.nan, np.float32)
        head_np[:, :2 * A] = ref.head_rows(N, A)
        abuf, a = guarded(N, A)
        ebuf, e = guarded(N, A)
        call("dm_sac_act", None if warm else dev(head_np), N, A, ld, SEED, ctr_of(ctr), warm, det, dev(lo), dev(hi), a, e)
        torch.cuda.synchronize()
        assert guard_ok(abuf, a) and guard_ok(ebuf, e)
        v, d = ref.act(np.nan_to_num(head_np), N, A, ld, SEED, ctr, warm, det, lo, hi)
        tag = "act N%d A%d ld%d %s" % (N, A, ld, mode)
        within(tag + " act", a, v["act"], d["act"])
        within(tag + " act_env", e, v["act_env"], d["act_env"])
        if warm:
            assert bool((host(e) >= lo[None, :]).all()) and bool((host(e) < hi[None, :]).all())


# ------------------------------------------------------------------------------------------------------------------ replay ring
def _store_buffers(N, D, A, cap, last0, counter):
    G = {k: guarded(*s, fill=0.0) for k, s in dict(r_obs=(cap * N, D), r_act=(cap * N, A), r_rew=(cap * N,), r_done=(cap * N,),
                                                   r_next=(cap * N, D), ep_acc=(2 * N,), ep_hist=(2 * ref.EP_HIST,)).items()}
    G["last_obs"], G["ring"], G["counter"] = filled(last0), ints([0, 0, 0, 0]), ints([counter])
    return G


def _store_step(G, N, D, A, cap, I):
    v = lambda k: G[k][1]
    call("dm_sac_store", N, D, A, cap, v("last_obs"), dev(I["act"]), dev(I["rew"]), dev(I["done"]), dev(I["obs"]), dev(I["terminal_obs"]),
         v("r_obs"), v("r_act"), v("r_rew"), v("r_done"), v("r_next"), v("last_obs"), v("ring"), v("counter"), v("ep_acc"), v("ep_hist"))
    torch.cuda.synchronize()
    assert all(guard_ok(*G[k]) for k in G)


def _hist(t, n):
    h = host(t).astype(np.float64)
    return collections.Counter(zip(h[:n].tolist(), h[ref.EP_HIST:ref.EP_HIST + n].tolist()))


@pytest.mark.parametrize("N,D,A,cap", [(1, 98, 23, 1), (5, 67, 28, 3), (70, 130, 70, 4)])
@checked
def test_store(N, D, A, cap):
    """Seven steps with mixed done patterns: ring rows, last_obs, ep_acc bit-exact, position / fill / ticket / counter after each
    (N = 1: the ticket's N - 1 == 0; cap = 1: the position stays 0; D, A = 130, 70 loop past the 64-thread block).  The history
    is compared as a multiset while it has not wrapped; once the wrap falls inside a step nothing is asserted about which of
    that step's episodes survive: their order is that of the atomics."""
    last0 = np.random.default_rng(N).standard_normal((N, D)).astype(np.float32)
    S, G = ref.new_store_state(N, D, A, cap, last0, counter=5), _store_buffers(N, D, A, cap, last0, 5)
    for step in range(7):
        I = ref.store_inputs(N, D, A, step)
        _store_step(G, N, D, A, cap, I)
        ref.store(S, N, D, A, cap, **I)
        for k in ("r_obs", "r_act", "r_rew", "r_done", "r_next", "last_obs", "ep_acc"):
            assert same_bits(G[k][1], S[k]), (step, k)
        assert G["ring"][1].tolist() == S["ring"].tolist() and int(G["counter"][1]) == S["counter"], step
        n = int(S["ring"][3])
        if n <= ref.EP_HIST:
            assert _hist(G["ep_hist"][1], n) == collections.Counter(e for s in S["episodes"] for e in s)
    assert any(S["episodes"]) and not all(len(s) == N for s in S["episodes"])


@checked
def test_store_history_wraps():
    """125 episodes through the 100-entry history, five per step: 100 % 5 == 0, so the survivors are exactly the last 20 steps'."""
    N, D, A, cap = 5, 3, 2, 2
    last0 = np.zeros((N, D), np.float32)
    S, G = ref.new_store_state(N, D, A, cap, last0), _store_buffers(N, D, A, cap, last0, 0)
    for step in range(25):
        I = ref.store_inputs(N, D, A, step, all_done=True)
        _store_step(G, N, D, A, cap, I)
        ref.store(S, N, D, A, cap, **I)
    assert G["ring"][1].tolist() == [25 % cap, cap, 0, 125] and int(G["counter"][1]) == 25
    want = collections.Counter(e for s in S["episodes"][5:] for e in s)
    assert _hist(G["ep_hist"][1], ref.EP_HIST) == want and sum(want.values()) == 100


# ---------------------------------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize("D", [5, 98])
@pytest.mark.parametrize("B", [1, 100, 257])
@checked
def test_gather(B, D):
    """Rows restated from the hash over the filled part of a partly filled ring (the unfilled rows are NaN), contents bit-exact,
    the action columns of xpi / xt untouched; total = 1 (one env, one stored step) makes every index 0; idx_out = NULL."""
    A, K = 4, D + 4
    for N, cap, fill, with_idx, ctr in ((6, 5, 3, True, 9), (1, 4, 1, False, 10)):
        rng = np.random.default_rng(B + D + N)
        n = lambda *s: rng.standard_normal(s).astype(np.float32)
        R = dict(r_obs=n(cap * N, D), r_act=n(cap * N, A), r_rew=n(cap * N), r_done=(n(cap * N) > 0).astype(np.float32), r_next=n(cap * N, D))
        for k in R:
            R[k][fill * N:] = np.nan
        O = dict(obs2=guarded(2 * B, D), xq=guarded(B, K), xpi=guarded(B, K), xt=guarded(B, K), rew=guarded(B), done=guarded(B),
                 idx=ints([-1] * B))
        ring = torch.tensor([fill % cap, fill, 0, 0], dtype=torch.int32, device=DEV)
        call("dm_sac_gather", B, N, D, A, SEED, ctr_of(ctr), ring, *[dev(R[k]) for k in ("r_obs", "r_act", "r_rew", "r_done", "r_next")],
             *[O[k][1] for k in ("obs2", "xq", "xpi", "xt", "rew", "done")], O["idx"][1] if with_idx else None)
        torch.cuda.synchronize()
        assert all(guard_ok(*O[k]) for k in O)
        v, _ = ref.gather(B, N, D, A, SEED, ctr, fill, **R)
        assert int(v["idx"].max()) < fill * N and (fill * N > 1 or not v["idx"].any())
        assert O["idx"][1].tolist() == (v["idx"].tolist() if with_idx else [-1] * B)
        for k in ("obs2", "xq", "rew", "done"):
            assert same_bits(O[k][1], v[k]), k
        assert same_bits(O["xpi"][1][:, :D], v["xpi_obs"]) and same_bits(O["xt"][1][:, :D], v["xt_obs"])
        assert untouched(O["xpi"][1][:, D:]) and untouched(O["xt"][1][:, D:])
        assert not bool(torch.isnan(O["obs2"][1]).any())


# ---------------------------------------------------------------------------------------------------------------------- Polyak
@pytest.mark.parametrize("tau", [0.005, 1.0])
@pytest.mark.parametrize("n", [1, 1023, 1025, 2 * 1024 * 256 + 3])
@checked
def test_polyak(n, tau):
    """t (1 - tau) + tau p within three roundings, through the grid-stride second pass (n > 1024 x 256 threads); the counter goes
    up by one; counter = NULL gives the same bits."""
    rng = np.random.default_rng(n)
    p, t = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    v, d = ref.polyak(p, t, tau)
    outs = []
    for with_ctr in (True, False):
        tbuf, tt = filled(t)
        cbuf, c = ints([41])
        call("dm_sac_polyak", dev(p), tt, n, tau, c if with_ctr else None)
        torch.cuda.synchronize()
        assert guard_ok(tbuf, tt) and guard_ok(cbuf, c) and int(c) == (42 if with_ctr else 41)
        within("polyak n%d tau%g" % (n, tau), tt, v["t"], d["t"])
        outs.append(tt)
    assert same_bits(outs[0], outs[1])
    if tau == 1.0:
        assert same_bits(outs[0], p)


# ------------------------------------------------------------------------------------------------------------ host-side refusals
@checked
def test_bad_arguments_are_refused_before_any_launch():
    """Argument checks of the entry points: -22 from the host, nothing launched, every output keeps its fill."""
    A, R, K = 2, 4, 7
    z = lambda *s: torch.zeros(*s, device=DEV)
    outs = [guarded(64)[1] for _ in range(4)]
    o0, o1, o2, o3 = outs
    st, c = z(16), ctr_of(0)
    bad = [("dm_sac_head_fwd", (z(R, 2 * A), 2, 3, A, SEED, c, o0, o1, A, o2, o3, 0, -2.0, 3e-4)),             # Rpi > R
           ("dm_sac_head_fwd", (z(R, 2 * A), R, 2, A, SEED, c, o0, o1, A - 1, o2, o3, 0, -2.0, 3e-4)),         # lda < A
           ("dm_sac_head_fwd", (z(R, 2 * A), R, 2, A, SEED, c, o0, None, A, o2, o3, 0, -2.0, 3e-4)),           # R > Rpi, no a_next
           ("dm_sac_head_bwd", (z(R, 2 * A), R, A, SEED, c, z(2 * R, K), K, K - A + 1, st, o0, o1)),           # col + A > K
           ("dm_sac_linear_relu", (z(R, 8), 8, z(3, 8), z(3), o0, R, 3, 8, 2)),                                # O % nets != 0
           ("dm_sac_linear_relu", (z(R, 8), 7, z(4, 8), z(4), o0, R, 4, 8, 2)),                                # ldx < I
           ("dm_sac_linear_relu", (z(2, 129), 129, z(4, 129), z(4), o0, 2, 4, 129, 1)),                        # I = 129
           ("dm_sac_act", (z(R, 2 * A), R, A, 2 * A - 1, SEED, c, 0, 0, z(A), z(A) + 1, o0, o1))]              # ld < 2A
    for name, args in bad:
        with pytest.raises(RuntimeError, match=r"^%s failed \(-22\)$" % name):
            call(name, *args)
    torch.cuda.synchronize()
    assert all(untouched(o) for o in outs)
