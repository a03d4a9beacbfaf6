"""csrc/dm_vecnorm.hip through its C ABI on NaN-fenced buffers, against the numpy fp64 restatement (tests/vecnorm_ref.py).

Bounds (none of them taken from the kernels' output):
  running mean / var / count   1e-10 relative.  Per-chunk two-pass moments in fp64 merged by Chan's formula sit near 1e-13 on the
                               column 50 + 1e-3 g; E[x^2] - mean^2 in fp64 is off by 5e-7 .. 1.4e-5 there, an fp32 accumulator by more.
  obs / rew / terminal_obs     2^-23 |ref| + 1e-9: one rounding to fp32 plus fp64 reordering noise carried through the division by
                               the column's deviation (1e-3 at the smallest).
  returns                      1e-12 relative: one multiply-add per step, contracted or not.
Measured worst over all cases (pytest -s prints them per case): see DESIGN §24."""
import ctypes as C

import numpy as np
import pytest
import torch

from deepmimic_mujoco_amd import _lib
from kernel_helpers import DEV, GUARD, checked, guard_ok, guarded, lib, note, ptr, stream, within
from vecnorm_ref import VecNormalizeRef

pytestmark = pytest.mark.gpu
STEPS = 40


def guarded64(n, fill=0.0):
    """fp64 (buffer, view of n) with GUARD NaNs behind the view."""
    buf = torch.full((n + GUARD,), float("nan"), dtype=torch.float64, device=DEV)
    buf[:n] = fill
    return buf, buf[:n]


def guard_ok64(buf, view):
    return bool(torch.isnan(buf[view.numel():]).all())


class Norm:
    """A DmVecNorm over fenced device state, at RunningMeanStd's start values."""

    def __init__(self, N, D, **kw):
        self.N, self.D = N, D
        self.sbuf, self.state = guarded64(2 * D + 4)
        self.rbuf, self.returns = guarded64(N)
        nbytes = int(lib().dm_vecnorm_scratch_bytes(N, D))
        assert nbytes > 0 and nbytes % 8 == 0
        self.wbuf, self.scratch = guarded64(nbytes // 8, fill=float("nan"))
        self.init()
        d = dict(N=N, D=D, device=0, training=1, norm_obs=1, norm_reward=1, gamma=0.99, epsilon=1e-8, clip_obs=10.0, clip_reward=10.0)
        d.update(kw)
        s = self.state
        self.desc = _lib.DmVecNorm(obs_mean=s[:D].data_ptr(), obs_var=s[D:2 * D].data_ptr(), obs_count=s[2 * D:].data_ptr(),
                                   ret_stats=s[2 * D + 1:].data_ptr(), returns=self.returns.data_ptr(), scratch=self.scratch.data_ptr(),
                                   scratch_bytes=nbytes, **d)

    def init(self):
        D = self.D
        self.state.zero_()
        self.state[D:2 * D] = 1.0
        self.state[2 * D] = 1e-4
        self.state[2 * D + 2] = 1.0
        self.state[2 * D + 3] = 1e-4
        self.returns.zero_()

    def call(self, name, *args):
        rc = getattr(lib(), name)(C.byref(self.desc), *[ptr(a) if isinstance(a, torch.Tensor) else a for a in args], stream())
        assert rc == 0, (name, rc, lib().dm_vecnorm_last_error())

    def fences_ok(self):
        return guard_ok64(self.sbuf, self.state) and guard_ok64(self.rbuf, self.returns) and guard_ok64(self.wbuf, self.scratch)

    def stats(self):
        s, D = self.state.cpu().numpy(), self.D
        return dict(mean=s[:D], var=s[D:2 * D], count=s[2 * D:2 * D + 1], ret=s[2 * D + 1:2 * D + 4])


def ref_stats(ref):
    return dict(mean=ref.obs_rms.mean, var=ref.obs_rms.var, count=np.array([ref.obs_rms.count]),
                ret=np.array([ref.ret_rms.mean, ref.ret_rms.var, ref.ret_rms.count]))


def make_inputs(N, D, steps, seed):
    """[steps, N, D] observations and terminal observations, [steps, N] rewards and done flags.  Column 0: 50 + 1e-3 g (large mean,
    small spread); column 1: constant; column 2: unit normal with +-1000 in env 0 every fourth step; the rest normals of mixed
    scale.  Rewards in [0, 1) with 5000 in env 0 every seventh step.  One outlier among n samples normalises to about sqrt(n), so
    from N = 63 on (n >= 4 N at the outlier) both reach their clip of 10; at N = 1 no value can ((n - 1) / sqrt(n) < 10 for the
    41 samples there are).  Done: none for the first quarter of the steps, then all, then two mixed patterns."""
    rng = np.random.default_rng(seed)

    def table():
        x = rng.standard_normal((steps, N, D)) * (1.0 + (np.arange(D) % 5))
        x[:, :, 0] = 50.0 + 1e-3 * rng.standard_normal((steps, N))
        if D > 1:
            x[:, :, 1] = -3.5
        if D > 2:
            x[:, :, 2] = rng.standard_normal((steps, N))
            x[1::4, 0, 2] = 1000.0 * np.where(np.arange(len(x[1::4])) % 2 == 0, 1.0, -1.0)
        return x.astype(np.float32)
    obs, tobs = table(), table()
    rew = rng.random((steps, N))
    rew[3::7, 0] = 5000.0
    rew = rew.astype(np.float32)
    done = np.zeros((steps, N), np.uint8)
    for t in range(steps):
        phase = (4 * t // steps) % 4
        if phase == 1:
            done[t] = 1
        elif phase >= 2:
            done[t] = rng.random(N) < (0.3 if phase == 2 else 0.05)
    return obs, tobs, rew, done


def rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(got == ref, 0.0, np.abs(got - ref) / np.abs(ref))
    return float(np.max(r))


def run_steps(vn, inputs, inplace):
    """One dm_vecnorm_step per step of ``inputs`` into fresh fenced outputs (``inplace``: the fenced copies of the inputs themselves)
    -> per step (obs, rew, terminal_obs, returns, state) as numpy."""
    obs, tobs, rew, done = inputs
    N, D = vn.N, vn.D
    got = []
    for t in range(obs.shape[0]):
        o, tb, r = torch.tensor(obs[t], device=DEV), torch.tensor(tobs[t], device=DEV), torch.tensor(rew[t], device=DEV)
        d = torch.tensor(done[t], device=DEV)
        if inplace:
            bufs = [guarded(N, D), guarded(N), guarded(N, D)]
            for (b, v), src in zip(bufs, (o, r, tb)):
                v.copy_(src)
            vn.call("dm_vecnorm_step", bufs[0][1], bufs[1][1], d, bufs[2][1], bufs[0][1], bufs[1][1], bufs[2][1])
        else:
            bufs = [guarded(N, D), guarded(N), guarded(N, D)]
            vn.call("dm_vecnorm_step", o, r, d, tb, bufs[0][1], bufs[1][1], bufs[2][1])
        torch.cuda.synchronize()
        assert all(guard_ok(b, v) for b, v in bufs) and vn.fences_ok(), t
        got.append(tuple(v.cpu().numpy() for _, v in bufs) + (vn.returns.cpu().numpy().copy(), vn.state.cpu().numpy().copy()))
    return got


SHAPES = [(N, D) for N in (1, 63, 64, 65, 257) for D in (1, 67, 98, 130)] + [(4096, 98)]


@pytest.mark.parametrize("N,D", SHAPES, ids=["%dx%d" % s for s in SHAPES])
@checked
def test_forty_steps_against_the_restatement(N, D):
    case = SHAPES.index((N, D))
    gamma, inplace = (0.99, 0.5)[(case + case // 4) % 2], bool((case // 2 + case // 4) % 2)        # every N and every D meets both of each
    inputs = make_inputs(N, D, STEPS, seed=case)
    obs, tobs, rew, done = inputs
    vn = Norm(N, D, gamma=gamma)
    ref = VecNormalizeRef(N, D, gamma=gamma)
    # reset: the table's last step stands for the reset observations
    rb, rv = guarded(N, D)
    vn.returns.fill_(7.0)
    vn.call("dm_vecnorm_reset", torch.tensor(obs[-1], device=DEV), rv)
    torch.cuda.synchronize()
    want = ref.reset(obs[-1])
    assert guard_ok(rb, rv) and vn.fences_ok() and float(vn.returns.abs().max()) == 0.0
    within("reset obs", rv, want, 2.0 ** -23 * np.abs(want) + 1e-9)
    got = run_steps(vn, inputs, inplace)
    worst = dict(mean=0.0, var=0.0, count=0.0, ret=0.0, returns=0.0)
    clipped_obs = clipped_rew = 0
    for t in range(STEPS):
        o, r, tb = ref.step(obs[t], rew[t], done[t], tobs[t])
        g_o, g_r, g_tb, g_ret, g_state = got[t]
        tag = "step %d " % t
        within(tag + "obs", g_o, o, 2.0 ** -23 * np.abs(o) + 1e-9)
        within(tag + "rew", g_r, r, 2.0 ** -23 * np.abs(r) + 1e-9)
        within(tag + "terminal_obs", g_tb, tb, 2.0 ** -23 * np.abs(tb) + 1e-9)
        live = done[t] == 0
        assert np.array_equal(g_tb[live], tobs[t][live])                          # copied through
        assert np.all(g_ret[~live] == 0.0)
        clipped_obs += int((np.abs(o) == 10.0).sum())
        clipped_rew += int((np.abs(r) == 10.0).sum())
        st = dict(mean=g_state[:D], var=g_state[D:2 * D], count=g_state[2 * D:2 * D + 1], ret=g_state[2 * D + 1:2 * D + 4])
        for k, v in ref_stats(ref).items():
            worst[k] = max(worst[k], rel(st[k], v))
        worst["returns"] = max(worst["returns"], rel(g_ret, ref.returns))
    if N > 1:                                            # the inputs do reach both clips (a property of the reference alone)
        assert clipped_rew > 0 and (clipped_obs > 0 or D <= 2)
    for k in ("mean", "var", "count", "ret"):
        assert note("%dx%d running %s (relative)" % (N, D, k), worst[k], 1e-10, width=40) <= 1e-10
    assert note("%dx%d returns (relative)" % (N, D), worst["returns"], 1e-12, width=40) <= 1e-12


@pytest.mark.parametrize("kw", [dict(norm_obs=0), dict(norm_reward=0), dict(norm_obs=0, norm_reward=0), dict(training=0)], ids=str)
@checked
def test_flag_combinations(kw):
    N, D, steps = 65, 67, 6
    inputs = make_inputs(N, D, steps, seed=77)
    obs, tobs, rew, done = inputs
    vn = Norm(N, D, **kw)
    ref = VecNormalizeRef(N, D, **{k: bool(v) for k, v in kw.items()})
    if "training" in kw:                                 # frozen statistics that are not the start values
        vn.desc.training = 1
        ref.training = True
        run_steps(vn, tuple(x[:3] for x in make_inputs(N, D, 3, seed=78)), False)
        for t, x in enumerate(zip(*make_inputs(N, D, 3, seed=78))):
            ref.step(x[0], x[2], x[3], x[1])
        vn.desc.training = 0
        ref.training = False
    before = vn.state.clone()
    for inplace in (False, True):
        got = run_steps(vn, inputs, inplace)
        for t in range(steps):
            o, r, tb = ref.step(obs[t], rew[t], done[t], tobs[t])
            within("obs", got[t][0], o, 2.0 ** -23 * np.abs(o) + 1e-9)
            within("rew", got[t][1], r, 2.0 ** -23 * np.abs(r) + 1e-9)
            within("terminal_obs", got[t][2], tb, 2.0 ** -23 * np.abs(tb) + 1e-9)
            if not kw.get("norm_obs", 1):
                assert np.array_equal(got[t][0], obs[t]) and np.array_equal(got[t][2], tobs[t])
            if not kw.get("norm_reward", 1):
                assert np.array_equal(got[t][1], rew[t])
            assert rel(got[t][3], ref.returns) <= 1e-12
    st = vn.stats()
    for k, v in ref_stats(ref).items():
        assert rel(st[k], v) <= 1e-10, k
    if "training" in kw:
        assert torch.equal(vn.state, before)             # bit for bit
    if not kw.get("norm_obs", 1):
        assert torch.equal(vn.state[:2 * D + 1], before[:2 * D + 1]) and not torch.equal(vn.state[2 * D + 1:], before[2 * D + 1:])


def test_two_runs_are_bit_identical_and_a_captured_graph_replays_eager():
    N, D, steps = 257, 98, 8
    obs, tobs, rew, done = make_inputs(N, D, steps, seed=5)
    dev = [torch.tensor(x, device=DEV) for x in (obs, tobs, rew, done)]
    vn = Norm(N, D)
    outs = [torch.zeros(steps, N, D, device=DEV), torch.zeros(steps, N, device=DEV), torch.zeros(steps, N, D, device=DEV)]

    def eight():
        for t in range(steps):
            vn.call("dm_vecnorm_step", dev[0][t], dev[2][t], dev[3][t], dev[1][t], outs[0][t], outs[1][t], outs[2][t])

    def snapshot():
        torch.cuda.synchronize()
        return [x.clone() for x in outs] + [vn.state.clone(), vn.returns.clone()]

    runs = []
    for _ in range(2):
        vn.init()
        for o in outs:
            o.zero_()
        eight()
        runs.append(snapshot())
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    vn.init()
    for o in outs:
        o.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eight()
    graph.replay()
    replayed = snapshot()
    assert all(torch.equal(a, b) for a, b in zip(runs[0], replayed))
    assert vn.fences_ok()


@checked
def test_apply_at_other_row_counts_leaves_the_statistics_alone():
    N, D = 64, 98
    inputs = make_inputs(N, D, 5, seed=9)
    vn = Norm(N, D)
    ref = VecNormalizeRef(N, D)
    run_steps(vn, inputs, False)
    for t in range(5):
        ref.step(inputs[0][t], inputs[2][t], inputs[3][t], inputs[1][t])
    before, ret_before = vn.state.clone(), vn.returns.clone()
    rng = np.random.default_rng(1)
    for n in (1, 17, N + 5, 1000):
        x = (rng.standard_normal((n, D)) * 3.0).astype(np.float32)
        x[:, 0] += 50.0
        r = (rng.random(n) * 30.0).astype(np.float32)
        (ob, ov), (rb, rv) = guarded(n, D), guarded(n)
        vn.call("dm_vecnorm_apply", n, torch.tensor(x, device=DEV), ov, torch.tensor(r, device=DEV), rv)
        xi = torch.tensor(x, device=DEV)
        vn.call("dm_vecnorm_apply", n, xi, xi, None, None)                       # in place, observations alone
        torch.cuda.synchronize()
        assert guard_ok(ob, ov) and guard_ok(rb, rv) and vn.fences_ok()
        want_o, want_r = ref.normalize_obs(x), ref.normalize_reward(r)
        within("apply obs n=%d" % n, ov, want_o, 2.0 ** -23 * np.abs(want_o) + 1e-9)
        within("apply rew n=%d" % n, rv, want_r, 2.0 ** -23 * np.abs(want_r) + 1e-9)
        assert torch.equal(xi, ov)
        assert torch.equal(vn.state, before) and torch.equal(vn.returns, ret_before)
