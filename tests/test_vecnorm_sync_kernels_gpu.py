"""The synchronised entry points of csrc/dm_vecnorm.hip (dm_vecnorm_step_sync, dm_vecnorm_reset_sync, dm_vecnorm_sync_pack,
dm_vecnorm_sync_merge) through the C ABI on NaN-fenced buffers, one process standing for one rank of W: the other ranks' rows of the
all-reduce buffer are written by the host from the numpy restatement (tests/vecnorm_sync_ref.py).

Bounds, those of tests/test_vecnorm_kernels_gpu.py: running / base / acc 1e-10 relative, returns 1e-12 relative; the normalised
outputs bit-equal to dm_vecnorm_apply given the same running statistics; where the scheme promises exactness, torch.equal."""
import ctypes as C

import numpy as np
import pytest
import torch

from deepmimic_mujoco_amd import _lib
from deepmimic_mujoco_amd.vec_env import Box
from deepmimic_mujoco_amd.vec_normalize import HipVecNormalize
from kernel_helpers import DEV, checked, guard_ok, guarded, lib, note, ptr, stream
from test_vecnorm_kernels_gpu import Norm, guard_ok64, guarded64, make_inputs, rel
from vecnorm_sync_ref import SyncRankRef, sync as ref_sync

pytestmark = pytest.mark.gpu
STEPS, EVERY = 12, 4


class SyncNorm(Norm):
    """``Norm`` plus fenced base / acc / gather and the DmVecNormSync over them: rank ``rank`` of ``world``."""

    def __init__(self, N, D, world=1, rank=0, **kw):
        S = 2 * D + 4
        self.S, self.world, self.rank = S, world, rank
        self.bbuf, self.base = guarded64(S)
        self.abuf, self.acc = guarded64(S)
        self.gbuf, self.gather = guarded64(world * S, fill=float("nan"))
        super().__init__(N, D, **kw)
        self.sync = _lib.DmVecNormSync(world=world, rank=rank, base=self.base.data_ptr(), acc=self.acc.data_ptr(), gather=self.gather.data_ptr())

    def init(self):
        super().init()
        self.base.copy_(self.state)
        self.acc.zero_()

    def call_sync(self, name, *args):
        rc = getattr(lib(), name)(C.byref(self.desc), *[ptr(a) if isinstance(a, torch.Tensor) else a for a in args], C.byref(self.sync), stream())
        assert rc == 0, (name, rc, lib().dm_vecnorm_last_error())

    def fences_ok(self):
        return (super().fences_ok() and guard_ok64(self.bbuf, self.base) and guard_ok64(self.abuf, self.acc)
                and guard_ok64(self.gbuf, self.gather))

    def rows(self):
        return self.gather.view(self.world, self.S)

    def sync_with(self, others):
        """pack, the host standing in for the all-reduce (``others``: rank -> row), merge.  The pack is checked on the way."""
        self.call_sync("dm_vecnorm_sync_pack")
        torch.cuda.synchronize()
        rows = self.rows()
        assert torch.equal(rows[self.rank], self.acc)
        assert all(not rows[r].any() for r in range(self.world) if r != self.rank)
        for r, row in others.items():
            rows[r].copy_(torch.tensor(row, dtype=torch.float64))
        self.call_sync("dm_vecnorm_sync_merge")
        torch.cuda.synchronize()


def step_sync(vn, t, dev, outs=None):
    """One dm_vecnorm_step_sync of step t of the device inputs (obs, tobs, rew, done) into fresh fenced outputs (or ``outs``)."""
    N, D = vn.N, vn.D
    bufs = outs or [guarded(N, D), guarded(N), guarded(N, D)]
    vn.call_sync("dm_vecnorm_step_sync", dev[0][t], dev[2][t], dev[3][t], dev[1][t], bufs[0][1], bufs[1][1], bufs[2][1])
    return bufs


SHAPES = [(1, 1), (3, 5), (257, 67), (64, 98)]
CASES = [(N, D, W) for N, D in SHAPES for W in (1, 2, 5)]


@pytest.mark.parametrize("N,D,W", CASES, ids=["%dx%d-W%d" % c for c in CASES])
@checked
def test_twelve_steps_and_three_syncs_against_the_restatement(N, D, W):
    case = CASES.index((N, D, W))
    me = W // 2                                          # rows before and behind this rank's own
    gamma = (0.99, 0.5)[case % 2]
    inputs = [make_inputs(N, D, STEPS, seed=1000 + 10 * case + r) for r in range(W)]
    refs = [SyncRankRef(N, D, gamma=gamma) for _ in range(W)]
    vn = SyncNorm(N, D, world=W, rank=me, gamma=gamma)
    obs, tobs, rew, done = inputs[me]
    dev = [torch.tensor(x, device=DEV) for x in inputs[me]]
    # reset: the table's last step stands for the reset observations
    rb, rv = guarded(N, D)
    vn.returns.fill_(7.0)
    vn.call_sync("dm_vecnorm_reset_sync", dev[0][-1], rv)
    ab, av = guarded(N, D)
    vn.call("dm_vecnorm_apply", N, dev[0][-1], av, None, None)
    torch.cuda.synchronize()
    for r, ref in enumerate(refs):
        ref.reset(inputs[r][0][-1])
    assert guard_ok(rb, rv) and vn.fences_ok() and float(vn.returns.abs().max()) == 0.0 and torch.equal(rv, av)
    worst = dict(running=0.0, base=0.0, acc=0.0, returns=0.0)

    def compare():
        ref = refs[me]
        worst["running"] = max(worst["running"], rel(vn.state.cpu().numpy(), ref.running_row()))
        worst["base"] = max(worst["base"], rel(vn.base.cpu().numpy(), ref.base_row()))
        worst["acc"] = max(worst["acc"], rel(vn.acc.cpu().numpy(), ref.acc_row()))
        worst["returns"] = max(worst["returns"], rel(vn.returns.cpu().numpy(), ref.returns))
    compare()
    for t in range(STEPS):
        bufs = step_sync(vn, t, dev)
        # the frozen transform with the statistics this step left: bit for bit what the step wrote
        (ob, ov), (qb, qv), (tb, tv) = guarded(N, D), guarded(N), guarded(N, D)
        vn.call("dm_vecnorm_apply", N, dev[0][t], ov, dev[2][t], qv)
        vn.call("dm_vecnorm_apply", N, dev[1][t], tv, None, None)
        torch.cuda.synchronize()
        assert all(guard_ok(b, v) for b, v in bufs) and vn.fences_ok(), t
        live = torch.tensor(done[t] == 0, device=DEV)
        assert torch.equal(bufs[0][1], ov) and torch.equal(bufs[1][1], qv), t
        assert torch.equal(bufs[2][1][~live], tv[~live]) and torch.equal(bufs[2][1][live], dev[1][t][live]), t
        assert float(vn.returns[~live].abs().sum()) == 0.0
        for r, ref in enumerate(refs):
            ref.step(inputs[r][0][t], inputs[r][2][t], inputs[r][3][t])
        compare()
        if (t + 1) % EVERY == 0:
            vn.sync_with({r: refs[r].acc_row() for r in range(W) if r != me})
            ref_sync(refs)
            assert vn.fences_ok()
            assert torch.equal(vn.state, vn.base) and not vn.acc.any()
            compare()
    for k in ("running", "base", "acc"):
        assert note("%dx%d W=%d %s (relative)" % (N, D, W, k), worst[k], 1e-10, width=40) <= 1e-10
    assert note("%dx%d W=%d returns (relative)" % (N, D, W), worst["returns"], 1e-12, width=40) <= 1e-12
    assert float(vn.state[2 * D]) == pytest.approx(1e-4 + W * N * (STEPS + 1), rel=1e-14)


def run_some(vn, inputs, steps):
    dev = [torch.tensor(x, device=DEV) for x in inputs]
    for t in range(steps):
        step_sync(vn, t, dev)
    torch.cuda.synchronize()


def test_an_empty_acc_leaves_base_alone_and_a_world_of_one_keeps_its_running_statistics():
    N, D = 65, 67
    inputs = make_inputs(N, D, 6, seed=21)
    vn = SyncNorm(N, D, world=1, rank=0)
    run_some(vn, inputs, 5)
    running = vn.state.clone()                           # merge(base, acc) as the last step formed it
    assert not torch.equal(running, vn.base) and float(vn.acc[2 * D]) == 5 * N
    vn.sync_with({})
    assert torch.equal(vn.state, running) and torch.equal(vn.base, running) and not vn.acc.any()
    vn.sync_with({})                                     # nothing seen since: the row is empty
    assert torch.equal(vn.state, running) and torch.equal(vn.base, running) and not vn.acc.any()
    # W = 3 with every row empty, and with only the others' rows empty
    wide = SyncNorm(N, D, world=3, rank=1)
    run_some(wide, inputs, 5)
    assert torch.equal(wide.state, running)
    empty = np.zeros(2 * D + 4)
    wide.sync_with({0: empty, 2: empty})
    assert torch.equal(wide.state, running) and torch.equal(wide.base, running)
    wide.sync_with({0: empty, 2: empty})
    assert torch.equal(wide.base, running) and vn.fences_ok() and wide.fences_ok()


def test_the_merge_depends_on_the_row_order_alone_and_two_runs_are_bit_identical():
    N, D, W = 64, 98, 3
    sets = [make_inputs(N, D, 4, seed=31 + r) for r in range(W)]

    def acc_of(k):
        vn = SyncNorm(N, D, world=1, rank=0)
        run_some(vn, sets[k], 4)
        return vn.acc.cpu().numpy().copy()
    rows = [acc_of(k) for k in range(W)]

    def merged(rank, order):
        """The rank that saw ``sets[order[rank]]``, the other rows placed by the host in ``order``."""
        vn = SyncNorm(N, D, world=W, rank=rank)
        run_some(vn, sets[order[rank]], 4)
        vn.sync_with({r: rows[order[r]] for r in range(W) if r != rank})
        assert vn.fences_ok()
        return vn.state.clone()
    as0, as1, as2 = merged(0, (0, 1, 2)), merged(1, (0, 1, 2)), merged(2, (0, 1, 2))
    assert torch.equal(as0, as1) and torch.equal(as0, as2)           # what every rank of a real group holds
    assert torch.equal(as0, merged(0, (0, 1, 2)))                    # and again
    swapped = merged(0, (1, 0, 2))                                   # the rows permuted between the ranks: another order of the same merges
    assert torch.equal(swapped, merged(1, (1, 0, 2)))
    assert float(swapped[2 * D]) == float(as0[2 * D]) and float(swapped[2 * D + 3]) == float(as0[2 * D + 3])
    assert note("rows permuted (relative)", rel(swapped.cpu().numpy(), as0.cpu().numpy()), 1e-10) <= 1e-10


def test_a_captured_graph_of_step_sync_and_the_sync_launches_replays_eager():
    N, D, steps = 257, 98, 8
    obs, tobs, rew, done = make_inputs(N, D, steps, seed=5)
    dev = [torch.tensor(x, device=DEV) for x in (obs, tobs, rew, done)]
    vn = SyncNorm(N, D, world=1, rank=0)
    outs = [torch.zeros(steps, N, D, device=DEV), torch.zeros(steps, N, device=DEV), torch.zeros(steps, N, D, device=DEV)]
    inplace = dev[0].clone()

    def eight():
        for t in range(steps):
            vn.call_sync("dm_vecnorm_step_sync", dev[0][t], dev[2][t], dev[3][t], dev[1][t], outs[0][t], outs[1][t], outs[2][t])
            if t == 3:                                   # both launches around the collective, between two steps
                vn.call_sync("dm_vecnorm_sync_pack")
                vn.call_sync("dm_vecnorm_sync_merge")
        # the policy_forward route's form: observations normalised in place, no terminal observations
        vn.call_sync("dm_vecnorm_step_sync", inplace[0], dev[2][0], dev[3][0], None, inplace[0], outs[1][0], None)

    def snapshot():
        torch.cuda.synchronize()
        return [x.clone() for x in outs] + [inplace.clone(), vn.state.clone(), vn.base.clone(), vn.acc.clone(), vn.returns.clone()]

    def fresh():
        vn.init()
        for o in outs:
            o.zero_()
        inplace.copy_(dev[0])
        torch.cuda.synchronize()
    runs = []
    for _ in range(2):
        fresh()
        eight()
        runs.append(snapshot())
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    base, acc = runs[0][5], runs[0][6]
    assert float(base[2 * D]) == 1e-4 + 4 * N and float(acc[2 * D]) == 5 * N          # base after the sync, acc since
    fresh()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eight()
    graph.replay()
    replayed = snapshot()
    assert all(torch.equal(a, b) for a, b in zip(runs[0], replayed))
    assert vn.fences_ok()


def test_refused_calls_launch_nothing():
    N, D = 8, 5
    vn = SyncNorm(N, D, world=2, rank=1)
    run_some(vn, make_inputs(N, D, 2, seed=3), 2)
    before = [x.clone() for x in (vn.sbuf, vn.bbuf, vn.abuf, vn.gbuf, vn.rbuf)]
    o, r, d = torch.zeros(N, D, device=DEV), torch.zeros(N, device=DEV), torch.zeros(N, dtype=torch.uint8, device=DEV)
    out = guarded(N, D)
    for bad in (dict(world=0), dict(rank=2), dict(rank=-1), dict(base=None), dict(acc=None), dict(gather=None)):
        y = _lib.DmVecNormSync(**dict(dict(world=2, rank=1, base=vn.base.data_ptr(), acc=vn.acc.data_ptr(), gather=vn.gather.data_ptr()), **bad))
        L = lib()
        assert L.dm_vecnorm_step_sync(C.byref(vn.desc), ptr(o), ptr(r), ptr(d), None, ptr(out[1]), ptr(r), None, C.byref(y), stream()) == -22
        assert L.dm_vecnorm_reset_sync(C.byref(vn.desc), ptr(o), ptr(out[1]), C.byref(y), stream()) == -22
        assert L.dm_vecnorm_sync_pack(C.byref(vn.desc), C.byref(y), stream()) == -22
        assert L.dm_vecnorm_sync_merge(C.byref(vn.desc), C.byref(y), stream()) == -22
    assert lib().dm_vecnorm_sync_merge(C.byref(vn.desc), None, stream()) == -22
    torch.cuda.synchronize()
    after = (vn.sbuf, vn.bbuf, vn.abuf, vn.gbuf, vn.rbuf)
    assert all(torch.equal(a.nan_to_num(nan=-1.0), b.nan_to_num(nan=-1.0)) for a, b in zip(after, before))
    assert bool(torch.isnan(out[0]).all())


# ------------------------------------------------------------------------------------------ the wrapper on the device
class DeviceScript:
    """A batch env on the device that replays ``make_inputs``; the actions are ignored."""

    def __init__(self, N, D, steps, seed):
        self.num_envs, self.device = N, DEV
        self.observation_space, self.action_space = Box(-np.inf, np.inf, (D,), np.float32), Box(-1.0, 1.0, (2,), np.float32)
        self.obs, self.tobs, self.rew, self.done = (torch.tensor(x, device=DEV) for x in make_inputs(N, D, steps + 1, seed))
        self.t = 0

    def reset_tensor(self):
        return self.obs[-1].clone()

    def step_tensor(self, actions):
        t = self.t
        self.t += 1
        return dict(obs=self.obs[t].clone(), rew=self.rew[t].clone(), done=self.done[t].clone(), terminal_obs=self.tobs[t].clone())

    def close(self):
        pass


def spy(vn):
    names, inner = [], vn._call

    def call(entry, *args):
        names.append(entry)
        return inner(entry, *args)
    vn._call = call
    return names


def test_without_a_sync_group_the_wrapper_makes_the_calls_it_made_and_computes_the_same_bits():
    N, D, steps = 65, 67, 10
    vn = HipVecNormalize(DeviceScript(N, D, steps, seed=41))
    assert not vn.synced and vn._base is None and vn._acc is None and vn._sync is None
    names = spy(vn)
    act = torch.zeros(N, 2, device=DEV)
    first = vn.reset_tensor().clone()
    got = []
    for t in range(steps):
        out = vn.step_tensor(act)
        got.append((out["obs"].clone(), out["rew"].clone(), out["terminal_obs"].clone()))
    again = vn.normalize_obs(vn.out["obs_raw"])
    env = vn.venv
    inplace, rew_out = env.obs[0].clone(), torch.zeros(N, device=DEV)
    vn.training = False
    vn.step_inplace(inplace, env.rew[0], env.done[0], rew_out)
    torch.cuda.synchronize()
    assert names == ["dm_vecnorm_reset"] + ["dm_vecnorm_step"] * steps + ["dm_vecnorm_apply", "dm_vecnorm_step"]
    assert torch.equal(again, got[-1][0])
    # the same object class driven through the entry points directly, as before this option existed
    twin = HipVecNormalize(DeviceScript(N, D, steps, seed=41))
    L, s = lib(), stream()
    o = torch.zeros(N, D, device=DEV)
    assert L.dm_vecnorm_reset(C.byref(twin._desc), ptr(env.obs[-1]), ptr(o), s) == 0
    assert torch.equal(o, first)
    for t in range(steps):
        o, r, tb = torch.zeros(N, D, device=DEV), torch.zeros(N, device=DEV), torch.zeros(N, D, device=DEV)
        assert L.dm_vecnorm_step(C.byref(twin._desc), ptr(env.obs[t]), ptr(env.rew[t]), ptr(env.done[t]), ptr(env.tobs[t]), ptr(o), ptr(r), ptr(tb), s) == 0
        assert torch.equal(o, got[t][0]) and torch.equal(r, got[t][1]) and torch.equal(tb, got[t][2]), t
    torch.cuda.synchronize()
    assert torch.equal(twin._state, vn._state) and torch.equal(twin.returns, vn.returns)


def test_with_a_sync_group_the_wrapper_takes_the_sync_entry_points():
    """One process without a process group: a world of one.  The statistics are those of the plain wrapper regrouped (1e-10)."""
    N, D, steps = 65, 67, 6
    vn, plain = HipVecNormalize(DeviceScript(N, D, steps, seed=43), sync_group="world"), HipVecNormalize(DeviceScript(N, D, steps, seed=43))
    names = spy(vn)
    act = torch.zeros(N, 2, device=DEV)
    vn.reset_tensor(), plain.reset_tensor()
    for t in range(steps):
        a, b = vn.step_tensor(act), plain.step_tensor(act)
        if t == 2:
            vn.sync()
            assert torch.equal(vn._state, vn._base) and not vn._acc.any()
    env = vn.venv
    inplace, rew_out = env.obs[0].clone(), torch.zeros(N, device=DEV)
    vn.step_inplace(inplace, env.rew[0], env.done[0], rew_out)
    torch.cuda.synchronize()
    assert names == (["dm_vecnorm_reset_sync"] + ["dm_vecnorm_step_sync"] * 3 + ["dm_vecnorm_sync_pack", "dm_vecnorm_sync_merge"]
                     + ["dm_vecnorm_step_sync"] * 4)
    assert vn.sync_calls == 1 and float(vn._acc[2 * D]) == 4 * N
    plain.step_inplace(env.obs[0].clone(), env.rew[0], env.done[0], torch.zeros(N, device=DEV))
    assert rel(vn._state.cpu().numpy(), plain._state.cpu().numpy()) <= 1e-10
    assert rel(vn.returns.cpu().numpy(), plain.returns.cpu().numpy()) <= 1e-12
    sd = vn.state_dict()
    back = HipVecNormalize(DeviceScript(N, D, steps, seed=43))
    back.load_state_dict(sd)
    assert torch.equal(back._state, vn._state)
