"""bf16 rollout buffers (``PPO(buffer_dtype=torch.bfloat16)``, BASELINE config 5) on the fused rollout and learner paths.

Kernel level: the bf16 forms of dm_policy_forward / dm_rollout_store / dm_ppo_gather / dm_flat_adam_step_gather beside their fp32
forms on the same inputs, every comparison ``torch.equal`` on bit patterns.  bf16 arrays are views at ODD element offsets of larger
int16 buffers pre-filled with 0x7FC0 (only 2-byte alignment holds), fp32 arrays are offset views of NaN-filled buffers; what lies
in front of and behind every output must still be there afterwards.  Rollout level: fp32 and bf16 buffers give the same rollout
bit for bit on every path.  Learner level: bf16 buffers take the epoch graph and the two-graph multi-rank path."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from kernel_helpers import BF16_NAN, DEV, GUARD, lib as _lib, offset as _offset, ptr as _p, stream as _stream

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QNAN16 = BF16_NAN
NAMES = ["walk", "run", "dance_b", "spinkick"]
BF = torch.bfloat16
# (N, D, A): humanoid3d at the sizes of configs 3 and 5, G1-shaped rows (85 = G1 DPEnv, 98 = G1 DPCombinedEnv, 90 = neither) with an N
# that is no multiple of 32, one workgroup plus one row, one row
SHAPES = [(4096, 67, 28), (8192, 67, 28), (1000, 90, 23), (1000, 85, 23), (1000, 98, 23), (33, 67, 28), (1, 67, 28)]
# values whose rounding is the point: up across a binade (halfway, even is above), halfway cases to even in both directions, just
# above / below halfway, negative zero, fp32 denormals, the observation guard's magnitude
SPECIAL = [1.99609375 + 2.0 ** -9, -(1.99609375 + 2.0 ** -9), 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -23,
           1.0 + 2.0 ** -8 - 2.0 ** -23, -0.0, 0.0, 1e-40, -1e-41, 2.0 ** -149, 2.0 ** -127 + 2.0 ** -135, 100.0, -100.0, 99.8046875,
           -99.70703125, 63.75 + 0.125, 3.0e-39, 0.333251953125, -7.00390625]


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


class Out:
    """An output array as an offset view of a guard-filled buffer: fp32 behind NaN, bf16 at an odd element behind 0x7FC0."""

    def __init__(self, shape, dtype=torch.float32, off=1):
        self.n, self.off, self.bf = int(np.prod(shape)), off, dtype == BF
        if self.bf:
            self.buf = torch.full((self.n + off + GUARD,), QNAN16, dtype=torch.int16, device=DEV)
            self.v = self.buf[off:off + self.n].view(BF).view(*shape)
            assert self.v.data_ptr() % 4 == 2 * (off % 2)
        else:
            self.buf = torch.full((self.n + off + GUARD,), float("nan"), device=DEV)
            self.v = self.buf[off:off + self.n].view(*shape)

    def guards_ok(self):
        rest = torch.cat([self.buf[:self.off], self.buf[self.off + self.n:]])
        return bool((rest == QNAN16).all()) if self.bf else bool(torch.isnan(rest).all())


def _with_specials(x, seed):
    """Scatter SPECIAL (and a spread of magnitudes up to 100) over a random tensor, first and last elements included."""
    g = torch.Generator().manual_seed(seed)
    flat = x.reshape(-1).clone()
    n = flat.numel()
    sp = torch.tensor(SPECIAL, dtype=torch.float64).to(torch.float32)
    pos = torch.randint(0, n, (min(n, 8 * len(SPECIAL)),), generator=g)
    flat[pos] = sp.repeat(8)[:pos.numel()]
    big = torch.randint(0, n, (max(1, n // 16),), generator=g)
    flat[big] = (torch.rand(big.numel(), generator=g) * 200 - 100)
    k = min(n, len(SPECIAL))
    flat[:k // 2] = sp[:k // 2]
    flat[n - (k - k // 2):] = sp[:k - k // 2]
    return flat.view(x.shape)


def test_bf16_reference_conversion_is_what_the_cases_assume():
    """The special inputs do what their comment says under torch's conversion (the reference of every kernel test below)."""
    x = torch.tensor(SPECIAL, dtype=torch.float64).to(torch.float32).to(DEV)
    y = x.to(BF).float().cpu()
    assert y[0] == 2.0 and y[1] == -2.0                     # across the binade
    assert y[2] == 1.0 and y[3] == 1.0 + 2.0 ** -6          # ties to even: down, up
    assert y[4] == 1.0 + 2.0 ** -7 and y[5] == 1.0          # just above / below halfway
    assert math.copysign(1.0, float(y[6])) == -1.0 and y[6] == 0.0


# ------------------------------------------------------------------------------------------------ dm_policy_forward_bf16
def _policy(D, A, arch=(256, 128), seed=3):
    from deepmimic_mujoco_amd.ppo import MlpPolicy
    torch.manual_seed(seed)
    pol = MlpPolicy(obs_dim=D, act_dim=A, net_arch=arch).to(DEV)
    with torch.no_grad():
        pol.log_std.copy_(torch.linspace(-1.0, 0.5, A))
    return pol


@pytest.mark.parametrize("det", [0, 1], ids=["sampled", "deterministic"])
@pytest.mark.parametrize("copy", [True, False], ids=["obs_copy", "no_obs_copy"])
@pytest.mark.parametrize("N,D,A", SHAPES)
def test_policy_forward_bf16_beside_fp32(N, D, A, copy, det):
    """Same inputs, seed and counter through both entry points: act_env / logp / val / mean_out bit-equal, act and obs_copy equal to
    the fp32 launch's narrowed by torch (round to nearest even), guards intact."""
    from deepmimic_mujoco_amd.ppo import FusedPolicyForward
    pol = _policy(D, A)
    fwd = FusedPolicyForward(pol, DEV)
    fwd.pack()
    g = torch.Generator().manual_seed(N + D)
    obs = _offset(_with_specials(torch.randn(N, D, generator=g), 5).to(DEV), 1)
    lo, hi = torch.full((A,), -0.5, device=DEV), torch.linspace(0.2, 1.5, A, device=DEV)
    ctr = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    outs = {}
    for dt in (torch.float32, BF):
        o = dict(act=Out((N, A), dt, off=3), act_env=Out((N, A)), logp=Out((N,), off=2), val=Out((N,), off=3), mean=Out((N, A), off=5),
                 obs_copy=Out((N, D), dt, off=1 if N % 2 else 5))
        fwd(obs, 0x5EED, ctr, 3, lo, hi, o["act"].v, o["act_env"].v, o["logp"].v, o["val"].v,
            obs_copy=o["obs_copy"].v if copy else None, mean_out=o["mean"].v, deterministic=bool(det))
        outs[dt] = o
    torch.cuda.synchronize()
    a, b = outs[torch.float32], outs[BF]
    assert all(x.guards_ok() for o in (a, b) for x in o.values())
    for k in ("act_env", "logp", "val", "mean"):
        assert _same(a[k].v, b[k].v), k
    assert b["act"].v.dtype == BF and _same(b["act"].v, a["act"].v.to(BF))
    if det:
        assert _same(a["act"].v, a["mean"].v)
    if copy:
        assert _same(a["obs_copy"].v, obs) and _same(b["obs_copy"].v, obs.to(BF))
    else:
        assert bool((b["obs_copy"].buf == QNAN16).all()) and bool(torch.isnan(a["obs_copy"].buf).all())
    assert torch.isfinite(a["logp"].v).all() and int(ctr.item()) == 5


def test_policy_forward_rejects_mixed_storage_types():
    from deepmimic_mujoco_amd.ppo import FusedPolicyForward
    fwd = FusedPolicyForward(_policy(67, 28), DEV)
    z = lambda *s, dt=torch.float32: torch.zeros(*s, device=DEV, dtype=dt)
    with pytest.raises(ValueError):
        fwd(z(4, 67), 1, z(1, dt=torch.int32), 0, z(28), z(28), z(4, 28, dt=BF), z(4, 28), z(4), z(4), obs_copy=z(4, 67))
    with pytest.raises(ValueError):
        fwd(z(4, 67), 1, z(1, dt=torch.int32), 0, z(28), z(28), z(4, 28, dt=torch.float16), z(4, 28), z(4), z(4))


# ------------------------------------------------------------------------------------------------ dm_rollout_store_bf16
@pytest.mark.parametrize("alias", [False, True], ids=["separate_last_obs_out", "last_obs_out_is_last_obs"])
@pytest.mark.parametrize("N,D,A", SHAPES)
def test_rollout_store_bf16_beside_fp32(N, D, A, alias):
    """b_obs / b_act equal to the fp32 form's narrowed by torch, the fp32 outputs and last_obs_out bit-equal, counter bumped once —
    also when last_obs_out IS last_obs, as every rollout loop passes it."""
    L = _lib()
    g = torch.Generator().manual_seed(3 * N + A)
    last0 = _with_specials(torch.randn(N, D, generator=g), 1).to(DEV)
    act = _offset(_with_specials(torch.randn(N, A, generator=g), 2).to(DEV), 3)
    val, logp, rew = (_offset(torch.randn(N, generator=g).to(DEV), k) for k in (1, 2, 3))
    done = _offset((torch.rand(N, generator=g) < 0.3).to(torch.uint8).to(DEV), 5)
    new = _offset(torch.randn(N, D, generator=g).to(DEV), 1)
    res = {}
    for dt in (torch.float32, BF):
        last = _offset(last0, 1)
        o = dict(b_obs=Out((N, D), dt, off=1 if N % 2 else 3), b_act=Out((N, A), dt, off=1), b_val=Out((N,)), b_logp=Out((N,), off=2),
                 b_rew=Out((N,), off=3), b_done=Out((N,), off=5), last_out=Out((N, D), off=7))
        lo_ptr = last if alias else o["last_out"].v
        ctr = torch.full((1,), 41, dtype=torch.int32, device=DEV)
        fn = L.dm_rollout_store_bf16 if dt == BF else L.dm_rollout_store
        rc = fn(N, D, A, _p(last), _p(act), _p(val), _p(logp), _p(rew), _p(done), _p(new), _p(o["b_obs"].v), _p(o["b_act"].v),
                _p(o["b_val"].v), _p(o["b_logp"].v), _p(o["b_rew"].v), _p(o["b_done"].v), _p(lo_ptr), _p(ctr), _stream())
        assert rc == 0
        torch.cuda.synchronize()
        assert all(x.guards_ok() for x in o.values())
        assert int(ctr.item()) == 42
        assert _same(lo_ptr, new)
        if not alias:
            assert _same(last, last0)
        res[dt] = o
    a, b = res[torch.float32], res[BF]
    assert _same(a["b_obs"].v, last0) and _same(a["b_act"].v, act)
    assert _same(b["b_obs"].v, a["b_obs"].v.to(BF)) and _same(b["b_act"].v, a["b_act"].v.to(BF))
    for k in ("b_val", "b_logp", "b_rew", "b_done"):
        assert _same(a[k].v, b[k].v), k
    assert _same(a["b_val"].v, val) and _same(a["b_done"].v, done.float())
    if alias:
        assert bool(torch.isnan(b["last_out"].buf).all())


# ------------------------------------------------------------------------------------------------ the gathers
def _flat_bf16(n, D, A, seed, off):
    g = torch.Generator().manual_seed(seed)
    f32 = dict(obs=_with_specials(torch.randn(n, D, generator=g), 3), act=_with_specials(torch.randn(n, A, generator=g), 4))
    flat = {k: _offset(v.to(DEV).to(BF), off) for k, v in f32.items()}            # bf16 arrays at an odd element
    for j, k in enumerate(("adv", "ret", "logp")):
        flat[k] = _offset(torch.randn(n, generator=g).to(DEV), j + 1)
    return flat


def _index(n, B, seed):
    """torch.randperm rows with repeats planted, as a view at an odd element of a larger int64 buffer."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    idx = torch.randperm(n, device=DEV, generator=g)
    idx = idx.repeat((B + n - 1) // n)[:B].clone()
    if B >= 4:
        idx[1] = idx[0]
        idx[B - 1] = idx[B // 2]
    idx[0] = n - 1 if B > 1 else idx[0]                                             # the last row of the buffer is read to its end
    if B >= 4:
        idx[2] = 0
    buf = torch.zeros(B + 8, dtype=torch.int64, device=DEV)
    v = buf[3:3 + B]
    v.copy_(idx)
    return v


def _gather_outs(B, D, A):
    return dict(obs=Out((B, D), off=1), act=Out((B, A), off=3), adv=Out((B,), off=1), ret=Out((B,), off=2), logp=Out((B,), off=3))


def _check_gather(o, flat, idx):
    assert all(x.guards_ok() for x in o.values())
    for k in ("obs", "act", "adv", "ret", "logp"):
        assert _same(o[k].v, flat[k][idx].float()), k


@pytest.mark.parametrize("B", [2048, 2047, 1], ids=["B2048", "B2047", "B1"])
@pytest.mark.parametrize("N,D,A", SHAPES)
def test_gather_bf16_equals_indexing_then_widening(N, D, A, B):
    L = _lib()
    flat, idx = _flat_bf16(N, D, A, N + B, 1), _index(N, B, B)
    o = _gather_outs(B, D, A)
    rc = L.dm_ppo_gather_bf16(_p(idx), B, _p(flat["obs"]), D, _p(flat["act"]), A, _p(flat["adv"]), _p(flat["ret"]), _p(flat["logp"]),
                              *(_p(o[k].v) for k in ("obs", "act", "adv", "ret", "logp")), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    _check_gather(o, flat, idx)


def test_gather_bf16_every_row_alignment_and_long_rows():
    """Rows of 1, 7, 8, 9, 15, 16, 17, 134 and 1024 elements from every one of the 8 positions within 16 bytes."""
    L = _lib()
    for D, A in ((1, 1), (7, 9), (8, 15), (16, 17), (134, 3), (1024, 1024)):
        n, B = 40, 40
        for off in range(1, 9):
            flat = _flat_bf16(n, D, A, D + off, off)
            idx = _index(n, B, off)
            o = _gather_outs(B, D, A)
            rc = L.dm_ppo_gather_bf16(_p(idx), B, _p(flat["obs"]), D, _p(flat["act"]), A, _p(flat["adv"]), _p(flat["ret"]), _p(flat["logp"]),
                                      *(_p(o[k].v) for k in ("obs", "act", "adv", "ret", "logp")), _stream())
            assert rc == 0
            torch.cuda.synchronize()
            _check_gather(o, flat, idx)


@pytest.mark.parametrize("begin", [1, 0])
@pytest.mark.parametrize("B", [2048, 2047, 1], ids=["B2048", "B2047", "B1"])
@pytest.mark.parametrize("N,D,A", [(8192, 67, 28), (1000, 98, 23), (33, 67, 28)])
def test_gather_bf16_riding_on_adam_norm_launch(N, D, A, B, begin):
    """dm_flat_adam_step_gather_bf16: gathered rows as above; p / m / v / state the bits dm_flat_adam_step_gather leaves with an fp32
    gather of the widened buffer on the same gradient."""
    from deepmimic_mujoco_amd import _lib as mod
    L = _lib()
    flat, idx = _flat_bf16(N, D, A, 7 * N + B, 1), _index(N, B, B + 1)
    wide = dict(flat, obs=flat["obs"].float(), act=flat["act"].float())
    n = 104377
    g = torch.Generator().manual_seed(B)
    p0, g0, m0 = (torch.randn(n, generator=g).to(DEV) * s for s in (1.0, 0.01, 0.001))
    v0 = (torch.rand(n, generator=g) * 1e-4).to(DEV)
    res = {}
    for kind in ("fp32", "bf16"):
        p, gr, m, v = p0.clone(), g0.clone(), m0.clone(), v0.clone()
        st2 = torch.zeros(2 + 1024, device=DEV)
        st2[1] = 3.0
        o = _gather_outs(B, D, A)
        src = flat if kind == "bf16" else wide
        gs = mod.DmGatherSpecBf16() if kind == "bf16" else mod.DmGatherSpec()
        gs.idx, gs.B, gs.D, gs.A = idx.data_ptr(), B, D, A
        gs.obs, gs.act, gs.adv, gs.ret, gs.logp = (src[k].data_ptr() for k in ("obs", "act", "adv", "ret", "logp"))
        gs.o_obs, gs.o_act, gs.o_adv, gs.o_ret, gs.o_logp = (o[k].v.data_ptr() for k in ("obs", "act", "adv", "ret", "logp"))
        fn = L.dm_flat_adam_step_gather_bf16 if kind == "bf16" else L.dm_flat_adam_step_gather
        rc = fn(_p(p), _p(gr), _p(m), _p(v), n, 4e-4, 0.9, 0.999, 1e-5, 0.5, 1.0, _p(st2), int(st2.numel()), begin, C.byref(gs), _stream())
        assert rc == 0
        torch.cuda.synchronize()
        _check_gather(o, flat, idx)
        res[kind] = (p, m, v, st2)
    for x, y in zip(res["fp32"], res["bf16"]):
        assert _same(x, y)
    assert not torch.equal(res["bf16"][0], p0) and float(res["bf16"][3][1]) == 3.0 + begin


# ------------------------------------------------------------------------------------------------ rollouts
PATHS = {   # name: (PPO keywords, env sub_batches, needs _fused_policy_ok, rollout_path())
    "policy_forward": (dict(), 1, True, "policy_forward"),
    "policy_forward_sub2": (dict(rollout_graph=False), 2, True, "policy_forward"),
    "policy_forward_graph": (dict(rollout_graph=True), 2, True, "policy_forward"),
    "sample_store": (dict(fused_policy=False), 1, False, "sample_store"),
    "pipelined_eager": (dict(fused_policy=False, rollout_graph=False), 2, False, "sample_store"),
    "captured": (dict(fused_policy=False, rollout_graph=True), 2, False, "graph"),
}
KEYS32 = ("rew", "done", "val", "logp", "adv", "ret")


def _make_env(robot, K, seed=9):
    from deepmimic_mujoco_amd.deepmimic_env import HipDeepMimicVecEnv
    if robot == "g1":
        return HipDeepMimicVecEnv(256, motion="walk", robot="unitree_g1", seed=seed, sub_batches=K)
    return HipDeepMimicVecEnv(1024, motion=NAMES, seed=seed, sub_batches=K)


def _stat_eq(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def _rollouts(robot, path, dt, calls=2, T=8):
    from deepmimic_mujoco_amd.ppo import PPO
    kw, K, need_fp, name = PATHS[path]
    env = _make_env(robot, K)
    ppo = PPO(env, net_arch=(256, 128), n_steps=T, batch_size=2048, n_epochs=1, seed=4, buffer_dtype=dt, **kw)
    assert ppo._fused_rollout_ok()
    assert ppo._fused_policy_ok() == need_fp
    assert ppo.rollout_path() == name
    out = []
    for _ in range(calls):
        buf = ppo.collect_rollouts()
        torch.cuda.synchronize()
        out.append(({k: v.clone() for k, v in buf.items()}, {k: ppo.stats[k] for k in ("ep_rew_mean", "ep_len_mean", "episodes", "explained_variance")}))
    env.close()
    return out


@pytest.mark.parametrize("robot,path", [("humanoid3d", p) for p in PATHS] + [("g1", "policy_forward"), ("g1", "policy_forward_sub2")])
def test_rollout_with_bf16_buffers_is_the_fp32_rollout_bit_for_bit(robot, path):
    """Two PPO objects, same env seed, policy seed and net, fp32 and bf16 buffers, two collect_rollouts() each.  The env and the policy
    never read the rollout buffer — the policy reads `last_obs` (fp32), the env reads the fp32 clamped action — so narrowing what is
    STORED cannot change a rollout: rew / done / val / logp / adv / ret are bit-equal, obs / act are the fp32 run's narrowed by
    torch, and the episode statistics are equal."""
    r32, r16 = _rollouts(robot, path, torch.float32), _rollouts(robot, path, BF)
    for call, ((b32, s32), (b16, s16)) in enumerate(zip(r32, r16)):
        assert b32["obs"].dtype == torch.float32 and b32["act"].dtype == torch.float32
        assert b16["obs"].dtype == BF and b16["act"].dtype == BF
        for k in KEYS32:
            assert b16[k].dtype == torch.float32 and _same(b32[k], b16[k]), (call, k)
        assert _same(b16["obs"], b32["obs"].to(BF)), call
        assert _same(b16["act"], b32["act"].to(BF)), call
        assert all(_stat_eq(s32[k], s16[k]) for k in s32), (call, s32, s16)
        assert float(b32["obs"].abs().max()) > 0 and float(b32["act"].abs().max()) > 0
    assert not torch.equal(r32[0][0]["act"], r32[1][0]["act"])           # the second call is a new rollout


# ------------------------------------------------------------------------------------------------ learner
LEARNERS = {"mlp_256_128_fp32": ((256, 128), torch.float32), "wide_1024_512_bf16": ((1024, 512), BF), "library_1024_512_fp32": ((1024, 512), torch.float32)}


@pytest.mark.parametrize("learner", list(LEARNERS))
def test_train_on_bf16_buffers_takes_the_epoch_graph_and_tracks_the_widened_twin(learner):
    """train() on a bf16 rollout takes the epoch graph; afterwards the static minibatch holds exactly the last gathered rows; loss and
    parameters agree with a twin trained on the widened copy of the same buffer within the project's bounds for this comparison
    (loss 2 %, parameters 2e-3).  The learner's inputs are bit-identical (previous assertion), so what can differ is the summation
    order of fp32 atomics in the weight-gradient kernels: where two identical fp32 runs come out bit-equal on the machine, the bf16
    run is held to bit-equality too.  The run prints which case held (not recorded here yet: no MI355X run of this file exists)."""
    from deepmimic_mujoco_amd.ppo import PPO
    arch, mlp_dt = LEARNERS[learner]
    T, B = 8, 2048
    env = _make_env("humanoid3d", 1)
    mk = lambda dt: PPO(env, net_arch=arch, n_steps=T, batch_size=B, n_epochs=2, seed=4, buffer_dtype=dt, mlp_dtype=mlp_dt)
    ppo = mk(BF)
    assert ppo._fused_policy_ok() and ppo.rollout_path() == "policy_forward"
    buf = {k: v.clone() for k, v in ppo.collect_rollouts().items()}
    assert buf["obs"].dtype == BF and buf["act"].dtype == BF
    n = T * env.num_envs
    flat = {k: v.reshape(n, *v.shape[2:]) for k, v in buf.items()}
    loss16 = ppo.train(buf, generator=torch.Generator(device=DEV).manual_seed(8))
    torch.cuda.synchronize()
    eg = getattr(ppo, "_eg", None)
    assert eg is not None and eg["flat"]["obs"].dtype == BF and eg["flat"]["act"].dtype == BF
    last = eg["perm"][n - B:]
    for k in ("obs", "act", "adv", "ret", "logp"):
        assert eg["gin"][k].dtype == torch.float32 and _same(eg["gin"][k], flat[k][last].float()), k
    par16 = ppo.optimizer.flat_p.detach().clone()
    wide = dict(buf, obs=buf["obs"].float(), act=buf["act"].float())
    twins = []
    for _ in range(2):
        tw = mk(torch.float32)
        twins.append((tw.train(wide, generator=torch.Generator(device=DEV).manual_seed(8)), tw.optimizer.flat_p.detach().clone()))
        assert getattr(tw, "_eg", None) is not None
    env.close()
    (l32, p32), (l32b, p32b) = twins
    reproducible = torch.equal(p32, p32b) and l32 == l32b
    step = float((par16 - p32).abs().max())
    print("%s: loss bf16-buffer %.9g fp32-twin %.9g, max |dp| %.3g, two fp32 runs bit-equal: %s, bf16 run bit-equal: %s"
          % (learner, loss16, l32, step, reproducible, torch.equal(par16, p32)))
    assert np.isfinite(loss16) and abs(loss16 - l32) < 0.02 * max(1.0, abs(l32))
    assert step < 2e-3, step
    if reproducible:
        assert torch.equal(par16, p32) and loss16 == l32


@pytest.mark.parametrize("arch", ["256,128", "1024,512,bf16"])
def test_two_ranks_with_bf16_buffers_take_the_two_graph_path(tmp_path, arch):
    """Two ranks on the one GPU over gloo, bf16 rollout buffers: train() takes the two-graph path and the replicas stay bit-identical."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29541" if arch == "256,128" else "29542", os.path.join(ROOT, "tests", "dist_two_rank_bf16_worker.py"),
           "--out", str(tmp_path), "--arch", arch.replace(",bf16", "")] + (["--bf16"] if arch.endswith("bf16") else [])
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    a, b = (torch.load(os.path.join(tmp_path, "rank%d.pt" % k)) for k in (0, 1))
    for x in (a, b):
        assert x["used_dist_graph"] and x["calls"] == 3 and x["buffer_dtype"] == "torch.bfloat16" and x["gather_ok"]
        assert x["rollout_path"] == "policy_forward"
    assert torch.equal(a["params"], b["params"]) and torch.isfinite(a["params"]).all()
    assert not torch.equal(a["params"], a["params0"])
    assert not torch.equal(a["obs0"], b["obs0"])
