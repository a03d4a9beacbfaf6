"""SAC(env, n_steps=n) on the MI355X: dm_sac_gather_nstep against the fp64 restatement of the n-step semantics (tests/sac_nstep_ref.py)
on rings written directly, n_steps = 1 against the two existing gathers bit for bit, three fused gradient steps at n_steps = 3 against
the fp64 SAC reference fed the fp64 n-step batch, a replayed graph against an eager twin while the ring moves and wraps, the launch
lists, and train.py --algo sac --n-step 3 end to end.

Bounds, none taken from the kernel's output (u = 2^-24, S = sum_{j<k} gamma^j |r_j|): |rew - ref| <= (2k + 1) u S (gamma^j by fp32
products is off by up to j u relative, any summation order adds at most (k - 1) u S, one final rounding), with a normaliser plus
sum_j gamma^j out_bound(r_j); |done' - ref| <= (k + 1) u; observations are the ring's bits without a normaliser and within out_bound
(2^-23 |ref| + 1e-9) with one; rows, k and actions are exact.  The learner: test_sac_gpu.py's HEAD_TOL, GRAD_TOL, PARAM_TOL."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import sac_ref64 as ref
from deepmimic_mujoco_amd import _lib
from kernel_helpers import DEV, guard_ok, guarded
from sac_helpers import BanditEnv, gather_rows, named_actor, named_critic, normals, opt_from, rel_l2, to_ref
from sac_nstep_ref import SHAPES as RINGS, done_bound, nstep_batch64, rew_bound, states, written_ring
from sac_vecnorm_ref import out_bound
from test_sac_gpu import GRAD_TOL, HEAD_TOL, PARAM_TOL, RAGGED, SHAPES
from test_sac_vecnorm_gpu import CAP, Case, SEED as CASE_SEED
from vecnorm_ref import VecNormalizeRef

pytestmark = pytest.mark.gpu
SEED, GAMMA, CLIP_REW, B = 7, 0.99, 0.5, 64
KINDS = {"full", "cut by done", "cut at newest", "done at newest", "wraps"}
# one gradient step of the parent commit, name for name (SAC._call is the one door to the library)
PARENT_LAUNCHES = ["dm_sac_gather", "dm_sac_linear_relu", "dm_sac_head_fwd", "dm_sac_linear_relu", "dm_sac_linear_relu", "dm_sac_critic_loss",
                   "dm_sac_relu_bwd_colsum", "dm_sac_relu_bwd_colsum", "dm_flat_adam_step", "dm_sac_linear_relu", "dm_sac_actor_loss",
                   "dm_sac_relu_bwd_colsum", "dm_sac_relu_bwd_colsum", "dm_sac_head_bwd", "dm_sac_relu_bwd_colsum", "dm_sac_relu_bwd_colsum",
                   "dm_flat_adam_step", "dm_sac_polyak"]


def _within(got, want, bnd, what):
    err = np.abs(got.detach().cpu().numpy().astype(np.float64) - want)
    worst = float(np.max(np.where(err == 0, 0.0, err / bnd)))
    print("measured %-38s worst error / bound %.3g" % (what, worst))
    assert np.all(err <= bnd), (what, worst)


def _gather_nstep(Bn, N, D, A, seed, ctr, state, ring, cap, n, gamma, vn=None):
    """One call of dm_sac_gather_nstep into NaN-guarded outputs (the action columns of xpi / xt preset to 0.25: not written)."""
    K = D + A
    bufs = dict(obs2=guarded(2 * Bn, D), xq=guarded(Bn, K), xpi=guarded(Bn, K, fill=0.25), xt=guarded(Bn, K, fill=0.25), rew=guarded(Bn),
                done=guarded(Bn))
    idx, k = torch.full((Bn,), -1, dtype=torch.int32, device=DEV), torch.full((Bn,), -1, dtype=torch.int32, device=DEV)
    _lib.call("dm_sac_gather_nstep", Bn, N, D, A, seed, ctr, state, ring["obs"], ring["act"], ring["rew"], ring["done"], ring["next_obs"],
              *[bufs[x][1] for x in ("obs2", "xq", "xpi", "xt", "rew", "done")], idx, cap, n, gamma, k,
              None if vn is None else C.byref(vn._desc), device=DEV)
    torch.cuda.synchronize()
    assert all(guard_ok(*bufs[x]) for x in bufs)
    return dict({x: v[1] for x, v in bufs.items()}, idx=idx, k=k)


def _normaliser(N, D, A):
    """A device normaliser whose statistics come from six real steps, and the fp64 restatement holding the same statistics."""
    from deepmimic_mujoco_amd.vec_normalize import HipVecNormalize
    rng = np.random.default_rng(5)
    vn = HipVecNormalize(BanditEnv(N, D, A, device="cuda"), clip_reward=CLIP_REW)
    t = lambda a, dt=torch.float32: torch.as_tensor(a, dtype=dt, device=DEV).contiguous()
    o, r = torch.zeros(N, D, device=DEV), torch.zeros(N, device=DEV)
    for _ in range(6):
        vn.normalize_step_(t(0.3 + 2.0 * rng.standard_normal((N, D))), t(1.5 * rng.standard_normal(N)), t(rng.random(N) < 0.3, torch.uint8),
                           None, o, r, None)
    vref = VecNormalizeRef(N, D, clip_reward=CLIP_REW)
    vref.obs_rms.mean, vref.obs_rms.var, vref.ret_rms.var = vn.obs_rms.mean, vn.obs_rms.var, float(vn.ret_rms.var[0])
    return vn, vref


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalizer"])
@pytest.mark.parametrize("shape,mod", RINGS, ids=["3-7-5-2", "7-5-98-23"])
def test_gather_nstep_matches_fp64(shape, mod, normalize):
    """64 rows (seed 7, counter 0) of a ring written directly, in three ring states, n = 1, 2, 3, 5, and n = 64 once.  Rows never
    stored are NaN, so a read past the newest step shows.  At (cap, 3) with n = 3 the drawn rows hold every kind of chain."""
    N, cap, D, A = shape
    host = written_ring(N, cap, D, A, mod)
    vn, vref = _normaliser(N, D, A) if normalize else (None, None)
    ctr = torch.zeros(1, dtype=torch.int32, device=DEV)
    for fill, pos in states(cap):
        ring = {k: torch.as_tensor(v, device=DEV) for k, v in host.items()}
        for v in ring.values():
            v[fill * N:] = float("nan")
        state = torch.tensor([pos, fill, 0, 0], dtype=torch.int32, device=DEV)
        rows = gather_rows(SEED, B, 0, fill * N)
        for n in (1, 2, 3, 5) + ((64,) if (fill, pos) == (cap, 3) else ()):
            got = _gather_nstep(B, N, D, A, SEED, ctr, state, ring, cap, n, GAMMA, vn)
            want = nstep_batch64(host, rows, N, cap, pos, n, GAMMA, vref)
            tag = "n%d fill%d pos%d " % (n, fill, pos)
            assert np.array_equal(got["idx"].cpu().numpy(), rows) and int(rows.max()) < fill * N
            assert np.array_equal(got["k"].cpu().numpy(), want["k"]), tag
            assert torch.equal(got["xq"][:, D:].cpu(), torch.as_tensor(host["act"][rows]))
            assert bool((got["xpi"][:, D:] == 0.25).all()) and bool((got["xt"][:, D:] == 0.25).all())
            obs, nxt = (got["obs2"][:B], got["xq"][:, :D], got["xpi"][:, :D]), (got["obs2"][B:], got["xt"][:, :D])
            assert all(torch.equal(x, obs[0]) for x in obs) and torch.equal(nxt[0], nxt[1])
            if normalize:
                _within(obs[0], want["obs"], out_bound(want["obs"]), tag + "obs")
                _within(nxt[0], want["next_obs"], out_bound(want["next_obs"]), tag + "next_obs")
                assert not np.array_equal(obs[0].cpu().numpy(), host["obs"][rows])
            else:
                assert np.array_equal(obs[0].cpu().numpy(), host["obs"][rows]) and np.array_equal(nxt[0].cpu().numpy(), host["next_obs"][want["last"]])
            _within(got["rew"], want["rew"], rew_bound(want), tag + "rew")
            _within(got["done"], want["done"], done_bound(want), tag + "done'")
            if (fill, pos) == (cap, 3) and n == 3:
                kinds = set().union(*want["kinds"])
                assert kinds >= KINDS, kinds
                assert int(want["k"].min()) == 1 and int(want["k"].max()) == 3
            if n == 64:
                assert int(want["k"].max()) <= cap
    if normalize:                                            # the clip of the reward transform was hit
        assert float(np.abs(nstep_batch64(host, rows, N, cap, 3, 1, GAMMA, vref)["rew"]).max()) == CLIP_REW


@pytest.mark.parametrize("Bn,N,D,A", [(1, 1, 1, 1), (63, 3, 67, 28), (65, 7, 98, 23), (257, 5, 130, 3)])
def test_n_steps_1_is_the_existing_gathers_bit_for_bit(Bn, N, D, A):
    """test_sac_vecnorm_gpu.py's ragged shapes and rings (one stored step of three, then the wrapped ring): with n_steps = 1 the new
    entry gives dm_sac_gather's bits with a NULL struct and dm_sac_gather_norm's with one, -0 rewards and clipped values included."""
    c = Case(N, D, A, seed=Bn)
    for steps in (1, CAP + 2):
        c.set_fill(min(steps, CAP))
        if steps > CAP:
            c.state[0] = steps % CAP
        c.ring["rew"][0] = -0.0
        for entry, vn in (("dm_sac_gather", None), ("dm_sac_gather_norm", c.vn)):
            bufs, idx = c.outputs(Bn)
            want = c.gather(Bn, entry, bufs, idx)
            got = _gather_nstep(Bn, N, D, A, CASE_SEED, c.ctr, c.state, c.ring, CAP, 1, GAMMA, vn)
            for k in want:
                assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), (entry, steps, k)
            assert torch.equal(got["idx"], idx) and bool((got["k"] == 1).all())


def _sac(D, A, arch, Bn=256, n=64, steps=8, normalize=False, n_steps=3, **kw):
    from deepmimic_mujoco_amd.sac import SAC
    from deepmimic_mujoco_amd.vec_normalize import HipVecNormalize
    torch.manual_seed(0)
    env = BanditEnv(n, D, A, device="cuda", seed=3, done_every=4)
    vn = HipVecNormalize(env) if normalize else None
    sac = SAC(env, net_arch=arch, batch_size=Bn, learning_starts=10 ** 9, seed=1, device="cuda", normalizer=vn, n_steps=n_steps, **kw)
    for _ in range(steps):
        sac.env_step()
    return env, sac


def _per_tensor(got, want, tol, what):
    for k in want:
        assert rel_l2(got[k], want[k]) < tol, (what, k, rel_l2(got[k], want[k]))


@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "normalizer"])
@pytest.mark.parametrize("D,A,arch,Bn,n", [pytest.param(*RAGGED, id="ragged"), pytest.param(*SHAPES[0], 256, 64, id="67-28-256-128")])
def test_fused_gradient_steps_at_n_steps_3_match_fp64(D, A, arch, Bn, n, normalize):
    """test_sac_gpu.py's three-step comparison with the n-step gather at the head of the launch sequence: the fp64 reference is fed
    the fp64 n-step batch of the rows restated from the hash.  The set-up is that file's and test_sac_vecnorm_gpu.py's (eight stored
    steps, their seeds) with a done every fourth step instead of every third: the dones fall on steps 3 and 7 and step 7 is the
    newest, so chains of 1, 2 and 3 rows occur, cut by a done (one of them the done at the newest step) or by n.  A chain cut at the
    newest step WITHOUT a done does not occur here; the kernel test above holds that kind.  DESIGN §27 records how sensitive this
    comparison is to a single ReLU unit near 0."""
    env, sac = _sac(D, A, arch, Bn, n, steps=8, normalize=normalize)
    g = torch.Generator(device="cuda").manual_seed(11)
    with torch.no_grad():
        sac.critic_target.add_(0.3 * sac.critic.abs() * torch.randn(sac.critic.shape, device="cuda", generator=g))
        sac.sac_state[0] = float(np.log(0.2))
        sac.policy.actor["bh"][A + 1] = -25.0
    vref = None
    if normalize:
        vn = sac.normalizer
        vref = VecNormalizeRef(n, D)
        vref.obs_rms.mean, vref.obs_rms.var, vref.ret_rms.var = vn.obs_rms.mean, vn.obs_rms.var, float(vn.ret_rms.var[0])
    pos, fill = sac.ring_state.tolist()[:2]
    assert (pos, fill) == (8, 8)
    host = {k: v.cpu().numpy() for k, v in sac.ring.items()}
    for step in range(3):
        S = to_ref(sac)
        opt, t = opt_from(sac)
        ctr = int(sac._learn_ctr)
        sac.gradient_step_fused()
        torch.cuda.synchronize()
        fb = sac._fb
        rows = gather_rows(sac._learn_seed, Bn, ctr, fill * n)
        assert np.array_equal(fb["idx"].cpu().numpy(), rows)
        b64 = nstep_batch64(host, rows, n, sac.cap_steps, pos, 3, sac.gamma, vref)
        assert np.array_equal(fb["k"].cpu().numpy(), b64["k"]) and set(b64["k"]) == {1, 2, 3}
        assert 0.0 < float(host["done"][b64["last"]].mean()) < 1.0
        _within(fb["rew"], b64["rew"], rew_bound(b64), "step %d rew" % step)
        _within(fb["done"], b64["done"], done_bound(b64), "step %d done'" % step)
        if normalize:
            _within(fb["obs2"][:Bn], b64["obs"], out_bound(b64["obs"]), "step %d obs" % step)
            _within(fb["obs2"][Bn:], b64["next_obs"], out_bound(b64["next_obs"]), "step %d next_obs" % step)
        else:
            assert np.array_equal(fb["obs2"][:Bn].cpu().numpy(), host["obs"][rows])
            assert np.array_equal(fb["obs2"][Bn:].cpu().numpy(), host["next_obs"][b64["last"]])
        eps = torch.as_tensor(normals(sac._learn_seed, 2 * Bn, ctr, A))
        r = ref.train_step(S, opt, t, {k: torch.as_tensor(b64[k]) for k in ("obs", "act", "rew", "next_obs", "done")}, eps[:Bn], eps[Bn:])
        assert rel_l2(fb["xpi"][:, D:], r["a_pi"]) < HEAD_TOL and rel_l2(fb["xt"][:, D:], r["a_next"]) < HEAD_TOL
        assert rel_l2(fb["logp"][:Bn], r["logp"]) < HEAD_TOL and rel_l2(fb["logp"][Bn:], r["logp_next"]) < HEAD_TOL
        st = sac.sac_state.cpu()
        assert abs(float(st[0]) - float(S["log_alpha"])) < 1e-6
        assert abs(float(st[6]) - r["critic_loss"]) < 1e-4 * max(1.0, abs(r["critic_loss"]))
        assert abs(float(st[7]) - r["actor_loss"]) < 1e-4 * max(1.0, abs(r["actor_loss"]))
        _per_tensor(named_actor(sac, fb["g_actor"]), r["g_actor"], GRAD_TOL, "g_actor")
        for i in (0, 1):
            _per_tensor(named_critic(sac, fb["g_critic"], i), r["g_critic"]["qf%d" % i], GRAD_TOL, "g_qf%d" % i)
        _per_tensor(named_actor(sac, sac.actor), S["actor"], PARAM_TOL, "actor")
        for i in (0, 1):
            _per_tensor(named_critic(sac, sac.critic, i), S["qf%d" % i], PARAM_TOL, "qf%d" % i)
            _per_tensor(named_critic(sac, sac.critic_target, i), S["tgt%d" % i], PARAM_TOL, "tgt%d" % i)
        assert int(sac._learn_ctr) == ctr + 1


def _state(sac):
    return [t.clone() for t in sac.state_tensors()] + [sac._fb[k].clone() for k in ("g_actor", "g_critic", "obs2", "xq", "xt", "rew", "done", "idx", "k")]


def test_a_replayed_graph_follows_the_ring_as_it_moves_and_wraps():
    """Twins with the same seeds and a ring of five steps, one replaying its captured graph, one launching eagerly: a gradient step
    after each of seven further env steps (the position passes 0 twice); n_steps is fixed, so the graph is never captured again."""
    D, A, arch, Bn, n = RAGGED
    (_, g), (_, e) = _sac(D, A, arch, Bn, n, steps=3, buffer_size=5 * n), _sac(D, A, arch, Bn, n, steps=3, buffer_size=5 * n, use_hip_graph=False)
    assert g.use_hip_graph and not e.use_hip_graph and g.cap_steps == 5
    graph, seen = None, set()
    for it in range(8):
        g.train(1), e.train(1)
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(_state(g), _state(e))):
            assert torch.equal(a, b), (it, i)
        graph = graph or g._graph
        assert g._graph is graph
        seen.add(tuple(g.ring_state.tolist()[:2]))
        assert int(g._fb["k"].min()) >= 1 and int(g._fb["k"].max()) <= 3
        g.env_step(), e.env_step()
    assert seen == {(3, 3), (4, 4), (0, 5), (1, 5), (2, 5), (3, 5), (4, 5)} and g._n_updates == 8


def test_the_launch_lists():
    """n_steps = 1 is the parent's launch sequence name for name; n_steps = 3 differs from it in its first name only, with or without
    a normaliser."""
    lists = {}
    for key, kw in (("default", dict(n_steps=1)), ("n3", dict(n_steps=3)), ("n3 normalizer", dict(n_steps=3, normalize=True))):
        _, sac = _sac(*RAGGED[:3], RAGGED[3], RAGGED[4], **kw)
        names, call = [], sac._call
        sac._call = lambda name, *a, _n=names, _c=call: (_n.append(name), _c(name, *a))[1]
        sac.gradient_step_fused()
        torch.cuda.synchronize()
        lists[key] = names
    assert lists["default"] == PARENT_LAUNCHES
    for key in ("n3", "n3 normalizer"):
        assert lists[key] == ["dm_sac_gather_nstep"] + PARENT_LAUNCHES[1:], key


def test_train_py_sac_n_step_end_to_end(capsys):
    from deepmimic_mujoco_amd import train
    steps = 40
    train.main(["--algo", "sac", "--n-step", "3", "--envs", "64", "--arch", "64,64", "--buffer-size", "10000", "--total", str(64 * steps), "--json"])
    line = json.loads([x for x in capsys.readouterr().out.splitlines() if x.startswith("{")][-1])
    assert line["workload"] == "sac" and line["n_steps"] == 3 and line["total_timesteps"] == 64 * steps and line["n_updates"] > 0
    assert all(np.isfinite(line[k]) for k in ("critic_loss", "actor_loss", "ent_coef"))
