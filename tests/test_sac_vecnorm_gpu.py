"""SAC(env, normalizer=HipVecNormalize(env)) on the MI355X: dm_sac_gather_norm against the composition dm_sac_gather +
dm_vecnorm_apply (bit for bit) and against the fp64 restatement, the flag combinations, a replayed graph under moving statistics and
the re-capture rule, three fused gradient steps against the fp64 SAC reference, the collection path against a plain twin, the launch
list with and without a normaliser, and train.py --algo sac --normalize end to end.

Bounds (none taken from the kernels' output): a normalised output is within 2^-23 |ref| + 1e-9 of the fp64 value (one rounding to
fp32); running statistics within 1e-10 relative (test_vecnorm_kernels_gpu.py's bound); gradients, parameters and heads
within test_sac_gpu.py's GRAD_TOL / PARAM_TOL / HEAD_TOL, on that file's basis."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import sac_ref64 as ref
from deepmimic_mujoco_amd import _lib
from kernel_helpers import DEV, guard_ok, guarded
from sac_helpers import BanditEnv, gather_rows, named_actor, named_critic, normals, opt_from, rel_l2, to_ref
from sac_vecnorm_ref import RecordingBandit, normalize_batch64, out_bound, stats_rel_err
from test_sac_gpu import GRAD_TOL, HEAD_TOL, PARAM_TOL, RAGGED, SHAPES
from vecnorm_ref import VecNormalizeRef

pytestmark = pytest.mark.gpu
SEED, CTR, CAP = 0x5AC1EA12 + 104729, 5, 3
CLIP_OBS, CLIP_REW = 10.0, 10.0


def _close(got, want64, what):
    got, want64 = got.detach().cpu().numpy().astype(np.float64), np.asarray(want64, np.float64)
    err, bnd = np.abs(got - want64), out_bound(want64)
    print("measured %-30s worst error / bound %.3g" % (what, float(np.max(err / bnd))))
    assert np.all(err <= bnd), (what, float(np.max(err / bnd)))


def _columns(rng, rows, D, spread):
    """[rows, D]: column 0 constant (-3.5, +- spread on alternate rows), column 1 at 50 +- 1e-3, the rest normals of mixed scale."""
    x = rng.standard_normal((rows, D)) * (1.0 + (np.arange(D) % 5))
    x[:, 0] = -3.5 + spread * np.where(np.arange(rows) % 2 == 0, 1.0, -1.0)
    if D > 1:
        x[:, 1] = 50.0 + 1e-3 * rng.standard_normal(rows)
    return x.astype(np.float32)


class Case:
    """A normaliser whose statistics come from six real steps (dm_vecnorm_step), the restatement fed the same, and a replay ring of
    CAP steps filled with rows of the same character: in column 0 the ring is the constant +- 1 against a scale of about
    sqrt(1e-4 (1 + 3.5^2) / 6N + 1e-8), so both sides of clip_obs are hit; every third reward is +- 500 against a return deviation of
    about 3, beyond clip_reward."""

    def __init__(self, N, D, A, seed):
        from deepmimic_mujoco_amd.vec_normalize import HipVecNormalize
        rng = np.random.default_rng(seed)
        self.N, self.D, self.A = N, D, A
        self.vn = HipVecNormalize(BanditEnv(N, D, A, device="cuda"), clip_obs=CLIP_OBS, clip_reward=CLIP_REW)
        self.ref = VecNormalizeRef(N, D, clip_obs=CLIP_OBS, clip_reward=CLIP_REW)
        t = lambda a, dt=torch.float32: torch.as_tensor(a, dtype=dt, device=DEV).contiguous()
        o, r = torch.zeros(N, D, device=DEV), torch.zeros(N, device=DEV)
        for _ in range(6):
            obs, rew, done = _columns(rng, N, D, 0.0), (3.0 * rng.standard_normal(N)).astype(np.float32), (rng.random(N) < 0.3).astype(np.uint8)
            self.vn.normalize_step_(t(obs), t(rew), t(done, torch.uint8), None, o, r, None)
            self.ref.step(obs, rew, done)
        rows = CAP * N
        rew = 3.0 * rng.standard_normal(rows)
        rew[::3] = 500.0 * np.where(np.arange(len(rew[::3])) % 2 == 0, 1.0, -1.0)
        self.host = dict(obs=_columns(rng, rows, D, 1.0), next_obs=_columns(rng, rows, D, 1.0),
                         act=rng.uniform(-1, 1, (rows, A)).astype(np.float32), rew=rew.astype(np.float32),
                         done=(rng.random(rows) < 0.4).astype(np.float32))
        self.ring = {k: t(v) for k, v in self.host.items()}
        self.ctr = torch.full((1,), CTR, dtype=torch.int32, device=DEV)

    def set_fill(self, steps):
        """ring_state of `steps` stored vec-env steps; the rows behind them are NaN: a read there shows in the output."""
        self.state = torch.tensor([steps % CAP, steps, 0, 0], dtype=torch.int32, device=DEV)
        live = steps * self.N
        for k, v in self.host.items():
            self.ring[k].copy_(torch.as_tensor(v, device=DEV))
            self.ring[k][live:] = float("nan")
        return live

    def outputs(self, B):
        D, K = self.D, self.D + self.A
        bufs = dict(obs2=guarded(2 * B, D), xq=guarded(B, K), xpi=guarded(B, K, fill=0.25), xt=guarded(B, K, fill=0.25), rew=guarded(B),
                    done=guarded(B))
        return bufs, torch.full((B,), -1, dtype=torch.int32, device=DEV)

    def gather(self, B, entry, bufs, idx):
        R = self.ring
        args = [B, self.N, self.D, self.A, SEED, self.ctr, self.state, R["obs"], R["act"], R["rew"], R["done"], R["next_obs"]] + \
               [bufs[k][1] for k in ("obs2", "xq", "xpi", "xt", "rew", "done")] + [idx]
        if entry == "dm_sac_gather_norm":
            args.append(C.byref(self.vn._desc))
        _lib.call(entry, *args, device=DEV)
        torch.cuda.synchronize()
        assert all(guard_ok(*bufs[k]) for k in bufs), entry
        return {k: v[1] for k, v in bufs.items()}

    def composition(self, B):
        """dm_sac_gather, then dm_vecnorm_apply on obs2 and on rew, laid out as dm_sac_gather_norm lays them out."""
        D = self.D
        bufs, idx = self.outputs(B)
        g = self.gather(B, "dm_sac_gather", bufs, idx)
        plain = {k: v.clone() for k, v in g.items()}
        obs2, rew = torch.empty_like(g["obs2"]), torch.empty_like(g["rew"])
        self.vn._call("dm_vecnorm_apply", 2 * B, g["obs2"], obs2, None, None)
        self.vn._call("dm_vecnorm_apply", B, None, None, g["rew"], rew)
        torch.cuda.synchronize()
        xq, xpi, xt = g["xq"].clone(), g["xpi"].clone(), g["xt"].clone()
        xq[:, :D], xpi[:, :D], xt[:, :D] = obs2[:B], obs2[:B], obs2[B:]
        return dict(obs2=obs2, xq=xq, xpi=xpi, xt=xt, rew=rew, done=g["done"].clone()), plain, idx


@pytest.mark.parametrize("B,N,D,A", [(1, 1, 1, 1), (63, 3, 67, 28), (65, 7, 98, 23), (257, 5, 130, 3)])
def test_gather_norm_is_the_composition_and_matches_fp64(B, N, D, A):
    """(B, N, D, A): the smallest call; the humanoid and G1 widths one under and one over a wave of 64 rows-per-launch, with D beyond
    one pass of the 64 threads of a block; 130 columns (three passes, the last of two threads) with more rows than 256.  Ring: one
    stored step of three, then the wrapped ring (fill 3, position 2)."""
    c = Case(N, D, A, seed=B)
    for steps in (1, CAP + 2):
        live = c.set_fill(min(steps, CAP))
        if steps > CAP:
            c.state[0] = steps % CAP
        want, plain, idx_c = c.composition(B)
        bufs, idx = c.outputs(B)
        got = c.gather(B, "dm_sac_gather_norm", bufs, idx)
        rows = gather_rows(SEED, B, CTR, live)
        assert np.array_equal(idx.cpu().numpy(), rows) and torch.equal(idx, idx_c) and int(rows.max()) < live
        for k in want:                                      # all five layouts and rew, bit for bit; NaN nowhere
            assert torch.equal(got[k], want[k]) and bool(torch.isfinite(got[k]).all()), (steps, k)
        # done and the action columns of xq: the ring's bits; the action columns of xpi / xt are not written
        ix = torch.as_tensor(rows, device=DEV, dtype=torch.long)
        assert torch.equal(got["done"], c.ring["done"][ix]) and torch.equal(got["xq"][:, D:], c.ring["act"][ix])
        assert bool((got["xpi"][:, D:] == 0.25).all()) and bool((got["xt"][:, D:] == 0.25).all())
        # against the restatement in fp64
        raw = {k: c.host[k][rows] for k in c.host}
        b64 = normalize_batch64(c.ref, raw)
        tag = "B%d fill%d " % (B, steps)
        _close(got["obs2"][:B], b64["obs"], tag + "obs2 obs")
        _close(got["obs2"][B:], b64["next_obs"], tag + "obs2 next_obs")
        _close(got["xq"][:, :D], b64["obs"], tag + "xq")
        _close(got["xpi"][:, :D], b64["obs"], tag + "xpi")
        _close(got["xt"][:, :D], b64["next_obs"], tag + "xt")
        _close(got["rew"], b64["rew"], tag + "rew")
        assert not torch.equal(got["obs2"], plain["obs2"])
        if B >= 63 and steps > CAP:                         # >= 9 live rows, >= 63 draws: both signs of both outliers are drawn
            col0 = got["obs2"][:, 0]
            assert float(col0.max()) == CLIP_OBS and float(col0.min()) == -CLIP_OBS
            assert float(got["rew"].max()) == CLIP_REW and float(got["rew"].min()) == -CLIP_REW
            if D > 1:                                       # 50 +- 1e-3 is resolved: distinct values, none clipped
                col1 = got["obs2"][:, 1]
                assert float(col1.abs().max()) < CLIP_OBS and len(torch.unique(col1)) > min(B, 3 * N) // 2


@pytest.mark.parametrize("norm_obs,norm_reward", [(False, True), (True, False), (False, False)])
def test_a_half_switched_off_is_a_plain_copy(norm_obs, norm_reward):
    B, N, D, A = 65, 7, 98, 23
    c = Case(N, D, A, seed=7)
    c.set_fill(CAP)
    both, plain, _ = c.composition(B)                       # with both flags on
    c.vn.norm_obs, c.vn.norm_reward = norm_obs, norm_reward
    bufs, idx = c.outputs(B)
    got = c.gather(B, "dm_sac_gather_norm", bufs, idx)
    for k in ("obs2", "xq", "xpi", "xt"):
        assert torch.equal(got[k], (both if norm_obs else plain)[k]), k
    assert torch.equal(got["rew"], (both if norm_reward else plain)["rew"]) and torch.equal(got["done"], plain["done"])
    assert not torch.equal(both["obs2"], plain["obs2"]) and not torch.equal(both["rew"], plain["rew"])


def _sac(D, A, arch, B=256, n=64, steps=8, normalize=True, env_cls=BanditEnv, done_every=3, **kw):
    from deepmimic_mujoco_amd.sac import SAC
    from deepmimic_mujoco_amd.vec_normalize import HipVecNormalize
    torch.manual_seed(0)
    env = env_cls(n, D, A, device="cuda", seed=3, done_every=done_every)
    vn = HipVecNormalize(env) if normalize else None
    sac = SAC(env, net_arch=arch, batch_size=B, learning_starts=kw.pop("learning_starts", 10 ** 9), seed=1, device="cuda", normalizer=vn, **kw)
    for _ in range(steps):
        sac.env_step()
    return env, sac


def _state(sac):
    return [t.clone() for t in sac.state_tensors()] + [sac._fb[k].clone() for k in ("g_actor", "g_critic", "obs2", "xq", "xt", "rew", "idx")]


def test_a_replayed_graph_sees_the_statistics_of_the_moment():
    """Twins with the same seeds, one replaying a captured graph, one launching eagerly: a gradient step, four env steps that move the
    statistics, a gradient step (the graph is the one captured before the statistics moved), then clip_obs changed on both and a
    third gradient step (the graph must be captured again: the clip is a launch argument)."""
    (_, g), (_, e) = _sac(*RAGGED[:3], RAGGED[3], RAGGED[4]), _sac(*RAGGED[:3], RAGGED[3], RAGGED[4], use_hip_graph=False)
    assert g.use_hip_graph and not e.use_hip_graph

    def step_and_compare(what):
        g.train(1), e.train(1)
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(_state(g), _state(e))):
            assert torch.equal(a, b), (what, i)
        # and the minibatch is the ring rows under the statistics as they are NOW
        idx = g._fb["idx"].long()
        assert torch.equal(g._fb["obs2"][:g.batch_size], g.normalizer.normalize_obs(g.ring["obs"][idx]))
        assert torch.equal(g._fb["rew"], g.normalizer.normalize_reward(g.ring["rew"][idx]))

    step_and_compare("first")
    graph, stats = g._graph, g.normalizer._state.clone()
    for _ in range(4):
        g.env_step(), e.env_step()
    assert not torch.equal(g.normalizer._state, stats) and torch.equal(g.normalizer._state, e.normalizer._state)
    step_and_compare("moved statistics")
    assert g._graph is graph                                 # replayed, not captured again
    g.normalizer.clip_obs = e.normalizer.clip_obs = 0.5
    step_and_compare("clip_obs changed")
    assert g._graph is not graph and float(g._fb["obs2"].abs().max()) == 0.5
    graph = g._graph
    step_and_compare("unchanged settings")
    assert g._graph is graph and g._n_updates == 4


def _per_tensor(got, want, tol, what):
    for k in want:
        assert rel_l2(got[k], want[k]) < tol, (what, k, rel_l2(got[k], want[k]))


@pytest.mark.parametrize("D,A,arch,B,n", [pytest.param(*RAGGED, id="ragged"), pytest.param(*SHAPES[0], 256, 64, id="67-28-256-128")])
def test_fused_gradient_steps_with_the_normaliser_match_fp64(D, A, arch, B, n):
    """test_sac_gpu.py's three-step comparison with the normaliser in the launch sequence.  The fp64 reference is fed the batch it
    normalises itself, in fp64 and without the cast to fp32, from the raw ring rows restated from the hash; its statistics are the
    device's fp64 statistics (held to the restatement in the collection test)."""
    env, sac = _sac(D, A, arch, B, n)
    vn = sac.normalizer
    g = torch.Generator(device="cuda").manual_seed(11)
    with torch.no_grad():
        sac.critic_target.add_(0.3 * sac.critic.abs() * torch.randn(sac.critic.shape, device="cuda", generator=g))
        sac.sac_state[0] = float(np.log(0.2))
        sac.policy.actor["bh"][A + 1] = -25.0
    vref = VecNormalizeRef(n, D)
    vref.obs_rms.mean, vref.obs_rms.var, vref.ret_rms.var = vn.obs_rms.mean, vn.obs_rms.var, float(vn.ret_rms.var[0])
    total = int(sac.ring_state[1]) * n
    for step in range(3):
        S = to_ref(sac)
        opt, t = opt_from(sac)
        ctr = int(sac._learn_ctr)
        sac.gradient_step_fused()
        torch.cuda.synchronize()
        fb, R = sac._fb, sac.ring
        rows = gather_rows(sac._learn_seed, B, ctr, total)
        assert np.array_equal(fb["idx"].cpu().numpy(), rows)
        idx = torch.as_tensor(rows, device="cuda", dtype=torch.long)
        raw = {k: R[k][idx].cpu().numpy() for k in ("obs", "act", "rew", "done", "next_obs")}
        assert 0.0 < float(raw["done"].mean()) < 1.0
        b64 = normalize_batch64(vref, raw)
        _close(fb["obs2"][:B], b64["obs"], "step %d obs" % step)
        _close(fb["obs2"][B:], b64["next_obs"], "step %d next_obs" % step)
        _close(fb["rew"], b64["rew"], "step %d rew" % step)
        assert not np.array_equal(fb["obs2"][:B].cpu().numpy(), raw["obs"])
        eps = torch.as_tensor(normals(sac._learn_seed, 2 * B, ctr, A))
        r = ref.train_step(S, opt, t, {k: torch.as_tensor(v) for k, v in b64.items()}, eps[:B], eps[B:])
        assert rel_l2(fb["xpi"][:, D:], r["a_pi"]) < HEAD_TOL and rel_l2(fb["xt"][:, D:], r["a_next"]) < HEAD_TOL
        assert rel_l2(fb["logp"][:B], r["logp"]) < HEAD_TOL and rel_l2(fb["logp"][B:], r["logp_next"]) < HEAD_TOL
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


def test_collection_stores_raw_and_feeds_the_statistics():
    """Warm-up actions are hash-uniform, so a plain twin takes the same ones: ring, ring state, episode accumulators and episode
    history are its bits (the ring of five steps wraps twice in twelve).  dm_sac_store hands out the slots of the episode history by
    an atomic ticket, so WHICH slot an env's episode lands in is not fixed between two runs: every env finishes once here (step 7, 64
    episodes for 100 slots, none overwritten) and the history is compared as the sorted returns and lengths, bit for bit.  Then, past
    warm-up, the action is the actor's on the NORMALISED last observation."""
    D, A, arch, n = 67, 28, (256, 128), 64
    kw = dict(B=256, n=n, steps=12, buffer_size=5 * n, done_every=7)
    (_, s), (penv, p) = _sac(D, A, arch, **kw), _sac(D, A, arch, normalize=False, env_cls=RecordingBandit, **kw)
    torch.cuda.synchronize()
    for k in s.ring:
        assert torch.equal(s.ring[k], p.ring[k]), k
    assert torch.equal(s.ring_state, p.ring_state) and s.ring_state.tolist()[:3] == [12 % 5, 5, 0]
    assert s.ring_state.tolist()[3] == n and torch.equal(s.ep_acc, p.ep_acc) and torch.equal(s._last_obs, p._last_obs)
    hs, hp = s.ep_hist.view(2, -1), p.ep_hist.view(2, -1)
    assert torch.equal(hs.sort(1).values, hp.sort(1).values) and int((hs[1] == 7).sum()) == n
    vref = VecNormalizeRef(n, D)
    seen = vref.reset(penv.first.cpu().numpy())
    for rec in penv.log:
        seen, _, _ = vref.step(rec["obs"].cpu().numpy(), rec["rew"].cpu().numpy(), rec["done"].cpu().numpy())
    err = stats_rel_err(s.normalizer, vref)
    print("measured statistics after 12 steps: worst relative error %.3g" % err)
    assert err < 1e-10 and s.normalizer.obs_rms.count == pytest.approx(1e-4 + n * 13)
    _close(s._obs_norm, np.clip((penv.log[-1]["obs"].cpu().numpy().astype(np.float64) - vref.obs_rms.mean)
                                / np.sqrt(vref.obs_rms.var + 1e-8), -10, 10), "obs_norm")
    # past warm-up
    s.learning_starts = 0
    S, ctr, pos = to_ref(s), int(s._roll_ctr), int(s.ring_state[0])
    norm64, raw64 = s._obs_norm.double().cpu(), s._last_obs.double().cpu()
    s.env_step()
    torch.cuda.synchronize()
    act = s.ring["act"][pos * n:(pos + 1) * n]
    eps = torch.as_tensor(normals(s._roll_seed, n, ctr, A))
    mu, ls = ref.actor_dist(S, norm64)
    assert rel_l2(act, torch.tanh(mu + ls.exp() * eps)) < HEAD_TOL
    mu, ls = ref.actor_dist(S, raw64)
    assert rel_l2(act, torch.tanh(mu + ls.exp() * eps)) > 10 * HEAD_TOL        # not the actor on the raw observation
    assert torch.equal(s.ring["obs"][pos * n:(pos + 1) * n], raw64.float().cuda())


def test_the_launch_list_changes_in_one_name_only():
    """Without a normaliser a gradient step is the launch sequence it was: dm_sac_gather, no dm_sac_gather_norm.  With one, the
    reverse, at the same length."""
    lists = []
    for normalize in (False, True):
        _, sac = _sac(*RAGGED[:3], RAGGED[3], RAGGED[4], normalize=normalize)
        names, call = [], sac._call
        sac._call = lambda name, *a: (names.append(name), call(name, *a))[1]
        sac.gradient_step_fused()
        torch.cuda.synchronize()
        lists.append(names)
    plain, norm = lists
    assert plain[0] == "dm_sac_gather" and "dm_sac_gather_norm" not in plain and plain.count("dm_sac_gather") == 1
    assert norm[0] == "dm_sac_gather_norm" and "dm_sac_gather" not in norm
    assert len(plain) == len(norm) and plain[1:] == norm[1:]


def test_train_py_sac_normalize_end_to_end(tmp_path, capsys):
    from deepmimic_mujoco_amd import train
    from deepmimic_mujoco_amd.deepmimic_env import HipDeepMimicVecEnv
    from deepmimic_mujoco_amd.vec_normalize import HipVecNormalize
    save, steps = str(tmp_path / "sac.pt"), 40
    train.main(["--algo", "sac", "--normalize", "--envs", "64", "--arch", "64,64", "--buffer-size", "10000", "--total", str(64 * steps),
                "--eval-envs", "64", "--json", "--save", save])
    line = json.loads([x for x in capsys.readouterr().out.splitlines() if x.startswith("{")][-1])
    assert line["workload"] == "sac" and line["normalize"] is True and line["total_timesteps"] == 64 * steps and line["n_updates"] > 0
    assert line["eval"]["episodes"] > 0 and np.isfinite(line["eval"]["ep_rew_mean"])
    assert os.path.exists(save) and os.path.exists(save + ".vecnormalize")
    env = HipDeepMimicVecEnv(64, motion="walk", seed=21)
    vn = HipVecNormalize.load(save + ".vecnormalize", env)
    assert vn.obs_rms.count == pytest.approx(1e-4 + 64 * (1 + steps)) and float(np.abs(vn.obs_rms.mean).max()) > 0
    assert vn.ret_rms.count == pytest.approx(1e-4 + 64 * steps)
    env.close()
