"""The batched evaluator (deepmimic_mujoco_amd/evaluation.py) on the GPU against a reference loop written here: a second env with the
same constructor arguments, ``reset_tensor(idx_init)``, the plain ``step_tensor`` on ALL envs every step, bookkeeping on the host in
Python floats, and a ``get_state`` snapshot after every step.  Lengths, reasons, returns (bit for bit), terminal observations (bit for
bit) and — where finished envs are no longer launched — the frozen engine state must agree.

"Frozen": after the evaluation a finished env's ``get_state`` is bit for bit the reference's snapshot right after that env's terminal
step.  That holds for every env on the compacted humanoid path (``dm_step_active`` does not launch a finished env).  On the routes
that keep stepping all envs (``compact=False``, Unitree G1) only the bookkeeping is frozen, the engine state of an env that was done
early moves on; there the state check covers the envs whose terminal step is the evaluation's last step."""
import numpy as np
import pytest
import torch

from deepmimic_mujoco_amd import evaluation
from deepmimic_mujoco_amd.evaluation import BatchEvaluator, evaluate_policy, policy_act_fn

pytestmark = pytest.mark.gpu

N_WALK, STEPS_WALK = 76, 24


def reference_loop(env, act_fn, start_frames, max_steps):
    t = torch
    n = env.num_envs
    obs = env.reset_tensor(t.as_tensor(np.asarray(start_frames, np.int32), device=env.device))
    alive, ep_len, ep_ret = [True] * n, [0] * n, [0.0] * n
    ep_reason, last_obs, snap = [None] * n, [None] * n, [None] * n
    with t.no_grad():
        for _ in range(max_steps):
            out = env.step_tensor(act_fn(obs))
            rew, done, reason, o = (out[k].cpu().numpy() for k in ("rew", "done", "reason", "obs"))
            state = [s.cpu().numpy() for s in env.engine.get_state()]
            for i in range(n):
                if not alive[i]:
                    continue
                ep_len[i] += 1
                ep_ret[i] += float(rew[i])
                if done[i] or ep_len[i] == max_steps:
                    ep_reason[i] = int(reason[i]) if done[i] else evaluation.TRUNCATED
                    last_obs[i] = o[i].copy()
                    snap[i] = [s[i].copy() for s in state]
                    alive[i] = False
    assert not any(alive)
    return dict(ep_len=np.array(ep_len, np.int32), ep_ret=np.array(ep_ret, np.float64), ep_reason=np.array(ep_reason, np.int32),
                last_obs=np.stack(last_obs), snap=snap)


def use(env, steps=3):
    """Leave ``env`` as an earlier run would: mid-episode, with warm starts and controls of its own.  The evaluator's results must not
    depend on it (a reset alone keeps both, as the reference's does)."""
    g = torch.Generator(device="cpu").manual_seed(5)
    env.reset_tensor()
    for _ in range(steps):
        a = (torch.rand(env.num_envs, env.action_space.shape[0], generator=g) - 0.5).to(env.device)
        env.step_tensor(a * torch.as_tensor(env.action_space.high, device=env.device))


def check(result, ref, env, max_steps, all_frozen):
    ep_len, ep_reason = result.ep_len.cpu().numpy(), result.ep_reason.cpu().numpy()
    print("lengths", ep_len.tolist(), "reasons", ep_reason.tolist())
    assert result.ep_len.dtype == torch.int32 and result.ep_ret.dtype == torch.float64
    assert np.array_equal(ep_len, ref["ep_len"])
    assert np.array_equal(ep_reason, ref["ep_reason"])
    assert np.array_equal(result.ep_ret.cpu().numpy().view(np.int64), ref["ep_ret"].view(np.int64))            # bit for bit
    assert np.array_equal(result.last_obs.cpu().numpy().view(np.int32), ref["last_obs"].view(np.int32))
    assert result.steps_run <= max_steps
    state = [s.cpu().numpy() for s in env.engine.get_state()]
    for i in range(len(ep_len)):
        if all_frozen or ep_len[i] == result.steps_run:
            for got, want in zip(state, ref["snap"][i]):
                assert np.array_equal(got[i].view(np.int32), want.view(np.int32)), "env %d is not frozen at its terminal state" % i


# ------------------------------------------------------------------------------------------ humanoid walk
def _walk_env(n=N_WALK):
    from deepmimic_mujoco_amd.deepmimic_env import HipDeepMimicVecEnv
    return HipDeepMimicVecEnv(n, motion="walk", auto_reset=False)


@pytest.fixture(scope="module")
def walk():
    """(eval env, reference env, act_fn, reference record) of the 76-frame walk case; the reference is computed once."""
    from deepmimic_mujoco_amd.ppo import MlpPolicy
    env, ref_env = _walk_env(), _walk_env()
    torch.manual_seed(0)
    policy = MlpPolicy(67, 28, (256, 128)).to(env.device)
    lo, hi = (torch.as_tensor(b, device=env.device) for b in (env.action_space.low, env.action_space.high))
    pad = torch.zeros(128, 67, device=env.device)

    def act_fn(obs):
        # a plain torch forward, always on 128 rows: the GEMM shape (and with it the library's choice of kernel) is then the same for
        # the 76-env and the 32-env runs, which the rounds test compares bit for bit
        with torch.no_grad():
            n = obs.shape[0]
            pad[:n] = obs
            return torch.clamp(policy(pad, deterministic=True)[0][:n], lo, hi)
    ref = reference_loop(ref_env, act_fn, np.arange(N_WALK), STEPS_WALK)         # on a freshly built env
    use(env)
    yield env, ref_env, act_fn, ref
    env.close()
    ref_env.close()


def test_walk_reference_loop_has_early_ends_and_cuts(walk):
    """Preconditions of the comparison, on the reference loop alone: the case exercises both ways an episode ends."""
    ref = walk[3]
    ln = ref["ep_len"]
    print("reference lengths", ln.tolist(), "reasons", ref["ep_reason"].tolist())
    assert int(np.sum((ln < STEPS_WALK))) >= 10
    assert int(np.sum(ref["ep_reason"] == evaluation.TRUNCATED)) >= 10
    assert len(set(ln.tolist())) >= 4


@pytest.mark.parametrize("compact, sync_every", [(True, 16), (True, 1), (False, 16), (False, 1)])
def test_walk_evaluator_equals_the_reference_loop(walk, compact, sync_every):
    env, _, act_fn, ref = walk
    ev = BatchEvaluator(env, compact=compact, sync_every=sync_every)
    assert ev.compact == compact
    res = ev.run(act_fn, np.arange(N_WALK), STEPS_WALK)
    assert res.start_frames.cpu().tolist() == list(range(N_WALK))
    check(res, ref, env, STEPS_WALK, all_frozen=compact)
    live_steps = int(ref["ep_len"].sum())
    if compact:                                   # finished envs leave the launch at the next read of the live count at the latest
        assert live_steps <= ev.launched_env_steps <= N_WALK * STEPS_WALK
        if sync_every == 1:
            assert ev.launched_env_steps == live_steps
    else:
        assert ev.launched_env_steps == N_WALK * res.steps_run


def test_walk_sub_batches_and_idle_envs(walk):
    """Two engines (bookkeeping per engine slice) and fewer episodes than envs: the first 50 frames on an 80-env, two-engine env."""
    from deepmimic_mujoco_amd.deepmimic_env import HipDeepMimicVecEnv
    _, _, act_fn, ref = walk
    env = HipDeepMimicVecEnv(80, motion="walk", auto_reset=False, sub_batches=2)
    try:
        res = BatchEvaluator(env, sync_every=4).run(act_fn, np.arange(50), STEPS_WALK)
        assert res.ep_len.shape == (50,)
        assert np.array_equal(res.ep_len.cpu().numpy(), ref["ep_len"][:50])
        assert np.array_equal(res.ep_reason.cpu().numpy(), ref["ep_reason"][:50])
        assert np.array_equal(res.ep_ret.cpu().numpy().view(np.int64), ref["ep_ret"][:50].view(np.int64))
        assert np.array_equal(res.last_obs.cpu().numpy().view(np.int32), ref["last_obs"][:50].view(np.int32))
    finally:
        env.close()


def test_seeded_random_start_frames(walk):
    """``start_frames=None``: the engine's own reference-state initialisation; the frames it drew are reported."""
    env, _, act_fn, _ = walk
    res = BatchEvaluator(env).run(act_fn, None, 2)
    sf = res.start_frames.cpu().numpy()
    assert sf.shape == (N_WALK,) and sf.min() >= 0 and sf.max() < evaluation.clip_length(env) and len(set(sf.tolist())) > 8
    assert res.steps_run == 2 and res.ep_len.cpu().tolist() == [2] * N_WALK
    assert set(res.ep_reason.cpu().tolist()) <= {evaluation.TRUNCATED, 1, 2}


def test_callback_appends_eval_batch_csv(walk, tmp_path):
    """``EvalDashboardCallback(batch_env=...)``: one row of the six fields per evaluation point, next to log.csv."""
    from deepmimic_mujoco_amd.eval_dashboard import EvalDashboardCallback
    env, _, act_fn, ref = walk
    cb = EvalDashboardCallback(None, "run", out_root=str(tmp_path), max_steps=STEPS_WALK, batch_env=env)
    rec = cb.batch_evaluation(act_fn, 123)
    cb.batch_evaluation(act_fn, 456)
    lines = (tmp_path / "run_videos" / "eval_batch.csv").read_text().splitlines()
    assert lines[0] == "global_step,episodes,ep_rew_mean,ep_rew_std,ep_len_mean,frac_reached_cap" and len(lines) == 3
    row = [float(x) for x in lines[1].split(",")]
    assert row == [123.0, 76.0, float(np.mean(ref["ep_ret"])), float(np.std(ref["ep_ret"])), float(np.mean(ref["ep_len"])), 0.0]
    assert rec == dict(zip(evaluation.RECORD_FIELDS, [123, 76] + row[2:])) and lines[2].startswith("456,76,")
    assert len(cb.batch_history) == 2 and not (tmp_path / "run_videos" / "log.csv").exists()


def test_rounds_on_a_smaller_env_give_the_same_episodes(walk):
    """``evaluate_policy(start_frames="all")`` on 32 envs: three rounds (32 + 32 + 12) reproduce the 76-env run."""
    _, _, act_fn, ref = walk
    env = _walk_env(32)
    try:
        rew, ln = evaluate_policy(act_fn, env, start_frames="all", max_steps=STEPS_WALK, return_episode_rewards=True)
        assert len(rew) == len(ln) == N_WALK
        assert ln == ref["ep_len"].tolist()
        assert np.array_equal(np.array(rew, np.float64).view(np.int64), ref["ep_ret"].view(np.int64))
        mean, std = evaluate_policy(act_fn, env, start_frames="all", max_steps=STEPS_WALK)
        assert mean == float(np.mean(ref["ep_ret"])) and std == float(np.std(ref["ep_ret"]))
    finally:
        env.close()


def test_ppo_route_is_the_fused_deterministic_forward(walk):
    from deepmimic_mujoco_amd.deepmimic_env import HipDeepMimicVecEnv
    from deepmimic_mujoco_amd.ppo import PPO, FusedPolicyForward
    env = walk[0]
    train_env, ref_env = HipDeepMimicVecEnv(64, motion="walk"), _walk_env()         # the reference loop runs on a freshly built env
    try:
        ppo = PPO(train_env, n_steps=8, batch_size=64, seed=3)
        assert FusedPolicyForward.supported(ppo.policy, ppo.device)
        before = {k: v.clone() for k, v in ppo.policy.state_dict().items()}
        act_fn = policy_act_fn(ppo, env)
        with pytest.raises(ValueError):
            policy_act_fn(ppo, env, deterministic=False)
        ref = reference_loop(ref_env, act_fn, np.arange(N_WALK), STEPS_WALK)
        res = BatchEvaluator(env).run(act_fn, np.arange(N_WALK), STEPS_WALK)
        check(res, ref, env, STEPS_WALK, all_frozen=True)
        # the fused route is the deterministic policy, clamped as collect_rollouts clamps: PPO.predict up to the kernel's rounding
        obs = env.reset_tensor(torch.arange(N_WALK, dtype=torch.int32, device=env.device)).clone()
        assert torch.allclose(act_fn(obs), ppo.predict(obs, deterministic=True), atol=1e-5)
        after = ppo.policy.state_dict()
        assert all(torch.equal(before[k], after[k]) for k in before) and ppo.num_timesteps == 0
    finally:
        train_env.close()
        ref_env.close()


def test_predict_routes_of_sac_and_of_a_ppo_the_fused_forward_does_not_support(walk):
    """``policy_act_fn`` hands both to ``model.predict(deterministic=True)``: the same episodes as with that call written out."""
    from deepmimic_mujoco_amd.ppo import PPO, FusedPolicyForward
    from deepmimic_mujoco_amd.sac import SAC
    env = walk[0]
    ppo = PPO(env, net_arch=(48, 40), n_steps=8, batch_size=76, seed=1)
    assert not FusedPolicyForward.supported(ppo.policy, ppo.device)
    sac = SAC(env, net_arch=(64, 64), buffer_size=76 * 4, seed=1)
    ev = BatchEvaluator(env)
    for model in (ppo, sac):
        got = ev.run(policy_act_fn(model, env), np.arange(N_WALK), 12)
        want = ev.run(lambda obs: model.predict(obs, deterministic=True), np.arange(N_WALK), 12)
        assert torch.equal(got.ep_len, want.ep_len) and torch.equal(got.ep_ret, want.ep_ret) and torch.equal(got.last_obs, want.last_obs)
        assert float(got.ep_ret.abs().sum()) > 0
    mean, std = evaluate_policy(sac, env, max_steps=12)
    assert np.isfinite(mean) and std >= 0


def test_three_wave_engine_keeps_its_kernel_when_few_envs_are_left():
    """An engine of 3 072 envs steps with the three-wave kernel; ``dm_step_active`` must keep it when fewer than 3 072 envs are still
    listed (the variant comes from the engine's size, not from the list's): compacted and uncompacted runs agree bit for bit."""
    n, max_steps = 3072, 40
    env = _walk_env(n)
    try:
        zero = torch.zeros(n, env.action_space.shape[0], device=env.device)
        frames = np.arange(n) % evaluation.clip_length(env)
        ev = BatchEvaluator(env, compact=True, sync_every=2)
        a = ev.run(lambda obs: zero, frames, max_steps)
        assert ev.launched_env_steps < n * a.steps_run              # launches of fewer than 3 072 slots took place
        ln = a.ep_len.cpu().numpy()
        print("lengths", sorted(set(ln.tolist())))
        assert ln.min() + 2 < ln.max()                              # ... while other envs had steps to go
        b = BatchEvaluator(env, compact=False).run(lambda obs: zero, frames, max_steps)
        for f in ("ep_len", "ep_reason", "ep_ret", "ep_terms", "last_obs"):
            assert torch.equal(getattr(a, f), getattr(b, f)), f
    finally:
        env.close()


def test_train_runs_the_final_evaluation(capsys):
    """``train.py --eval-envs``: the ``--json`` line carries the six fields of a final evaluation from all 76 start frames."""
    import json
    from deepmimic_mujoco_amd import train
    train.main(["--envs", "64", "--horizon", "8", "--minibatch", "64", "--epochs", "1", "--total", "512", "--eval-envs", "32", "--json"])
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1]
    rec = json.loads(line)["eval"]
    assert tuple(rec) == evaluation.RECORD_FIELDS and rec["episodes"] == 76 and rec["global_step"] == 512
    assert 1 <= rec["ep_len_mean"] <= 1000 and 0 <= rec["frac_reached_cap"] <= 1 and np.isfinite(rec["ep_rew_mean"])


@pytest.mark.parametrize("env_name, robot", [("deep_mimic_mujoco", "unitree_g1"), ("dp_combined_env", "humanoid3d")])
def test_train_builds_the_evaluation_twin_of_the_other_envs(env_name, robot):
    from deepmimic_mujoco_amd import train
    args = train.build_parser().parse_args(["--env", env_name, "--robot", robot, "--eval-envs", "16"])
    env = train._eval_batch_env(args, args.motion.split(","), 0)
    try:
        assert env.num_envs == 16 and not env.auto_reset and evaluation.is_combined(env) == (env_name == "dp_combined_env")
        zero = torch.zeros(16, env.action_space.shape[0], device=env.device)
        rec = evaluation.evaluation_record(lambda obs: zero, env, 5, max_steps=6)
        assert rec["episodes"] == (16 if evaluation.is_combined(env) else evaluation.clip_length(env)) and rec["ep_len_mean"] <= 6
    finally:
        env.close()


# ------------------------------------------------------------------------------------------ Unitree G1
def test_g1_evaluator_equals_its_reference_loop():
    from deepmimic_mujoco_amd.deepmimic_env import HipDeepMimicVecEnv
    n, max_steps = 16, 17
    frames = np.linspace(0, 75, n).astype(np.int32)
    make = lambda: HipDeepMimicVecEnv(n, motion="walk", robot="unitree_g1", auto_reset=False)
    env, ref_env = make(), make()
    try:
        zero = torch.zeros(n, env.action_space.shape[0], device=env.device)
        act_fn = lambda obs: zero
        ref = reference_loop(ref_env, act_fn, frames, max_steps)
        print("G1 reference lengths", ref["ep_len"].tolist(), "reasons", ref["ep_reason"].tolist())
        assert int(np.sum(ref["ep_reason"] != evaluation.TRUNCATED)) >= 3 and int(np.sum(ref["ep_reason"] == evaluation.TRUNCATED)) >= 3
        for sync_every in (16, 1):                 # first on the env as built (never reset: train.py's first evaluation point), then used
            ev = BatchEvaluator(env, sync_every=sync_every)
            assert not ev.compact                  # the G1 engine has no slot-list step: all envs are stepped, the bookkeeping is frozen
            check(ev.run(act_fn, frames, max_steps), ref, env, max_steps, all_frozen=False)
            use(env)
    finally:
        env.close()
        ref_env.close()
