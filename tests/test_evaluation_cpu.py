"""The host side of the batched evaluator (deepmimic_mujoco_amd/evaluation.py): refusals, the episode -> start-frame plan, the
statistics of an evaluation record, the command-line switch and the declarations of the two new entry points.  No GPU."""
import os
import re
import types

import numpy as np
import pytest
import torch

from deepmimic_mujoco_amd import _lib, evaluation
from deepmimic_mujoco_amd.evaluation import EvalResult

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_an_auto_resetting_env_is_refused():
    env = types.SimpleNamespace(auto_reset=True, num_envs=4, engines=[], out={})
    with pytest.raises(ValueError, match="auto_reset=False"):
        evaluation.BatchEvaluator(env)
    with pytest.raises(ValueError, match="auto_reset=False"):                 # an object that does not say is not trusted either
        evaluation.BatchEvaluator(types.SimpleNamespace(num_envs=4))
    with pytest.raises(ValueError, match="sync_every"):
        evaluation.BatchEvaluator(types.SimpleNamespace(auto_reset=False, num_envs=4), sync_every=0)


@pytest.mark.parametrize("n_envs, L, episodes, rounds", [(32, 76, 76, [(0, 32), (32, 32), (64, 12)]),      # N < L: three rounds
                                                         (128, 76, 76, [(0, 76)]),                       # N > L: one, 52 envs idle
                                                         (128, 76, 200, [(0, 128), (128, 72)]),          # frames wrap around
                                                         (76, 76, 76, [(0, 76)]), (1, 3, 3, [(0, 1), (1, 1), (2, 1)])])
def test_all_start_frames_and_rounds(n_envs, L, episodes, rounds):
    frames = evaluation.episode_frames(episodes, L)
    assert frames.tolist() == [e % L for e in range(episodes)]
    plan = evaluation.plan_rounds(episodes, n_envs)
    assert plan == rounds and len(plan) == -(-episodes // n_envs)
    assert sum(c for _, c in plan) == episodes and all(1 <= c <= n_envs for _, c in plan)
    covered = np.concatenate([frames[s:s + c] for s, c in plan])
    assert covered.tolist() == frames.tolist()                                 # every episode once, in order
    with pytest.raises(ValueError):
        evaluation.plan_rounds(0, n_envs)


def test_start_frames_are_resolved_before_anything_runs():
    eng = types.SimpleNamespace(clip_len={0: 76})
    env = types.SimpleNamespace(engine=eng, num_envs=32, motions=["walk"])
    n, frames = evaluation.resolve_frames(env, None, "all")
    assert n == 76 and frames.tolist() == list(range(76))
    n, frames = evaluation.resolve_frames(env, 100, "all")
    assert n == 100 and frames[76:].tolist() == list(range(24))
    assert evaluation.resolve_frames(env, None, None) == (32, None) and evaluation.resolve_frames(env, 5, None) == (5, None)
    n, frames = evaluation.resolve_frames(env, 5, [3, 9])
    assert n == 5 and frames.tolist() == [3, 9, 3, 9, 3]
    g1 = types.SimpleNamespace(engine=types.SimpleNamespace(clip_len=76), num_envs=8, motions=["walk"])
    assert evaluation.resolve_frames(g1, None, "all")[0] == 76
    multi = types.SimpleNamespace(engine=eng, num_envs=32, motions=["walk", "run"])
    with pytest.raises(ValueError, match="single-clip"):                       # its envs follow clips of different lengths
        evaluation.resolve_frames(multi, None, "all")
    assert evaluation.resolve_frames(multi, None, [1, 2])[0] == 2
    with pytest.raises(ValueError):
        evaluation.resolve_frames(env, None, "some")


def _result(ret, ln, reason):
    n = len(ret)
    return EvalResult(ep_len=torch.tensor(ln, dtype=torch.int32), ep_ret=torch.tensor(ret, dtype=torch.float64),
                      ep_terms=torch.zeros(n, 5, dtype=torch.float64), ep_reason=torch.tensor(reason, dtype=torch.int32),
                      last_obs=torch.zeros(n, 67), start_frames=torch.arange(n, dtype=torch.int32), steps_run=max(ln))


def test_statistics_of_hand_made_results():
    T = evaluation.TRUNCATED
    # two rounds; caps: one episode ended by the engine at 1000 (reason 3), one truncated at 1000, one truncated at 24 (no cap)
    a = _result([10.0, 20.5, 3.25], [1000, 1000, 24], [3, T, T])
    b = _result([0.5, 90.0], [17, 999], [1, T])
    s = evaluation.episode_statistics([a, b], 1000)
    ret = np.array([10.0, 20.5, 3.25, 0.5, 90.0])
    assert s["episodes"] == 5
    assert s["ep_rew_mean"] == float(np.mean(ret)) and s["ep_rew_std"] == float(np.std(ret))
    assert s["ep_len_mean"] == (1000 + 1000 + 24 + 17 + 999) / 5
    assert s["frac_reached_cap"] == 2 / 5                                      # truncated at 24 or 999 is not "reached the cap"
    one = evaluation.episode_statistics(a, 1000)
    assert one["episodes"] == 3 and one["frac_reached_cap"] == 2 / 3
    assert evaluation.episode_statistics(_result([1.0], [24], [T]), 1000)["frac_reached_cap"] == 0.0
    assert set(evaluation.RECORD_FIELDS) == {"global_step"} | set(s)
    assert evaluation.TRUNCATED == -1


def test_evaluate_policy_returns_sb3s_shapes(monkeypatch):
    """(mean, std) or (rewards, lengths), over all rounds in episode order; the rounds themselves are replaced by hand-made results."""
    rounds = [_result([1.0, 2.0], [5, 6], [1, 1]), _result([6.0], [7], [-1])]
    env = types.SimpleNamespace(ENV_CFG=types.SimpleNamespace(MAX_EP_LENGTH=1000))
    monkeypatch.setattr(evaluation, "run_episodes", lambda *a, **k: rounds)
    mean, std = evaluation.evaluate_policy(None, env)
    assert mean == 3.0 and std == float(np.std([1.0, 2.0, 6.0]))
    rew, ln = evaluation.evaluate_policy(None, env, return_episode_rewards=True)
    assert rew == [1.0, 2.0, 6.0] and ln == [5, 6, 7] and all(isinstance(x, int) for x in ln)


def test_policy_act_fn_routes_without_a_gpu():
    from deepmimic_mujoco_amd.ppo import ExtractedPolicy
    env = types.SimpleNamespace(device=torch.device("cpu"))
    f = lambda obs: obs[:, :28]
    assert evaluation.policy_act_fn(f, env) is f                               # a callable is passed through
    with pytest.raises(TypeError):
        evaluation.policy_act_fn(3, env)
    pol = ExtractedPolicy(os.path.join(ROOT, "tests", "golden", "policy_kat.npz"))
    obs = torch.linspace(-1, 1, 3 * 67).reshape(3, 67)
    act = evaluation.policy_act_fn(pol, env)(obs)
    assert torch.equal(act, torch.clamp(pol.act(obs[:, :66]), -0.5, 0.5)) and act.shape == (3, 28)      # src/play_extracted.py:36-38


def test_train_parses_eval_envs():
    from deepmimic_mujoco_amd import train
    ap = train.build_parser()
    assert ap.parse_args([]).eval_envs == 0
    assert ap.parse_args(["--eval-envs", "76", "--eval-every", "1000"]).eval_envs == 76


def test_dashboard_callback_defaults_to_no_batch_env():
    from deepmimic_mujoco_amd.eval_dashboard import EvalDashboardCallback
    cb = EvalDashboardCallback(None, "run")
    assert cb.batch_env is None and cb.batch_start_frames == "all" and cb.batch_history == []


def test_new_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "deepmimic_hip.h")).read()
    assert re.search(r"\bint\s+dm_eval_advance\s*\(", header) and re.search(r"\bint\s+dm_step_active\s*\(", header)
    assert re.search(r"#define\s+DM_EVAL_TRUNCATED\s+\(-1\)", header)
    assert "dm_eval_advance" in _lib.EXPORTS and "dm_step_active" in _lib.EXPORTS
    L = _lib.load_library()
    assert len(L.dm_eval_advance.argtypes) == 19 and len(L.dm_step_active.argtypes) == 10
    assert hasattr(_lib.HipEngine, "step_active")
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    assert "dm_eval_advance" in text and "dm_step_active" in text
    with open(os.path.join(ROOT, "deepmimic_mujoco_amd", "csrc", "Makefile")) as f:
        assert "dm_eval.hip" in f.read()
