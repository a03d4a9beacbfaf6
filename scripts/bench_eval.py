"""Batched evaluation (deepmimic_mujoco_amd/evaluation.py): `--envs` episodes, up to `--max-steps` steps (default: the env's own
MAX_EP_LENGTH), finished envs leaving the launch (`compact`, dm_step_active / dmg1_step_active) against all envs stepped to the end
(`compact=False`), alternating, `--runs` evaluations each after one warm-up evaluation, wall time per evaluation with a device
synchronisation on both sides; the arms must give identical lengths and returns.

Default: the reference's exported walk policy on humanoid walk (tests/golden/policy_kat.npz with its own protocol: obs[:66], clip
+-0.5), env i from frame i mod 76; the one-episode, host-stepped `eval_dashboard_rollout(figures=False)` is timed on a few start frames
as the per-episode cost it replaces.  `--robot unitree_g1` (walk, env i from frame i mod L) and `--env dp_combined_env` (the G1
combined task, the engine's seeded start states) take `--policy zero` or `fresh` (a seeded, untrained [256, 128] net) and add a third
arm: `compact="all"` with the slot list launched in the caller's order instead of longest-first.  Prints one JSON line.

    python scripts/bench_eval.py [--envs 4096] [--max-steps N] [--runs 3] [--sync-every 16] [--dashboard-episodes 4]
                                 [--robot unitree_g1] [--env dp_combined_env] [--policy zero|fresh]
"""
import argparse
import contextlib
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _DashboardModel:
    """What eval_dashboard_rollout asks of a model, around the extracted policy."""

    def __init__(self, act_fn, device):
        self.act_fn, self.device, self.policy = act_fn, device, self

    def predict(self, obs, deterministic=True):
        return self.act_fn(torch.as_tensor(obs, dtype=torch.float32, device=self.device))

    def predict_values(self, obs):
        return torch.zeros(obs.shape[0])

    def save(self, path):
        pass


class _FromFrame:
    """A one-env DPEnv whose ``reset()`` starts at ``frame`` (DPEnv.reset draws a random one)."""

    def __init__(self, env):
        self.env, self.frame = env, 0

    def reset(self):
        self.env.episode_reward, self.env.episode_length = 0, 0
        return self.env.reset_model(idx_init=self.frame)

    def __getattr__(self, name):
        return getattr(self.env, name)


def _build(args):
    """(make_env, frames or None, act_fn factory, workload name): the env of one arm, its start frames and its policy."""
    from deepmimic_mujoco_amd.deepmimic_env import HipDeepMimicVecEnv
    from deepmimic_mujoco_amd.evaluation import policy_act_fn
    from deepmimic_mujoco_amd.ppo import ExtractedPolicy, MlpPolicy
    combined = args.env == "dp_combined_env"
    if combined:
        if args.robot != "unitree_g1":
            raise SystemExit("--env dp_combined_env is measured on --robot unitree_g1")
        from deepmimic_mujoco_amd.g1 import HipG1CombinedVecEnv
        make = lambda: HipG1CombinedVecEnv(args.envs, auto_reset=False)
    else:
        make = lambda: HipDeepMimicVecEnv(args.envs, motion="walk", robot=args.robot, auto_reset=False)

    def policy(env):
        if args.policy == "extracted":
            if args.robot != "humanoid3d":
                raise SystemExit("--policy extracted is the humanoid walk policy; use zero or fresh on the G1")
            return policy_act_fn(ExtractedPolicy(os.path.join(ROOT, "tests", "golden", "policy_kat.npz")), env)
        n_act = env.action_space.shape[0]
        if args.policy == "zero":
            zero = torch.zeros(args.envs, n_act, device=env.device)
            return lambda obs: zero
        torch.manual_seed(0)                                            # "fresh": a seeded, untrained net of the reference's [256, 128]
        net = MlpPolicy(env.observation_space.shape[0], n_act, (256, 128)).to(env.device)
        lo, hi = (torch.as_tensor(b, device=env.device) for b in (env.action_space.low, env.action_space.high))
        return lambda obs: torch.clamp(net(obs, deterministic=True)[0], lo, hi)
    return make, combined, policy, "eval_%s_%s_%s_policy" % (args.robot, "combined" if combined else "walk", args.policy)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--max-steps", type=int, default=None, help="default: the env's own MAX_EP_LENGTH (1000 DPEnv, 2000 combined)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--sync-every", type=int, default=16)
    ap.add_argument("--dashboard-episodes", type=int, default=4, help="humanoid3d only")
    ap.add_argument("--robot", default="humanoid3d", choices=["humanoid3d", "unitree_g1"])
    ap.add_argument("--env", default="deep_mimic_mujoco", choices=["deep_mimic_mujoco", "dp_combined_env"])
    ap.add_argument("--policy", default=None, choices=["extracted", "zero", "fresh"], help="default: extracted (humanoid3d), zero (unitree_g1)")
    args = ap.parse_args()
    args.policy = args.policy or ("extracted" if args.robot == "humanoid3d" else "zero")
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval.py measures on the GPU; none is visible")
    from deepmimic_mujoco_amd.deepmimic_env import DPEnv
    from deepmimic_mujoco_amd.eval_dashboard import eval_dashboard_rollout
    from deepmimic_mujoco_amd.evaluation import BatchEvaluator, clip_length, episode_frames, episode_statistics, max_ep_length

    make, combined, policy, workload = _build(args)
    g1 = args.robot == "unitree_g1"
    modes = {"compact": "all" if g1 else True, "all_envs": False}
    sched = {}
    if g1:                                  # third arm: "all" without the longest-first pass over the slot list (dmg1_set_active_schedule)
        modes["compact_unordered"] = "all"
        sched = {"compact": 1, "compact_unordered": 0}
    # the combined task starts from the engine's seeded draw, keyed by the env's reset count: there every arm has an env of its own
    # (same seed), and the arms stay in step — evaluation k of one arm runs the episodes of evaluation k of the others
    envs = {k: make() for k in modes} if combined else dict.fromkeys(modes, make())
    env = envs["compact"]
    args.max_steps = max_ep_length(env) if args.max_steps is None else args.max_steps
    frames = None if combined else episode_frames(args.envs, clip_length(env))
    act = {k: policy(e) for k, e in envs.items()}
    arms = {k: BatchEvaluator(envs[k], compact=m, sync_every=args.sync_every) for k, m in modes.items()}
    assert all(arms[k].compact == (k != "all_envs") for k in arms)

    def one(k):
        if k in sched:
            for e in envs[k].engines:
                e.set_active_schedule(sched[k])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = arms[k].run(act[k], frames, args.max_steps)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    _, first = one("compact")                                           # warm-up evaluation (also the record the arms must reproduce)
    if combined:
        for k in arms:
            if k != "compact":
                one(k)
    wall = {k: [] for k in arms}
    launched, live = {}, []
    for _ in range(args.runs):
        ref = None
        for k in arms:
            dt, res = one(k)
            wall[k].append(dt)
            launched[k] = arms[k].launched_env_steps
            ref = ref or (first if not combined else res)
            assert torch.equal(res.ep_len, ref.ep_len) and torch.equal(res.ep_ret, ref.ep_ret), "%s differs from the other arms" % k
        live.append(int(ref.ep_len.sum()))
        first = ref
    ln = first.ep_len.cpu().numpy()
    stats = episode_statistics(first, max_ep_length(env))
    med = {k: statistics.median(v) for k, v in wall.items()}
    spread = {k: max(v) - min(v) for k, v in wall.items()}
    out = {"workload": workload, "envs": args.envs, "max_steps": args.max_steps, "sync_every": args.sync_every,
           "runs": args.runs, "steps_run": int(first.steps_run),
           "wall_s": {k: {"median": round(med[k], 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in wall.items()},
           "episodes_per_s": {k: round(args.envs / med[k], 1) for k in arms},
           "speedup_compact": round(med["all_envs"] / med["compact"], 3),
           "compact_faster_beyond_spread": bool(med["all_envs"] - med["compact"] > max(spread.values())),
           "spread_s": {k: round(v, 4) for k, v in spread.items()},
           "env_steps_live": live[-1], "env_steps_launched": launched,
           "survival": {"median_len": float(np.median(ln)), "frac_reached_cap": stats["frac_reached_cap"],
                        "ep_len_mean": stats["ep_len_mean"], "ep_rew_mean": round(stats["ep_rew_mean"], 4)}}
    if g1:
        out["schedule_gain_s"] = round(med["compact_unordered"] - med["compact"], 4)
        out["schedule_faster_beyond_spread"] = bool(med["compact_unordered"] - med["compact"] > max(spread["compact"], spread["compact_unordered"]))
    if combined:
        out["env_steps_live_per_run"] = live                            # (each evaluation draws its own start states)

    if args.dashboard_episodes > 0 and not g1:                                   # the path this replaces: one env, stepped from the host
        single = _FromFrame(DPEnv("walk"))
        model = _DashboardModel(act["compact"], env.device)
        per_ep, per_step = [], []
        with tempfile.TemporaryDirectory() as tmp:
            for e in range(args.dashboard_episodes):
                single.frame = int(e * clip_length(env) // args.dashboard_episodes)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(sys.stderr):            # its "Eval: LEN ..." line; stdout carries the JSON line alone
                    n_steps, _ = eval_dashboard_rollout(model, single, e, "bench_eval", out_root=tmp, max_steps=args.max_steps, figures=False)
                dt = time.perf_counter() - t0
                per_ep.append(dt)
                per_step.append(dt / n_steps)
        out["dashboard_rollout"] = {"episodes": args.dashboard_episodes, "s_per_episode_median": round(statistics.median(per_ep), 4),
                                    "ms_per_env_step_median": round(1e3 * statistics.median(per_step), 4)}
        # the same episodes, one after the other on the host-stepped path, at its cost per env step
        out["dashboard_rollout"]["s_for_the_same_episodes"] = round(statistics.median(per_step) * int(ln.sum()), 1)
        single.close()
    for e in set(envs.values()):
        e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
