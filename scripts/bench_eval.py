"""Batched evaluation (deepmimic_mujoco_amd/evaluation.py) of the reference's exported walk policy (tests/golden/policy_kat.npz with its
own protocol: obs[:66], clip +-0.5): `--envs` episodes on humanoid walk, env i from frame i mod 76, up to `--max-steps` steps.
`compact=True` (finished envs leave the launch, dm_step_active) against `compact=False` (all envs stepped to the end), alternating,
`--runs` evaluations each after one warm-up evaluation, wall time per evaluation; both must give identical lengths and returns.
The existing one-episode, host-stepped `eval_dashboard_rollout(figures=False)` is timed on a few start frames as the per-episode cost
it replaces.  Prints one JSON line.

    python scripts/bench_eval.py [--envs 4096] [--max-steps 1000] [--runs 3] [--sync-every 16] [--dashboard-episodes 4]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--max-steps", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--sync-every", type=int, default=16)
    ap.add_argument("--dashboard-episodes", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval.py measures on the GPU; none is visible")
    from deepmimic_mujoco_amd.deepmimic_env import DPEnv, HipDeepMimicVecEnv
    from deepmimic_mujoco_amd.eval_dashboard import eval_dashboard_rollout
    from deepmimic_mujoco_amd.evaluation import BatchEvaluator, clip_length, episode_frames, episode_statistics, policy_act_fn
    from deepmimic_mujoco_amd.ppo import ExtractedPolicy

    env = HipDeepMimicVecEnv(args.envs, motion="walk", auto_reset=False)
    act_fn = policy_act_fn(ExtractedPolicy(os.path.join(ROOT, "tests", "golden", "policy_kat.npz")), env)
    frames = episode_frames(args.envs, clip_length(env))
    arms = {"compact": BatchEvaluator(env, compact=True, sync_every=args.sync_every),
            "all_envs": BatchEvaluator(env, compact=False, sync_every=args.sync_every)}

    def one(ev):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = ev.run(act_fn, frames, args.max_steps)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    _, first = one(arms["compact"])                                     # warm-up evaluation (also the record the arms must reproduce)
    wall = {k: [] for k in arms}
    launched = {}
    for _ in range(args.runs):
        for k, ev in arms.items():
            dt, res = one(ev)
            wall[k].append(dt)
            launched[k] = ev.launched_env_steps
            assert torch.equal(res.ep_len, first.ep_len) and torch.equal(res.ep_ret, first.ep_ret), "%s differs from the first evaluation" % k
    ln = first.ep_len.cpu().numpy()
    stats = episode_statistics(first, env.ENV_CFG.MAX_EP_LENGTH)
    med = {k: statistics.median(v) for k, v in wall.items()}
    spread = {k: max(v) - min(v) for k, v in wall.items()}
    out = {"workload": "eval_walk_extracted_policy", "envs": args.envs, "max_steps": args.max_steps, "sync_every": args.sync_every,
           "runs": args.runs, "steps_run": int(first.steps_run),
           "wall_s": {k: {"median": round(med[k], 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in wall.items()},
           "episodes_per_s": {k: round(args.envs / med[k], 1) for k in arms},
           "speedup_compact": round(med["all_envs"] / med["compact"], 3),
           "compact_faster_beyond_spread": bool(med["all_envs"] - med["compact"] > max(spread.values())),
           "env_steps_live": int(ln.sum()), "env_steps_launched": launched,
           "survival": {"median_len": float(np.median(ln)), "frac_reached_cap": stats["frac_reached_cap"],
                        "ep_len_mean": stats["ep_len_mean"], "ep_rew_mean": round(stats["ep_rew_mean"], 4)}}

    if args.dashboard_episodes > 0:                                     # the path this replaces: one env, stepped from the host
        single = _FromFrame(DPEnv("walk"))
        model = _DashboardModel(act_fn, env.device)
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
    env.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
