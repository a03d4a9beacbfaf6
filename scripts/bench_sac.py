"""SAC throughput: microseconds per gradient step (B = 256, [1024,512], humanoid3d 67 / 28) of the torch learner, the fused
learner run eagerly and the captured fused learner, and `learn` env-steps/s on the humanoid walk env at 32 and 4 096 envs.
Prints one JSON line.

    python scripts/bench_sac.py [--steps 200] [--learn-steps 300] [--one-step-only]

--one-step-only: a few captured gradient steps and nothing else (for `rocprofv3 --kernel-trace --stats`).
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class _Box:
    def __init__(self, lo, hi, n):
        import numpy as np
        self.low, self.high, self.shape = np.full(n, lo, np.float32), np.full(n, hi, np.float32), (n,)


class RandomEnv:
    """Random observations / rewards with the step_tensor surface: fills the ring for the gradient-step timings."""

    def __init__(self, n, D, A):
        self.num_envs, self.device = n, torch.device("cuda")
        self.observation_space, self.action_space = _Box(-1, 1, D), _Box(-1, 1, A)
        self.out = dict(obs=torch.randn(n, D, device="cuda"), rew=torch.randn(n, device="cuda"),
                        done=(torch.rand(n, device="cuda") < 0.05).to(torch.uint8), terminal_obs=torch.randn(n, D, device="cuda"))

    def reset_tensor(self):
        return self.out["obs"]

    def step_tensor(self, actions):
        return self.out


def time_steps(fn, steps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--learn-steps", type=int, default=300, help="vec-env steps of each learn measurement (after learning_starts)")
    ap.add_argument("--one-step-only", action="store_true")
    args = ap.parse_args()
    from deepmimic_mujoco_amd.sac import SAC

    res = {"workload": "sac", "batch_size": 256, "arch": "1024,512", "obs_dim": 67, "act_dim": 28}
    env = RandomEnv(256, 67, 28)
    sacs = {}
    for name, fused in (("torch", False), ("fused", True)):
        s = SAC(env, net_arch=(1024, 512), batch_size=256, learning_starts=10 ** 9, buffer_size=256 * 64, fused=fused)
        for _ in range(64):
            s.env_step()
        sacs[name] = s
    if args.one_step_only:
        s = sacs["fused"]
        s.train(1)
        torch.cuda.synchronize()
        for _ in range(10):
            s._graph.replay()
        torch.cuda.synchronize()
        print(json.dumps({"workload": "sac", "captured_steps": 11}))
        return
    res["us_per_grad_step_torch"] = time_steps(sacs["torch"].gradient_step_torch, args.steps)
    res["us_per_grad_step_fused_eager"] = time_steps(sacs["fused"].gradient_step_fused, args.steps)
    sacs["fused"]._capture()
    res["us_per_grad_step_captured"] = time_steps(sacs["fused"]._graph.replay, args.steps)
    res["captured_over_torch"] = res["us_per_grad_step_captured"] / res["us_per_grad_step_torch"]

    from deepmimic_mujoco_amd.deepmimic_env import HipDeepMimicVecEnv
    for n in (32, 4096):
        venv = HipDeepMimicVecEnv(n, motion="walk", seed=1234)
        s = SAC(venv, net_arch=(1024, 512), buffer_size=1_000_000, learning_starts=100)
        s.learn(max(200, 2 * n), log_interval=0)        # past learning_starts, graph captured
        torch.cuda.synchronize()
        t0, n0 = time.perf_counter(), s.num_timesteps
        s.learn(n0 + args.learn_steps * n, log_interval=0)
        torch.cuda.synchronize()
        res["learn_env_steps_per_s_%d" % n] = (s.num_timesteps - n0) / (time.perf_counter() - t0)
        venv.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
