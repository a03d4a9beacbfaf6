"""Worker of tests/test_dist_vecnorm_sync.py (not collected by pytest): one rank of a 2-rank PPO run over gloo, both ranks on the one
GPU, through HipVecNormalize(sync_group="world") — one set of running statistics over the ranks.  Records the raw rows
the normaliser was fed, so that the test can feed them to the numpy restatement.  Launched by
`python -m torch.distributed.run --nproc-per-node 2 tests/dist_vecnorm_sync_worker.py --out DIR`."""
import argparse
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ITERATIONS, T, ENVS = 2, 6, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    torch.cuda.set_device(0)
    from deepmimic_mujoco_amd.deepmimic_env import HipDeepMimicVecEnv
    from deepmimic_mujoco_amd.ppo import PPO
    from deepmimic_mujoco_amd.vec_normalize import HipVecNormalize
    env = HipDeepMimicVecEnv(ENVS, motion="spinkick", device=0, seed=1234 + 7919 * rank)
    vn = HipVecNormalize(env, sync_group="world")
    resets, rows, entries = [], [], []
    inner_reset, inner_step, inner_call = env.reset_tensor, vn.normalize_step_, vn._call

    def reset_tensor(*a):
        obs = inner_reset(*a)
        resets.append(obs.detach().cpu().clone())
        return obs

    def normalize_step_(obs, rew, done, tobs, obs_out, rew_out, tobs_out):
        rows.append((obs.detach().cpu().clone(), rew.detach().cpu().clone(), done.detach().cpu().clone()))      # before the in-place transform
        return inner_step(obs, rew, done, tobs, obs_out, rew_out, tobs_out)

    def call(entry, *a):
        entries.append(entry)
        return inner_call(entry, *a)
    env.reset_tensor, vn.normalize_step_, vn._call = reset_tensor, normalize_step_, call
    ppo = PPO(vn, net_arch=(256, 128), n_steps=T, batch_size=128, n_epochs=1, seed=3)
    its = []
    for it in range(ITERATIONS):
        buf = ppo.collect_rollouts()
        torch.cuda.synchronize()
        state = vn._state.detach().cpu().clone()
        clean = bool(torch.equal(vn._state, vn._base)) and not bool(vn._acc.any())
        ppo.train(buf, generator=torch.Generator(device=ppo.device).manual_seed(17 + rank))
        torch.cuda.synchronize()
        its.append(dict(state=state, clean=clean, params=ppo.optimizer.flat_p.detach().cpu().clone(), sync_calls=vn.sync_calls,
                        stat=ppo.stats.get("vecnorm_sync_calls"), grad_calls=ppo.optimizer.calls, obs_norm=buf["obs"][0, :4].float().cpu().clone(),
                        finite=bool(torch.isfinite(buf["obs"].float()).all())))
    torch.save(dict(its=its, resets=resets, rows=rows, entries=entries, rollout_path=ppo.rollout_path(), world=vn._world, rank=vn._rank),
               os.path.join(args.out, "rank%d.pt" % rank))
    env.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
