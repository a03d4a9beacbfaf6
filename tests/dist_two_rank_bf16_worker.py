"""Worker of tests/test_bf16_buffers_gpu.py (not collected by pytest): one rank of a 2-rank PPO run over gloo with both ranks on the
one GPU and bf16 rollout buffers (PPO(buffer_dtype=torch.bfloat16), BASELINE config 5's storage type) — the rollout on the one-launch
policy path, the learner on the two captured graphs around the all-reduce, fed by dm_ppo_gather_bf16.  Launched by
`python -m torch.distributed.run --nproc-per-node 2 tests/dist_two_rank_bf16_worker.py --out DIR`."""
import argparse
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--arch", default="256,128")
    ap.add_argument("--bf16", action="store_true", help="PPO(mlp_dtype=torch.bfloat16): the dm_ppo_wide_grad learner")
    args = ap.parse_args()
    arch = tuple(int(x) for x in args.arch.split(","))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    torch.cuda.set_device(0)
    from deepmimic_mujoco_amd.deepmimic_env import HipDeepMimicVecEnv
    from deepmimic_mujoco_amd.ppo import PPO
    env = HipDeepMimicVecEnv(64, motion="spinkick", device=0, seed=1234 + 7919 * rank)
    ppo = PPO(env, net_arch=arch, n_steps=6, batch_size=128, n_epochs=1, seed=3, buffer_dtype=torch.bfloat16,
              mlp_dtype=torch.bfloat16 if args.bf16 else torch.float32)
    assert not args.bf16 or ppo._wide_ok
    params0 = ppo.optimizer.flat_p.detach().cpu().clone()
    buf = ppo.collect_rollouts()
    gen = torch.Generator(device=ppo.device).manual_seed(17 + rank)
    ppo.train(buf, generator=gen)
    torch.cuda.synchronize()
    dg = getattr(ppo, "_dg", None)
    gather_ok = False
    if dg is not None:      # the static minibatch holds the last gathered rows, widened exactly
        gather_ok = all(torch.equal(dg["gin"][k], dg["flat"][k][dg["idx"]].float()) for k in ("obs", "act", "adv", "ret", "logp"))
    res = dict(params=ppo.optimizer.flat_p.detach().cpu().clone(), params0=params0, calls=ppo.optimizer.calls, used_dist_graph=dg is not None,
               gather_ok=gather_ok, buffer_dtype=str(buf["obs"].dtype), rollout_path=ppo.rollout_path(), loss=ppo.stats["loss"],
               obs0=buf["obs"][0, :4].float().cpu().clone())
    env.close()
    torch.save(res, os.path.join(args.out, "rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
