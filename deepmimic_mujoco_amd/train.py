"""Training driver — the build's counterpart of src/sb3_ppo.py:244-314 / src/ppo.py:16-40.

    python -m deepmimic_mujoco_amd.train --motion walk --envs 4096 --horizon 32 --total 2000000
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m deepmimic_mujoco_amd.train ...
    python -m deepmimic_mujoco_amd.train --algo sac --motion getup_facedown --arch 1024,512 --envs 32   (src/sac_sb3.py)

One process per GPU; every rank owns `--envs` environments (sharded, no collective on the env path)
and a policy replica; gradients are all-reduced once per optimizer step (RCCL over xGMI).
"""
import argparse
import json
import os
import time

import torch
import torch.distributed as dist


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--algo", default="ppo", choices=["ppo", "sac"], help="sac: SB3 SAC of src/sac_sb3.py (one GPU, sac.py)")
    ap.add_argument("--buffer-size", type=int, default=5_000_000, help="--algo sac: replay transitions (src/sac_sb3.py)")
    ap.add_argument("--learning-starts", type=int, default=100, help="--algo sac: uniform-action env steps before learning")
    ap.add_argument("--gradient-steps", type=int, default=1, help="--algo sac: gradient steps per vec-env step")
    ap.add_argument("--n-step", type=int, default=1,
                    help="--algo sac: n-step returns, SB3's SAC(n_steps=): 1 .. 64, gathered on the device inside the sample launch")
    ap.add_argument("--motion", default="walk", help="clip name or comma list (multi-clip: env i -> clip i mod k)")
    ap.add_argument("--env", default="deep_mimic_mujoco", choices=["deep_mimic_mujoco", "dp_combined_env"],
                    help="env_name of src/sb3_ppo.py:247-248 (dp_combined_env: walk/run/getup state machine on humanoid3d)")
    ap.add_argument("--robot", default="humanoid3d", choices=["humanoid3d", "unitree_g1"],
                    help="src/sb3_ppo.py:251 trains unitree_g1 (its dp_combined_env is hard-wired to it)")
    ap.add_argument("--integrator", default="model", choices=["model", "RK4", "Euler"],
                    help="time integration of the training env and of the --eval-envs twin, on either robot: model = the XML's (RK4); "
                         "Euler = MuJoCo's semi-implicit Euler with implicit joint damping, one forward evaluation per step instead of four")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=32)          # 32 x 4096 = the reference's 4096 x 32 batch
    ap.add_argument("--epochs", type=int, default=20)           # src/sb3_ppo.py:259
    ap.add_argument("--minibatch", type=int, default=4096)      # :271
    ap.add_argument("--lr", type=float, default=4e-4)           # :260
    ap.add_argument("--arch", default="256,128")                # :265 ([1024,512] is BASELINE config 3)
    ap.add_argument("--total", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--bf16-buffer", action="store_true", help="store rollout obs/actions in bf16 (config 5)")
    ap.add_argument("--bf16-learner", action="store_true",
                    help="PPO(mlp_dtype=bfloat16): bf16 matrix-pipe products in the learner (dm_ppo_wide_grad for [256,128] .. [1024,512]-class "
                         "nets; fp32 master weights, loss, gradients and Adam) — 106 us instead of 378 us per optimizer step on MLP(1024,512)")
    ap.add_argument("--bf16x3-learner", action="store_true",
                    help="PPO(mlp_dtype=\"bf16x3\"): the reference's fp32 accuracy on the bf16 matrix pipe for nets beyond the fused fp32 "
                         "[256,128] class (dm_ppo_wide3_grad: split operands, three MFMAs per product); not with --bf16-learner")
    ap.add_argument("--save", default="")
    ap.add_argument("--sub-batches", type=int, default=1,
                    help="> 1: the env batch as that many engines, each on its own probed concurrent HIP stream (double-buffered rollout: "
                         "one sub-batch simulates while the policy runs on another; Unitree G1: 2 is ~10 %% faster than 1)")
    ap.add_argument("--rollout-graph", action="store_true", help="with --sub-batches > 1: capture the rollout as one hipGraph")
    ap.add_argument("--json", action="store_true", help="print a JSON throughput summary on rank 0")
    ap.add_argument("--eval-every", type=int, default=0, help="eval dashboard every N global steps (src/sb3_ppo.py:313 EVAL_N); 0 = off")
    ap.add_argument("--eval-envs", type=int, default=0,
                    help="> 0: batched deterministic evaluation (evaluation.py) on that many auto_reset=False envs on rank 0: at every "
                         "--eval-every point (eval_batch.csv) and once after training (\"eval\" of the --json line); finished envs leave "
                         "the launches on either robot (compact=\"all\"); 0 = off")
    ap.add_argument("--renderer", default="stick", choices=["stick", "raycast"],
                    help="frames of the eval dashboard: host-side stick figure, or ray-cast on the device (raycast.py)")
    ap.add_argument("--debug-log", default="", metavar="DIR",
                    help="keep the reference's episode_debug_log on the device (debug_log.py): the last --debug-log-steps steps of every env; "
                         "after each rollout the rings of envs whose step ended with a sim error or an out-of-bounds observation are "
                         "written to DIR as deepmimic_episode_<time>_env<i>.json")
    ap.add_argument("--debug-log-steps", type=int, default=64, help="--debug-log: steps kept per env")
    ap.add_argument("--normalize", action="store_true",
                    help="train through HipVecNormalize (SB3's VecNormalize with the running statistics on the device, vec_normalize.py): "
                         "PPO's env is wrapped; --algo sac keeps the raw env, stores raw transitions and normalises every sampled minibatch "
                         "inside the gather launch (SAC(normalizer=)); --save P also writes P.vecnormalize, evaluations go through the "
                         "frozen statistics; with several ranks (PPO) every rank folds its own rows into the agreed statistics and the "
                         "ranks merge them once per rollout (HipVecNormalize(sync_group=\"world\"): two launches around one small "
                         "all-reduce), P.vecnormalize is rank 0's after a final merge")
    ap.add_argument("--norm-clip-obs", type=float, default=10.0, help="--normalize: clip_obs")
    ap.add_argument("--norm-clip-reward", type=float, default=10.0, help="--normalize: clip_reward")
    ap.add_argument("--no-norm-reward", action="store_true", help="--normalize: observations only (norm_reward=False)")
    ap.add_argument("--run-name", default="run")
    ap.add_argument("--eval-dir", default="~/deep_mimic")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="gloo + several ranks on one GPU only rehearses the multi-rank path")
    return ap


def _eval_batch_env(args, motions, local_rank):
    """The auto_reset=False twin of the training env with --eval-envs envs (one engine)."""
    from .deepmimic_env import HipDeepMimicVecEnv
    if args.env == "dp_combined_env":
        from .combined_env import HipCombinedVecEnv
        return HipCombinedVecEnv(args.eval_envs, robot=args.robot, device=local_rank, seed=4321, auto_reset=False, integrator=args.integrator)
    if args.robot == "unitree_g1":
        return HipDeepMimicVecEnv(args.eval_envs, motion=motions[0], robot="unitree_g1", device=local_rank, seed=4321, auto_reset=False,
                                  integrator=args.integrator)
    return HipDeepMimicVecEnv(args.eval_envs, motion=motions if len(motions) > 1 else motions[0], device=local_rank, seed=4321,
                              auto_reset=False, integrator=args.integrator)


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.bf16_learner and args.bf16x3_learner:
        ap.error("--bf16-learner and --bf16x3-learner are mutually exclusive")
    if args.eval_envs < 0:
        ap.error("--eval-envs must be >= 0")
    if not 1 <= args.n_step <= 64 or (args.n_step != 1 and args.algo != "sac"):
        ap.error("--n-step takes 1 .. 64 and belongs to --algo sac")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.algo == "sac" and world > 1:
        ap.error("--algo sac runs one learner on one GPU (SB3's SAC has no data-parallel mode): launch it without torch.distributed")
    if world > 1 and "RANK" not in os.environ:
        ap.error("WORLD_SIZE=%d without RANK: several ranks are started by torch.distributed.run (see the module docstring)" % world)
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group("gloo")
            local_rank = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    rank = dist.get_rank() if world > 1 else 0

    from .deepmimic_env import HipDeepMimicVecEnv
    from .ppo import PPO

    motions = args.motion.split(",")
    sb = args.sub_batches if args.envs % args.sub_batches == 0 else 1
    if args.env == "dp_combined_env":                                   # src/sb3_ppo.py:276-278
        from .combined_env import HipCombinedVecEnv
        env = HipCombinedVecEnv(args.envs, robot=args.robot, device=local_rank, seed=1234 + 7919 * rank, integrator=args.integrator,
                                **({"sub_batches": sb} if args.robot == "unitree_g1" else {}))      # (the humanoid3d variant has one engine)
    elif args.robot == "unitree_g1":                                    # src/sb3_ppo.py:274-275 with robot = "unitree_g1"
        env = HipDeepMimicVecEnv(args.envs, motion=motions[0], robot="unitree_g1", device=local_rank, seed=1234 + 7919 * rank, sub_batches=sb,
                                 integrator=args.integrator)
    else:
        env = HipDeepMimicVecEnv(args.envs, motion=motions if len(motions) > 1 else motions[0], device=local_rank,
                                 seed=1234 + 7919 * rank, sub_batches=sb, integrator=args.integrator)
    # before the first rollout: a captured rollout graph holds the recorder's launches
    dlog = env.enable_debug_log(steps=args.debug_log_steps) if args.debug_log else None
    dlog_dir = os.path.expanduser(args.debug_log) if world == 1 else os.path.join(os.path.expanduser(args.debug_log), "rank%d" % rank)
    if args.algo == "sac":
        return _train_sac(args, env, motions, local_rank)
    vn = None
    if args.normalize:
        from .vec_normalize import HipVecNormalize
        env = vn = HipVecNormalize(env, norm_reward=not args.no_norm_reward, clip_obs=args.norm_clip_obs, clip_reward=args.norm_clip_reward,
                                   sync_group="world" if world > 1 else None)
    ppo = PPO(env, net_arch=tuple(int(x) for x in args.arch.split(",")), n_steps=args.horizon,
              batch_size=args.minibatch, n_epochs=args.epochs, learning_rate=args.lr, seed=args.seed,
              buffer_dtype=torch.bfloat16 if args.bf16_buffer else torch.float32, rollout_graph=args.rollout_graph,
              mlp_dtype=torch.bfloat16 if args.bf16_learner else "bf16x3" if args.bf16x3_learner else torch.float32)
    hist = []
    dash = None
    batch_env = _eval_batch_env(args, motions, local_rank) if args.eval_envs > 0 and rank == 0 else None
    if args.eval_every > 0 and rank == 0:                               # src/sb3_ppo.py:273-313: one eval env next to the batch
        from .eval_dashboard import EvalDashboardCallback
        if args.env == "dp_combined_env":
            from .combined_env import DPCombinedEnv
            eval_env = DPCombinedEnv(robot=args.robot, device=local_rank, renderer=args.renderer)
        else:
            from .deepmimic_env import DPEnv
            eval_env = DPEnv(motions[0], robot=args.robot, device=local_rank, renderer=args.renderer)
        dash = EvalDashboardCallback(eval_env, args.motion + "_" + args.run_name, every_n_global_steps=args.eval_every, out_root=args.eval_dir,
                                     batch_env=batch_env)

    def _cb(p):
        hist.append(dict(p.stats, timesteps=p.num_timesteps * world))
        if dlog is not None:
            dlog.dump(dlog_dir)
        if dash is not None:
            dash(p)
        return True
    t0 = time.perf_counter()
    ppo.learn(args.total, log_interval=0 if args.json else 1, callback=_cb)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if vn is not None and vn.synced and args.save:
        vn.sync()                                                       # every rank: the saved statistics are the agreed ones
    if rank == 0:
        if args.save:
            ppo.save(os.path.expanduser(args.save))
            if vn is not None:
                vn.save(os.path.expanduser(args.save) + ".vecnormalize")
        final_eval = None
        if batch_env is not None:                                       # the final policy, one deterministic episode per start frame
            from .evaluation import evaluation_record
            final_eval = evaluation_record(ppo, batch_env, ppo.num_timesteps * world, normalizer=vn)
            if not args.json:
                print("final evaluation: %(episodes)d episodes  ep_rew_mean %(ep_rew_mean).3f +- %(ep_rew_std).3f  ep_len_mean %(ep_len_mean).1f  "
                      "reached the cap %(frac_reached_cap).2f" % final_eval, flush=True)
        if args.json:
            steady = hist[1:] if len(hist) > 1 else hist
            roll = sum(h["rollout_s"] for h in steady) / len(steady)
            trn = sum(h["train_s"] for h in steady) / len(steady)
            per_it = args.envs * args.horizon * world
            print(json.dumps({"workload": "ppo", "integrator": args.integrator, "n_gpus": world, "envs_per_gpu": args.envs, "horizon": args.horizon,
                              "arch": args.arch, "epochs": args.epochs, "minibatch": args.minibatch,
                              "buffer_dtype": str(ppo.buffer_dtype).replace("torch.", ""), "rollout_path": ppo.rollout_path(),
                              "normalize": vn is not None,
                              "learner": ppo.learner_path(),
                              "iterations": len(hist), "rollout_env_steps_per_s": per_it / roll,
                              "train_s_per_iter": trn, "overall_env_steps_per_s": per_it / (roll + trn),
                              "mean_reward_last": hist[-1]["mean_reward"], "wall_s": dt,
                              "grad_allreduce_calls": ppo.grad_sync.calls,
                              "vecnorm_sync_calls": vn.sync_calls if vn is not None else 0,
                              "ep_rew_mean": hist[-1]["ep_rew_mean"], "ep_len_mean": hist[-1]["ep_len_mean"],
                              "explained_variance": hist[-1]["explained_variance"], "episodes": hist[-1]["episodes"],
                              "curve": [(h["timesteps"], h["ep_rew_mean"], h["ep_len_mean"]) for h in hist[::max(1, len(hist) // 200)]],
                              **({"eval": final_eval} if final_eval is not None else {}),
                              **({"debug_log": dict(zip(("captures", "triggers"), dlog.counts()), files=dlog.files)} if dlog is not None else {})}))
    if batch_env is not None:
        batch_env.close()
    env.close()
    if world > 1:
        dist.destroy_process_group()


def _train_sac(args, env, motions, local_rank):
    """src/sac_sb3.py: SAC(MlpPolicy, net_arch=[1024, 512] by --arch, buffer_size) with SB3's other defaults; one learner."""
    from .sac import SAC
    vn = None
    if args.normalize:                              # on the inner env: SAC normalises at replay-sample time, not at store time
        from .vec_normalize import HipVecNormalize
        vn = HipVecNormalize(env, norm_reward=not args.no_norm_reward, clip_obs=args.norm_clip_obs, clip_reward=args.norm_clip_reward)
    sac = SAC(env, net_arch=tuple(int(x) for x in args.arch.split(",")), buffer_size=args.buffer_size,
              learning_starts=args.learning_starts, gradient_steps=args.gradient_steps, seed=args.seed, normalizer=vn, n_steps=args.n_step)
    hist = []
    dash = None
    batch_env = _eval_batch_env(args, motions, local_rank) if args.eval_envs > 0 else None
    if args.eval_every > 0:
        from .eval_dashboard import EvalDashboardCallback
        if args.env == "dp_combined_env":
            from .combined_env import DPCombinedEnv
            eval_env = DPCombinedEnv(robot=args.robot, device=local_rank, renderer=args.renderer)
        else:
            from .deepmimic_env import DPEnv
            eval_env = DPEnv(motions[0], robot=args.robot, device=local_rank, renderer=args.renderer)
        dash = EvalDashboardCallback(eval_env, args.motion + "_" + args.run_name, every_n_global_steps=args.eval_every, out_root=args.eval_dir,
                                     batch_env=batch_env)

    dlog = getattr(env, "debug_log", None)          # --debug-log: enable_debug_log() ran in main

    def _cb(m):
        hist.append(dict(m.stats))
        if dlog is not None:
            dlog.dump(os.path.expanduser(args.debug_log))
        if not args.json:
            print("steps %(total_timesteps)d  ep_rew_mean %(ep_rew_mean).3f  ep_len_mean %(ep_len_mean).1f  critic %(critic_loss).4f  "
                  "actor %(actor_loss).4f  ent_coef %(ent_coef).4f  fps %(fps).0f" % m.stats, flush=True)
        if dash is not None:
            dash(m)
        return True
    t0 = time.perf_counter()
    # stats (one synchronisation) every ~100 k transitions: the loop in between never waits for the device
    sac.learn(args.total, callback=_cb, log_interval=max(1, 100_000 // env.num_envs))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if args.save:
        sac.save(os.path.expanduser(args.save))
        if vn is not None:
            vn.save(os.path.expanduser(args.save) + ".vecnormalize")
    final_eval = None
    if batch_env is not None:
        from .evaluation import evaluation_record
        final_eval = evaluation_record(sac, batch_env, sac.num_timesteps, normalizer=vn)
        batch_env.close()
    if args.json:
        last = hist[-1] if hist else {}
        print(json.dumps({"workload": "sac", "integrator": args.integrator, "envs": env.num_envs, "arch": args.arch, "buffer_size": args.buffer_size,
                          "gradient_steps": args.gradient_steps, "n_steps": sac.n_steps, "normalize": vn is not None, "total_timesteps": sac.num_timesteps, "n_updates": sac._n_updates,
                          "env_steps_per_s": sac.num_timesteps / dt, "wall_s": dt,
                          "ep_rew_mean": last.get("ep_rew_mean"), "ep_len_mean": last.get("ep_len_mean"),
                          "critic_loss": last.get("critic_loss"), "actor_loss": last.get("actor_loss"), "ent_coef": last.get("ent_coef"),
                          "curve": [(h["total_timesteps"], h["ep_rew_mean"]) for h in hist[::max(1, len(hist) // 200)]],
                          **({"eval": final_eval} if final_eval is not None else {}),
                          **({"debug_log": dict(zip(("captures", "triggers"), dlog.counts()), files=dlog.files)} if dlog is not None else {})}))
    env.close()


if __name__ == "__main__":
    main()
