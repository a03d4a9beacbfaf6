"""SHA-256 digests of what PPO's rollout paths and one update compute, for comparing two versions of the package bit for bit.

Public API only, so the same file runs against any version that has ``PPO.rollout_path()``.  Per case: build env and PPO from fixed
seeds, two ``collect_rollouts()``, one ``train()``, one more ``collect_rollouts()``; print ``rollout_path()``, a digest per rollout
over obs, act, rew, done, val, logp, adv, ret, ``stats["episodes"]`` after each, and a digest of the flat parameters after the
update.  Humanoid `walk`, N = 256, T = 16, [256,128], minibatch 1024, one epoch unless the case says otherwise.

    python scripts/rollout_digest.py [--cases a,b] [--out digest.json] [--dump tensors.pt]
    python scripts/rollout_digest.py --compare a.pt b.pt        # largest |a - b| per case and tensor of two --dump files

One JSON line per case, then one JSON object with all of them (also written to ``--out``).
"""
import argparse
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KEYS = ("obs", "act", "rew", "done", "val", "logp", "adv", "ret")
BF = torch.bfloat16
CASES = {   # name: (PPO keywords, env sub_batches, env keywords)
    "policy_forward": (dict(), 1, {}),
    "policy_forward_sub2_host": (dict(rollout_graph=False), 2, {}),
    "policy_forward_sub2_captured": (dict(), 2, {}),
    "sample_store_sub2_host": (dict(fused_policy=False, rollout_graph=False), 2, {}),
    "sample_store_sub2_captured": (dict(fused_policy=False), 2, {}),
    "plain_sub2_captured": (dict(fused_policy=False, fused_rollout=False), 2, {}),
    "sample_store": (dict(fused_policy=False), 1, {}),
    "plain": (dict(fused_policy=False, fused_rollout=False), 1, {}),
    "policy_forward_bf16_buffers": (dict(buffer_dtype=BF), 1, {}),
    "sample_store_bf16_buffers": (dict(fused_policy=False, buffer_dtype=BF), 1, {}),
    "g1_policy_forward": (dict(), 1, dict(robot="unitree_g1")),
    "wide_1024_512_bf16": (dict(net_arch=(1024, 512), mlp_dtype=BF, batch_size=4096), 1, {}),
}


def sha(tensors):
    h = hashlib.sha256()
    for t in tensors:
        t = t.detach().contiguous().cpu()
        h.update(t.view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def run_case(name, dump):
    from deepmimic_mujoco_amd.deepmimic_env import HipDeepMimicVecEnv
    from deepmimic_mujoco_amd.ppo import PPO
    kw, K, ekw = CASES[name]
    dev = torch.device("cuda", 0)
    env = HipDeepMimicVecEnv(256, motion="walk", seed=3, **dict(ekw, **({"sub_batches": K} if K > 1 else {})))
    ppo = PPO(env, **dict(dict(net_arch=(256, 128), n_steps=16, batch_size=1024, n_epochs=1, seed=0), **kw))
    rec = {"case": name, "rollout_path": ppo.rollout_path(), "rollouts": [], "episodes": []}
    for i in range(3):
        buf = ppo.collect_rollouts()
        torch.cuda.synchronize()
        rec["rollouts"].append(sha(buf[k] for k in KEYS))
        rec["episodes"].append(int(ppo.stats["episodes"]))
        if dump is not None:
            dump[name + "/rollout%d" % i] = {k: buf[k].detach().float().cpu().clone() for k in KEYS}
        if i == 1:
            ppo.train(buf, generator=torch.Generator(device=dev).manual_seed(8))
            torch.cuda.synchronize()
            flat = torch.cat([p.detach().reshape(-1) for p in ppo.policy.parameters()])
            rec["params"] = sha([flat])
            if dump is not None:
                dump[name + "/params"] = {"flat": flat.cpu().clone()}
    env.close()
    return rec


def compare(a, b):
    a, b = torch.load(a), torch.load(b)
    out = {}
    for key in a:
        d = {k: float((a[key][k].double() - b[key][k].double()).abs().max()) for k in a[key]}
        out[key] = {k: v for k, v in d.items() if v != 0.0}
    print(json.dumps({"max_abs_diff_nonzero": {k: v for k, v in out.items() if v}, "compared": len(out)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out")
    ap.add_argument("--dump")
    ap.add_argument("--compare", nargs=2)
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    if not torch.cuda.is_available():
        raise SystemExit("rollout_digest.py runs the GPU paths; no GPU is visible")
    dump = {} if args.dump else None
    recs = []
    for name in args.cases.split(","):
        recs.append(run_case(name, dump))
        print(json.dumps(recs[-1]), flush=True)
    out = {"workload": "rollout_digest", "device": torch.cuda.get_device_name(0), "cases": recs}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    if args.dump:
        torch.save(dump, args.dump)


if __name__ == "__main__":
    main()
