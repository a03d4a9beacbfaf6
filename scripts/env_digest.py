"""SHA-256 digests of what the environment classes return through their numpy surface, for comparing two versions of the package
bit for bit.

Public API only, so the same file runs against any version that has the eight classes.  Per case: ``seed(3)`` (batch classes) or
``random.seed(0)`` (single-env classes), ``reset()``, 40 ``step(actions)`` calls with actions drawn uniformly inside
``action_space`` from ``np.random.default_rng(1)`` (random torques make envs fall: auto-reset and ``terminal_observation`` are on
the path), then ``render()``.  Printed per case: one digest over obs, rew, done and the fully materialised infos of every step,
one digest of the rendered frame, and whether the engine state survived ``render()`` bit for bit (asserted).  Single-env cases
reset when an episode ends and finish with one ``force_state`` step.

    python scripts/env_digest.py [--cases a,b] [--out digest.json] [--dump arrays.npz]
    python scripts/env_digest.py --compare a.npz b.npz        # largest |a - b| per case and array of two --dump files

One JSON line per case, then one JSON object with all of them (also written to ``--out``).
"""
import argparse
import hashlib
import json
import os
import random
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, STEPS = 64, 40


def _batch(cls, *a, **kw):
    def make():
        from deepmimic_mujoco_amd import combined_env, deepmimic_env, g1
        mod = {"HipDeepMimicVecEnv": deepmimic_env, "HipCombinedVecEnv": combined_env}.get(cls, g1)
        return getattr(mod, cls)(N, *a, **kw)
    return make


def _single(cls, **kw):
    def make():
        from deepmimic_mujoco_amd import combined_env, deepmimic_env
        return getattr(deepmimic_env if cls == "DPEnv" else combined_env, cls)(**kw)
    return make


BATCH = {
    "HipDeepMimicVecEnv": _batch("HipDeepMimicVecEnv", motion="walk"),
    "HipDeepMimicVecEnv_sub2": _batch("HipDeepMimicVecEnv", motion="walk", sub_batches=2),
    "HipDeepMimicVecEnv_walk_run": _batch("HipDeepMimicVecEnv", motion=["walk", "run"]),
    "HipCombinedVecEnv_humanoid3d": _batch("HipCombinedVecEnv", robot="humanoid3d"),
    "HipG1VecEnv": _batch("HipG1VecEnv", motion="walk"),
    "HipG1VecEnv_sub2": _batch("HipG1VecEnv", motion="walk", sub_batches=2),
    "HipG1CombinedVecEnv": _batch("HipG1CombinedVecEnv"),
    "HipG1CombinedVecEnv_sub2": _batch("HipG1CombinedVecEnv", sub_batches=2),
}
SINGLE = {   # name: (constructor, steps)
    "DPEnv": (_single("DPEnv", motion="walk"), STEPS),
    "DPEnv_no_mocap": (_single("DPEnv", load_mocap=False), 5),
    "G1DPEnv": (_single("DPEnv", motion="walk", robot="unitree_g1"), STEPS),
    "DPCombinedEnv_humanoid3d": (_single("DPCombinedEnv", robot="humanoid3d"), STEPS),
    "G1CombinedEnv": (_single("DPCombinedEnv"), STEPS),
}


def _feed_info(h, info):
    for k in sorted(info):
        v = info[k]
        h.update(k.encode())
        if isinstance(v, np.ndarray):
            h.update(np.ascontiguousarray(v).tobytes())
        elif isinstance(v, float):
            h.update(struct.pack("<d", v))
        else:
            h.update(repr(v).encode())
    h.update(b"|")


def _feed(h, rec, obs, rew, done, infos):
    obs, rew, done = np.asarray(obs), np.asarray(rew, np.float64), np.asarray(done, bool)
    for a in (obs, rew, done):
        h.update(np.ascontiguousarray(a).tobytes())
    for info in infos:
        _feed_info(h, info)
    rec["obs"].append(obs.astype(np.float64))
    rec["rew"].append(rew)
    rec["done"].append(done)


def _actions(rng, space, n=None):
    shape = space.shape if n is None else (n,) + space.shape
    return rng.uniform(space.low, space.high, shape).astype(np.float32)


def _render(env, engine, rec):
    before = [t.clone() for t in engine.get_state()]
    frame = np.ascontiguousarray(env.render())
    after = engine.get_state()
    assert all(bool((a == b).all()) for a, b in zip(before, after)), "render() changed the engine state"
    rec["frame"] = frame
    return hashlib.sha256(frame.tobytes()).hexdigest()


def run_batch(name):
    env = BATCH[name]()
    env.seed(3)
    rng, h, rec = np.random.default_rng(1), hashlib.sha256(), {"obs": [], "rew": [], "done": []}
    obs = env.reset()
    h.update(np.ascontiguousarray(obs).tobytes())
    n_done = 0
    for _ in range(STEPS):
        obs, rew, done, infos = env.step(_actions(rng, env.action_space, env.num_envs))
        _feed(h, rec, obs, rew, done, list(infos))
        n_done += int(done.sum())
    out = {"case": name, "class": type(env).__name__, "steps": h.hexdigest(), "episodes_ended": n_done,
           "frame": _render(env, env.engine, rec)}
    env.close()
    return out, rec


def run_single(name):
    make, steps = SINGLE[name]
    random.seed(0)
    env = make()
    random.seed(0)
    rng, h, rec = np.random.default_rng(1), hashlib.sha256(), {"obs": [], "rew": [], "done": []}
    obs = env.reset()
    h.update(np.ascontiguousarray(obs).tobytes())
    n_done = 0
    for _ in range(steps):
        obs, rew, done, info = env.step(_actions(rng, env.action_space))
        _feed(h, rec, obs, rew, done, [info])
        if done:
            n_done += 1
            h.update(np.ascontiguousarray(env.reset()).tobytes())
    state = [t[0].double().cpu().numpy() for t in env._eng.get_state()[:2]]
    state[1] = state[1] * 0.5                               # a state the engine is not in already
    obs, rew, done, info = env.step(_actions(rng, env.action_space), force_state=tuple(state))
    _feed(h, rec, obs, rew, done, [info])
    out = {"case": name, "class": type(env).__name__, "steps": h.hexdigest(), "episodes_ended": n_done,
           "counters": [int(env.episode_length), float(env.episode_reward)], "frame": _render(env, env._eng, rec)}
    env.close()
    return out, rec


def compare(a, b):
    a, b = np.load(a), np.load(b)
    diff = {k: float(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max()) for k in a.files}
    print(json.dumps({"max_abs_diff_nonzero": {k: v for k, v in diff.items() if v != 0.0}, "compared": len(diff)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(list(BATCH) + list(SINGLE)))
    ap.add_argument("--out")
    ap.add_argument("--dump")
    ap.add_argument("--compare", nargs=2)
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("env_digest.py steps the GPU engines; no GPU is visible")
    recs, dump = [], {}
    for name in args.cases.split(","):
        out, rec = (run_batch if name in BATCH else run_single)(name)
        recs.append(out)
        print(json.dumps(out), flush=True)
        for k, v in rec.items():
            dump[name + "/" + k] = np.asarray(v)
    out = {"workload": "env_digest", "device": torch.cuda.get_device_name(0), "cases": recs}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    if args.dump:
        np.savez_compressed(args.dump, **dump)


if __name__ == "__main__":
    main()
