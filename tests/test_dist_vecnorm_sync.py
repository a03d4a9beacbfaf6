"""One set of VecNormalize statistics over the ranks of a data-parallel PPO run, rehearsed with two gloo ranks on the
one GPU of the test box: fresh child processes, two in all per test."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _launch(port, tail, timeout=600):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port)] + tail
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r


@pytest.mark.gpu
def test_two_ranks_one_gpu_share_one_set_of_running_statistics(tmp_path):
    import torch
    from vecnorm_sync_ref import SyncRankRef, sync as ref_sync
    _launch(29541, [os.path.join(ROOT, "tests", "dist_vecnorm_sync_worker.py"), "--out", str(tmp_path)])
    a, b = (torch.load(os.path.join(tmp_path, "rank%d.pt" % k)) for k in (0, 1))
    its, T, N, D = 2, 6, 64, 67
    assert (a["world"], a["rank"], b["world"], b["rank"]) == (2, 0, 2, 1)
    for x in (a, b):
        assert x["rollout_path"] == "policy_forward" and len(x["its"]) == its and len(x["resets"]) == 1 and len(x["rows"]) == its * T
        # the synchronised entry points and nothing else of the normaliser; pack and merge once per rollout
        assert x["entries"] == ["dm_vecnorm_reset_sync"] + (["dm_vecnorm_step_sync"] * T + ["dm_vecnorm_sync_pack", "dm_vecnorm_sync_merge"]) * its
    for k in range(its):
        ia, ib = a["its"][k], b["its"][k]
        assert torch.equal(ia["state"], ib["state"]) and ia["state"].numel() == 2 * D + 4      # the 2 D + 4 doubles, bit for bit
        assert ia["clean"] and ib["clean"]
        assert torch.equal(ia["params"], ib["params"]) and torch.isfinite(ia["params"]).all()
        assert ia["sync_calls"] == ib["sync_calls"] == ia["stat"] == ib["stat"] == k + 1        # sync calls == iterations
        assert ia["grad_calls"] == ib["grad_calls"] == 3 * (k + 1)
        assert ia["finite"] and ib["finite"] and not torch.equal(ia["obs_norm"], ib["obs_norm"])
    # each rank's raw observations differ: other envs, other reset frames, other noise
    assert not torch.equal(a["resets"][0], b["resets"][0])
    assert all(not torch.equal(ra[0], rb[0]) for ra, rb in zip(a["rows"], b["rows"]))
    # the restatement, fed what each rank's normaliser was fed
    refs = [SyncRankRef(N, D) for _ in range(2)]
    for ref, x in zip(refs, (a, b)):
        ref.reset(x["resets"][0].numpy())
    rel = lambda g, r: float(np.max(np.where(g == r, 0.0, np.abs(g - r) / np.abs(r))))
    for k in range(its):
        for t in range(k * T, (k + 1) * T):
            for ref, x in zip(refs, (a, b)):
                obs, rew, done = (v.numpy() for v in x["rows"][t])
                assert obs.shape == (N, D) and rew.shape == (N,) and done.shape == (N,)
                ref.step(obs, rew, done)
        ref_sync(refs)
        worst = rel(a["its"][k]["state"].numpy(), refs[0].running_row())
        print("two ranks against the restatement, iteration %d: %.3g (bound 1e-10)" % (k, worst))
        assert worst <= 1e-10
    assert refs[0].obs_rms.count == pytest.approx(1e-4 + 2 * N * (1 + its * T), rel=1e-14)


@pytest.mark.gpu
def test_train_normalize_under_two_ranks(tmp_path):
    save = str(tmp_path / "policy.pt")
    r = _launch(29542, ["-m", "deepmimic_mujoco_amd.train", "--normalize", "--json", "--dist-backend", "gloo", "--motion", "spinkick", "--envs", "64",
                        "--horizon", "6", "--minibatch", "128", "--epochs", "1", "--total", "1536", "--save", save])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1                               # rank 0 alone reports
    rec = json.loads(lines[0])
    assert rec["normalize"] is True and rec["n_gpus"] == 2 and rec["iterations"] == 2
    assert rec["vecnorm_sync_calls"] == rec["iterations"] + 1          # once per rollout, and once more before rank 0 saves
    assert rec["grad_allreduce_calls"] == 3 * rec["iterations"]
    assert os.path.exists(save) and os.path.exists(save + ".vecnormalize")
    with np.load(save + ".vecnormalize", allow_pickle=False) as z:
        assert z["obs_mean"].shape == (67,) and np.isfinite(z["obs_var"]).all()
        assert float(z["obs_count"][0]) == pytest.approx(1e-4 + 2 * 64 * (1 + 2 * 6), rel=1e-12)      # both ranks' rows
