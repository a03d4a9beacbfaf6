"""bench.py --gpus N is its own launcher: N ranks rendezvous, and a mismatch is refused, without a GPU."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env=None, timeout=240):
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, env=e, timeout=timeout)


def test_bench_gpus_2_launches_two_ranks_by_itself():
    r = _run(["--gpus", "2", "--dist-backend", "gloo", "--dry-launch"])
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line == {"dry_launch": True, "n_gpus": 2, "ranks_seen": [0, 1], "self_launched": True}


def test_bench_refuses_a_world_size_that_is_not_gpus():
    r = _run(["--gpus", "8", "--dry-launch"], env={"RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "must agree" in (r.stderr + r.stdout)


def test_bench_refuses_to_fold_ranks_when_gpus_are_missing():
    """No GPU here: `--gpus 2` (nccl) must exit non-zero instead of reporting n_gpus 1."""
    import torch
    if torch.cuda.device_count() >= 2:
        return
    r = _run(["--gpus", "2"])
    assert r.returncode != 0 and "never folded" in (r.stderr + r.stdout)


def _fake_outputs(n, obs_dim=67, terms_dim=5):
    import torch
    g = torch.Generator().manual_seed(0)
    return dict(obs=torch.randn(n, obs_dim, generator=g), rew=torch.rand(n, generator=g),
                done=(torch.rand(n, generator=g) < 0.1).to(torch.uint8), terms=torch.rand(n, terms_dim, generator=g),
                reason=torch.randint(0, 4, (n,), dtype=torch.int32, generator=g), terminal_obs=torch.randn(n, obs_dim, generator=g))


def test_dump_outputs_writes_every_output_as_float32(tmp_path):
    """--dump-outputs: one float32 .npy per array dm_step returns, values unchanged."""
    import numpy as np
    import bench
    out = _fake_outputs(4096)
    bench.dump_outputs(out, str(tmp_path), 0, 1)
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(k + ".npy" for k in out)
    for k, v in out.items():
        a = np.load(tmp_path / (k + ".npy"))
        assert a.dtype == np.float32 and a.shape == tuple(v.shape)
        assert np.array_equal(a, v.float().numpy())


def test_dump_outputs_samples_fixed_rows_under_64_mb(tmp_path):
    """Outputs larger than the 64 MB cap: the same seeded rows every time, their indices stored beside them; with several
    ranks each rank writes its own prefixed files within its share of the cap."""
    import numpy as np
    import bench
    n = 160000                                   # 160 k envs x 568 B per row = 91 MB of outputs
    out = _fake_outputs(n)
    bench.dump_outputs(out, str(tmp_path / "a"), 0, 1)
    bench.dump_outputs(out, str(tmp_path / "b"), 0, 1)
    total = sum(p.stat().st_size for p in (tmp_path / "a").iterdir())
    assert total <= bench.DUMP_BYTES
    idx = np.load(tmp_path / "a" / "env_index.npy")
    assert idx.dtype == np.float64 and 0 < len(idx) < n and np.all(np.diff(idx) > 0)
    assert np.array_equal(idx, np.load(tmp_path / "b" / "env_index.npy"))
    rows = idx.astype(np.int64)
    for k, v in out.items():
        assert np.array_equal(np.load(tmp_path / "a" / (k + ".npy")), v.float().numpy()[rows])
    bench.dump_outputs(out, str(tmp_path / "c"), 1, 2)
    names = sorted(p.name for p in (tmp_path / "c").iterdir())
    assert names == sorted("rank1_" + k + ".npy" for k in list(out) + ["env_index"])
    assert sum(p.stat().st_size for p in (tmp_path / "c").iterdir()) <= bench.DUMP_BYTES // 2


def test_bench_offers_full_and_dump_outputs():
    r = _run(["--help"], timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout
