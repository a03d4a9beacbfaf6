"""The host arithmetic of the two engines (csrc/dm_tables_host.h, csrc/dm_g1_tables_host.h) on a CPU, under the host sanitizers.

tests/host/host_tables.hip (own main, no kernels, no HIP runtime call) is compiled once with hipcc and
-fsanitize=address,undefined on the host side, and run directly:

* digest: on the packaged models and the walk clip of each robot it runs the model check, the table builders, the G1 hull
  clustering and the clip packing, and prints a 64-bit FNV-1a and a byte count per table.  tests/golden/host_tables_digest.json holds
  what the code BEFORE the host layer was split into headers produced for the same inputs (a program that included the two
  translation units of that commit and called their static functions, the clip loops lifted verbatim; same sanitizer flags, and the
  library's -O3 flags gave the same digests): the tables are byte-identical.
* reject: one index field of a model at a time set one below and one past its range; the check function alone must answer
  DM_EINVAL with a message that names the field.  One below is -1 for every field whose range starts at 0; geom_mesh and dof_parent
  admit -1 (no mesh, no parent), so their low case is -2.

Every run must end with status 0 and an empty stderr: the sanitizers report nothing.
"""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "host_tables.hip")
MAKEFILE = os.path.join(os.path.dirname(HERE), "deepmimic_mujoco_amd", "csrc", "Makefile")
DM_EINVAL = -22


def _hipcc():
    m = re.search(r"^HIPCC\s*\?=\s*(\S+)", open(MAKEFILE).read(), re.M)
    return os.environ.get("HIPCC") or m.group(1)


def _run(args):
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", "%s\n%s\n%s" % (" ".join(args), r.stdout, r.stderr)
    return r.stdout


def _write_clip(path, mocap):
    tables = [np.ascontiguousarray(a, np.float64) for a in mocap.tables()]
    with open(path, "wb") as f:
        f.write(np.int64(len(tables[0])).tobytes())
        for a in tables:
            f.write(a.tobytes())


@pytest.fixture(scope="module")
def host(tmp_path_factory, model):
    """The program, built with the sanitizers, and its input files: both packaged models, the walk clip of each robot."""
    from deepmimic_mujoco_amd import g1
    from deepmimic_mujoco_amd.config import MotionConfig
    from deepmimic_mujoco_amd.mocap import MocapDM
    d = tmp_path_factory.mktemp("host_tables")
    exe = str(d / "host_tables")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    r = subprocess.run([_hipcc(), "-std=c++17", "-O1", "-g", "-Wall", "--offload-arch=gfx950", *san, "-o", exe, SRC],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    paths = {k: str(d / k) for k in ("h_model", "h_clip", "g1_model", "g1_clip")}
    g1_model = g1.load_g1_model()[1]
    open(paths["h_model"], "wb").write(bytes(model.cstruct))
    open(paths["g1_model"], "wb").write(bytes(g1_model))
    mc = MocapDM(model=model)
    mc.load_mocap(MotionConfig("walk").mocap_path)
    _write_clip(paths["h_clip"], mc)
    _write_clip(paths["g1_clip"], g1._g1_mocap("walk")[1])
    return {"exe": exe, "paths": paths, "humanoid": model.cstruct, "g1": g1_model}


def test_tables_are_byte_identical_to_the_recorded_ones(host):
    p = host["paths"]
    out = _run([host["exe"], "digest", p["h_model"], p["h_clip"], p["g1_model"], p["g1_clip"]])
    got = {name: {"fnv1a64": h, "bytes": int(n)} for name, h, n in (line.split() for line in out.splitlines())}
    want = json.load(open(os.path.join(HERE, "golden", "host_tables_digest.json")))
    assert sorted(want) == ["g1_clip_rows", "g1_clus", "g1_com_rows", "g1_dev", "g1_oidx", "g1_reset_rows", "g1_verts",
                            "humanoid_clip_rows", "humanoid_dev", "humanoid_reset_rows"]
    assert got == want


def _field_groups(robot, s):
    """(field, entry, lo, hi): the range [lo, hi) the check holds that entry of the packaged model to."""
    from deepmimic_mujoco_amd import g1, model as hm
    d = g1 if robot == "g1" else hm
    nv, nbody, ngeom, njnt = d.NV, d.NBODY, d.NGEOM, d.NJNT
    groups = [("body_parent", 5, 0, 5), ("dof_parent", 10, -1, 10), ("dof_body", 3, 0, nbody), ("dof_jnt", 3, 0, njnt),
              ("act_dof", 2, 0, nv), ("geom_body", 4, 0, nbody), ("pair_geom1", 0, 0, ngeom), ("pair_geom2", 1, 0, ngeom),
              ("ee_geom", 1, 0, ngeom), ("torso_body", None, 0, nbody), ("rfoot_geom", None, 0, ngeom),
              ("lfoot_geom", None, 0, ngeom), ("floor_geom", None, 0, ngeom)]
    if robot == "humanoid":
        groups.append(("body_dofadr", 3, 0, nv - s.body_dofnum[3] + 1))
    else:
        groups += [("geom_mesh", 50, -1, g1.NMESH), ("mesh_vertnum", 0, 0, g1.NMESHVERT + 1),
                   ("mesh_vertadr", 0, 0, g1.NMESHVERT - s.mesh_vertnum[0] + 1), ("extra_geom", 7, 0, ngeom),
                   ("rew_qposadr", 0, 0, g1.NQ), ("rew_dofadr", 1, 0, nv), ("rew_jnt", 2, 0, njnt)]
    return groups


@pytest.mark.parametrize("robot", ["humanoid", "g1"])
def test_an_index_out_of_range_is_refused_by_name(host, robot):
    s = host[robot]
    cases = []
    for field, entry, lo, hi in _field_groups(robot, s):
        off = getattr(type(s), field).offset + 4 * (entry or 0)
        cases += [(field, off, lo - 1), (field, off, hi)]
    model_path = host["paths"]["g1_model" if robot == "g1" else "h_model"]
    out = _run([host["exe"], "reject", robot, model_path] + ["%d:%d" % (off, v) for _, off, v in cases]).splitlines()
    assert len(out) == len(cases) >= 28
    for (field, off, v), line in zip(cases, out):
        rc, _, msg = line.partition(" ")
        assert int(rc) == DM_EINVAL and field in msg, (field, v, line)


def test_the_packaged_models_are_in_range(host):
    """The cases above start from models the check accepts, and their chosen entries sit inside the ranges they leave."""
    for robot in ("humanoid", "g1"):
        s = host[robot]
        for field, entry, lo, hi in _field_groups(robot, s):
            v = getattr(s, field)
            v = v if entry is None else v[entry]
            assert lo <= v < hi, (robot, field, v)
