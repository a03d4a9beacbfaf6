#!/usr/bin/env python
"""Records tests/golden/g1_step_bits.npz on an MI355X: what tests/test_g1_step_bits_gpu.py compares with.

The recording is taken from the library of the commit BEFORE a change to the G1 engine, so build that commit in a worktree and
point --root at it; this file and the test's compute() come from the tree that holds the change:

    git worktree add ../parent <commit> && make -C ../parent/deepmimic_mujoco_amd/csrc
    python tests/golden/make_g1_step_bits.py --root ../parent -o tests/golden/g1_step_bits.npz

The commit's hash goes into the file ("commit"): `git rev-parse HEAD` in --root, or --commit where the tree has no repository.
Both pipelines run, and nothing is written unless they agree bit for bit and two runs of the same pipeline do: the file holds
one copy.  With --check FILE nothing is written either: both pipelines are compared with FILE and the exit status tells whether
all arrays were equal.
"""
import argparse, os, subprocess, sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=os.path.dirname(TESTS), help="tree whose package and library run")
    ap.add_argument("--commit", help="hash of the commit that --root holds")
    ap.add_argument("-o", "--out", default=os.path.join(HERE, "g1_step_bits.npz"))
    ap.add_argument("--check", metavar="FILE")
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path[:0] = [root, TESTS]
    import numpy as np
    import deepmimic_mujoco_amd._lib as L
    assert os.path.dirname(os.path.dirname(os.path.abspath(L.__file__))) == root, L.__file__
    import test_g1_step_bits_gpu as T
    runs = {"pipeline 1": T.compute(1), "pipeline 2": T.compute(2)}
    if a.check:
        with np.load(a.check) as z:
            want = {k: z[k] for k in z.files if k != "commit"}
            print("recorded from commit %s" % z["commit"])
        bad = {name: T.differing(got, want) for name, got in runs.items()}
        for name, b in bad.items():
            print("library %s, %s against %s: %s" % (L.LIB_PATH, name, a.check, "differ: %s" % b if b else "all %d arrays equal" % len(want)))
        return 1 if any(bad.values()) else 0
    runs["pipeline 1 again"] = T.compute(1)
    got = runs["pipeline 1"]
    bad = {name: T.differing(r, got) for name, r in runs.items()}
    for name, b in bad.items():
        print("%s against pipeline 1: %s" % (name, "differ: %s" % b if b else "all %d arrays equal" % len(got)))
    if any(bad.values()):
        return 1
    commit = a.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=root, text=True).strip()
    np.savez_compressed(a.out, commit=np.array(commit), **got)
    T.test_fixture_takes_every_exit(got)
    print("recorded %d arrays of commit %s from %s into %s (%d bytes)" % (len(got), commit, L.LIB_PATH, a.out, os.path.getsize(a.out)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
