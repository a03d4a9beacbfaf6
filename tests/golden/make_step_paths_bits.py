#!/usr/bin/env python
"""Records tests/golden/step_paths_bits.npz on an MI355X: what tests/test_step_paths_bits_gpu.py compares with.

The recording is taken from the library of the commit BEFORE a change to step_body, so build that commit in a worktree and point
--root at it; this file and the test's compute() come from the tree that holds the change:

    git worktree add ../parent <commit> && make -C ../parent/deepmimic_mujoco_amd/csrc
    python tests/golden/make_step_paths_bits.py --root ../parent -o tests/golden/step_paths_bits.npz

--root defaults to this tree (to re-record after a change that is meant to move the bits).  With --check FILE nothing is written:
the run is compared with FILE array by array and the exit status tells whether all were equal.
"""
import argparse, os, sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", default=os.path.dirname(TESTS), help="tree whose package and library run")
    ap.add_argument("-o", "--out", default=os.path.join(HERE, "step_paths_bits.npz"))
    ap.add_argument("--check", metavar="FILE")
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path[:0] = [root, TESTS]
    import numpy as np, torch
    import deepmimic_mujoco_amd._lib as L
    assert os.path.dirname(os.path.dirname(os.path.abspath(L.__file__))) == root, L.__file__
    from deepmimic_mujoco_amd.model import load_model
    import test_step_paths_bits_gpu as T
    model = load_model()
    got = T.pack(T.compute(model, T.load_mocaps(model), torch))
    if a.check:
        with np.load(a.check) as z:
            diff = [k for k in sorted(set(z.files) | set(got)) if k not in got or k not in z.files or not np.array_equal(got[k], z[k])]
        print("library %s against %s: %s" % (L.LIB_PATH, a.check, "differ: %s" % diff if diff else "all %d arrays equal" % len(got)))
        return 1 if diff else 0
    np.savez_compressed(a.out, **got)
    print("recorded %d arrays per kernel variant from %s into %s (%d bytes); %d of %d words differ between the variants" % (
        len(got["names"]), L.LIB_PATH, a.out, os.path.getsize(a.out), np.count_nonzero(got["w3_xor_w2"]), got["w2"].size))
    return 0


if __name__ == "__main__":
    sys.exit(main())
