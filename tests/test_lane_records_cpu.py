"""The lane-major records of the step kernels (csrc/dm_tables.h, dm_build_lane_records) against the tables they copy, on the host.

tests/lane_records_check.cpp (own main, host compiler only, no HIP) fills a DmDev in which every 32-bit word holds its own
index pattern, builds the records and compares, for all 64 lanes and every geom and dof id, the bits of each record field with the
table entry it replaces: the hinge axes at b_dofadr + j for j < b_dofnum, b_invw[g_body[g]] / b_chain[g_body[g]] folded into the
contact-row record, entry 0 for lanes past a role's count; the chunk offsets the kernels address are static_asserts of the
program.  It is built and run twice, plain and with -fsanitize=address,undefined."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "lane_records_check.cpp")


def _compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


CXX = _compiler()
pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-o", exe, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout, r.stdout
    return r.stdout


def test_records_hold_the_table_bits(tmp_path):
    out = _build_and_run(tmp_path, "lane_records_check", [])
    # 64 lanes x (8 body + 3 axes + 11 dof + 3 geom fields) + 16 geoms x 6 + 34 dofs x 3
    assert "lane records: %d checks" % (64 * 25 + 16 * 6 + 34 * 3) in out, out


def test_records_under_address_and_ub_sanitizers(tmp_path):
    probe = subprocess.run([CXX, "-fsanitize=address,undefined", "-x", "c++", "-o", str(tmp_path / "probe"), "-"],
                           input="int main() { return 0; }\n", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the host compiler has no address / undefined-behaviour sanitizer runtime")
    _build_and_run(tmp_path, "lane_records_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
