#!/usr/bin/env python
"""Where the step kernels wait on LDS: per source line, the LDS accesses and the waits in front of their uses.  No GPU needed.

    python scripts/lds_wait_sites.py -o profiles/lds_wait_sites.json
    python scripts/lds_wait_sites.py --csrc OTHER/csrc -o parent.json
    python scripts/lds_wait_sites.py --compare parent.json branch.json [--lines 1247 1251]

dm_abi.hip is compiled with the Makefile's FLAGS plus `--cuda-device-only -S -gline-tables-only`; every ds_read*/ds_write*,
`s_waitcnt lgkmcnt` and `s_waitcnt vmcnt` of the four step kernels (and of the out-of-line device functions they call) is
counted under the `.loc` line in front of it, i.e. the innermost inlined source line.  A wait that names both counters counts
in both columns.  Next to the table go each kernel's totals and VALU count, and its VGPRs, spills and scratch bytes per lane from
the metadata of a second compile without line tables (the library's own code).
Lines with fewer than --min waits and accesses are summed into "other".  The counts are static: how often a line runs is not in them.
"""
import argparse, json, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deepmimic_mujoco_amd", "csrc")
KERNELS = ("dm_step_kernel", "dm_step_kernel_w3", "dm_step_combined_kernel", "dm_step_combined_kernel_w3")
META = {".vgpr_count": "vgprs", ".vgpr_spill_count": "vgpr_spills", ".sgpr_spill_count": "sgpr_spills",
        ".private_segment_fixed_size": "scratch_bytes"}
COLS = ("ds_read", "ds_write", "wait_lgkm", "wait_vm")


def makefile_var(text, name):
    m = re.search(r"^%s\s*\??=\s*(.*)$" % name, text, re.M)
    return m.group(1).strip() if m else ""


def assemble(csrc, extra=()):
    mk = open(os.path.join(csrc, "Makefile")).read()
    flags = makefile_var(mk, "FLAGS").replace("$(ARCH)", makefile_var(mk, "ARCH")).split()
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "dm_abi.s")
        subprocess.run([makefile_var(mk, "HIPCC"), *flags, "--cuda-device-only", "-S", *extra, "-o", asm, "dm_abi.hip"],
                       cwd=csrc, check=True)
        return open(asm).read().splitlines()


def count(lines):
    files, out, name, cur = {}, {}, None, None
    for line in lines:
        m = re.match(r'^\s*\.file\s+(\d+)\s+"[^"]*"\s+"([^"]*)"', line)
        if m:
            files[int(m.group(1))] = os.path.basename(m.group(2))
            continue
        m = re.match(r"^([A-Za-z_$][\w$.]*):", line)
        if m and not m.group(1).startswith(".L"):
            name, loc = m.group(1), (0, 0)
            cur = {"sites": {}, "totals": dict.fromkeys(COLS + ("valu",), 0)}
            continue
        if name is None:
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            out[name], name = cur, None
            continue
        m = re.match(r"^\s*\.loc\s+(\d+)\s+(\d+)", line)
        if m:
            loc = (int(m.group(1)), int(m.group(2)))
            continue
        s = line.split(";")[0].split()
        if not s or s[0].startswith(".") or s[0].endswith(":"):
            continue
        hit = []
        if s[0].startswith("ds_read"):
            hit.append("ds_read")
        elif s[0].startswith("ds_write"):
            hit.append("ds_write")
        elif s[0] == "s_waitcnt":
            hit += [c for c, k in (("wait_lgkm", "lgkmcnt"), ("wait_vm", "vmcnt")) if k in " ".join(s[1:])]
        elif s[0].startswith("v_") and not s[0].startswith("v_mfma"):
            cur["totals"]["valu"] += 1
        for c in hit:
            cur["totals"][c] += 1
            cur["sites"].setdefault(loc, dict.fromkeys(COLS, 0))[c] += 1
    return files, out


def metadata(lines):
    out = {}
    meta = "\n".join(lines).partition("amdhsa.kernels:")[2].partition(".end_amdgpu_metadata")[0]
    for entry in re.split(r"^  - ", meta, flags=re.M)[1:]:
        fields = dict(re.findall(r"^    (\.\w+):\s*(\S+)$", entry, re.M))
        out[fields.get(".name")] = {v: int(fields.get(k, 0)) for k, v in META.items()}
    return out


def report(csrc, min_count):
    files, fns = count(assemble(csrc, ["-gline-tables-only"]))
    meta = metadata(assemble(csrc))      # the build as the Makefile makes it: line tables shift the register allocation a little
    called = [n for n in fns if n not in meta]     # out-of-line device functions
    result = {"unit": "dm_abi.hip", "kernels": {}}
    for n in KERNELS + tuple(called):
        d = fns[n]
        rows, other = [], dict.fromkeys(COLS, 0)
        for (f, ln), c in d["sites"].items():
            if max(c["wait_lgkm"], c["ds_read"] + c["ds_write"]) >= min_count:
                rows.append({"file": files.get(f, str(f)), "line": ln, **c})
            else:
                for k in COLS:
                    other[k] += c[k]
        rows.sort(key=lambda r: (-r["wait_lgkm"], r["file"], r["line"]))
        result["kernels"][n] = {"totals": d["totals"], **({"meta": meta[n]} if n in meta else {}), "sites": rows, "other": other}
    return result


def compare(pa, pb, lines):
    A, B = (json.load(open(p))["kernels"] for p in (pa, pb))
    for n in A:
        if n not in B:
            continue
        print(n)
        for k in ("wait_lgkm", "wait_vm", "ds_read", "ds_write", "valu"):
            print("  %-14s %6d -> %6d" % (k, A[n]["totals"][k], B[n]["totals"][k]))
        for k in A[n].get("meta", {}):
            print("  %-14s %6d -> %6d" % (k, A[n]["meta"][k], B[n]["meta"][k]))
        for ln in lines:
            a, b = ([r for r in X[n]["sites"] if r["line"] == ln and r["file"] == "dm_kernels.hip"] for X in (A, B))
            print("  dm_kernels.hip:%d  reads %s -> %s   lgkm waits %s -> %s" % (
                ln, *(x[0]["ds_read"] if x else "<min" for x in (a, b)), *(x[0]["wait_lgkm"] if x else "<min" for x in (a, b))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--csrc", default=CSRC)
    ap.add_argument("-o", "--out")
    ap.add_argument("--min", type=int, default=4, help="lines below this many waits and accesses go into 'other'")
    ap.add_argument("--compare", nargs=2, metavar=("A.json", "B.json"))
    ap.add_argument("--lines", nargs="*", type=int, default=[], help="with --compare: dm_kernels.hip lines to print side by side")
    a = ap.parse_args()
    if a.compare:
        compare(*a.compare, a.lines)
        return 0
    text = json.dumps(report(a.csrc, a.min), indent=1)
    open(a.out, "w").write(text + "\n") if a.out else print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
