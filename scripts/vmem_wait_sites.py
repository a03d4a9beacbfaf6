#!/usr/bin/env python
"""Where the step kernels wait on vector memory: every `s_waitcnt vmcnt` with the loads it covers.  No GPU needed.

    python scripts/vmem_wait_sites.py -o profiles/vmem_wait_sites.json
    python scripts/vmem_wait_sites.py --csrc OTHER/csrc -o profiles/vmem_wait_sites_parent.json
    python scripts/vmem_wait_sites.py --compare parent.json branch.json

Sibling of lds_wait_sites.py (same compile: the Makefile's FLAGS plus `--cuda-device-only -S -gline-tables-only`).  The listing of
each of the four step kernels is walked top to bottom as one straight line (branches are not followed: a wait behind a join sees
the loads of the path that stands in front of it in the file).  Vector-memory instructions return in order, so `vmcnt(N)` covers
every one issued so far except the youngest N.  A wait is a TABLE wait if a `global_load*` is among them, else a SCRATCH wait if a
`scratch_load*` is (a spill coming back), else OTHER (stores only, or nothing left in flight on this path).  Its distance is the
number of VALU instructions between the youngest load it covers and the wait; a table wait is EXPOSED below --exposed VALU
(default 48: about 190 cycles at one wave's 4-cycle issue, an L2 hit).  Waits are booked to the phase of phase_profile.py whose
PROF() stamp follows their source line in dm_kernels.hip; code inlined from the helpers above the kernels, or from another
header, stays in the phase of the code around it.  The tool counts these waits and load kinds and nothing else; the counts are
static: how often a line runs is not in them.
"""
import argparse, json, os, re, sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lds_wait_sites import CSRC, KERNELS, assemble

PHASES = ["init/load", "kin+geom+com+cinert+cdof", "crb+M", "factor", "vel+rne+smooth", "collision", "rows+J",
          "Bsolve+AR", "warm+PGS", "finish", "RK/stage", "task+store"]


def phase_marks(csrc):
    """[(line, phase index)] of the PROF(i) stamps of dm_kernels.hip, and the first line of the kernels' own code."""
    marks, first = [], None
    for n, line in enumerate(open(os.path.join(csrc, "dm_kernels.hip")), 1):
        if first is None and line.startswith("__shared__ EnvLds g_S"):
            first = n
        m = re.match(r"\s*PROF\((\d+)\);", line)
        if m and first is not None:
            marks.append((n, int(m.group(1))))
    return marks, first


def phase_of(line, marks, first):
    if first is None or line < first:
        return None
    for n, i in marks:
        if line <= n:
            return i
    return None


def walk(lines, marks, first, exposed):
    files, out, name, cur = {}, {}, None, None
    for line in lines:
        m = re.match(r'^\s*\.file\s+(\d+)\s+"[^"]*"\s+"([^"]*)"', line)
        if m:
            files[int(m.group(1))] = os.path.basename(m.group(2))
            continue
        m = re.match(r"^([A-Za-z_$][\w$.]*):", line)
        if m and not m.group(1).startswith(".L"):
            name = m.group(1) if m.group(1) in KERNELS else None
            loc, phase, valu, flight = ("", 0), 0, 0, []      # flight: (mnemonic, VALU count at issue)
            cur = {"totals": dict(wait_vm=0, table=0, table_exposed=0, scratch=0, other=0), "phases": {}, "sites": {}}
            continue
        if name is None:
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            out[name], name = cur, None
            continue
        m = re.match(r"^\s*\.loc\s+(\d+)\s+(\d+)", line)
        if m:
            loc = (files.get(int(m.group(1)), m.group(1)), int(m.group(2)))
            if loc[0] == "dm_kernels.hip":
                p = phase_of(loc[1], marks, first)
                phase = phase if p is None else p
            continue
        s = line.split(";")[0].split()
        if not s or s[0].startswith(".") or s[0].endswith(":"):
            continue
        op = s[0]
        if op.startswith("v_"):
            valu += 1
        elif op.startswith(("global_", "scratch_", "buffer_", "flat_")):
            flight.append((op, valu))
        elif op == "s_waitcnt":
            m = re.search(r"vmcnt\((\d+)\)", " ".join(s[1:]))
            if not m:
                continue
            keep = int(m.group(1))
            covered, flight = (flight[:len(flight) - keep], flight[len(flight) - keep:]) if keep < len(flight) else ([], flight)
            loads = [c for c in covered if "_load" in c[0]]
            kind = "table" if any(c[0].startswith("global_load") for c in loads) else \
                   "scratch" if any(c[0].startswith("scratch_load") for c in loads) else "other"
            dist = valu - loads[-1][1] if loads else None
            hit = [kind] + (["table_exposed"] if kind == "table" and dist < exposed else [])
            ph = cur["phases"].setdefault(PHASES[phase] if phase < len(PHASES) else str(phase),
                                          dict(wait_vm=0, table=0, table_exposed=0, scratch=0, other=0))
            site = cur["sites"].setdefault((loc, kind), dict(file=loc[0], line=loc[1], kind=kind, waits=0, loads=0, min_valu=None))
            site["waits"] += 1
            site["loads"] += len(loads)
            if dist is not None:
                site["min_valu"] = dist if site["min_valu"] is None else min(site["min_valu"], dist)
            for k in ["wait_vm"] + hit:
                cur["totals"][k] += 1
                ph[k] += 1
    for d in out.values():
        d["sites"] = sorted(d["sites"].values(), key=lambda r: (r["file"], r["line"], r["kind"]))
    return out


def compare(pa, pb):
    A, B = (json.load(open(p))["kernels"] for p in (pa, pb))
    for n in A:
        if n not in B:
            continue
        print(n)
        for k in A[n]["totals"]:
            print("  %-14s %5d -> %5d" % (k, A[n]["totals"][k], B[n]["totals"][k]))
        print("  exposed table waits per phase")
        for ph in PHASES:
            a, b = (X[n]["phases"].get(ph, {}).get("table_exposed", 0) for X in (A, B))
            ta, tb = (X[n]["phases"].get(ph, {}).get("table", 0) for X in (A, B))
            print("    %-26s %3d of %3d -> %3d of %3d" % (ph, a, ta, b, tb))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--csrc", default=CSRC)
    ap.add_argument("-o", "--out")
    ap.add_argument("--exposed", type=int, default=48, help="a table wait with fewer VALU instructions behind its youngest load is exposed")
    ap.add_argument("--compare", nargs=2, metavar=("A.json", "B.json"))
    a = ap.parse_args()
    if a.compare:
        compare(*a.compare)
        return 0
    marks, first = phase_marks(a.csrc)
    result = {"unit": "dm_abi.hip", "exposed_below_valu": a.exposed,
              "kernels": walk(assemble(a.csrc, ["-gline-tables-only"]), marks, first, a.exposed)}
    text = json.dumps(result, indent=1)
    open(a.out, "w").write(text + "\n") if a.out else print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
