#!/usr/bin/env python
"""Where the step kernels pay the VALU-writes-SGPR hazard: `v_readlane` counts, `s_nop` by argument and the triplets
`v_readlane_b32 sN` -> `s_nop` -> `v_fma / v_fmac / v_mul ... sN` by source region.  No GPU needed.

    python scripts/hazard_nop_sites.py -o profiles/hazard_nop_sites.json
    python scripts/hazard_nop_sites.py --csrc OTHER/csrc -o profiles/hazard_nop_sites_parent.json
    python scripts/hazard_nop_sites.py --compare profiles/hazard_nop_sites_parent.json profiles/hazard_nop_sites.json

A VALU read of an SGPR needs two wait states after the VALU (v_readlane) that wrote it; where the compiler has nothing else to
issue, it pads with `s_nop 1`, and the broadcast and its FMA run at full latency.  dm_abi.hip is compiled as
scripts/lds_wait_sites.py does (Makefile FLAGS plus `--cuda-device-only -S -gline-tables-only`).  An instruction belongs to the
first region of REGIONS that holds a line of its inlining chain (the `.loc` comment); the regions are cut at text anchors of
csrc/dm_kernels.hip, so they follow the source when lines move.  Register counts, spills and scratch bytes per lane come from a
second compile without line tables (the library's own code).  The counts are static: how often a region runs is not in them.
"""
import argparse, json, os, re, sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lds_wait_sites import CSRC, KERNELS, assemble, metadata       # noqa: E402

# region -> (first line matches, the line after its last matches); searched in this order
REGIONS = (
    ("factor", r"---- L\^T D L on the columns", r"publish the factor in the sparse MuJoCo layout"),
    ("m_columns", r"---- M by COLUMNS", r"---- L\^T D L on the columns"),
    ("triangular_solves", r"float solve_LT\(", r"void load_factor_row\("),
    ("fwd_smooth_other", r"float fwd_smooth\(", r"float euler_damped_solve\("),
    ("build_row", r"void build_row\(", r"float fwd_constraint_wide\("),
    ("fwd_constraint_wide", r"float fwd_constraint_wide\(", r"float fwd_constraint\("),
    ("fwd_constraint", r"float fwd_constraint\(", r"void store_state\("),
)
USES = ("v_fma_f32", "v_fmac_f32", "v_mul_f32", "v_rcp_f32")


def region_lines(csrc):
    src = open(os.path.join(csrc, "dm_kernels.hip")).read().splitlines()
    def find(pat):
        hits = [n + 1 for n, l in enumerate(src) if re.search(pat, l)]
        assert hits, "anchor %r not in dm_kernels.hip" % pat
        return hits[0]
    return [(name, find(a), find(b)) for name, a, b in REGIONS]


def count(lines, regions):
    out, name, cur, chain = {}, None, None, ()
    def region():
        for rname, a, b in regions:
            if any(a <= ln < b for ln in chain):
                return rname
        return "other"
    for line in lines:
        m = re.match(r"^([A-Za-z_$][\w$.]*):", line)
        if m and not m.group(1).startswith(".L"):
            name, chain, prev = m.group(1), (), []
            cur = {"v_readlane": 0, "s_nop": {}, "valu": 0, "triplets": {}, "v_readlane_by_region": {}, "s_nop_by_region": {}}
            continue
        if name is None:
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            out[name], name = cur, None
            continue
        if re.match(r"^\s*\.loc\s", line):
            chain = tuple(int(x) for x in re.findall(r"dm_kernels\.hip:(\d+):", line))
            continue
        s = line.split(";")[0].replace(",", " ").split()
        if not s or s[0].startswith(".") or s[0].endswith(":"):
            continue
        r = region()
        if s[0].startswith("v_") and not s[0].startswith("v_mfma"):
            cur["valu"] += 1
        if s[0] == "v_readlane_b32":
            cur["v_readlane"] += 1
            cur["v_readlane_by_region"][r] = cur["v_readlane_by_region"].get(r, 0) + 1
        if s[0] == "s_nop":
            cur["s_nop"][s[1]] = cur["s_nop"].get(s[1], 0) + 1
            cur["s_nop_by_region"][r] = cur["s_nop_by_region"].get(r, 0) + 1
        # readlane sN ; s_nop ; <use of sN>: counted under the region of the use
        if len(prev) == 2 and prev[0][0] == "v_readlane_b32" and prev[1][0] == "s_nop" and s[0].split("_e")[0] in USES:
            sreg = prev[0][1]
            if any(a.lstrip("-|") .rstrip("|") == sreg for a in s[2:]):
                cur["triplets"][r] = cur["triplets"].get(r, 0) + 1
        prev = (prev + [s])[-2:]
    return out


def report(csrc):
    regions = region_lines(csrc)
    fns = count(assemble(csrc, ["-gline-tables-only"]), regions)
    meta = metadata(assemble(csrc))
    result = {"unit": "dm_abi.hip", "regions": {n: [a, b] for n, a, b in regions}, "kernels": {}}
    for n in KERNELS + tuple(k for k in fns if k not in meta and any(fns[k]["triplets"].values())):
        d = fns[n]
        d["s_nop_total"] = sum(d["s_nop"].values())
        d["triplets_total"] = sum(d["triplets"].values())
        result["kernels"][n] = {**({"meta": meta[n]} if n in meta else {}), **d}
    return result


def compare(pa, pb):
    A, B = (json.load(open(p))["kernels"] for p in (pa, pb))
    for n in A:
        if n not in B:
            continue
        print(n)
        for k in ("v_readlane", "s_nop_total", "triplets_total", "valu"):
            print("  %-22s %6d -> %6d" % (k, A[n][k], B[n][k]))
        for k in sorted(set(A[n]["s_nop"]) | set(B[n]["s_nop"]), key=int):
            print("  s_nop %-16s %6d -> %6d" % (k, A[n]["s_nop"].get(k, 0), B[n]["s_nop"].get(k, 0)))
        for k in sorted(set(A[n]["triplets"]) | set(B[n]["triplets"])):
            print("  triplets %-13s %6d -> %6d" % (k, A[n]["triplets"].get(k, 0), B[n]["triplets"].get(k, 0)))
        for k in A[n].get("meta", {}):
            print("  %-22s %6d -> %6d" % (k, A[n]["meta"][k], B[n]["meta"][k]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--csrc", default=CSRC)
    ap.add_argument("-o", "--out")
    ap.add_argument("--compare", nargs=2, metavar=("A.json", "B.json"))
    a = ap.parse_args()
    if a.compare:
        compare(*a.compare)
        return 0
    text = json.dumps(report(a.csrc), indent=1)
    open(a.out, "w").write(text + "\n") if a.out else print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
