#!/usr/bin/env python
"""One SHA-256 per kernel (and out-of-line device function) of libdeepmimic_hip.so's device code.  No GPU needed.

    python scripts/kernel_isa_digest.py -o branch.json            # every translation unit of csrc/Makefile, its flags
    python scripts/kernel_isa_digest.py --csrc OTHER/csrc --units dm_abi.hip dm_g1.hip -o parent.json
    python scripts/kernel_isa_digest.py --compare parent.json branch.json

Each unit is compiled with the Makefile's FLAGS plus `--cuda-device-only -S`; the assembly is cut at the function labels,
comments are dropped and the function index in local labels (.LBB<n>_) is normalised, so a kernel that merely moved to
another file or position hashes the same; --compare matches kernels by their name up to the parameter list.  Next to it go the digest of the sorted mnemonics (equal = the same instructions in
another order) and the kernel's register counts and segment sizes from the metadata.  Text is hashed and compared, nothing else.
"""
import argparse, hashlib, json, os, re, subprocess, sys, tempfile

META = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deepmimic_mujoco_amd", "csrc")


def makefile_var(text, name):
    m = re.search(r"^%s\s*\??=\s*(.*)$" % name, text, re.M)
    return m.group(1).strip() if m else ""


def digest_unit(csrc, unit, hipcc, flags):
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "unit.s")
        subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", "-o", asm, unit], cwd=csrc, check=True)
        lines = open(asm).read().splitlines()
    out, name, body = {}, None, []
    for line in lines:
        m = re.match(r"^([A-Za-z_$][\w$.]*):", line)
        if m and not m.group(1).startswith(".L"):
            name, body = m.group(1), []
        elif name and re.match(r"^\.Lfunc_end\d+:", line):
            text = "\n".join(body)
            ops = sorted(s.split()[0] for s in body if s[0] in " \t" and not s.lstrip().startswith("."))
            out[name] = {"sha256": hashlib.sha256(text.encode()).hexdigest(), "instructions": len(ops), "unit": unit,
                         "opcodes_sha256": hashlib.sha256(" ".join(ops).encode()).hexdigest()}     # digest of the sorted mnemonics
            name = None
        elif name:
            s = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0].rstrip())
            if s.strip():
                body.append(s)
    # the kernels' entries of the metadata block: register counts and segment sizes
    meta = "\n".join(lines).partition("amdhsa.kernels:")[2].partition(".end_amdgpu_metadata")[0]
    for entry in re.split(r"^  - ", meta, flags=re.M)[1:]:
        fields = dict(re.findall(r"^    (\.\w+):\s*(\S+)$", entry, re.M))
        if fields.get(".name") in out:
            out[fields[".name"]]["meta"] = {k: int(fields[k]) for k in META}
    return out


def by_name(D):
    """Keys cut before the parameter list (_ZN <length><identifier>.. E <parameters>), where that stays unique: a kernel whose
    argument struct was renamed keeps its entry."""
    def cut(k):
        name, at, unit = k.partition("@")
        i = 3 if name.startswith("_ZN") else len(name)
        while i < len(name) and name[i].isdigit():
            j = i
            while name[j].isdigit():
                j += 1
            i = j + int(name[i:j])
        return name[:i] + at + unit
    short = {}
    for k in D:
        short.setdefault(cut(k), []).append(k)
    return {(c if len(ks) == 1 else k): D[k] for c, ks in short.items() for k in ks}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--csrc", default=CSRC)
    ap.add_argument("--units", nargs="*", help="translation units (default: SRCS of the Makefile)")
    ap.add_argument("-o", "--out")
    ap.add_argument("--compare", nargs=2, metavar=("A.json", "B.json"))
    a = ap.parse_args()
    if a.compare:
        A, B = (by_name(json.load(open(p))) for p in a.compare)
        diff = sorted(k for k in set(A) | set(B) if A.get(k, {}).get("sha256") != B.get(k, {}).get("sha256"))
        same_ops = {k: k in A and k in B and all(A[k][f] == B[k][f] for f in ("opcodes_sha256", "meta")) for k in diff}
        print(json.dumps({"entries": [len(A), len(B)], "differ": diff, "same_opcodes_and_metadata": same_ops}, indent=1))
        return 1 if diff else 0
    mk = open(os.path.join(a.csrc, "Makefile")).read()
    flags = makefile_var(mk, "FLAGS").replace("$(ARCH)", makefile_var(mk, "ARCH")).split()
    result = {}
    for unit in a.units or makefile_var(mk, "SRCS").split():
        for name, d in digest_unit(a.csrc, unit, makefile_var(mk, "HIPCC"), flags).items():
            result[name if name not in result else "%s@%s" % (name, unit)] = d
    text = json.dumps(result, indent=1, sort_keys=True)
    open(a.out, "w").write(text + "\n") if a.out else print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
