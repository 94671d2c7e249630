#!/usr/bin/env python
"""dev: which kernels of the two gfx950 code objects differ between two source trees (profiles/ssdiff_unit_isa_diff.txt; no GPU).

    python scripts/dev_isa_diff.py OLD_TREE NEW_TREE [--keep DIR] [--flag=-DNAME ...]

Each unit (csrc/hank_hip.hip, csrc/hank_ssdiff.hip) of each tree is compiled with the Makefile's flags (and every --flag, e.g. --flag=-DHANK_XSTAMP for
the instrumented build) plus -S --cuda-device-only.
The assembly is split at the kernel labels; comments and assembler directives are dropped; the function number in local labels
(.LBB<n>_) and the namespace of a unit that renames it (_ZN8hank_ssd -> _ZN4hank) are normalised. What remains of a kernel is its
instructions and labels: the names whose text differs are printed with their resource lines (registers, scratch — a spill shows
there —, LDS and occupancy from the compiler's "Kernel info" block) from both trees, the others only counted. Exit status 1 if any kernel of OLD is missing in NEW."""
import argparse
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

UNITS = ("hank_hip.hip", "hank_ssdiff.hip")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unused-result"]


def compile_unit(tree, unit, out):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = Path(tree) / "julia-newtonraphsonhank_amd" / "csrc" / unit
    if out.exists():      # (--keep: what an earlier run left is taken as it is)
        return out
    subprocess.run([hipcc] + FLAGS + ["-S", "--cuda-device-only", "-o", str(out), str(src)], check=True, capture_output=True, timeout=1800)
    return out


def norm(s):
    return re.sub(r"\.LBB\d+_", ".LBB_", s.replace("_ZN8hank_ssd", "_ZN4hank"))


def kernels(asm):
    """{normalised kernel name: (instruction text, {resource: value})} of one assembly file"""
    out, name, body, res, mode = {}, None, [], {}, None
    for raw in Path(asm).read_text().splitlines():
        m = re.match(r"^(_Z\w+):", raw)
        if m:
            name, body, res, mode = norm(m.group(1)), [], {}, "code"
            continue
        if name is None:
            continue
        l = raw.strip()
        if mode == "code":
            if l.startswith(".amdhsa_kernel"):
                mode = "descriptor"      # (a device function that was not inlined has none and is not listed)
            elif l.startswith(".Lfunc_end"):
                name = None
            elif l and not l.startswith((";", "//")) and (not l.startswith(".") or l.startswith(".LBB")):
                body.append(norm(l.split(";")[0].rstrip()))
        elif mode == "descriptor" and l == "; Kernel info:":
            mode = "info"
        elif mode == "info":
            m = re.match(r"^; (NumVgprs|NumAgprs|TotalNumSgprs|ScratchSize|LDSByteSize|Occupancy): (\d+)", l)
            if m:
                res[m.group(1)] = m.group(2)
            elif not l.startswith(";"):
                out[name] = ("\n".join(body), res)
                name = None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--flag", action="append", default=[], help="one more compiler flag for both trees (repeatable)")
    ap.add_argument("--keep", help="leave the four assembly files in this directory, and reuse those already there")
    a = ap.parse_args()
    FLAGS.extend(a.flag)
    d = Path(a.keep) if a.keep else Path(tempfile.mkdtemp())
    d.mkdir(parents=True, exist_ok=True)
    jobs = [(tree, u, d / f"{tag}_{u}.s") for tag, tree in (("old", a.old), ("new", a.new)) for u in UNITS]
    with ThreadPoolExecutor(4) as ex:
        list(ex.map(lambda j: compile_unit(*j), jobs))
    missing = 0
    for u in UNITS:
        old, new = kernels(d / f"old_{u}.s"), kernels(d / f"new_{u}.s")
        same = [k for k in old if k in new and old[k][0] == new[k][0]]
        diff = [k for k in old if k in new and old[k][0] != new[k][0]]
        gone, added = [k for k in old if k not in new], [k for k in new if k not in old]
        print(f"{u}: {len(old)} kernels in OLD, {len(new)} in NEW; {len(same)} identical, {len(diff)} differ, {len(gone)} only in OLD, {len(added)} only in NEW")
        dem = subprocess.run(["c++filt"], input="\n".join(diff + gone + added) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        names = dict(zip(diff + gone + added, dem))
        for k in diff:
            print(f"  differs: {names[k]}")
            print("    OLD " + ", ".join(f"{r} {v}" for r, v in old[k][1].items()))
            print("    NEW " + ", ".join(f"{r} {v}" for r, v in new[k][1].items()))
        for k in gone:
            print(f"  only in OLD: {names[k]}")
        for k in added:
            print(f"  only in NEW: {names[k]}")
        missing += len([k for k in gone if "k_ss_" in k or u == "hank_hip.hip"])      # (the second unit of OLD may hold unused copies)
    if not a.keep:
        shutil.rmtree(d)
    sys.exit(1 if missing else 0)


if __name__ == "__main__":
    main()
