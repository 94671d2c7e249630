#!/usr/bin/env python
"""dev: which kernels of the two gfx950 code objects a run launches (profiles/kernel_coverage.txt).

    python scripts/dev_kernel_coverage.py --list
        the kernel symbols of csrc/hank_hip.hip and csrc/hank_ssdiff.hip, demangled (hipcc -S --cuda-device-only, as
        tests/test_isa_hazards.py; no GPU)
    python scripts/dev_kernel_coverage.py --stats DIR_OR_CSV [...] [--out FILE]
        every kernel with its launch count, summed over the kernel-stats CSVs of a `rocprofv3 --kernel-trace --stats
        --output-format csv` run (all *kernel_stats.csv below a directory: one per traced process). A kernel at zero launches is
        printed with its reason from REASONS when it has one, `(no reason recorded)` otherwise. --only REGEX keeps the kernels whose
        demangled name matches (a run of one test module: profiles/ss_diff_kernel_coverage.txt, --only k_ss_)."""
import argparse
import csv
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "julia-newtonraphsonhank_amd" / "csrc"
UNITS = ("hank_hip.hip", "hank_ssdiff.hip")      # the library's translation units (csrc/Makefile)

# why a kernel is at zero in a run (regex on the demangled name -> one line). The per-period tangent kernels are instantiated for row
# groups 1, 2, 4 and both lane widths; ensure_tanwork (csrc/hank_hip.hip) picks among them by batch width. Every instance is launched
# by tests/test_gpu_launch_lanes.py (profiles/launch_lanes_kernel_coverage.txt); a run without that module shows these at zero.
_LANES = "; tests/test_gpu_launch_lanes.py alone launches it"
REASONS = {
    r"k_(tan|fused)_fwd<1, (double|HIP_vector_type<double, 2u>), true>": "source-stationary form (16-lane groups and up) with 1 row group: the default gives that form 2; dev knob HANK_RG_F=1" + _LANES,
    r"k_(tan|fused)_fwd<2, (double|HIP_vector_type<double, 2u>), false>": "target-stationary gather with 2 row groups: the default takes that gather only below 16-lane groups, with 1; HANK_RG_F=2 / HANK_FWD_SS=0" + _LANES,
    r"k_(tan|fused)_fwd<4,": "4 forward row groups: never the default; dev knob HANK_RG_F=4" + _LANES,
    r"k_(tan|fused)_back<1,": "1 backward row group: never the default; dev knob HANK_RG_B=1" + _LANES,
    r"k_(tan|fused)_back<4, double>": "4 backward row groups, one direction per lane: the per-period launches at an odd N >= 129, which the default sends to the wide "
                                      "sweeps where those exist" + _LANES,
    r"k_tan_back<4, HIP_vector_type<double, 2u> >": "4 backward row groups, two directions per lane: hank_jvp on the per-period launches at an even N >= 256, which the default "
                                                    "sends to the wide sweeps where those exist" + _LANES,
}


def kernel_symbols():
    """[(mangled, demangled)] of every kernel descriptor in the gfx950 assembly of both units, in the order the compiler emits them."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    syms = []
    with tempfile.TemporaryDirectory() as d:
        for unit in UNITS:
            out = Path(d) / "hank.s"
            subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only",
                            "-o", str(out), str(CSRC / unit)], check=True, capture_output=True, timeout=900)
            syms += re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", out.read_text(), re.M)
    dem = subprocess.run(["c++filt"], input="\n".join(syms) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(dem) == len(syms)
    return list(zip(syms, dem))


def _key(name):
    """rocprofv3 prints some names with a leading return type: compare without it and without blanks."""
    name = name.strip()
    if name.startswith("void "):
        name = name[5:]
    return re.sub(r"\s+", "", name)


def launch_counts(paths):
    counts, files = {}, []
    for p in map(Path, paths):
        files += sorted(p.rglob("*kernel_stats.csv")) if p.is_dir() else [p]
    for f in files:
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                counts[_key(row["Name"])] = counts.get(_key(row["Name"]), 0) + int(row["Calls"])
    return counts, files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--list", action="store_true", help="print the kernel symbols and stop (no GPU needed)")
    ap.add_argument("--stats", nargs="*", default=[], help="kernel-stats CSVs, or directories searched for them")
    ap.add_argument("--out", help="write the report here as well")
    ap.add_argument("--only", help="list only the kernels whose demangled name matches this regex")
    a = ap.parse_args()
    kernels = kernel_symbols()
    if a.only:
        kernels = [k for k in kernels if re.search(a.only, k[1])]
    if a.list or not a.stats:
        for _, d in kernels:
            print(d)
        print(f"{len(kernels)} kernels", file=sys.stderr)
        return
    counts, files = launch_counts(a.stats)
    lines, zero = [], 0
    for _, d in sorted(kernels, key=lambda k: k[1]):
        n = counts.pop(_key(d), 0)
        if n:
            lines.append(f"{n:>9}  {d}")
        else:
            zero += 1
            why = next((r for pat, r in REASONS.items() if re.search(pat, d)), "(no reason recorded)")
            lines.append(f"{0:>9}  {d}\n{'':>11}not launched: {why}")
    head = [f"# {len(kernels)} kernels{f' matching {a.only}' if a.only else ''} in the gfx950 code objects of csrc/hank_hip.hip and csrc/hank_ssdiff.hip, {len(kernels) - zero} launched, {zero} not",
            f"# launch counts summed over {len(files)} kernel-stats CSV(s) of one rocprofv3 --kernel-trace --stats run"]
    if counts and not a.only:
        head.append(f"# {len(counts)} traced kernel name(s) outside the code object (torch, rocBLAS/hipBLASLt, ...) are not listed")
    text = "\n".join(head + lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
