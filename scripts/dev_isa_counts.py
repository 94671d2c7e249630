#!/usr/bin/env python3
"""Static instruction counts of a persistent kernel's period loop in cross-compiled gfx950 assembly.

    for u in hank_hip hank_ssdiff; do      # the library's two translation units
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -S --cuda-device-only \
          -Rpass-analysis=kernel-resource-usage -o $u.s csrc/$u.hip 2>> resources.txt; done
    scripts/dev_isa_counts.py hank_hip.s[,hank_ssdiff.s] [resources.txt] [kernel-name-substring ...]

The period loop is taken to be the longest backward branch of the kernel (label .. the branch that jumps back to it;
jumps to the kernel's exit block, which the compiler may place first, are not loops).
Counted inside it: VALU, SALU, lane reads/writes of spilled scalars, 64-bit address arithmetic, memory instructions by
mnemonic. With the remarks file: VGPRs, SGPRs, scratch and occupancy of the same kernels.
"""
import collections
import re
import sys

DEFAULT = ["k_xdual_backILi4ELi768E", "k_xfwdILi4ELb1ELi768E"]
NOT_SALU = ("s_waitcnt", "s_nop", "s_barrier", "s_branch", "s_cbranch", "s_load", "s_buffer_load", "s_sleep", "s_endpgm",
            "s_setprio", "s_memrealtime", "s_memtime", "s_getreg", "s_setreg", "s_sendmsg", "s_code_end", "s_waitcnt_depctr")
ADDR64 = ("v_lshl_add_u64", "v_mad_u64_u32", "v_mad_i64_i32", "v_lshlrev_b64", "v_add_co_u32", "v_addc_co_u32",
          "v_add_co_ci_u32", "v_sub_co_u32", "v_subb_co_u32")
MEM = ("global_", "buffer_", "flat_", "scratch_", "ds_")


def functions(lines):
    """{name: (first, last)} line ranges of the functions of an assembly file"""
    out, name, first = {}, None, 0
    for i, ln in enumerate(lines):
        m = re.match(r"^(_Z\w+):", ln)
        if m and name is None:
            name, first = m.group(1), i
        elif name and ln.startswith(".Lfunc_end"):
            out[name] = (first, i)
            name = None
    return out


def period_loop(body):
    """(first, last) of the longest backward branch inside body (relative line numbers)"""
    labels = {}
    for i, ln in enumerate(body):
        m = re.match(r"^(\.LBB\w+):", ln)
        if m:
            labels[m.group(1)] = i
    def leaves(at):      # the block at a label is the kernel's exit (the compiler may place it first: every early return jumps "back" to it)
        for ln in body[at + 1:at + 4]:
            if re.match(r"^\s+s_endpgm", ln):
                return True
        return False
    best = (0, 0)
    for i, ln in enumerate(body):
        m = re.match(r"^\s+s_c?branch\w*\s+(\.LBB\w+)", ln)
        if m and m.group(1) in labels and labels[m.group(1)] < i and i - labels[m.group(1)] > best[1] - best[0] and not leaves(labels[m.group(1)]):
            best = (labels[m.group(1)], i)
    return best


def count(body):
    c = collections.Counter()
    mem = collections.Counter()
    for ln in body:
        m = re.match(r"^\s+([a-z]\w+)", ln)
        if not m:
            continue
        op = m.group(1)
        c["instructions"] += 1
        if op.startswith("v_"):
            c["VALU"] += 1
            if op.startswith(("v_readlane", "v_writelane")):
                c["v_readlane+v_writelane"] += 1
            if op.startswith(ADDR64):
                c["64-bit address"] += 1
        elif op.startswith("s_"):
            if op.startswith("s_cbranch") or op.startswith("s_branch"):
                c["branches"] += 1
            elif not op.startswith(NOT_SALU):
                c["SALU"] += 1
        elif op.startswith(MEM):
            c["memory"] += 1
            mem[re.sub(r"_e(32|64)$", "", op)] += 1
    return c, mem


def resources(path):
    out, name = {}, None
    for ln in open(path):
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+(\w[\w /\[\]]*?): (\S+) \[", ln)
        if m and name:
            out[name][m.group(1).strip()] = m.group(2)
    return out


def main():
    args = sys.argv[1:]
    asm = args.pop(0)
    res = resources(args.pop(0)) if args and not args[0].startswith("k_") else {}
    want = args or DEFAULT
    lines = [ln for f in asm.split(",") for ln in open(f).read().split("\n")]      # (both units: their functions have distinct names)
    fns = functions(lines)
    for w in want:
        for name, (a, b) in fns.items():
            if w not in name:
                continue
            body = lines[a:b]
            lo, hi = period_loop(body)
            c, mem = count(body[lo:hi + 1])
            print(f"{name}: period loop lines +{lo}..+{hi}")
            for k in ("instructions", "VALU", "SALU", "branches", "v_readlane+v_writelane", "64-bit address", "memory"):
                print(f"   {k}: {c[k]}")
            print("   by mnemonic: " + ", ".join(f"{k} {v}" for k, v in sorted(mem.items())))
            wc, _ = count(body)
            print(f"   whole kernel: VALU {wc['VALU']}, SALU {wc['SALU']}, v_readlane+v_writelane {wc['v_readlane+v_writelane']}, 64-bit address {wc['64-bit address']}")
            if name in res:
                print("   resources: " + ", ".join(f"{k} {v}" for k, v in res[name].items()))


if __name__ == "__main__":
    main()
