"""The dynamic LDS of the six persistent sweeps (hank_xsweep.h) is laid out by ONE function per kernel in hank_xlds.h: the kernel takes
its pointers from the struct, the host sizes the launch from the same struct's `bytes`. A piece that outgrew the size would let a
workgroup write past its LDS or into ctl[] (the group placement and a vote's outcome), so the layout is checked here piece by piece,
and `bytes` against the formulas of the size functions the layouts replace (transcribed below from the commit before them: the
schedule decisions x_supported / x_tan_fits / x_dual_back_fits were tuned on those numbers and must not move). Plain integers in a
header without device code: compiled alone by the host compiler here, no GPU and no library."""
import itertools
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "julia-newtonraphsonhank_amd" / "csrc"
CTL = 64
NE, NA, PS, DS = range(1, 17), (1, 63, 64, 127, 2048, 4000), (1, 2, 8, 299, 499), (1, 2, 4)
MAIN = """#include "hank_xlds.h"
#include <cstdio>
#include <cstring>
#include <initializer_list>
using namespace hank;
static void put(std::initializer_list<unsigned long long> v) { for (unsigned long long x : v) printf("%llu ", x); printf("\\n"); }
int main() {      // one question per line of standard input: kernel n_e n_a P D val; one line of byte offsets (declared order, ctl, bytes) each
    static_assert(XCTL_BYTES == 64, "the test's CTL");
    char k[32];
    int ne, na, P, D, val;
    while (scanf("%31s %d %d %d %d %d", k, &ne, &na, &P, &D, &val) == 6) {
        if (!strcmp(k, "primal_back")) { const XLdsPrimalBack L = xlds_primal_back(ne, na, P); put({L.Vsh, L.Pish, L.ash, L.xsh, L.ctl, L.bytes}); }
        else if (!strcmp(k, "vfi")) { const XLdsVfi L = xlds_vfi(ne, na); put({L.Vsh, L.Pish, L.ash, L.redsh, L.ctl, L.bytes}); }
        else if (!strcmp(k, "stat")) { const XLdsStat L = xlds_stat(ne); put({L.tile, L.redsh, L.ctl, L.bytes}); }
        else if (!strcmp(k, "tan_back")) { const XLdsTanBack L = xlds_tan_back(ne, P, D); put({L.tile, L.rhosh, L.pxsh, L.dxsh, L.srcsh, L.ctl, L.bytes}); }
        else if (!strcmp(k, "dual_back")) { const XLdsDualBack L = xlds_dual_back(ne, na, P, D); put({L.tile, L.ash, L.xsh, L.dxsh, L.ctl, L.bytes}); }
        else if (!strcmp(k, "fwd")) { const XLdsFwd L = xlds_fwd(ne, P, D, val != 0); put({L.tile, L.aggsh, L.Pish, L.closh, L.srcsh, L.ctl, L.bytes}); }
        else return 2;
    }
    return 0;
}
"""


def tile_sl(D):
    """XTileT<D>::SL: the slots of a tangent tile entry"""
    return {1: 1, 2: 2, 4: 6}[D]


def slots_sl(NSL):
    """XSlots<NSL>::SL: the slots of a tile entry that carries NSL numbers"""
    return NSL if NSL <= 2 else (6 if NSL <= 6 else 10)


# ---- what each kernel keeps in LDS: (name, elements, bytes per element, read or written 16 bytes at a time), in declared order, ctl excluded
def pieces(kernel, ne, na, P, D, val):
    if kernel == "primal_back":
        return [("Vsh", ne * 64, 8, False), ("Pish", ne * ne, 8, False), ("ash", na, 8, False), ("xsh", 4 * P, 8, False)]
    if kernel == "vfi":
        return [("Vsh", ne * 64, 8, False), ("Pish", ne * ne, 8, False), ("ash", na, 8, False), ("redsh", 16, 8, False)]
    if kernel == "stat":
        return [("tile", ne * 64, 8, False), ("redsh", 16, 8, False)]
    if kernel == "tan_back":
        SL = tile_sl(D)
        return [("tile", SL * ne * 64, 8, SL >= 2), ("rhosh", P, 8, False), ("pxsh", 3 * P, 8, False), ("dxsh", 3 * P * D, 8, D >= 2), ("srcsh", P, 4, False)]
    if kernel == "dual_back":
        SL = slots_sl(D + 1)
        return [("tile", SL * ne * 64, 8, SL >= 2), ("ash", na, 8, False), ("xsh", 4 * P, 8, True), ("dxsh", 3 * P * D, 8, D >= 2)]
    if kernel == "fwd":
        NSL = D + val
        SL, NAP = slots_sl(NSL), 2 * NSL
        return [("tile", SL * ne * 64, 8, SL >= 2), ("aggsh", ne * 64 * NAP, 8, NAP >= 2), ("Pish", ne * ne, 8, False), ("closh", P * ne, 4, False), ("srcsh", P, 4, False)]
    raise KeyError(kernel)


# ---- the size functions of the commit before hank_xlds.h (x_lds_* in hank_xsweep.h), line by line: sizeof(double) = 8, sizeof(int) = 4
def parent_bytes(kernel, ne, na, P, D, val):
    if kernel == "primal_back":
        return 8 * (ne * 64 + ne * ne + na + 4 * P) + CTL
    if kernel == "vfi":
        return 8 * (ne * 64 + ne * ne + na + 16) + CTL
    if kernel == "stat":
        return 8 * (ne * 64 + 16) + CTL
    if kernel == "tan_back":
        return 8 * (tile_sl(D) * ne * 64 + P + 1 + 3 * P + 1 + 3 * P * D) + 4 * P + CTL
    if kernel == "dual_back":
        return 8 * (slots_sl(D + 1) * ne * 64 + na + 1 + 4 * P + 3 * P * D) + CTL
    if kernel == "fwd":
        NSL = D + val
        NAP = 2 * NSL
        return 8 * (slots_sl(NSL) * ne * 64 + ne * ne + 1 + ne * 64 * NAP) + 4 * (P * ne + P) + CTL
    raise KeyError(kernel)


def shapes():
    """every kernel at n_e = 1..16, the n_a that make a last member full, one row or many, short and long horizons, every D; the forward
    sweep with and without the value, and the Float64 sweep (D = 0 with the value)"""
    for ne in NE:
        yield ("stat", ne, 1, 1, 1, 0)
        for na in NA:
            yield ("vfi", ne, na, 1, 1, 0)
            for P in PS:
                yield ("primal_back", ne, na, P, 1, 0)
                for D in DS:
                    yield ("dual_back", ne, na, P, D, 0)
        for P in PS:
            for D in DS:
                yield ("tan_back", ne, 1, P, D, 0)
                yield ("fwd", ne, 1, P, D, 0)
                yield ("fwd", ne, 1, P, D, 1)
            yield ("fwd", ne, 1, P, 0, 1)


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    """hank_xlds.h compiled ALONE by the host compiler (it is plain C++: no HIP, no library); every shape asked in one run."""
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/lib/llvm/bin/clang++") if c and Path(c).exists()), None)
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("xlds")
    (d / "main.cpp").write_text(MAIN)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", str(CSRC), "-o", str(d / "xlds"), str(d / "main.cpp")], check=True, capture_output=True, timeout=120)
    asked = list(shapes())
    out = subprocess.run([str(d / "xlds")], input="".join(" ".join(str(v) for v in s) + "\n" for s in asked), check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()
    assert len(out) == len(asked)
    return [(s, [int(v) for v in line.split()]) for s, line in zip(asked, out)]


def test_every_kernel_and_shape_is_asked(layouts):
    asked = {s for s, _ in layouts}
    assert {s[0] for s in asked} == {"primal_back", "vfi", "stat", "tan_back", "dual_back", "fwd"}
    assert {s for s in asked if s[0] == "dual_back"} == {("dual_back", ne, na, P, D, 0) for ne, na, P, D in itertools.product(NE, NA, PS, DS)}
    assert {s for s in asked if s[0] == "fwd"} == {("fwd", ne, 1, P, D, v) for ne, P, D, v in itertools.product(NE, PS, DS, (0, 1))} | {("fwd", ne, 1, P, 0, 1) for ne in NE for P in PS}
    assert {s for s in asked if s[0] == "tan_back"} == {("tan_back", ne, 1, P, D, 0) for ne, P, D in itertools.product(NE, PS, DS)}


def test_pieces_in_order_disjoint_as_long_as_stated_and_aligned(layouts):
    """A piece runs from its offset to the next piece's: it must hold its element count, and what is left over is a pad of less than
    16 bytes. Pieces of doubles, and int pieces behind them, sit on multiples of 8; an int piece behind an ODD count of ints can only
    sit on an odd multiple of 4 (tan_back's ctl at odd P; fwd's srcsh and ctl at odd P n_e, odd P (n_e + 1)): the size the layouts
    must reproduce puts it there, and nothing reads ints wider than 4 bytes."""
    for s, off in layouts:
        ps = pieces(*s)
        assert len(off) == len(ps) + 2, s
        assert off[0] == 0, s
        ints = 0                       # ints stated since the last piece of doubles
        for i, (name, count, size, wide) in enumerate(ps):
            length = off[i + 1] - off[i]
            assert 0 <= count * size <= length < count * size + 16, (s, name, off)
            assert off[i] % 8 == (4 if ints % 2 else 0), (s, name, off)
            if wide:
                assert off[i] % 16 == 0, (s, name, off)
            ints = ints + count if size == 4 else 0
        assert off[len(ps)] % 8 == (4 if ints % 2 else 0), (s, "ctl", off)


def test_ctl_is_the_last_64_bytes(layouts):
    for s, off in layouts:
        ctl, total = off[-2], off[-1]
        assert total == ctl + CTL, (s, off)
        assert ctl >= off[-3], (s, off)


def test_bytes_equal_the_replaced_size_functions(layouts):
    for s, off in layouts:
        assert off[-1] == parent_bytes(*s), (s, off)
