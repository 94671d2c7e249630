"""The Dual-pass persistent sweeps reach the record and a launch's dpol through buffer descriptors with 32-bit offsets, and the work
units (which keep their pointer) with a 32-bit index (XRecOff and unit_ld, hank_xsweep.h). x_addr_fits (hank_xaddr.h) is the ONE
predicate the host asks where it chooses the schedule: every stream's bytes, plus room for the largest lane offset (XADDR_MARGIN =
2^24, which must hold a whole period of a group's dpol: G D 8 bytes), stay below 2^32. Plain integers in a header without device
code: compiled alone by the host compiler here, no GPU and no library."""
import shutil
import subprocess
from pathlib import Path

import pytest

MARGIN = 1 << 24
LIM = (1 << 32) - MARGIN
XG, XD_MAX, XUCAP, XRW = 8, 4, 64, 63
CSRC = Path(__file__).resolve().parent.parent / "julia-newtonraphsonhank_amd" / "csrc"
MAIN = """#include "hank_xaddr.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char **argv) {      // seven integers per question on the command line, one answer per line
    static_assert(hank::XADDR_MARGIN == (1ull << 24), "the test's MARGIN");
    for (int i = 1; i + 6 < argc; i += 7) {
        unsigned long long a[7];
        for (int k = 0; k < 7; k++) a[k] = strtoull(argv[i + k], nullptr, 10);
        printf("%d\\n", hank::x_addr_fits(a[0], a[1], a[2], a[3], a[4], a[5], a[6]) ? 1 : 0);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def fits(tmp_path_factory):
    """hank_xaddr.h compiled ALONE by the host compiler (it is plain C++: no HIP, no library) into a program that answers."""
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/lib/llvm/bin/clang++") if c and Path(c).exists()), None)
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("xaddr")
    (d / "main.cpp").write_text(MAIN)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", str(CSRC), "-o", str(d / "xaddr"), str(d / "main.cpp")], check=True, capture_output=True, timeout=120)

    def ask(*a):
        assert len(a) == 7
        out = subprocess.run([str(d / "xaddr")] + [str(int(v)) for v in a], check=True, capture_output=True, text=True, timeout=30).stdout.split()
        assert out in (["0"], ["1"]), out
        return out == ["1"]
    return ask


def _carve(sizes):
    off = 0
    for s in sizes:
        off = (off + 255) // 256 * 256 + s
    return off


def record_bytes(n_a, n_e, P):
    """the record's one allocation as hank_create carves it (256-byte aligned pieces)."""
    G = n_a * n_e
    d8 = P * G * 8
    return _carve([d8] * 9 + [(P + 1) * G * 8, P * G * 4, P * G * 4, P * n_e * (n_a + 1) * 4, P * n_e * 4, P * G * 16, P * G * 16])


def _shape(fits, n_a, n_e, T):
    P, G, members = T - 1, n_a * n_e, (n_a + XRW - 1) // XRW
    return fits(record_bytes(n_a, n_e, P), P, XG, G, XD_MAX, members, XUCAP)


def test_the_benched_shapes_fit(fits):
    assert record_bytes(2000, 11, 299) < 1 << 30          # (0.79 GB: far below the limit)
    assert _shape(fits, 2000, 11, 300)                    # the headline: 2000x11, T = 300, N = 32
    assert _shape(fits, 1000, 7, 500)                     # 1000x7, T = 500, N = 32


def test_each_stream_just_below_and_just_above_the_limit(fits):
    small = (1 << 20, 10, 8, 1000, 4, 2, 64)              # every stream tiny
    assert fits(*small)
    # the record
    assert fits(LIM, *small[1:]) and not fits(LIM + 1, *small[1:])
    assert not fits((1 << 32) - 1, *small[1:]) and not fits(1 << 32, *small[1:]) and not fits((1 << 32) + 1, *small[1:])
    # dpol: P groups G D 8 bytes; G = 2^16, D = 4, groups = 8 -> 2^24 bytes a period (the margin holds one period of one group: 2^21)
    G = 1 << 16
    per = 8 * G * 4 * 8
    P_ok = LIM // per
    assert fits(1 << 20, P_ok, 8, G, 4, 2, 64) and not fits(1 << 20, P_ok + 1, 8, G, 4, 2, 64)
    assert not fits(1 << 20, (1 << 32) // per, 8, G, 4, 2, 64)       # exactly 2^32 bytes
    # the work units: P members ucap 8 bytes
    per_u = 32 * 64 * 8
    P_u = LIM // per_u
    assert fits(1 << 20, P_u, 1, 100, 1, 32, 64) and not fits(1 << 20, P_u + 1, 1, 100, 1, 32, 64)
    # the margin itself: one period of a group's dpol (the largest lane offset) must fit in it
    assert fits(1 << 20, 1, 1, MARGIN // 32, 4, 2, 64) and not fits(1 << 20, 1, 1, MARGIN // 32 + 1, 4, 2, 64)


def test_no_wraparound_in_the_products(fits):
    """sizes whose products pass 2^64 in 32-bit or wrap in careless 64-bit arithmetic must not look small."""
    assert not fits(1 << 20, 1 << 20, 8, 1 << 20, 4, 32, 64)          # 2^48 bytes of dpol
    assert not fits(1 << 40, 10, 8, 1000, 4, 2, 64)
