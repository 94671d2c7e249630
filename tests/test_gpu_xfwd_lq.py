"""The Dual pass's forward sweep on the packed lottery record (k_xfwd<D, true, ., true> in hank_xsweep.h).

In front of a persistent Dual pass the lottery (k_lottery_lq) writes, next to lo / lw / ig, one 16-byte record per source,
{double w; int lo; int flags}, flags bit 0 = "ig is zero" (the source is clamped at either end of the grid). The sweep loads that
record with one instruction instead of three and takes ig from the wealth grid's inverse gaps, iga[l] = 1 / (a[l+1] - a[l]) (last
entry 0), staged in LDS between srcsh and ctl (xlds_fwd_lq in hank_xlds.h). Its results must be the three-load instance's, which
the launches and the CPU oracle stand for here:

  sweep cases   both entry points at N = 17 and 32 (D = 4: four and five tile slots; 17 leaves the last group one direction) under
                the forced persistent schedule, against the oracle at rel 1e-10 + abs 1e-12 and the launches at 1e-12 (policy
                partials bit for bit): the calibrated shapes n_a = 63, 64, 130 x n_e = 2, 11 at T = 6 (one member, a second member
                of one row, three members) and every raw-grid economy of cases.FWD_ECONOMIES — the low clamp (dense-bottom, both,
                deep-prefix), sources capped at the top (short-top, both, swing), virtual rows that carry mass (swing, collapse) and
                units of more than 64 sources, whose later trips and rare units read the record inside the period (deep-prefix)
  record case   after a Dual pass: lq.w == lw, lq.lo == lo and ig == (flags & 1 ? 0 : iga[lo]) bit for bit at every entry. On
                `short-top` the value function caps the policy AT the last grid point: such a source is interior (searchsortedfirst
                finds the last point itself), w = 1 at lo = n_a - 2 with ig != 0 — the bracket and weight of a top clamp, and only
                the flag tells them apart. test_short_top_has_a_source_on_the_last_grid_point asserts on the CPU that the oracle's
                policy has such sources
  layout case   hank_xlds.h compiled alone by the host compiler: xlds_fwd_lq keeps xlds_fwd's pieces where they are, the table
                on a multiple of 16 behind srcsh, ctl last"""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import cases
from cases import FAMILY, FWD_ECONOMIES, against_oracle_and_launches, raw_block, raw_economy

CSRC = Path(__file__).resolve().parent.parent / "julia-newtonraphsonhank_amd" / "csrc"
T = 6
NS = (17, 32)


def _check(seen, what):
    assert len(seen) == 1
    for sched, env, st, info in seen:
        assert st["schedule"] == 1 and st["fallbacks"] == 0, (what, st)
        assert info["last_tangent_family_name"] == FAMILY["xcd"], (what, info)


@pytest.mark.gpu
@pytest.mark.parametrize("n_a", (63, 64, 130))
@pytest.mark.parametrize("n_e", (2, 11))
def test_calibrated_shapes(hank, n_e, n_a):
    _check(against_oracle_and_launches(hank, cases.shape(n_a, n_e, T), [("xcd", {})], NS), (n_a, n_e))


def _raw_shape(name):
    ec = raw_economy(name)
    return ec["args"], ec["V"], ec["D"], ec["x"], ec["orc"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", FWD_ECONOMIES)
def test_raw_grid_economies(hank, name):
    _check(against_oracle_and_launches(hank, _raw_shape(name), [("xcd", {})], NS), name)


def _on_last_point(ec):
    """the oracle's policy (P, n_a, n_e) of a raw economy and where it sits exactly on the last grid point"""
    pol = ec["orc"].block(ec["x"], None, ec["V"], ec["D"])[2]
    return pol, pol == ec["grid"][-1]


def test_short_top_has_a_source_on_the_last_grid_point():
    """(CPU) the record case's premise: `short-top` has sources whose policy IS the last grid point — interior for searchsortedfirst,
    bracket n_a - 2 with weight exactly 1 and a finite inverse gap — and `dense-bottom` has sources clamped at the first."""
    ec = raw_economy("short-top")
    grid = ec["grid"]
    pol, on = _on_last_point(ec)
    assert on.sum() >= 8, on.sum()
    m0 = np.searchsorted(grid, pol[on], side="left")              # searchsortedfirst: grid[m0 - 1] < pol <= grid[m0]
    assert np.all(m0 == grid.size - 1)
    gap = grid[-1] - grid[-2]
    assert np.all((pol[on] - grid[-2]) / gap == 1.0) and np.isfinite(1.0 / gap) and 1.0 / gap != 0.0
    ec = raw_economy("dense-bottom")
    assert np.any(ec["orc"].block(ec["x"], None, ec["V"], ec["D"])[2] <= ec["grid"][0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("short-top", "dense-bottom"))
def test_packed_record_is_the_lottery(hank, name):
    """lo, lw, ig, lq and iga read back after a Dual pass on the persistent sweeps (N = 32: k_xdual_back<4> and the packed-record
    instance of k_xfwd<4, true>), entry by entry and bit for bit."""
    ec = raw_economy(name)
    grid, n_a = ec["grid"], ec["grid"].size
    hb = raw_block(hank, ec["args"], "xcd")
    hb.set_boundary(ec["V"], ec["D"])
    y = np.random.default_rng(41).standard_normal((2, ec["x"].shape[1], 32))
    hb.primal_jvp(ec["x"], y)
    st, info = hb.stats(), hb.info()
    assert st["schedule"] == 1 and st["fallbacks"] == 0 and info["last_tangent_family_name"] == FAMILY["xcd"], (st, info)
    rec = hb.lottery_record()
    pol = hb.policy_seq()                                         # (n_a, n_e, P), like the record's arrays
    hb.close()
    lo, lw, ig, lq, iga = rec["lo"], rec["lw"], rec["ig"], rec["lq"], rec["iga"]
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)      # noqa: E731
    want = np.empty(n_a)
    want[:-1], want[-1] = 1.0 / (grid[1:] - grid[:-1]), 0.0
    assert np.array_equal(bits(iga), bits(want)), "iga"
    assert np.array_equal(lq["lo"], lo), "lq.lo"
    assert np.array_equal(bits(lq["w"]), bits(lw)), "lq.w"
    assert np.all((lq["flags"] == 0) | (lq["flags"] == 1)), "flags"
    assert lo.min() >= 0 and lo.max() <= n_a - 2
    assert np.array_equal(bits(np.where(lq["flags"] & 1, 0.0, iga[lo])), bits(ig)), "ig == (flags & 1 ? 0 : iga[lo])"
    low = pol <= grid[0]
    assert np.array_equal(lq["flags"] == 1, low | (pol > grid[-1])), "the flag is set exactly at the clamps"
    if name == "short-top":      # on the last grid point: a top clamp's bracket and weight, told apart by the flag alone
        on = pol == grid[-1]
        assert on.sum() >= 8
        assert np.all(lo[on] == n_a - 2) and np.all(lw[on] == 1.0) and np.all(ig[on] != 0.0) and np.all(lq["flags"][on] == 0)
    else:
        assert low.sum() >= 8 and np.all(lo[low] == 0) and np.all(lw[low] == 0.0) and np.all(ig[low] == 0.0)


# ---- the layout (CPU: hank_xlds.h is plain C++) ---------------------------------------------------------------------------------
MAIN = """#include "hank_xlds.h"
#include <cstdio>
using namespace hank;
int main() {      // n_e n_a P D per line of standard input -> xlds_fwd's offsets and bytes, then xlds_fwd_lq's
    int ne, na, P, D;
    while (scanf("%d %d %d %d", &ne, &na, &P, &D) == 4) {
        const XLdsFwd F = xlds_fwd(ne, P, D, true);
        const XLdsFwdLq L = xlds_fwd_lq(ne, na, P, D);
        printf("%u %u %u %u %u %u %zu  %u %u %u %u %u %u %u %zu\\n", F.tile, F.aggsh, F.Pish, F.closh, F.srcsh, F.ctl, F.bytes,
               L.tile, L.aggsh, L.Pish, L.closh, L.srcsh, L.iga, L.ctl, L.bytes);
    }
    return 0;
}
"""
LAYOUT_SHAPES = [(ne, na, P, D) for ne in range(1, 17) for na in (2, 63, 64, 127, 2000, 2048) for P in (1, 2, 5, 8, 299) for D in (1, 2, 4)]


def test_layout_keeps_the_sweeps_pieces_and_ends_with_ctl(tmp_path):
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/lib/llvm/bin/clang++") if c and Path(c).exists()), None)
    assert cxx, "no host C++ compiler"
    (tmp_path / "main.cpp").write_text(MAIN)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", str(CSRC), "-o", str(tmp_path / "xlds"), str(tmp_path / "main.cpp")], check=True, capture_output=True, timeout=120)
    out = subprocess.run([str(tmp_path / "xlds")], input="".join("%d %d %d %d\n" % s for s in LAYOUT_SHAPES), check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()
    assert len(out) == len(LAYOUT_SHAPES)
    for (ne, na, P, D), line in zip(LAYOUT_SHAPES, out):
        v = [int(x) for x in line.split()]
        F, L = v[:7], v[7:]
        s = (ne, na, P, D)
        assert L[:5] == F[:5], (s, "xlds_fwd's pieces moved")                # tile, aggsh, Pish, closh, srcsh
        srcsh, iga, ctl, total = L[4], L[5], L[6], L[7]
        assert iga % 16 == 0 and srcsh + 4 * P <= iga < srcsh + 4 * P + 16, (s, "the table: aligned, right behind srcsh")
        assert ctl == iga + 8 * na and ctl % 8 == 0, (s, "ctl right behind the table")
        assert total == ctl + 64, (s, "ctl is the last piece")
        assert total - F[6] == 8 * na + (iga - F[5]), (s, "the carve grows by the table and its pad")
