"""The source walk of the persistent forward sweeps (k_xfwd in hank_xsweep.h) after two changes to how its ds_add_f64 meet the LDS:

  slot-major tile   k_xfwd<D, true, ., true> (the Dual pass on the packed record) keeps its tile [column][slot][lane] (hank_xlds.h:
                    xtile_soa_at) instead of [column][lane][SL]. Same sums in the same order: the bits must not move. The instance
                    that reads the three-array record, k_xfwd<D, true>, keeps the old tile and makes the same sums — HANK_XFWD_PACKED=0
                    sends the Dual pass through it, and the aggregate and its partials must agree byte for byte
  transposed walk   (HANK_XFWD_FLAT_TR; measured slower and built off by default, DESIGN.md section 4 — the checks hold for either
                    build) a FLAT work unit (more than 3/2 sources per row of its target run) deals a trip's 64 sources four apart inside each
                    16-lane group, in every k_xfwd. The terms of a tile entry arrive in another lane order: rows with three or more
                    contributors may move in the last bits, so every kernel that carries the value must walk the same units the same
                    way — hank_primal's aggregate equals the Dual pass's bit for bit — and the suite's tolerances hold against the
                    oracle (rel 1e-10 + abs 1e-12) and the launches (1e-12, policy partials bit for bit)

Shapes: the calibrated n_a = 63, 64, 130 x n_e = 2, 11 at T = 6 and the six raw-grid economies of cases.FWD_ECONOMIES (both clamps,
virtual rows that carry mass, units of more than 64 sources), both entry points at N = 17 and 32 under the forced persistent
schedule. That the transposed arm runs is asserted on the CPU from the oracle's policy alone (work_units below restates
k_xunits_fwd's cut as cases.forward_edges does): several economies have flat units, and one has a flat unit of more than 64 lanes,
whose second trip (i0 = 64) takes the same map."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import cases
from cases import FAMILY, FWD_ECONOMIES, XRW, against_oracle_and_launches, raw_block, raw_economy

CSRC = Path(__file__).resolve().parent.parent / "julia-newtonraphsonhank_amd" / "csrc"
T = 6
NS = (17, 32)
XFLAT_NUM, XFLAT_DEN = 3, 2          # csrc/hank_device.h


def work_units(grid, pol):
    """the work units of a policy sequence pol (P, n_a, n_e): (t, member, column, cnt sources, ta, tb, lanes) each, lanes = cnt + the
    virtual lanes of the unit that walks source row 0 of an open column (cases.forward_edges' loop, which keeps only the counts)."""
    P, n_a, n_e = pol.shape
    S = -(-n_a // XRW)
    m0 = np.searchsorted(grid, pol, side="left")
    clo = (m0 == 0).sum(axis=1)
    lo = np.where(m0 == 0, -1, np.where(m0 >= n_a, n_a - 2, m0 - 1))
    anyclo = (clo > 0).any(axis=1)
    prev = np.concatenate([[False], anyclo[:-1]])
    out = []
    for t in range(P):
        for e in range(n_e):
            st = np.searchsorted(lo[t, :, e], np.arange(n_a + 1), side="left")
            for m in range(S):
                r0, nrows = m * XRW, min(XRW, n_a - m * XRW)
                ta = 0
                while ta < nrows:
                    ja = st[max(r0 + ta - 1, 0)]
                    has0 = ja == 0 and clo[t, e] <= 0 and prev[t]
                    lanes = lambda b: (st[r0 + b] - ja) + (S if has0 and st[r0 + b] > ja else 0)       # noqa: E731
                    tb = ta + 1
                    while tb < nrows and lanes(tb + 1) <= 64:
                        tb += 1
                    if st[r0 + tb] > ja:
                        out.append((t, m, e, int(st[r0 + tb] - ja), ta, tb, int(lanes(tb))))
                    ta = tb
    return out


def flat(u):
    """k_xfwd's unit_flat on a unit of work_units"""
    _, _, _, cnt, ta, tb, _ = u
    return XFLAT_DEN * cnt > XFLAT_NUM * (tb - ta)


def _policy(ec):
    return ec["orc"].block(ec["x"], None, ec["V"], ec["D"])[2]


def test_the_transposed_arm_runs():
    """(CPU) from the oracle's policy alone: the work-unit cut agrees with cases.forward_edges' counts; at least two of the raw-grid
    economies have flat units in some member and column, next to units that are not flat; one has a flat unit of more than 64 lanes."""
    have, wide = [], []
    for name in FWD_ECONOMIES:
        ec = raw_economy(name)
        pol = _policy(ec)
        us = work_units(ec["grid"], pol)
        fe = cases.forward_edges(ec["grid"], pol)
        assert len(us) == fe["units"].sum() and max(u[6] for u in us) == fe["longest"], name
        fl = [u for u in us if flat(u)]
        print(f"{name}: {len(us)} units, {len(fl)} flat, {sum(1 for u in fl if u[6] > 64)} flat of more than 64 lanes, "
              f"most sources per target row of a flat unit {max((u[3] / (u[5] - u[4]) for u in fl), default=0):.1f}")
        if fl and len(fl) < len(us):
            have.append(name)
        if any(u[6] > 64 for u in fl):
            wide.append(name)
    assert len(have) >= 2, have
    assert wide, "no flat unit with a trip at i0 = 64"


def _check(seen, what):
    assert len(seen) == 1
    for sched, env, st, info in seen:
        assert st["schedule"] == 1 and st["fallbacks"] == 0, (what, st)
        assert info["last_tangent_family_name"] == FAMILY["xcd"], (what, info)


def _bits(hank, shape, what):
    """under the forced persistent schedule at N = 32: a repeated Dual pass returns the same bits; hank_primal's aggregate is the Dual
    pass's bit for bit; the Dual pass on the three-array record (old tile) returns the packed-record instance's bytes."""
    m, V, D, xhh, _ = shape
    args = m if isinstance(m, tuple) else cases.model_args(m)
    y = np.random.default_rng(7).standard_normal((xhh.shape[0], xhh.shape[1], 32))
    got = {}
    for packed in (None, 0):
        hb = raw_block(hank, args, "xcd", HANK_XFWD_PACKED=packed)
        hb.set_boundary(V, D)
        agg, dagg = hb.primal_jvp(xhh, y)
        hb.primal(xhh * 1.01)                                     # (another record: the next call is no memo hit)
        agg2, dagg2 = hb.primal_jvp(xhh, y)
        assert np.array_equal(agg, agg2) and np.array_equal(dagg, dagg2), (what, packed, "a repeated Dual pass")
        hb.primal(xhh * 1.01)
        assert np.array_equal(hb.primal(xhh), agg), (what, packed, "hank_primal's aggregate against the Dual pass's")
        st = hb.stats()
        assert st["schedule"] == 1 and st["fallbacks"] == 0, (what, packed, st)
        hb.close()
        got[packed] = (agg, dagg)
    assert got[None][0].tobytes() == got[0][0].tobytes(), (what, "agg: slot-major tile against the [lane][SL] tile")
    assert got[None][1].tobytes() == got[0][1].tobytes(), (what, "dagg: slot-major tile against the [lane][SL] tile")


@pytest.mark.gpu
@pytest.mark.parametrize("n_a", (63, 64, 130))
@pytest.mark.parametrize("n_e", (2, 11))
def test_calibrated_shapes(hank, n_e, n_a):
    shape = cases.shape(n_a, n_e, T)
    _check(against_oracle_and_launches(hank, shape, [("xcd", {})], NS), (n_a, n_e))
    _bits(hank, shape, (n_a, n_e))


@pytest.mark.gpu
@pytest.mark.parametrize("name", FWD_ECONOMIES)
def test_raw_grid_economies(hank, name):
    ec = raw_economy(name)
    shape = (ec["args"], ec["V"], ec["D"], ec["x"], ec["orc"])
    _check(against_oracle_and_launches(hank, shape, [("xcd", {})], NS), name)
    _bits(hank, shape, name)


# ---- the slot-major layout (CPU: hank_xlds.h is plain C++) ------------------------------------------------------------------------
MAIN = """#include "hank_xlds.h"
#include <cstdio>
using namespace hank;
int main() {      // n_e P D per line of standard input -> the tile piece's offset and length, bytes, the slot-major tile's bytes, then every entry's offset
    int ne, P, D;
    while (scanf("%d %d %d", &ne, &P, &D) == 3) {
        const XLdsFwd F = xlds_fwd(ne, P, D, true);
        const XLdsFwdLq L = xlds_fwd_lq(ne, 64, P, D);
        printf("%u %u %zu %zu %d", L.tile, L.aggsh - L.tile, F.bytes, xtile_soa_bytes(ne, D + 1), XTILE_SOA_SLOT);
        for (int c = 0; c < ne; c++) for (int k = 0; k < D + 1; k++) for (int l = 0; l < 64; l++) printf(" %u", xtile_soa_at(D + 1, c, k, l));
        printf("\\n");
    }
    return 0;
}
"""
LAYOUT_SHAPES = [(ne, P, D) for ne in (1, 2, 3, 7, 11, 16) for P in (1, 5, 299) for D in (1, 2, 4)]


def test_slot_major_tile_layout(tmp_path):
    """xtile_soa_at: [column][slot][lane] in doubles — a bijection onto the first n_e (D + 1) 64 doubles of the tile piece, lanes
    contiguous, slots 512 bytes apart, inside the piece xlds_fwd states; `bytes` is what tests/test_xlds_host.py pins for xlds_fwd."""
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/lib/llvm/bin/clang++") if c and Path(c).exists()), None)
    assert cxx, "no host C++ compiler"
    (tmp_path / "main.cpp").write_text(MAIN)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", str(CSRC), "-o", str(tmp_path / "xlds"), str(tmp_path / "main.cpp")], check=True, capture_output=True, timeout=120)
    out = subprocess.run([str(tmp_path / "xlds")], input="".join("%d %d %d\n" % s for s in LAYOUT_SHAPES), check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()
    assert len(out) == len(LAYOUT_SHAPES)
    for (ne, P, D), line in zip(LAYOUT_SHAPES, out):
        v = [int(x) for x in line.split()]
        tile, length, total, soa, slot = v[:5]
        at = np.array(v[5:]).reshape(ne, D + 1, 64)
        NSL = D + 1
        SL = NSL if NSL <= 2 else (6 if NSL <= 6 else 10)
        s = (ne, P, D)
        assert tile == 0 and tile % 16 == 0 and length == 8 * SL * ne * 64, (s, "the tile piece")
        assert total == 8 * (SL * ne * 64 + ne * ne + 1 + ne * 64 * 2 * NSL) + 4 * (P * ne + P) + 64, (s, "bytes moved")
        assert slot == 64 and soa == 8 * NSL * ne * 64 and soa <= length, (s, "the slot-major tile lies inside the piece")
        assert np.array_equal(np.sort(at.ravel()), 8 * np.arange(ne * NSL * 64)), (s, "not a bijection onto the tile's doubles")
        assert np.all(np.diff(at, axis=2) == 8) and np.all(np.diff(at, axis=1) == 512) and np.all(np.diff(at, axis=0) == 512 * NSL), s
