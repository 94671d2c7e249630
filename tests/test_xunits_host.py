"""The cut of one column's walk into the forward sweeps' work units is stated once, in hank_xunits.h: plain integers, compiled ALONE
by the host compiler here (no GPU, no library) and compared with a numpy transcription of k_xunits_fwd's greedy walk — "extend the
unit while it has at most 64 lanes" — on the steady-state policy of the 2000x11 fixture and on synthetic start tables: slope one,
flat (over 200 sources on 63 targets), a clamped prefix, a vanished mass point (clo = 0 while the virtual rows hold mass) and n_a
that is no multiple of 63.

What a cut must satisfy, asserted on every case: the units' target runs [ta, tb) are disjoint and in order, and every target row a
source touches lies in exactly one (a run without sources makes no unit, as in k_xunits_fwd); a unit has cnt + nv <= 64 lanes unless
it is a single target row, which cannot be split (k_xfwd walks such a unit in trips); every source whose bracket touches the
member's rows is walked; the sources on the seam between two neighbouring units are in both."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "julia-newtonraphsonhank_amd" / "csrc"
XRW = 63
MAIN = """#include "hank_xunits.h"
#include <cstdio>
#include <vector>
int main() {      // per table: n_a, start[0 .. n_a], q, then q lines "clo vnz r0 nrows Sact e m" -> "n mlo mhi anyv" and n lines "x y"
    int na;
    static_assert(hank::XU_ROWS == 63 && hank::XU_LANES == 64, "the sweeps' geometry");
    while (scanf("%d", &na) == 1) {
        std::vector<int> st(na + 1);
        for (int &v : st) if (scanf("%d", &v) != 1) return 1;
        int q;
        if (scanf("%d", &q) != 1) return 1;
        for (int k = 0; k < q; k++) {
            int clo, vnz, r0, nrows, Sact, e, m, u[2 * hank::XU_ROWS];
            if (scanf("%d %d %d %d %d %d %d", &clo, &vnz, &r0, &nrows, &Sact, &e, &m) != 7) return 1;
            const hank::XuCut c = hank::xu_cut_column(st.data(), na, clo, vnz != 0, r0, nrows, Sact, e, m, u, hank::XU_ROWS);
            printf("%d %d %d %d\\n", c.n, c.mlo, c.mhi, c.anyv);
            for (int i = 0; i < c.n; i++) printf("%d %d\\n", u[2 * i], u[2 * i + 1]);
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def cutter(tmp_path_factory):
    """hank_xunits.h compiled alone into a program that cuts the columns it is given."""
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/lib/llvm/bin/clang++") if c and Path(c).exists()), None)
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("xunits")
    (d / "main.cpp").write_text(MAIN)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", str(CSRC), "-o", str(d / "xunits"), str(d / "main.cpp")], check=True, capture_output=True, timeout=120)

    def cut(columns):
        """columns: [(start, clo, vnz, e)] of one grid -> per column and member (n, mlo, mhi, anyv, units (n, 2))"""
        text = []
        for start, clo, vnz, e in columns:
            na = len(start) - 1
            S = (na + XRW - 1) // XRW
            text.append("%d\n%s\n%d\n" % (na, " ".join(map(str, start)), S))
            text += ["%d %d %d %d %d %d %d\n" % (clo, vnz, m * XRW, min(XRW, na - m * XRW), S, e, m) for m in range(S)]
        out = subprocess.run([str(d / "xunits")], input="".join(text), check=True, capture_output=True, text=True, timeout=120).stdout.split()
        v, k, res = list(map(int, out)), 0, []
        for start, clo, vnz, e in columns:
            per = []
            for m in range((len(start) - 1 + XRW - 1) // XRW):
                n = v[k]
                per.append((n, v[k + 1], v[k + 2], v[k + 3], np.array(v[k + 4:k + 4 + 2 * n], dtype=np.int64).reshape(n, 2)))
                k += 4 + 2 * n
            res.append(per)
        assert k == len(v)
        return res
    return cut


def start_table(lo, clo):
    """lottery_body's segment offsets: start[r] = first source j >= clo with bracket lo_j >= r, start[n_a] = n_a"""
    n = lo.size
    return np.concatenate([clo + np.searchsorted(lo[clo:], np.arange(n), side="left"), [n]]).astype(np.int64)


def walk(start, clo, vnz, r0, nrows, Sact, e, m):
    """k_xunits_fwd's walk of one column for one member as a serial loop (the greedy form its bisection stands for)"""
    na = len(start) - 1
    S = lambda r: min(max(int(start[min(max(r, 0), na)]), 0), na)      # noqa: E731
    units, mlo, mhi, anyv, ta = [], m, m, 0, 0
    while ta < nrows:
        ja = S(max(r0 + ta - 1, 0))
        has0 = ja == 0 and clo <= 0 and vnz
        lanes = lambda b: (lambda c2: c2 + (Sact if has0 and c2 > 0 else 0))(max(S(r0 + b) - ja, 0))      # noqa: E731
        tb = ta + 1
        while tb < nrows and lanes(tb + 1) <= 64:
            tb += 1
        cnt = max(S(r0 + tb) - ja, 0)
        nv = Sact if has0 and cnt > 0 else 0
        if cnt > 0:
            units.append((e | ja << 4 | cnt << 16, ta | tb << 8 | nv << 16))
            mlo, mhi = min(mlo, ja // XRW), max(mhi, (ja + cnt - 1) // XRW)
            anyv |= 1 if nv else 0
        ta = tb
    return len(units), mlo, mhi, anyv, np.array(units, dtype=np.int64).reshape(len(units), 2)


def check_column(got, lo, clo, vnz, e):
    """one column's cut against the walk, and the four properties of the docstring"""
    na = lo.size
    start = start_table(lo, clo)
    Sact = (na + XRW - 1) // XRW
    j = np.arange(na)
    for m, (n, mlo, mhi, anyv, u) in enumerate(got):
        r0, nrows = m * XRW, min(XRW, na - m * XRW)
        wn, wlo, whi, wv, wu = walk(start, clo, vnz, r0, nrows, Sact, e, m)
        assert (n, mlo, mhi, anyv) == (wn, wlo, whi, wv) and np.array_equal(u, wu), (e, m)
        ee, ja, cnt = u[:, 0] & 15, (u[:, 0] >> 4) & 4095, u[:, 0] >> 16
        ta, tb, nv = u[:, 1] & 255, (u[:, 1] >> 8) & 255, u[:, 1] >> 16
        assert np.all(ee == e) and np.all(cnt > 0) and np.all(ta < tb) and np.all(tb <= nrows)
        assert np.all(ta[1:] >= tb[:-1]), "target runs in order, disjoint"
        assert np.all((cnt + nv <= 64) | (tb - ta == 1)), (e, m, cnt, nv)
        walked = np.zeros(na, bool)
        for k in range(n):
            walked[ja[k]:ja[k] + cnt[k]] = True
        touches = (j >= clo) & (lo + 1 >= r0) & (lo <= r0 + nrows - 1)
        assert np.all(walked[touches]), "a source whose bracket touches the member's rows is not walked"
        rows = np.zeros(nrows, int)
        for k in range(n):
            rows[ta[k]:tb[k]] += 1
        touched = np.zeros(na + 1, bool)
        touched[lo[clo:]] = True
        touched[lo[clo:] + 1] = True
        assert np.all(rows <= 1) and np.all(rows[touched[r0:r0 + nrows]] == 1), "a target row with sources lies in exactly one unit"
        for k in range(n - 1):
            if ta[k + 1] == tb[k]:      # neighbours: the sources with bracket r0 + tb - 1 feed rows on both sides of the seam
                seam = j[(j >= clo) & (lo == r0 + tb[k] - 1)]
                assert np.all((seam >= ja[k]) & (seam < ja[k] + cnt[k]) & (seam >= ja[k + 1]) & (seam < ja[k + 1] + cnt[k + 1])), (e, m, k)
        if vnz and clo == 0 and m == 0 and n:
            assert nv[0] == Sact and ja[0] == 0 and anyv == 1, "the unit that walks source row 0 of an open column carries the virtual lanes"


def brackets(grid, pol):
    """lottery_body's bracket per source and the clamped prefix of a monotone policy column"""
    hi = np.searchsorted(grid, pol, side="left")
    lo = np.where(hi == 0, 0, np.where(hi >= grid.size, grid.size - 2, hi - 1))
    return lo.astype(np.int64), int(np.count_nonzero(hi == 0))


def test_steady_state_policy_of_the_fixture(cutter):
    d = np.load(ROOT / "examples" / "fixtures" / "ks_ss_2000x11.npz")
    grid, pol = d["a_grid"], d["policy"]
    cols = [brackets(grid, pol[:, e]) for e in range(pol.shape[1])]
    for vnz in (0, 1):
        got = cutter([(start_table(lo, clo), clo, vnz, e) for e, (lo, clo) in enumerate(cols)])
        for e, (lo, clo) in enumerate(cols):
            check_column(got[e], lo, clo, vnz, e)
        per_member = np.sum([[g[0] for g in col] for col in got], axis=0)
        assert per_member.max() <= 64 and max(g[0] for col in got for g in col) <= 4, per_member      # (11-20 units per member at the steady state)


SYNTH = {
    # name: (lo per source, clo)
    "slope-one": (np.minimum(np.arange(200), 198), 0),
    "flat": (np.minimum(np.arange(260) * 63 // 260, 61), 0),                         # 260 sources on the first 63 targets of 260
    "flat-top": (np.minimum(70 + np.arange(300) * 50 // 300, 298), 0),               # ... on targets in the middle of the grid
    "clamped-prefix": (np.concatenate([np.zeros(90, int), np.arange(110) // 2]), 90),
    "vanished-mass-point": (np.minimum(np.arange(130) // 3, 128), 0),                 # clo = 0 while the virtual rows hold mass
    "one-row-over-64": (np.concatenate([np.full(100, 5), 6 + np.arange(89)]), 0),     # 100 sources on one target row: a unit that cannot be split
    "127": (np.minimum(np.arange(127) * 2 // 3, 125), 0),                             # n_a = 2 * 63 + 1: a last member of one row
    "64": (np.minimum(np.arange(64), 62), 3),
    "63": (np.minimum(np.arange(63) // 2, 61), 0),
}


@pytest.mark.parametrize("name", sorted(SYNTH))
def test_synthetic_start_tables(cutter, name):
    lo, clo = SYNTH[name]
    lo = np.asarray(lo, dtype=np.int64)
    assert np.all(np.diff(lo[clo:]) >= 0) and lo.max() <= lo.size - 2
    for vnz in (0, 1):
        for e in (0, 10):
            check_column(cutter([(start_table(lo, clo), clo, vnz, e)])[0], lo, clo, vnz, e)
    if name == "flat":
        n0 = cutter([(start_table(lo, clo), clo, 0, 0)])[0][0]
        assert n0[0] >= 5, "260 sources on one member's rows need at least five units"


def test_a_table_that_is_no_lottery_stays_in_range(cutter):
    """garbage start values (a policy that was not monotone: the call fails, but the cut still runs) are clamped into [0, n_a]"""
    rng = np.random.default_rng(5)
    start = rng.integers(-500, 900, 131)
    for per in cutter([(start, 0, 1, 2)]):
        for n, mlo, mhi, anyv, u in per:
            ja, cnt = (u[:, 0] >> 4) & 4095, u[:, 0] >> 16
            assert n <= XRW and np.all(ja >= 0) and np.all(ja + cnt <= 130) and 0 <= mlo <= mhi <= 2
