"""The bracket of the persistent backward sweeps (k_xprimal_back, k_xdual_back<1 | 2 | 4>; csrc/hank_xsweep.h) is named in
straight-line code from the preloaded knots when it is the one of the period before or a neighbour of it; every other lane — no
guess yet, a bracket that moved by two knots or more — goes through the search, behind a wave-uniform branch. A bracket is unique,
so neither path may change a bit: the persistent family (HANK_SCHEDULE=xcd) against the per-period launches on the policy and its
partials bit for bit, on the aggregates at 1e-12, for the Float64 sweep and the Dual pass at N = 8, 16, 32 (D = 1, 2, 4 partials per
group), on the raw-grid economies of tests/cases.py — `swing` and `collapse` move r by -0.6 / +1.5 between periods, which moves
brackets by many knots at once — a calibrated 130x3, a 64-row grid (two members, the second with one row) and `constrained`:
`short-top` with the borrowing constraint five grid points above the first one (in the economies of tests/cases.py the constraint
IS the first grid point, so the interpolated policy never falls below it and the rule that cuts the partials there never fires).

The CPU test at the end measures on the oracle's value path that these economies really hold every case the front and the search
distinguish, so the GPU tests cannot silently stop exercising the slow path."""
import numpy as np
import pytest

from cases import close, expected_family, model_args, raw_block, raw_economy, shape

RAW = ("swing", "collapse", "deep-prefix", "dense-bottom", "short-top")
MEASURED = RAW + ("constrained",)        # what the CPU test at the end measures
ECONOMIES = MEASURED + ("ks130x3", "ks64x3")
NS = (8, 16, 32)             # with 8 groups: D = 1, 2, 4


_OWN = {}


def _economy(name):
    """-> (HouseholdBlock's arguments, V_T (n_a, n_e), D_0, xhh (2, P), oracle)"""
    if name in RAW:
        ec = raw_economy(name)
        return ec["args"], ec["V"], ec["D"], ec["x"], ec["orc"]
    if name == "constrained":
        if name not in _OWN:
            from oracle.oracle import Oracle
            ec = raw_economy("short-top")
            args = ec["args"][:5] + (float(ec["grid"][5]),) + ec["args"][6:]
            _OWN[name] = (args, ec["V"], ec["D"], ec["x"], Oracle(*args[:6]))
        return _OWN[name]
    m, V, D, xhh, orc = shape({"ks130x3": 130, "ks64x3": 64}[name], 3, 12)
    return model_args(m), V, D, xhh, orc


def _sweeps(hank, name, sched, y):
    """the Float64 sweep and the Dual pass at every width of NS under one schedule (each from a record of another x: no memo hit)
    -> {"primal": (agg, policy), N: (agg, dagg, policy, dpolicy)}; the family of every Dual pass and no fallback asserted"""
    args, V, D, xhh, _ = _economy(name)
    hb = raw_block(hank, args, sched)
    hb.set_boundary(V, D)
    hb.primal(xhh * 1.01)
    out = {"primal": (hb.primal(xhh), hb.policy_seq())}
    for N in NS:
        hb.primal(xhh * 1.01)
        agg, dagg = hb.primal_jvp(xhh, np.ascontiguousarray(y[:, :, :N]))
        fam = hb.info()["last_tangent_family_name"]
        assert fam == expected_family(sched, "dual", N), (name, sched, N, fam)
        out[N] = (agg, dagg, hb.policy_seq(), hb.dpolicy_seq(N))
    st = hb.stats()
    assert st["fallbacks"] == 0 and st["schedule"] == {"launch": 0, "xcd": 1}[sched], (name, sched, st)
    hb.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ECONOMIES)
def test_persistent_backward_sweeps_equal_the_launches_bit_for_bit(hank, name):
    xhh = _economy(name)[3]
    y = np.random.default_rng(41).standard_normal(xhh.shape + (max(NS),))
    ref, got = _sweeps(hank, name, "launch", y), _sweeps(hank, name, "xcd", y)
    assert np.array_equal(got["primal"][1], ref["primal"][1]), f"{name} primal: policy_seq"
    close(got["primal"][0], ref["primal"][0], 1e-12, what=f"{name} primal agg vs launch")
    for N in NS:
        (agg, dagg, pol, dpol), (agg0, dagg0, pol0, dpol0) = got[N], ref[N]
        assert np.array_equal(pol, pol0), f"{name} N={N}: policy_seq"
        assert np.array_equal(pol, got["primal"][1]), f"{name} N={N}: policy_seq of the Dual pass against the Float64 sweep's"
        assert np.array_equal(dpol, dpol0), f"{name} N={N}: dpolicy_seq"
        close(agg, agg0, 1e-12, what=f"{name} N={N} agg vs launch")
        close(dagg, dagg0, 1e-12, what=f"{name} N={N} dagg vs launch")


# ---- what the economies hold, measured on the CPU --------------------------------------------------------------------------
_MEASURED = {}


def _knots_and_brackets(name):
    if name not in _MEASURED:
        _MEASURED[name] = _measure(name)
    return _MEASURED[name]


def _measure(name):
    """the EGM step of csrc/hank_kernels.h restated in numpy on the oracle's value path: the knots s_t (P, n_a, n_e), and per period
    and point the bracket the kernels record (ib: the interpolation's bracket, 0 below the first knot, n_a - 2 above the last), the
    two flat outcomes and whether the borrowing constraint binds. The interpolated policy must be the oracle's."""
    args, V, _, xhh, orc = _economy(name)
    grid, z, Pi, beta, gamma, bc = (np.asarray(args[0]), np.asarray(args[1]), np.asarray(args[2]), args[3], args[4], args[5])
    n_a, n_e, P = grid.size, z.size, xhh.shape[1]
    s, ib = np.empty((P, n_a, n_e)), np.empty((P, n_a, n_e), dtype=np.int64)
    below, above, binds = (np.empty((P, n_a, n_e), dtype=bool) for _ in range(3))
    pol = np.empty((P, n_a, n_e))
    Vn = np.asarray(V, dtype=np.float64)
    for t in range(P - 1, -1, -1):
        r, w = xhh[0, t], xhh[1, t]
        cm = (beta * (Vn @ Pi.T)) ** (-1.0 / gamma)             # E[a, e] = sum_k Pi[e, k] V[a, k]
        s[t] = ((cm - w * z[None, :]) + grid[:, None]) / (1.0 + r)
        assert np.all(np.diff(s[t], axis=0) > 0), (name, t, "knots not sorted")
        for e in range(n_e):
            k = s[t, :, e]
            i = np.clip(np.searchsorted(k, grid, side="right") - 1, 0, n_a - 2)
            below[t, :, e], above[t, :, e] = grid < k[0], grid > k[-1]
            f = (grid - k[i]) / (k[i + 1] - k[i])
            g = np.where(below[t, :, e], grid[0], np.where(above[t, :, e], grid[-1], (1.0 - f) * grid[i] + f * grid[i + 1]))
            ib[t, :, e] = np.where(below[t, :, e], 0, np.where(above[t, :, e], n_a - 2, i))
            binds[t, :, e] = bc > g
            pol[t, :, e] = np.maximum(g, bc)
        st, Vd, _ = orc.value_function(Vn, r, w, 1)
        assert st == 0, (name, t, st)
        Vn = Vd[..., 0]
    close(pol, orc.block(xhh, None, np.asarray(V), _economy(name)[2])[2], what=f"{name}: the restated policy against the oracle's")
    return s, ib, below, above, binds


def test_the_economies_hold_every_case_of_the_bracket_front_and_of_the_search():
    """over the raw-grid economies and `constrained`: a point inside the knots whose bracket is the one of the period before (the guess), one knot up,
    one knot down, two or more up, two or more down; a point below the first knot and one above the last; a point where the
    borrowing constraint binds; and the first period of every sweep has no guess at all (P >= 2: later periods have one)."""
    seen = dict.fromkeys(("unchanged", "+1", "-1", ">=2 up", ">=2 down", "x < s0", "x > sN", "constraint binds"), 0)
    for name in MEASURED:
        s, ib, below, above, binds = _knots_and_brackets(name)
        assert s.shape[0] >= 2
        inside = ~(below | above)[:-1]                             # period t, its guess the bracket recorded in period t + 1
        move = (ib[:-1] - ib[1:])[inside]
        counts = {"unchanged": np.sum(move == 0), "+1": np.sum(move == 1), "-1": np.sum(move == -1), ">=2 up": np.sum(move >= 2),
                  ">=2 down": np.sum(move <= -2), "x < s0": below.sum(), "x > sN": above.sum(), "constraint binds": binds.sum()}
        print(name, {k: int(v) for k, v in counts.items()}, "largest moves", int(move.min()), int(move.max()))
        for k, v in counts.items():
            seen[k] += int(v)
    assert all(v > 0 for v in seen.values()), seen
    # the offsets on r are there for the far moves: they must come from the economies that carry them
    for name in ("swing", "collapse"):
        _, ib, below, above, _ = _knots_and_brackets(name)
        move = (ib[:-1] - ib[1:])[~(below | above)[:-1]]
        assert np.sum(move >= 2) > 0 and np.sum(move <= -2) > 0, (name, int(move.min()), int(move.max()))
