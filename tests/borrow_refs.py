"""The references of the borrowing-limit path (hank_set_borrow_path, hank_jvp_borrow, hank_vjp_borrow, hank_fake_news_borrow), shared by
tests/test_borrow_host.py (CPU) and tests/test_gpu_borrow.py.

1. `KIND`: the kind's row of tests/path_refs.py, whose `oracle_path_sweeps` is the loop, built from the unchanged oracle with ONE `Oracle` per limit —
   its constructor takes borrow_cons — so period t's `value_function` runs at amin_t. The tangent in amin: the same step with an oracle
   whose limit lies far below the grid gives the unconstrained dual g; the constrained set C_t is where the DiffRules rule of max holds
   against amin_t, (amin_t > g) | (signbit(amin_t) < signbit(g)); and KrusellSmith.jl:76-80 restated on duals says what amin's partial
   adds there: policy += damin_t, consumption -= damin_t, Value = (1 + r) c^-gamma += gamma (1 + r) c^(-gamma - 1) damin_t. The terms
   are ADDED to the constrained oracle's own duals (whose partials on C_t are exact zeros), and only where damin is not zero: with
   damin = 0 the reference IS the constant-limit oracle's loop, bit for bit.
2. `borrow_case`: the economies of `shock_refs.shock_case`; their wealth grid 50 (k / (n_a - 1))^2 has several points below the limits
   chosen here (`limits`: two or three points at n_a = 33, eight to twelve at 130), so nothing is added to it. `borrow_path` cycles
   through: strictly inside a bracket; exactly on a grid point; a[0]; below a[0]; and tightens and relaxes between them.
3. the dense pair (Jx, Ja) and its products are path_refs' (Ja has Jb's layout: the leading shape ())."""
import numpy as np

import cases
import path_refs
import shock_refs
from oracle.oracle import Oracle

HORIZONS = shock_refs.HORIZONS
WIDTHS = shock_refs.WIDTHS
FAR_BELOW = -1e300
_CASES, _ORC = {}, {}


LIMIT_LO, LIMIT_HI = 0.19, 0.45


def limits(a):
    """the named limits on grid a: k1 the first point at or above LIMIT_LO, K the last at or below LIMIT_HI (33 rows: a[2] = 0.195 and
    a[3] = 0.439; 130 rows: a[8] and a[12]). Every binding limit lies in [LIMIT_LO, LIMIT_HI]: above what the most productive state
    saves at the bottom of the grid where that can be had (0.05 .. 0.46 by economy, measured), below w z_0 = 0.5, the cash of the least
    productive state there — consumption stays positive."""
    k1 = int(np.searchsorted(a, LIMIT_LO, side="left"))
    K = int(np.searchsorted(a, LIMIT_HI, side="right")) - 1
    assert 1 <= k1 < K <= len(a) - 2
    return dict(inside=0.5 * (a[k1] + a[k1 + 1]), on=float(a[K]), first=float(a[0]), below=float(a[0]) - 0.05, on_lo=float(a[k1]),
                inside_hi=0.5 * (a[K - 1] + a[K]), k1=k1, K=K)


KINDS = ("inside", "on", "first", "below", "inside_hi", "on_lo", "inside", "below", "on", "inside_hi", "first")


G_MARGIN, C_MARGIN = 0.01, 0.04


def borrow_path(args, x, V):
    """amin (P,) of an economy, chosen PER ECONOMY and period so that, where it can be had, the limit constrains the bottom of EVERY
    column: the kinds are the first P of KINDS (the short horizons see a value inside a bracket first); going backward from V, period
    t's window is (G_t + G_MARGIN, cash_t - C_MARGIN) — G_t what the most saving column saves at a[0] without a limit, from the
    unchanged oracle at the value the later limits leave; cash_t = (1 + r_t) a[0] + w_t z_0 + tr_t, the least productive state's cash
    there, so consumption stays above C_MARGIN. "on" / "on_lo" take the last / first grid point a[k], k >= 1, inside the window,
    "inside_hi" / "inside" the last / first bracket midpoint inside it; with an empty window — or no grid point in it — the window
    is opened from below to the columns that save least, one at a time, and the kind keeps `limits`' fixed value if that fails too. -> (amin, kinds, window (P,): the window held)"""
    a, z = np.asarray(args[0]), np.asarray(args[1])
    n_hh, P = x.shape
    L = limits(a)
    kinds = tuple(KINDS[t % len(KINDS)] for t in range(P))
    free = oracle_at(args, FAR_BELOW)
    amin, held, Vn = np.zeros(P), np.zeros(P, dtype=bool), np.asarray(V)
    mids = 0.5 * (a[1:-1] + a[2:])                                             # brackets (a[k], a[k+1]), k >= 1
    for t in range(P - 1, -1, -1):
        tr = x[2, t] if n_hh > 2 else None
        kind = kinds[t]
        amin[t] = L[kind]
        if kind not in ("first", "below"):
            st, _, Ku = free.value_function(Vn, x[0, t], x[1, t], 1, tr)
            assert st == 0, (t, st)
            hi = (1.0 + x[0, t]) * a[0] + x[1, t] * z[0] + (x[2, t] if n_hh > 2 else 0.0) - C_MARGIN
            every = a[1:-1] if kind in ("on", "on_lo") else mids
            for m in range(len(z), 0, -1):                                    # every column if it can be had, else as many as can
                lo = float(np.sort(Ku[0, :, 0])[m - 1]) + G_MARGIN
                cand = every[(every > lo) & (every < hi)]
                if cand.size:
                    amin[t], held[t] = float(cand[-1] if kind in ("on", "inside_hi") else cand[0]), m == len(z)
                    break
        st, Vc, _ = oracle_at(args, amin[t]).value_function(Vn, x[0, t], x[1, t], 1, tr)
        assert st == 0, (t, st, amin[t])
        Vn = Vc[..., 0]
    return amin, kinds, held


def oracle_at(args, limit):
    """the Oracle of HouseholdBlock's args with borrow_cons = limit, one per (economy, limit)"""
    a, z, Pi, beta, gamma = args[:5]
    key = (np.asarray(a).tobytes(), np.asarray(z).tobytes(), np.asarray(Pi).tobytes(), float(beta), float(gamma), float(limit))
    if key not in _ORC:
        _ORC[key] = Oracle(a, z, Pi, beta, gamma, float(limit))
    return _ORC[key]


def borrow_case(family, name, n_a, n_e, T):
    """`shock_refs.shock_case` with amin (P,) the limit's path, kinds, bc the model's constant; cached"""
    key = (family, name, n_a, n_e, T)
    if key not in _CASES:
        c = dict(shock_refs.shock_case(family, name, n_a, n_e, T))
        del c["path"]
        amin, kinds, held = borrow_path(c["args"], c["x"], c["V"])
        c.update(amin=amin, kinds=kinds, window=held, bc=float(c["args"][5]))
        _CASES[key] = c
    return _CASES[key]


def with_limit(c, bc):
    """case c with the model's constant limit replaced (args and oracle)"""
    d = dict(c)
    d.update(args=c["args"][:5] + (float(bc),) + c["args"][6:], bc=float(bc), orc=oracle_at(c["args"], bc))
    return d


def raw_case(name):
    """a raw-grid economy of cases.raw_economy in the same form (Krusell-Smith, gamma = 2, nine periods), with a path whose limits sit
    deep in the grid's dense bottom: the interior constrained prefix spans many rows"""
    key = ("raw", name)
    if key not in _CASES:
        ec = cases.raw_economy(name)
        a = np.asarray(ec["grid"])
        P = ec["x"].shape[1]
        lim = a[0] + 0.5 * float(np.min(ec["x"][1])) * float(np.asarray(ec["args"][1])[0])      # half the least productive state's cash at a[0]
        k = int(np.searchsorted(a, lim, side="right")) - 1
        assert k >= 4, (name, k)
        vals = (0.5 * (a[k] + a[k + 1]), float(a[k]), float(a[0]), 0.5 * (a[k // 2] + a[k // 2 + 1]), float(a[0]) - 0.05)
        amin = np.array([vals[t % len(vals)] for t in range(P)])
        _CASES[key] = dict(args=ec["args"], V=ec["V"], D=ec["D"], x=ec["x"], gamma=float(ec["args"][4]), env={}, diet=1, orc=ec["orc"], amin=amin,
                           kinds=tuple(("inside", "on", "first", "inside", "below")[t % 5] for t in range(P)), bc=float(ec["args"][5]), n_het=3, grid=a, k=k)
    return _CASES[key]


def steady_case(econ, T=12):
    """ss_diff_cases.case(econ)'s model with its limit moved INSIDE the grid — the middle of the last bracket below a[0] + half the
    least productive state's cash there, so several grid points lie below it — at its own steady state (ss_diff_cases.steady_state,
    twice, as income_refs.two_state_hank does). -> dict(args at T, x (n_hh,), V, D, bc, gamma, n_het, k), cached"""
    key = ("steady", econ, T)
    if key not in _CASES:
        import ss_diff_cases as S
        c = S.case(econ)
        A = c["args"]
        a, z, x = np.asarray(A[0]), np.asarray(A[1]), np.asarray(c["x"])
        lim = a[0] + 0.5 * (x[1] * z[0] + (x[2] if len(x) > 2 else 0.0))
        k = int(np.searchsorted(a, lim, side="right")) - 1
        assert k >= 3, (econ, k)
        bc = 0.5 * (a[k - 1] + a[k])
        args = tuple(A[:5]) + (float(bc), T) + tuple(A[7:])
        orc = oracle_at(args, bc)
        V, pol, D, _ = S.steady_state(orc, x)
        V, pol, D, _ = S.steady_state(orc, x, V, D, tol_v=4.0 * np.finfo(np.float64).eps * np.abs(V).max(), cap=20_000)
        assert np.any(pol == bc), econ                    # (the least productive columns are constrained; the most productive one is not)
        _CASES[key] = dict(args=args, x=x, V=V, D=D, bc=float(bc), gamma=float(A[4]), n_het=c["n_het"], k=k, pol=pol)
    return _CASES[key]


def constrained(am, g):
    """the DiffRules rule of max(g, am): the partial is am's"""
    return (am > g) | (np.signbit(am) < np.signbit(g))


def _step(w, Vn, xd, pd, t):
    """period t at amin_t: `value_function` of the Oracle with borrow_cons = amin_t; the same step with the oracle whose limit lies far
    below the grid (w.orc) gives the unconstrained dual and so C_t, recorded as C; amin's partial is ADDED to the constrained oracle's
    own duals on C_t (exact zeros there, asserted), and only where damin_t is not zero"""
    n, gamma = w.n, w.gamma
    a, z = w.orc.a, w.orc.z
    amin = pd[t, 0]
    tr = xd[2, t] if w.n_hh > 2 else None
    st, Vc, Kc = oracle_at(w.model, amin).value_function(Vn, xd[0, t], xd[1, t], w.Nc, tr)
    assert st == 0, (t, st)
    st, _, Ku = w.orc.value_function(Vn, xd[0, t], xd[1, t], w.Nc, tr)
    assert st == 0, (t, st, "free")
    C = constrained(amin, Ku[..., 0])
    assert np.array_equal(Kc[..., 0], np.where(C, amin, Ku[..., 0])) and not np.any(Kc[C, 1:]), t
    if w.seeded and np.any(pd[t, 1:1 + n]):
        da = pd[t, 1:1 + n]
        r, wg, tr0 = xd[0, t, 0], xd[1, t, 0], (xd[2, t, 0] if w.n_hh > 2 else 0.0)
        cg = (1.0 + r) * a[:, None] + wg * z[None, :] + tr0 - Kc[..., 0]                  # :79
        Kc[C, 1:1 + n] += da                                                             # :76 the partial of max is amin's
        Vc[C, 1:1 + n] += (gamma * (1.0 + r) * cg ** (-gamma - 1.0))[C][:, None] * da   # :80 Value = (1 + r) c^-gamma, dc = -damin
    w.rec.setdefault("C", [None] * xd.shape[1])[t] = C
    return Vc, Kc


# the model is HouseholdBlock's args (the oracle's first five are read), gamma is always given; C (P, n_a, n_e): the constrained sets
KIND = path_refs.register(path_refs.Kind("borrow", "borrow", "amin", "args", lambda orc: (), lambda args, P: np.full(P, float(args[5])), _step,
                                         lambda args: oracle_at(args, FAR_BELOW), False, None, None, True))


def case_args(c, path=True):
    """(args, x, V, D, amin) of case c: the path, or the model's constant in every period"""
    P = c["x"].shape[1]
    return (c["args"], c["x"], c["V"], c["D"], c["amin"] if path else np.full(P, c["bc"]))
