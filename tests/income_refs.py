"""The references of the income path by productivity state (hank_set_income_path, hank_jvp_income, hank_vjp_income,
hank_fake_news_income), shared by tests/test_income_host.py (CPU), tests/test_gpu_income.py and tests/test_gpu_income_geometry.py.

1. `KIND`: the kind's row of tests/path_refs.py, whose `oracle_path_sweeps` is the loop — built from the unchanged oracle — and whose
   `jacobians`, `linear`, `path_bar` are the dense pair (Jx, Jy) and its products. Its backward step `_step` runs the oracle's EGM
   step once per productivity state; the forward walk has + y_t[e] in consumption and + dy in its tangent (`Kind.budget`).
2. `income_case`: the economies of `shock_refs.shock_case` with an income path that alternates in sign across e, decays in t and is
   scaled to 2 % of the smallest w z_e.
3. `geometry_case`, `rescaled_D0`, GEOM_M, GEOM_N: the economies and the widths of tests/test_gpu_income_geometry.py, whose
   conditions tests/test_income_host.py checks on the CPU."""
import numpy as np

import cases
import path_refs
import shock_refs

HORIZONS = shock_refs.HORIZONS
WIDTHS = shock_refs.WIDTHS
N_HET = 2
_CASES = {}


def income_path(z, x, scale=0.02):
    """y (n_e, P): y_t[e] = scale min(w z) (-1)^e 0.8^t"""
    n_e, P = len(z), x.shape[1]
    amp = scale * float(np.min(x[1]) * np.min(z))
    return np.ascontiguousarray(amp * ((-1.0) ** np.arange(n_e))[:, None] * (0.8 ** np.arange(P))[None, :])


def income_case(family, name, n_a, n_e, T):
    """`shock_refs.shock_case` (args, V, D, x, gamma, env, diet, orc) with y (n_e, P) the income path and n_het = 2, cached"""
    key = (family, name, n_a, n_e, T)
    if key not in _CASES:
        c = dict(shock_refs.shock_case(family, name, n_a, n_e, T))
        c.update(y=income_path(c["orc"].z, c["x"]), n_het=N_HET)
        del c["path"]
        _CASES[key] = c
    return _CASES[key]


def raw_case(name):
    """a raw-grid economy of cases.raw_economy in the same form (Krusell-Smith, gamma = 2, nine periods)"""
    key = ("raw", name)
    if key not in _CASES:
        ec = cases.raw_economy(name)
        _CASES[key] = dict(args=ec["args"], V=ec["V"], D=ec["D"], x=ec["x"], gamma=float(ec["args"][4]), env={}, diet=1, orc=ec["orc"],
                           y=income_path(ec["orc"].z, ec["x"]), n_het=N_HET, grid=ec["grid"])
    return _CASES[key]


def two_state_hank():
    """a one-asset HANK economy with FEWER productivity states than household inputs (n_e = 2 < n_hh = 3) at its own steady state:
    ss_diff_cases' hank30x3 grid, preferences and household prices (r, w, tr) with the lowest and the highest of its productivity
    states under a symmetric chain. -> dict(args: HouseholdBlock's at T = 12, orc, x (3,), V (30, 2), D (G,)), cached"""
    key = ("hank30x2",)
    if key not in _CASES:
        import ss_diff_cases as S
        from oracle.oracle import Oracle
        c = S.case("hank30x3")
        a = c["args"]
        z, Pi = np.array([a[1][0], a[1][-1]]), np.array([[0.9, 0.1], [0.1, 0.9]])
        orc = Oracle(a[0], z, Pi, a[3], a[4], a[5])
        V, pol, D, _ = S.steady_state(orc, c["x"])
        V, pol, D, _ = S.steady_state(orc, c["x"], V, D, tol_v=4.0 * np.finfo(np.float64).eps * np.abs(V).max(), cap=20_000)
        _CASES[key] = dict(args=(a[0], z, Pi) + tuple(a[3:6]) + (12,) + tuple(a[7:]), orc=orc, x=np.asarray(c["x"]), V=V, D=D)
    return _CASES[key]


def _step(w, Vn, xd, pd, t):
    """period t at y_t: a column's EGM step depends only on its own income and on the common V_{t+1}, so for each state e
    `Oracle.value_function` runs with the dual transfer tr = (tr_t + y_t[e], dtr_t + dy_t[e]) (Krusell-Smith: tr_t = 0) and column e
    of its Value and KD is kept; the columns are assembled into V_t and pol_t"""
    Vt, Kt = np.empty_like(Vn), np.empty_like(Vn)
    for e in range(w.orc.n_e):                                       # column e's step at ITS income, from the common V_{t+1}
        tr = (xd[2, t] if w.n_hh > 2 else 0.0) + pd[e, t]
        st, Ve, Ke = w.orc.value_function(Vn, xd[0, t], xd[1, t], w.Nc, tr)
        assert st == 0, (t, e, st)
        Vt[:, e], Kt[:, e] = Ve[:, e], Ke[:, e]
    return Vt, Kt


# outputs 0 and 1 (the entries serve no other at a path): the callers leave n_het = 2. mass (P, n_e): the column masses of Dseq.
KIND = path_refs.register(path_refs.Kind("income", "income", "y", "orc", lambda orc: (orc.n_e,), lambda orc, P: np.zeros((orc.n_e, P)), _step, lambda orc: orc,
                                         True, None, lambda res: {"mass": res["Dseq"].sum(axis=1)}, False))


# ---- 5. the economies of tests/test_gpu_income_geometry.py ------------------------------------------------------------------------------
# the cotangent and direction widths: tests/test_gpu_shock_geometry.py's lists, and M = 5 besides — k_inc_ybar's columns across the lanes
# stop at 32 where k_shk_bbar's go on to 64, so its (RO, MC) pairs are not that kernel's: (8, 8) is reached by M = 5 and 7 alone
# (tests/test_income_host.py holds the widths and the launch arithmetic together)
GEOM_M = (1, 2, 3, 4, 5, 6, 8, 16, 17, 32, 34, 64, 65, 66, 97, 130, 256)
GEOM_N = (2, 4, 16, 34, 64, 66, 129, 130, 256)
EDGE_ECONOMIES = shock_refs.EDGE_ECONOMIES
D0_SCALE = (0.5, 1.0, 1.5)


def geometry_case(kind, *key):
    """`shock_refs.geometry_case`'s economies — ("shape", n_a, n_e, T), ("raw", name); Krusell-Smith at gamma = 2, the record diet
    `raw_case` has — with y = income_path(orc.z, x) and n_het = 2 in place of the beta path and the three outputs, cached"""
    k = ("geometry", kind) + key
    if k not in _CASES:
        c = dict(shock_refs.geometry_case(kind, *key))
        c.update(y=income_path(c["orc"].z, c["x"]), n_het=N_HET)
        del c["path"]
        _CASES[k] = c
    return _CASES[k]


def rescaled_D0(c, scale=D0_SCALE):
    """a second D_0 (G,) of case c (three columns) whose column masses differ: column e scaled by scale[e], renormalised"""
    n_a, n_e = c["V"].shape
    assert n_e == len(scale)
    D = np.asarray(c["D"]).reshape((n_a, n_e), order="F") * np.asarray(scale)[None, :]
    return np.ascontiguousarray((D / D.sum()).reshape(-1, order="F"))
