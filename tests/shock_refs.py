"""The references of the discount-factor path (hank_set_discount_path, hank_jvp_shock, hank_vjp_shock, hank_fake_news_shock), shared by
tests/test_shock_host.py (CPU), tests/test_gpu_shock.py and tests/test_gpu_shock_geometry.py.

1. `KIND`: the kind's row of tests/path_refs.py, whose `oracle_path_sweeps` is the loop and whose `jacobians`, `linear`, `path_bar`
   are the dense pair (Jx, Jb) and its products. Its backward step `_step` is the plain oracle's with two changes per period, t
   descending — the oracle's model gets beta = beta_t before `Oracle.value_function`, and the function is handed a copy of the
   incoming dual value whose partials are dV + V dbeta_t / beta_t (beta enters KrusellSmith.jl:59-62 as beta E[V']: scaling V' by
   (1 + eps dbeta/beta) IS the beta tangent); the unaugmented output is carried on. The exact dual-number reference of the level
   and of the beta tangent. Nothing under oracle/ changes: the oracle's beta is restored after every step.
2. `shock_case`: the economies — the exact inputs of cases.entry_backward (both families, every gamma of cases.ENTRY_CASES, the grids
   of cases.ENTRY_GRIDS and ENTRY_WIDE) at a horizon T, with a smooth path of the household inputs and a beta path that swings 3 %.
3. `geometry_case`: the economies of tests/test_gpu_shock_geometry.py in one form; `check_path_edges`: the raw grids' edges under a
   path (tests/test_shock_host.py: on the oracle's policy)."""
import numpy as np

import cases
import path_refs
from oracle.oracle import Oracle

HORIZONS = (2, 3, 4, 12)
WIDTHS = (1, 3, 33)
_CASES = {}


def beta_path(beta, P, swing=0.03):
    """beta_t = beta (1 + swing cos(pi t / max(P - 1, 1))): +3 % in the first period, -3 % in the last (P = 1: +3 %)"""
    return beta * (1.0 + swing * np.cos(np.pi * np.arange(P) / max(P - 1, 1)))


def shock_case(family, name, n_a, n_e, T):
    """-> dict(args: HouseholdBlock's at T, V (n_a, n_e), D (G,), x (n_hh, P), beta: the model's, path (P,), gamma, env: the
    HANK_RECORD_DIET of the case, diet: what the context must report, orc, n_het: the family's count), cached"""
    key = (family, name, n_a, n_e, T)
    if key not in _CASES:
        gamma, rd, diet = cases.ENTRY_CASES[name]
        c = cases.entry_backward(family, gamma, n_a, n_e)
        P = T - 1
        t = np.arange(P)
        base = np.array(cases.ENTRY_BASE + ((cases.ENTRY_TR,) if family == "hank" else ()))
        dev = np.stack([0.1 * 0.8 ** t, 0.01 * 0.7 ** t, -0.02 * 0.9 ** t])[:len(base)]
        x = np.ascontiguousarray(base[:, None] * (1.0 + dev))
        G = n_a * n_e
        D = (1.0 + np.arange(G) % 7) / np.sum(1.0 + np.arange(G) % 7)
        _CASES[key] = dict(args=c["args"][:6] + (T,) + c["args"][7:], V=c["V"], D=D, x=x, beta=c["beta"], path=beta_path(c["beta"], P), gamma=gamma,
                           env={} if rd is None else {"HANK_RECORD_DIET": rd}, diet=diet, orc=Oracle(*c["args"][:6]), n_het=3 if family == "ks" else 4)
    return _CASES[key]


def _step(w, Vn, xd, pd, t):
    """period t at beta_t: the oracle's model gets beta = beta_t before `Oracle.value_function` (restored whatever happens), and the
    function is handed a copy of the incoming dual value whose partials are dV + V dbeta_t / beta_t; the unaugmented output is
    carried on"""
    orc, n = w.orc, w.n
    beta_model = orc.m.beta
    try:
        orc.m.beta = float(pd[t, 0])
        Va = Vn.copy()
        if w.seeded:
            Va[..., 1:1 + n] += Vn[..., :1] * (pd[t, 1:1 + n] / pd[t, 0])
        st, V, pol = orc.value_function(Va, xd[0, t], xd[1, t], w.Nc, xd[2, t] if w.n_hh > 2 else None)
    finally:
        orc.m.beta = beta_model
    assert st == 0, (t, st)
    return V, pol


KIND = path_refs.register(path_refs.Kind("shock", "discount", "path", "orc", lambda orc: (), lambda orc, P: np.full(P, orc.m.beta), _step, lambda orc: orc,
                                         False, 1e-3, None, True))


_GEOM = {}


def geometry_case(kind, *key):
    """the economies of tests/test_gpu_shock_geometry.py in one form: ("shape", n_a, n_e, T): cases.shape (n_e = 1: shape_one_column);
    ("raw", name): cases.raw_economy. Krusell-Smith at gamma = 2 throughout: three outputs.
    -> dict(args: HouseholdBlock's, V, D, x (2, P), orc, beta, gamma, n_het = 3, path: beta_path(beta, P), grid), cached"""
    if (kind,) + key not in _GEOM:
        if kind == "raw":
            ec = cases.raw_economy(*key)
            args, V, D, x, orc = ec["args"], ec["V"], ec["D"], ec["x"], ec["orc"]
        else:
            n_a, n_e, T = key
            m, V, D, x, orc = cases.shape_one_column(n_a, T) if n_e == 1 else cases.shape(n_a, n_e, T)
            args = m if isinstance(m, tuple) else cases.model_args(m)
        beta, gamma = float(args[3]), float(args[4])
        assert gamma == 2.0 and x.shape == (2, args[6] - 1)
        _GEOM[(kind,) + key] = dict(args=args, V=V, D=D, x=x, orc=orc, beta=beta, gamma=gamma, n_het=3, path=beta_path(beta, x.shape[1]),
                                    grid=np.asarray(args[0]))
    return _GEOM[(kind,) + key]


EDGE_ECONOMIES = tuple(cases.EDGE_GRIDS) + ("deep-prefix", "swing")


def check_path_edges(name, grid, pol):
    """a policy sequence pol (P, n_a, n_e) recorded under beta_path(beta, 9) still holds the edges of its raw-grid economy:
    cases.check_edges for the grids of cases.EDGE_GRIDS; cases.forward_edges' figures for "deep-prefix" (a clamped prefix of 200 rows
    or more, past row 128) and "swing" (every column clamped in period 1, none in period 2, 100 sources or more on one target row)"""
    if name in cases.EDGE_GRIDS:
        return cases.check_edges(name, grid, pol)
    f = cases.forward_edges(grid, pol)
    print(f"{name} ({grid.size} rows): clo per column {f['clo'].T.tolist()}, most sources on one target per period {f['sources'].max(axis=1).tolist()}, "
          f"all clamped {f['all_clamped'].astype(int).tolist()}, reopened {f['reopened'].astype(int).tolist()}")
    if name == "deep-prefix":
        assert f["past128"].any() and f["clo"].max() >= 200, (name, f["clo"].max())
    else:
        assert name == "swing" and f["all_clamped"][1] and f["reopened"][2] and f["sources"].max() >= 100, (name, f["sources"].max())
    return f
