"""The references of the discount-factor path (hank_set_discount_path, hank_jvp_shock, hank_vjp_shock, hank_fake_news_shock), shared by
tests/test_shock_host.py (CPU), tests/test_gpu_shock.py and tests/test_gpu_shock_geometry.py.

1. `oracle_shock_sweeps`: the loop of `sweep_refs.oracle_sweeps` with two changes per period, t descending — the oracle's model
   gets beta = beta_t before `Oracle.value_function`, and the function is handed a copy of the incoming dual value whose partials
   are dV + V dbeta_t / beta_t (beta enters KrusellSmith.jl:59-62 as beta E[V']: scaling V' by (1 + eps dbeta/beta) IS the
   beta tangent); the unaugmented output is carried on. The exact dual-number reference of the level and of the beta tangent.
   Nothing under oracle/ changes: the oracle's beta is restored when the loop ends.
2. `shock_case`: the economies — the exact inputs of cases.entry_backward (both families, every gamma of cases.ENTRY_CASES, the grids
   of cases.ENTRY_GRIDS and ENTRY_WIDE) at a horizon T, with a smooth path of the household inputs and a beta path that swings 3 %.
3. `StubShockBlock`: stands in for the device context under `SteadyStateJacobian.shock_jacobian` (the pattern of
   sweep_refs._StubBlock).
4. `oracle_shock_jacobians` (and `oracle_shock_grid_jacobians`, `shock_linear`, `shock_beta_bar`): the dense pair (Jx, Jb) from the
   oracle's unit tangents — one reference for every width of tests/test_gpu_shock_geometry.py, whose economies `geometry_case` puts in
   one form and whose raw grids' edges under a path `check_path_edges` asserts (tests/test_shock_host.py: on the oracle's policy)."""
import numpy as np

import cases
from oracle.oracle import SUPPORTED_N, Oracle, pad_N

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


def oracle_shock_sweeps(orc, x, V, D, beta_t, gamma=None, n_het=2, y=None, dbeta=None, groups=None):
    """x (n_hh, P), boundary V (n_a, n_e), D (G,), beta_t (P,); seeds y (n_hh, P, N) and dbeta (P, N), None = zeros (both None: the
    level alone, one zero direction). -> the dict of sweep_refs.oracle_sweeps: agg (P, n_het), dagg (P, n_het, N), agg2, dagg2,
    pol (P, n_a, n_e), dpol (P, n_a, n_e, N); with groups = (W (G, K), base[K]) (hank_set_group_outputs' arguments) also grp (P, K) and
    dgrp (P, K, N): the weighted dots of ForwardIteration.jl:303-307 of 1 (base 0), a' (1) or c (2) with the same dual D_t."""
    x = np.asarray(x, dtype=np.float64)
    beta_t = np.asarray(beta_t, dtype=np.float64)
    n_hh, P = x.shape
    assert beta_t.shape == (P,)
    n_a, n_e, a, z = orc.n_a, orc.n_e, orc.a, orc.z
    N = next((np.asarray(v).shape[-1] for v in (y, dbeta) if v is not None), 1)
    out = {k: [] for k in ("dagg", "dagg2", "dpol", "dgrp")}
    K = 0 if groups is None else np.asarray(groups[0]).shape[1]
    beta_model = orc.m.beta
    try:
        for c0 in range(0, N, SUPPORTED_N[-1]):
            n = min(N, c0 + SUPPORTED_N[-1]) - c0
            Nc = pad_N(n)
            xd = np.zeros((n_hh, P, 1 + Nc)); xd[..., 0] = x
            Vn = np.zeros((n_a, n_e, 1 + Nc)); Vn[..., 0] = V
            Dd = np.zeros((n_a, n_e, 1 + Nc)); Dd[..., 0] = np.asarray(D).reshape((n_a, n_e), order="F")
            if y is not None:
                xd[..., 1:1 + n] = y[:, :, c0:c0 + n]
            pol, val = [None] * P, [None] * P
            for t in range(P - 1, -1, -1):
                orc.m.beta = float(beta_t[t])                                   # change 1
                Va = Vn.copy()
                if dbeta is not None:                                           # change 2: dV + V dbeta_t / beta_t
                    Va[..., 1:1 + n] += Vn[..., :1] * (dbeta[t, c0:c0 + n] / beta_t[t])
                st, Vn, pol[t] = orc.value_function(Va, xd[0, t], xd[1, t], Nc, xd[2, t] if n_hh > 2 else None)
                assert st == 0, (t, st)
                val[t] = Vn
            agg, agg2 = np.zeros((P, n_het)), np.zeros(P)
            dagg, dagg2 = np.zeros((P, n_het, n)), np.zeros((P, n))
            grp, dgrp = np.zeros((P, K)), np.zeros((P, K, n))
            for t in range(P):
                Dd = orc.transition_step(pol[t], Dd, Nc)
                p0, dp, D0, dDt = pol[t][..., 0], pol[t][..., 1:1 + n], Dd[..., 0], Dd[..., 1:1 + n]
                tr, dtr = (xd[2, t, 0], xd[2, t, 1:1 + n]) if n_hh > 2 else (0.0, np.zeros(n))
                c0_ = (1.0 + xd[0, t, 0]) * a[:, None] + xd[1, t, 0] * z[None, :] + tr - p0
                dc = xd[0, t, 1:1 + n] * a[:, None, None] + xd[1, t, 1:1 + n] * z[None, :, None] + dtr - dp
                fs = [(p0, dp), (c0_, dc), (val[t][..., 0], val[t][..., 1:1 + n])]
                if n_het > 3:
                    fs.append((z[None, :] * c0_ ** (-gamma), (z[None, :] * (-gamma) * c0_ ** (-gamma - 1.0))[..., None] * dc))
                for o, (f0, df) in enumerate(fs[:n_het]):
                    agg[t, o] = np.sum(f0 * D0)
                    dagg[t, o] = np.einsum("aen,ae->n", df, D0) + np.einsum("ae,aen->n", f0, dDt)
                for k in range(K):
                    Wk = np.asarray(groups[0])[:, k].reshape((n_a, n_e), order="F")
                    f0, df = ((np.ones_like(p0), np.zeros_like(dp)), fs[0], fs[1])[int(groups[1][k])]
                    grp[t, k] = np.sum(Wk * f0 * D0)
                    dgrp[t, k] = np.einsum("aen,ae->n", df, Wk * D0) + np.einsum("ae,aen->n", Wk * f0, dDt)
                agg2[t] = np.sum(a[:, None] * D0)
                dagg2[t] = np.einsum("a,aen->n", a, dDt)
            out["dagg"].append(dagg); out["dagg2"].append(dagg2); out["dgrp"].append(dgrp)
            out["dpol"].append(np.stack([p[..., 1:1 + n] for p in pol]))
    finally:
        orc.m.beta = beta_model
    res = {k: np.concatenate(v, axis=-1) for k, v in out.items()}
    res.update(agg=agg, agg2=agg2, grp=grp, pol=np.stack([p[..., 0] for p in pol]), D=Dd[..., 0])
    return res


_JAC = {}


def _unit_sweeps(orc, x, V, D, beta_t, gamma, n_het):
    """`oracle_shock_sweeps` with cases.unit_tangents as y, and with dbeta = I, once per session and key (the oracle and the bits of
    every input); every output's block of either must exceed 1e-3"""
    x, V, D, beta_t = (np.ascontiguousarray(v, dtype=np.float64) for v in (x, V, D, beta_t))
    key = (id(orc), x.tobytes(), V.tobytes(), D.tobytes(), beta_t.tobytes(), gamma, n_het)
    if key not in _JAC:
        n_hh, P = x.shape
        sx = oracle_shock_sweeps(orc, x, V, D, beta_t, gamma, n_het, y=cases.unit_tangents(n_hh, P))
        sb = oracle_shock_sweeps(orc, x, V, D, beta_t, gamma, n_het, dbeta=np.eye(P))
        for o in range(n_het):
            assert np.abs(sx["dagg"][:, o, :]).max() > 1e-3 and np.abs(sb["dagg"][:, o, :]).max() > 1e-3, (o, n_het, x.shape, V.shape)
        _JAC[key] = (sx, sb)
    return _JAC[key]


def oracle_shock_jacobians(orc, x, V, D, beta_t, gamma, n_het):
    """the dense Jacobians of every heterogeneous output at the path beta_t, from the oracle's unit tangents: -> (Jx (n_het, P, n_hh, P),
    d output o at t / d input k at s — the layout cases.jt takes — and Jb (P, n_het, P), d output o at t / d beta_s as [t, o, s]).
    The tangent map is linear, so the pair is the reference of every width:
        dagg = Jx y + Jb dbeta (`shock_linear`), xhh_bar = cases.jt(Jx[:n_het], yb), beta_bar[s, m] = sum_{t,o} Jb[t, o, s] yb[t, o, m]
    (`shock_beta_bar`). Cached per session (`_unit_sweeps`)."""
    sx, sb = _unit_sweeps(orc, x, V, D, beta_t, gamma, n_het)
    n_hh, P = np.asarray(x).shape
    return np.ascontiguousarray(sx["dagg"].reshape(P, n_het, P, n_hh).transpose(1, 0, 3, 2)), sb["dagg"]


def oracle_shock_grid_jacobians(orc, x, V, D, beta_t, gamma, n_het):
    """the same pair for the grid-weighted aggregate of hank_get_grid_aggregates, from the same two sweeps:
    -> (J2x (P, n_hh, P) as [t, k, s], J2b (P, P) as [t, s])"""
    sx, sb = _unit_sweeps(orc, x, V, D, beta_t, gamma, n_het)
    n_hh, P = np.asarray(x).shape
    return np.ascontiguousarray(sx["dagg2"].reshape(P, P, n_hh).transpose(0, 2, 1)), sb["dagg2"]


def shock_linear(J, y, dbeta):
    """dagg (P, n_het, N) = Jx y + Jb dbeta of J = `oracle_shock_jacobians`' pair; y (n_hh, P, N) or None, dbeta (P, N) or None"""
    Jx, Jb = J
    N = next(v.shape[-1] for v in (y, dbeta) if v is not None)
    out = np.zeros((Jb.shape[0], Jb.shape[1], N))
    if y is not None:
        out += np.einsum("otks,ksn->ton", Jx, y)
    if dbeta is not None:
        out += np.einsum("tos,sn->ton", Jb, dbeta)
    return out


def shock_beta_bar(Jb, yb):
    """beta_bar (P, M): [s, m] = sum_{t,o} Jb[t, o, s] yb[t, o, m] over the outputs yb (P, n_het, M) holds"""
    return np.einsum("tos,tom->sm", Jb[:, :yb.shape[1], :], yb)


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


def shock_seeds(c, N, seed, t_only=None):
    """(y (n_hh, P, N), dbeta (P, N)): random directions of the inputs' and of beta's scale; t_only: dbeta in that period alone"""
    rng = np.random.default_rng(seed)
    n_hh, P = c["x"].shape
    y = rng.standard_normal((n_hh, P, N)) * 1e-2
    db = rng.standard_normal((P, N)) * 1e-2
    if t_only is not None:
        keep = np.zeros((P, 1)); keep[t_only] = 1.0
        db = db * keep
    return y, db


class StubShockBlock:
    """stands in for the device context under `shock_jacobian`: fake_news_shock hands out the F and Dv it was made with"""

    def __init__(self, F, Dv):
        self.F, self.Dv, self.calls = F, Dv, 0

    def fake_news_shock(self, n_het):
        self.calls += 1
        return self.F[..., :n_het].copy(), self.Dv[..., :n_het].copy()
