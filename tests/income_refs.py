"""The references of the income path by productivity state (hank_set_income_path, hank_jvp_income, hank_vjp_income,
hank_fake_news_income), shared by tests/test_income_host.py (CPU), tests/test_gpu_income.py and tests/test_gpu_income_geometry.py.

1. `oracle_income_sweeps`: the loop of `sweep_refs.oracle_sweeps` built from the unchanged oracle. A column's EGM step depends only on
   its own income and on the common V_{t+1}, so for each period t and each state e' `Oracle.value_function` runs with the dual transfer
   tr = (tr_t + y_t[e'], dtr_t + dy_t[e']) (Krusell-Smith: tr_t = 0) and column e' of its Value and KD is kept; the columns are
   assembled into V_t and pol_t. The forward loop is `shock_refs.oracle_shock_sweeps`' with + y_t[e] in consumption and + dy in its
   tangent. Outputs 0 and 1 (the entries serve no other at a path).
2. `income_case`: the economies of `shock_refs.shock_case` with an income path that alternates in sign across e, decays in t and is
   scaled to 2 % of the smallest w z_e.
3. `oracle_income_jacobians`, `income_linear`, `income_y_bar`: the dense pair (Jx, Jy) from unit tangents, cached, and the linear and
   transposed products of it.
4. `StubIncomeBlock`: stands in for the device context under `SteadyStateJacobian.income_jacobian` (the pattern of StubShockBlock).
5. `geometry_case`, `oracle_income_grid_jacobians`, `check_income_edges`, `rescaled_D0`, GEOM_M, GEOM_N: the economies, the grid
   aggregate's pair and the widths of tests/test_gpu_income_geometry.py, whose conditions tests/test_income_host.py checks on the CPU."""
import numpy as np

import cases
import shock_refs
from oracle.oracle import SUPPORTED_N, pad_N

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


def oracle_income_sweeps(orc, x, V, D, y=None, dx=None, dy=None):
    """x (n_hh, P), boundary V (n_a, n_e), D (G,), the path y (n_e, P) or None (zeros); seeds dx (n_hh, P, N) and dy (n_e, P, N), None =
    zeros (both None: the level alone, one zero direction). -> dict: agg (P, 2), dagg (P, 2, N) of (savings, consumption); agg2 (P,),
    dagg2 (P, N) the wealth grid's aggregate; pol (P, n_a, n_e), dpol (P, n_a, n_e, N); Dseq (P, n_a, n_e) the post-transition D_t;
    mass (P, n_e) its column masses."""
    x = np.asarray(x, dtype=np.float64)
    n_hh, P = x.shape
    n_a, n_e, a, z = orc.n_a, orc.n_e, orc.a, orc.z
    y = np.zeros((n_e, P)) if y is None else np.asarray(y, dtype=np.float64)
    assert y.shape == (n_e, P)
    N = next((np.asarray(v).shape[-1] for v in (dx, dy) if v is not None), 1)
    out = {k: [] for k in ("dagg", "dagg2", "dpol")}
    for c0 in range(0, N, SUPPORTED_N[-1]):
        n = min(N, c0 + SUPPORTED_N[-1]) - c0
        Nc = pad_N(n)
        xd = np.zeros((n_hh, P, 1 + Nc)); xd[..., 0] = x
        yd = np.zeros((n_e, P, 1 + Nc)); yd[..., 0] = y
        Vn = np.zeros((n_a, n_e, 1 + Nc)); Vn[..., 0] = V
        Dd = np.zeros((n_a, n_e, 1 + Nc)); Dd[..., 0] = np.asarray(D).reshape((n_a, n_e), order="F")
        if dx is not None:
            xd[..., 1:1 + n] = dx[:, :, c0:c0 + n]
        if dy is not None:
            yd[..., 1:1 + n] = dy[:, :, c0:c0 + n]
        pol = [None] * P
        for t in range(P - 1, -1, -1):
            Vt, Kt = np.empty_like(Vn), np.empty_like(Vn)
            for e in range(n_e):                                       # column e's step at ITS income, from the common V_{t+1}
                tr = (xd[2, t] if n_hh > 2 else 0.0) + yd[e, t]
                st, Ve, Ke = orc.value_function(Vn, xd[0, t], xd[1, t], Nc, tr)
                assert st == 0, (t, e, st)
                Vt[:, e], Kt[:, e] = Ve[:, e], Ke[:, e]
            Vn, pol[t] = Vt, Kt
        agg, agg2 = np.zeros((P, N_HET)), np.zeros(P)
        dagg, dagg2 = np.zeros((P, N_HET, n)), np.zeros((P, n))
        Dseq = np.zeros((P, n_a, n_e))
        for t in range(P):
            Dd = orc.transition_step(pol[t], Dd, Nc)
            p0, dp, D0, dDt = pol[t][..., 0], pol[t][..., 1:1 + n], Dd[..., 0], Dd[..., 1:1 + n]
            tr, dtr = (xd[2, t, 0], xd[2, t, 1:1 + n]) if n_hh > 2 else (0.0, np.zeros(n))
            c0_ = (1.0 + xd[0, t, 0]) * a[:, None] + xd[1, t, 0] * z[None, :] + tr + yd[None, :, t, 0] - p0
            dc = xd[0, t, 1:1 + n] * a[:, None, None] + xd[1, t, 1:1 + n] * z[None, :, None] + dtr + yd[None, :, t, 1:1 + n] - dp
            for o, (f0, df) in enumerate(((p0, dp), (c0_, dc))):
                agg[t, o] = np.sum(f0 * D0)
                dagg[t, o] = np.einsum("aen,ae->n", df, D0) + np.einsum("ae,aen->n", f0, dDt)
            agg2[t] = np.sum(a[:, None] * D0)
            dagg2[t] = np.einsum("a,aen->n", a, dDt)
            Dseq[t] = D0
        out["dagg"].append(dagg); out["dagg2"].append(dagg2)
        out["dpol"].append(np.stack([p[..., 1:1 + n] for p in pol]))
    res = {k: np.concatenate(v, axis=-1) for k, v in out.items()}
    res.update(agg=agg, agg2=agg2, pol=np.stack([p[..., 0] for p in pol]), Dseq=Dseq, mass=Dseq.sum(axis=1))
    return res


_JAC = {}


def _unit_sweeps(orc, x, V, D, y):
    """`oracle_income_sweeps` with cases.unit_tangents as dx, and with dy = the n_e P unit directions (e fastest), once per session
    and key (the oracle and the bits of every input)"""
    x, V, D = (np.ascontiguousarray(v, dtype=np.float64) for v in (x, V, D))
    n_hh, P = x.shape
    yy = np.zeros((orc.n_e, P)) if y is None else np.ascontiguousarray(y, dtype=np.float64)
    key = (id(orc), x.tobytes(), V.tobytes(), D.tobytes(), yy.tobytes())
    if key not in _JAC:
        sx = oracle_income_sweeps(orc, x, V, D, yy, dx=cases.unit_tangents(n_hh, P))
        sy = oracle_income_sweeps(orc, x, V, D, yy, dy=np.eye(orc.n_e * P).reshape((orc.n_e, P, orc.n_e * P), order="F"))
        _JAC[key] = (sx, sy)
    return _JAC[key]


def oracle_income_jacobians(orc, x, V, D, y=None):
    """the dense Jacobians of outputs 0 and 1 at the path y: -> (Jx (2, P, n_hh, P), d output o at t / d input k at s — the layout
    cases.jt takes — and Jy (P, 2, n_e, P), d output o at t / d y_s[e] as [t, o, e, s]). The tangent map is linear, so the pair is the
    reference of every width: dagg = Jx dx + Jy dy (`income_linear`), xhh_bar = cases.jt(Jx[:n_het], yb), y_bar = `income_y_bar`."""
    sx, sy = _unit_sweeps(orc, x, V, D, y)
    n_hh, P = np.asarray(x).shape
    return (np.ascontiguousarray(sx["dagg"].reshape(P, N_HET, P, n_hh).transpose(1, 0, 3, 2)),
            np.ascontiguousarray(sy["dagg"].reshape(P, N_HET, P, orc.n_e).transpose(0, 1, 3, 2)))


def income_linear_policies(orc, x, V, D, y, dx, dy):
    """dpol (P, n_a, n_e, N) of the directions dx (n_hh, P, N) or None and dy (n_e, P, N) or None, from the unit sweeps' policy
    partials (the map is linear)"""
    sx, sy = _unit_sweeps(orc, x, V, D, y)
    n_hh, P = np.asarray(x).shape
    N = next(v.shape[-1] for v in (dx, dy) if v is not None)
    out = np.zeros(sx["dpol"].shape[:3] + (N,))
    if dx is not None:
        out += sx["dpol"] @ np.asarray(dx).reshape((n_hh * P, N), order="F")
    if dy is not None:
        out += sy["dpol"] @ np.asarray(dy).reshape((orc.n_e * P, N), order="F")
    return out


def income_linear(J, dx, dy):
    """dagg (P, 2, N) = Jx dx + Jy dy of J = `oracle_income_jacobians`' pair; dx (n_hh, P, N) or None, dy (n_e, P, N) or None"""
    Jx, Jy = J
    N = next(v.shape[-1] for v in (dx, dy) if v is not None)
    out = np.zeros((Jy.shape[0], Jy.shape[1], N))
    if dx is not None:
        out += np.einsum("otks,ksn->ton", Jx, dx)
    if dy is not None:
        out += np.einsum("toes,esn->ton", Jy, dy)
    return out


def income_y_bar(Jy, yb):
    """y_bar (n_e, P, M): [e, s, m] = sum_{t,o} Jy[t, o, e, s] yb[t, o, m] over the outputs yb (P, n_het, M) holds"""
    return np.einsum("toes,tom->esm", Jy[:, :yb.shape[1]], yb)


def oracle_income_grid_jacobians(orc, x, V, D, y=None):
    """the same pair for the grid-weighted aggregate of hank_get_grid_aggregates, from the same two sweeps (the counterpart of
    shock_refs.oracle_shock_grid_jacobians): -> (J2x (P, n_hh, P) as [t, k, s], J2y (P, n_e, P) as [t, e, s])"""
    sx, sy = _unit_sweeps(orc, x, V, D, y)
    n_hh, P = np.asarray(x).shape
    return (np.ascontiguousarray(sx["dagg2"].reshape(P, P, n_hh).transpose(0, 2, 1)),
            np.ascontiguousarray(sy["dagg2"].reshape(P, P, orc.n_e).transpose(0, 2, 1)))


def income_grid_linear(J2, dx, dy):
    """dagg2 (P, N) = J2x dx + J2y dy of J2 = `oracle_income_grid_jacobians`' pair; dx (n_hh, P, N) or None, dy (n_e, P, N) or None"""
    return (0.0 if dx is None else np.einsum("tks,ksn->tn", J2[0], dx)) + (0.0 if dy is None else np.einsum("tes,esn->tn", J2[1], dy))


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


def check_income_edges(name, grid, pol):
    """a policy sequence pol (P, n_a, n_e) recorded under `income_path` still holds the edges of its raw-grid economy: the figures
    `shock_refs.check_path_edges` asks for under a beta path, as they are"""
    return shock_refs.check_path_edges(name, grid, pol)


def rescaled_D0(c, scale=D0_SCALE):
    """a second D_0 (G,) of case c (three columns) whose column masses differ: column e scaled by scale[e], renormalised"""
    n_a, n_e = c["V"].shape
    assert n_e == len(scale)
    D = np.asarray(c["D"]).reshape((n_a, n_e), order="F") * np.asarray(scale)[None, :]
    return np.ascontiguousarray((D / D.sum()).reshape(-1, order="F"))


def income_seeds(c, N, seed, t_only=None):
    """(dx (n_hh, P, N), dy (n_e, P, N)): random directions of the inputs' and of the path's scale; t_only: dy in that period alone"""
    rng = np.random.default_rng(seed)
    n_hh, P = c["x"].shape
    n_e = c["y"].shape[0]
    dx = rng.standard_normal((n_hh, P, N)) * 1e-2
    dy = rng.standard_normal((n_e, P, N)) * 1e-2
    if t_only is not None:
        keep = np.zeros((1, P, 1)); keep[0, t_only] = 1.0
        dy = dy * keep
    return dx, dy


class StubIncomeBlock:
    """stands in for the device context under `income_jacobian`: fake_news_income hands out the F and Dv it was made with"""

    def __init__(self, F, Dv):
        self.F, self.Dv, self.calls = F, Dv, 0

    def fake_news_income(self, n_het):
        self.calls += 1
        return self.F[..., :n_het].copy(), self.Dv[..., :n_het].copy()
