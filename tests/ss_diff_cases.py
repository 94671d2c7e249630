"""The dense reference of hank_ss_jvp / hank_ss_vjp (CPU only): the steady state's linear operators column by column from the CPU
oracle's dual arithmetic, then direct solves — independent of the fixed-point loops and of every kernel under test.

    B_V, P_V   d(Value, policy) / d value_next   Oracle.value_function, unit tangents on value_next, 32 columns per pass
    B_x, P_x   d(Value, policy) / d (r, w[, tr]) the same, tangents on the prices
    Lam, S_p   d D_new / d D_prev, d D_new / d policy   Oracle.transition_step with a Dual D and a Dual policy
    dV = solve(I - B_V, B_x dx)      da' = P_V dV + P_x dx      dD = solve(I - Lam + D 1', S_p da')
    dY_o = sum f_o dD + sum D df_o   from the closed forms: consumption (1+r) a + w z + tr - a', Value (1+r) c^-gamma, UCE z c^-gamma

The economies: Krusell-Smith 50x2 and 30x3 and the one-asset HANK with sticky wages 30x3 at the repository's steady states
(polished: the oracle's VFI to 1e-13 and its power method to 1e-15 from them, so that (V, D) is a fixed point far below the tests'
bounds), and `clamp`: a Krusell-Smith household on a grid that is dense at the bottom, at prices where the borrowing constraint
clamps more source rows of the low-income column than one row block of hank_vjp's widest geometry owns."""
import numpy as np

import cases
from conftest import ks_setup
from oracle.oracle import SUPPORTED_N, Oracle, pad_N

TOL = 1e-13            # the loops' tolerance in every GPU test
MAX_ITER = 20_000      # and their cap: a loop that does not converge ends the test
T_SHORT = 12           # periods of the contexts that record the stationary primal (the record is read at periods 0 and 1)


def _vf(orc, V, x, N=1):
    st, Vn, KD = orc.value_function(V, x[0], x[1], N, None if len(x) < 3 else x[2])
    assert st == 0, st
    return Vn, KD


def steady_state(orc, x, V0=None, D0=None, tol_v=1e-13, tol_d=1e-15, cap=200_000):
    """the oracle's own steady state at the household prices x: VFI (SteadyState.jl:132-141) to tol_v, the power method on
    transition_step to tol_d, renormalised. From ones (V0 None, the `clamp` economy) the value comes from Oracle.vfi; a warm start or
    a transfer input, which Oracle.vfi does not take, runs the same iteration on Oracle.value_function here (after Oracle.vfi it
    confirms the fixed point in one or two steps). x: (r, w) or (r, w, tr) floats. -> (V, policy, D (G,), vfi steps)"""
    if V0 is None and len(x) == 2:      # from ones: Oracle.vfi itself (no warm start there; the loop below is the same iteration)
        V0, _, steps0, _ = orc.vfi((orc.n_a, orc.n_e), x[0], x[1], tol_v, cap)
    V = np.ones((orc.n_a, orc.n_e)) if V0 is None else np.array(V0, dtype=np.float64)
    for k in range(1, cap + 1):
        Vn, KD = _vf(orc, V, x)
        diff = np.max(np.abs(Vn[..., 0] - V))
        V = Vn[..., 0]
        if diff < tol_v:
            break
    else:
        raise RuntimeError("the oracle's VFI did not converge")
    steps = k
    pol = KD[..., 0]
    D = np.full((orc.n_a, orc.n_e), 1.0 / orc.G) if D0 is None else np.asarray(D0, dtype=np.float64).reshape((orc.n_a, orc.n_e), order="F")
    pd = np.stack([pol, np.zeros_like(pol)], axis=-1)
    for _ in range(cap):
        Dn = orc.transition_step(pd, np.stack([D, np.zeros_like(D)], axis=-1), 1)[..., 0]
        diff = np.max(np.abs(Dn - D))
        D = Dn
        if diff < tol_d:
            break
    else:
        raise RuntimeError("the oracle's power method did not converge")
    D = D / D.sum()
    return V, pol, D.reshape(-1, order="F"), steps


def _unit_passes(G):
    for c0 in range(0, G, SUPPORTED_N[-1]):
        n = min(SUPPORTED_N[-1], G - c0)
        yield c0, n, pad_N(n)


def _seed(orc, M, c0, n, Nc, on):
    d = np.zeros((orc.n_a, orc.n_e, 1 + Nc))
    d[..., 0] = M
    if on:
        for k in range(n):
            e, a = divmod(c0 + k, orc.n_a)
            d[a, e, 1 + k] = 1.0
    return d


def operators(orc, x, V, pol, D):
    """the dense operators at the stationary point -> dict(BV, PV (G, G), Bx, Px (G, n_hh), Lam, Sp (G, G))"""
    G, n_hh = orc.G, len(x)
    Dm = np.asarray(D).reshape((orc.n_a, orc.n_e), order="F")
    BV, PV, Lam, Sp = (np.empty((G, G)) for _ in range(4))
    for c0, n, Nc in _unit_passes(G):
        Vn, KD = _vf(orc, _seed(orc, V, c0, n, Nc, True), x, Nc)
        BV[:, c0:c0 + n] = Vn[..., 1:1 + n].reshape((G, n), order="F")
        PV[:, c0:c0 + n] = KD[..., 1:1 + n].reshape((G, n), order="F")
        out = orc.transition_step(_seed(orc, pol, c0, n, Nc, False), _seed(orc, Dm, c0, n, Nc, True), Nc)
        Lam[:, c0:c0 + n] = out[..., 1:1 + n].reshape((G, n), order="F")
        out = orc.transition_step(_seed(orc, pol, c0, n, Nc, True), _seed(orc, Dm, c0, n, Nc, False), Nc)
        Sp[:, c0:c0 + n] = out[..., 1:1 + n].reshape((G, n), order="F")
    Nc = pad_N(n_hh)
    xd = [np.concatenate([[x[k]], np.eye(Nc)[k]]) for k in range(n_hh)]
    st, Vn, KD = orc.value_function(np.asarray(V), xd[0], xd[1], Nc, None if n_hh < 3 else xd[2])
    assert st == 0
    Bx = Vn[..., 1:1 + n_hh].reshape((G, n_hh), order="F")
    Px = KD[..., 1:1 + n_hh].reshape((G, n_hh), order="F")
    return dict(BV=BV, PV=PV, Bx=Bx, Px=Px, Lam=Lam, Sp=Sp)


def reference(orc, x, V, pol, D, n_het, gamma):
    """the dense Jacobians of the steady state's household objects in the household prices, by direct solves:
    JV, Jpol, JD (G, n_hh) and JY (n_het, n_hh), with rhoV = rho(B_V) and rhoD = |lambda_2(Lam)|."""
    G, n_hh = orc.G, len(x)
    op = operators(orc, x, V, pol, D)
    Dv = np.asarray(D, dtype=np.float64)
    JV = np.linalg.solve(np.eye(G) - op["BV"], op["Bx"])
    Jpol = op["PV"] @ JV + op["Px"]
    JD = np.linalg.solve(np.eye(G) - op["Lam"] + np.outer(Dv, np.ones(G)), op["Sp"] @ Jpol)
    r, w, tr = x[0], x[1], (x[2] if n_hh > 2 else 0.0)
    a = np.tile(orc.a, orc.n_e)
    z = np.repeat(orc.z, orc.n_a)
    p = np.asarray(pol).reshape(-1, order="F")
    c = (1.0 + r) * a + w * z + tr - p
    dc = -Jpol.copy()                      # d consumption / d x at every point
    dc[:, 0] += a
    dc[:, 1] += z
    if n_hh > 2:
        dc[:, 2] += 1.0
    u, uc = c ** (-gamma), -gamma * c ** (-gamma - 1.0)
    fs = [p, c, (1.0 + r) * u, z * u]
    dfs = [Jpol, dc, (1.0 + r) * uc[:, None] * dc, (z * uc)[:, None] * dc]
    dfs[2] = dfs[2].copy()
    dfs[2][:, 0] += u
    JY = np.stack([fs[o] @ JD + Dv @ dfs[o] for o in range(n_het)])
    ev = np.linalg.eigvals(op["BV"])
    el = np.sort(np.abs(np.linalg.eigvals(op["Lam"])))[::-1]
    assert abs(el[0] - 1.0) < 1e-9, el[:3]
    return dict(op=op, JV=JV, Jpol=Jpol, JD=JD, JY=JY, rhoV=float(np.max(np.abs(ev))), rhoD=float(el[1]), f=fs[:n_het])


def bound(rho, tol=TOL):
    """how far a fixed-point iteration stopped on increments <= tol (relative) can sit from its limit: the remaining geometric
    tail tol rho / (1 - rho), with a factor of 10 for the non-normal transient"""
    return 10.0 * tol / (1.0 - rho)


CLAMP_N_A, CLAMP_N_E = 190, 2


def clamp_grid():
    """100 evenly spaced rows below 0.04 (the constrained region of the low-income column ends near 0.03), 90 more up to 20"""
    return np.concatenate([np.linspace(0.0, 0.04, 100, endpoint=False), 0.04 + 20.0 * np.linspace(0.0, 1.0, CLAMP_N_A - 100) ** 3])


_CASES = {}
NAMES = ("ks50x2", "ks30x3", "hank30x3", "clamp")


def case(name):
    """-> dict(args: HouseholdBlock's constructor arguments (T = T_SHORT), orc, x (n_hh,), V (n_a, n_e), pol, D (G,), n_het: the
    family's count of outputs, gamma, ref: `reference` of it), cached per session"""
    if name in _CASES:
        return _CASES[name]
    if name in ("ks50x2", "ks30x3"):
        m, ss, orc = ks_setup(50, 2, 100) if name == "ks50x2" else ks_setup(30, 3, 40)
        x = np.array([ss.vars["r"], ss.vars["w"]])
        V0, D0, n_het = ss.value, ss.D, 3
        args = cases.model_args(m)
    elif name == "hank30x3":
        m, ss = cases.hank_economy(30, 3, 40, "one_asset_hank_wages.yaml")
        orc = cases.oracle_of(m)
        x = np.array([ss.vars["r"], ss.vars["om"], ss.vars["Tr"]])
        V0, D0, n_het = ss.value, ss.D, 4
        args = cases.model_args(m)
    else:
        m, ss, _ = ks_setup(30, 3, 40)
        pdm = m.heterogeneity["productivity"]
        z = np.array([pdm.grid[0], pdm.grid[-1]])
        Pi = np.array([[0.9, 0.1], [0.1, 0.9]])
        grid = clamp_grid()
        orc = Oracle(grid, z, Pi, m.params.β, m.params.γ, m.params.borrow_cons)
        x = np.array([0.6 * ss.vars["r"], ss.vars["w"]])
        V0, D0, n_het = None, None, 3
        args = cases.raw_args(grid, z, Pi, m, T_SHORT)
    V, pol, D, _ = steady_state(orc, x, V0, D0)
    if name == "clamp":
        clo = (pol <= orc.a[0]).sum(axis=0)
        print(f"clamp: {clo} source rows clamped per column, rows per block {cases.adj_rows_per_block(1)}, mass on row 0 {D.reshape((orc.n_a, orc.n_e), order='F')[0]}")
        assert clo.max() > cases.adj_rows_per_block(1), (clo, "the constraint must clamp more source rows than one block of the widest geometry owns")
        assert orc.G <= 400
    args = args[:6] + (T_SHORT,) + args[7:]
    gamma = args[4]
    _CASES[name] = dict(args=args, orc=orc, x=x, V=V, pol=pol, D=D, n_het=n_het, gamma=gamma, ref=reference(orc, x, V, pol, D, n_het, gamma))
    return _CASES[name]
