"""The dense reference of hank_ss_jvp / hank_ss_vjp (CPU only): the steady state's linear operators column by column from the CPU
oracle's dual arithmetic, then direct solves — independent of the fixed-point loops and of every kernel under test.

    B_V, P_V   d(Value, policy) / d value_next   Oracle.value_function, unit tangents on value_next, 32 columns per pass
    B_x, P_x   d(Value, policy) / d (r, w[, tr]) the same, tangents on the prices
    Lam, S_p   d D_new / d D_prev, d D_new / d policy   Oracle.transition_step with a Dual D and a Dual policy
    dV = solve(I - B_V, B_x dx)      da' = P_V dV + P_x dx      dD = solve(I - Lam + D 1', S_p da')
    dY_o = sum f_o dD + sum D df_o   from the closed forms: consumption (1+r) a + w z + tr - a', Value (1+r) c^-gamma, UCE z c^-gamma

The economies: Krusell-Smith 50x2 and 30x3 and the one-asset HANK with sticky wages 30x3 at the repository's steady states
(polished: the oracle's VFI to 1e-13, then to increments of four ulps of max V, and its power method to 1e-15 from them, so that
(V, D) is a fixed point far below the tests' bounds — see `case`), and `clamp`: a Krusell-Smith household on a grid that is dense
at the bottom, at prices where the borrowing constraint clamps more source rows of the low-income column than one row block of
hank_vjp's widest geometry owns. Five more (NEW_NAMES):
Krusell-Smith 40x16 and 40x5, and Krusell-Smith 40x3 at gamma = 1, 0.5 and 3, each at its own host steady state. `case` also
builds Krusell-Smith 64x4 (G = 256) for the fake-news module (tests/fake_news_refs.py), which is in none of the NAMES.

The module ends with the four fixed-point loops as plain numpy iterations on these operators under the device's stopping rules
(`jvp_loops`, `vjp_loops`): the step counts the GPU tests compare the device's `iters` with."""
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
# the first four run the widths 1, 3, 4, 33 (and `clamp`, `hank30x3` every lane geometry: tests/test_gpu_ss_diff.py); the rest:
# n_e = 16 (1024-thread blocks, the largest LDS tiles), n_e = 5 (the smallest above RB = 4 rows per wave instruction), and the
# curvatures of cases.CASES (record diet on at gamma = 1, off at 0.5 and 3) on Krusell-Smith 40x3
OLD_NAMES = ("ks50x2", "ks30x3", "hank30x3", "clamp")
NEW_NAMES = ("ks40x16", "ks40x5", "gamma1", "gamma0.5", "gamma3")
NAMES = OLD_NAMES + NEW_NAMES
_KS_SHAPE = {"ks50x2": (50, 2, 100), "ks30x3": (30, 3, 40), "ks40x16": (40, 16, 40), "ks40x5": (40, 5, 40),
             "ks64x4": (64, 4, 40)}      # G = 256, for tests/test_gpu_fake_news_dense.py alone: not in NAMES
_GAMMA = {"gamma1": 1.0, "gamma0.5": 0.5, "gamma3": 3.0}
_GAMMA_ECON = {}


def _ks_at_gamma(gamma):
    """Krusell-Smith 40x3 at gamma, in the manner of cases.economy: a fresh model, its gamma set, its steady state solved on the host"""
    if gamma not in _GAMMA_ECON:
        import hank_amd as h
        ov = {"T": 40, "dimensions": {"wealth": {"n": 40}, "productivity": {"n": 3}}}
        m = h.build_model_from_yaml(str(cases.ROOT / "examples" / "krusell_smith.yaml"), overrides=ov)
        m.params.γ = gamma
        ss, _ = h.get_SteadyStates(m, vfi="host")
        assert m.params.γ == gamma
        _GAMMA_ECON[gamma] = (m, ss, cases.oracle_of(m))
    return _GAMMA_ECON[gamma]


def case(name):
    """-> dict(args: HouseholdBlock's constructor arguments (T = T_SHORT), orc, x (n_hh,), V (n_a, n_e), pol, D (G,), n_het: the
    family's count of outputs, gamma, ref: `reference` of it), cached per session"""
    if name in _CASES:
        return _CASES[name]
    if name in _KS_SHAPE or name in _GAMMA:
        m, ss, orc = ks_setup(*_KS_SHAPE[name]) if name in _KS_SHAPE else _ks_at_gamma(_GAMMA[name])
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
    # ... and on to the VFI's rounding floor. Increments of 1e-13 leave V 1e-13 / (1 - rho) = 4e-12 from the fixed point; where V is
    # small (the top of the grid: 0.009 at gamma = 3) that is 4e-10 relative, and the policy's tangent at V then sits 5e-8 (gamma = 3,
    # on a scale of 97) from the one at the fixed point — four times the bound of the GPU tests, whose record is the fixed point's
    # to eleven more steps. 100 to 220 steps more in every economy.
    V, pol, D, _ = steady_state(orc, x, V, D, tol_v=4.0 * np.finfo(np.float64).eps * np.abs(V).max(), cap=20_000)
    if name == "clamp":
        clo = (pol <= orc.a[0]).sum(axis=0)
        print(f"clamp: {clo} source rows clamped per column, rows per block {cases.adj_rows_per_block(1)}, mass on row 0 {D.reshape((orc.n_a, orc.n_e), order='F')[0]}")
        assert clo.max() > cases.adj_rows_per_block(1), (clo, "the constraint must clamp more source rows than one block of the widest geometry owns")
        assert orc.G <= 400
    if name == "ks40x16":      # both clamps of the lottery among its sixteen columns
        clo, top = (pol <= orc.a[0]).sum(axis=0), (pol >= orc.a[-1]).sum(axis=0)
        print(f"ks40x16: source rows clamped at the bottom per column {clo}, at the top {top}")
        assert np.count_nonzero(clo) >= 2 and np.count_nonzero(top) >= 2 and orc.G == 640
    args = args[:6] + (T_SHORT,) + args[7:]
    gamma = args[4]
    _CASES[name] = dict(args=args, orc=orc, x=x, V=V, pol=pol, D=D, n_het=n_het, gamma=gamma, ref=reference(orc, x, V, pol, D, n_het, gamma))
    return _CASES[name]


# ---- the four loops as plain numpy iterations on the dense operators, under the device's stopping rules ----------------------------
# Nothing here comes from the device: the step counts the GPU tests compare `iters` with, and what test_ss_diff_host.py pins
# against the dense solves.
def iterate(A, src, tol=TOL, centre=None, cap=MAX_ITER, first=None):
    """v <- A v + src from zero until max |v_new - v| <= tol max |v_new| in EVERY column (k_ss_check); centre = D: every new iterate
    is centred, v_new -= D 1'v_new (k_ss_check_dist); first: the first iterate where it is not A 0 + src.
    -> (v, steps), steps = cap + 1 when the rule never held"""
    v = np.zeros_like(src)
    for k in range(1, cap + 1):
        vn = A @ v + src if first is None or k > 1 else first
        if centre is not None:
            vn = vn - np.outer(centre, vn.sum(axis=0))
        done = np.all(np.max(np.abs(vn - v), axis=0) <= tol * np.max(np.abs(vn), axis=0))
        v = vn
        if done:
            return v, k
    return v, cap + 1


def value_loop_start(c, dx):
    """the first iterate of the device's value loop. Its state is the knots' tangent ds, not dV: one step is dV_new = Y(ds, dx), then
    ds_new = X(dV_new, dx) (tan_back_body's two halves, B_V = Y X), and it starts from ds = 0 — not from the ds that belongs to dV = 0,
    which carries X's own price terms. So dV_1 = Y(0, dx), the prices' effect at a fixed policy and a fixed continuation value:
    dV = c^-gamma dr + (1 + r) u''(c) (a dr + z dw + dtr), from the closed form of Value; from dV_2 on the steps are B_V dV + B_x dx."""
    x, n_hh, gam, orc = c["x"], len(c["x"]), c["gamma"], c["orc"]
    a, z = np.tile(orc.a, orc.n_e), np.repeat(orc.z, orc.n_a)
    cons = (1.0 + x[0]) * a + x[1] * z + (x[2] if n_hh > 2 else 0.0) - np.asarray(c["pol"]).reshape(-1, order="F")
    dcdx = np.stack([a, z, np.ones(orc.G)][:n_hh], axis=1)
    return np.outer(cons ** (-gam), dx[0]) + (-gam * (1.0 + x[0]) * cons ** (-gam - 1.0))[:, None] * (dcdx @ dx)


def jvp_loops(c, dx, tol=TOL):
    """hank_ss_jvp's two loops: dV <- B_V dV + B_x dx from the device's first iterate (`value_loop_start`), then dD <- Lam dD + S_p da'
    from zero with da' of the CONVERGED loop (not of the dense solve). -> (dV, dD (G, N), (value steps, distribution steps))"""
    op = c["ref"]["op"]
    dV, kv = iterate(op["BV"], op["Bx"] @ dx, tol, first=value_loop_start(c, dx))
    dD, kd = iterate(op["Lam"], op["Sp"] @ (op["PV"] @ dV + op["Px"] @ dx), tol, centre=c["D"])
    return dV, dD, (kv, kd)


def output_partials(c):
    """the outputs' direct dependence at every point -> (fp, fc (n_het, G): df_o / da' and df_o / dc at fixed a'; dcdx (G, n_hh):
    dc / dx at fixed a'; u (G,): c^-gamma, Value's own dependence on r)"""
    x, n_hh, n_het, gam = c["x"], len(c["x"]), c["n_het"], c["gamma"]
    orc = c["orc"]
    G = orc.G
    a, z = np.tile(orc.a, orc.n_e), np.repeat(orc.z, orc.n_a)
    p = np.asarray(c["pol"]).reshape(-1, order="F")
    cons = (1.0 + x[0]) * a + x[1] * z + (x[2] if n_hh > 2 else 0.0) - p
    u, uc = cons ** (-gam), -gam * cons ** (-gam - 1.0)
    fp = np.stack([np.ones(G), -np.ones(G), -(1.0 + x[0]) * uc, -z * uc][:n_het])
    fc = np.stack([np.zeros(G), np.ones(G), (1.0 + x[0]) * uc, z * uc][:n_het])
    return fp, fc, np.stack([a, z, np.ones(G)][:n_hh], axis=1), u


def vjp_loops(c, yb, Vb, Db, tol=TOL, cap=MAX_ITER):
    """hank_ss_vjp's two loops; yb (n_het, M), Vb, Db (G, M), any of them None. The lambda loop with k_ss_lam's centring: e_0 = g -
    (D'g) 1, lam = e_0; e <- Lam'e - (D'e_in) 1, lam += e, until max |e| <= tol max |lam| in every column. Then pbar = S_p'lam + D
    sum_o yb_o df_o/da', and nu <- B_V'nu + (P_V'pbar + Vb) from zero under `iterate`'s rule.
    -> (xbar (n_hh, M), (nu steps, lambda steps))"""
    r, op, D = c["ref"], c["ref"]["op"], c["D"]
    n_het = c["n_het"] if yb is None else yb.shape[0]
    M = next(v.shape[1] for v in (yb, Vb, Db) if v is not None)
    yb = np.zeros((n_het, M)) if yb is None else yb
    fp, fc, dcdx, u = output_partials(c)
    g = np.stack(r["f"][:n_het]).T @ yb + (0.0 if Db is None else Db)
    e = g - D @ g
    lam, cen = e.copy(), np.zeros(M)
    for kl in range(1, cap + 1):
        e = op["Lam"].T @ e - cen
        lam = lam + e
        cen = D @ e
        if np.all(np.max(np.abs(e), axis=0) <= tol * np.max(np.abs(lam), axis=0)):
            break
    else:
        kl = cap + 1
    pbar = op["Sp"].T @ lam + D[:, None] * (fp[:n_het].T @ yb)
    src = op["PV"].T @ pbar + (0.0 if Vb is None else Vb)
    nu, kn = iterate(op["BV"].T, src, tol, cap=cap)
    direct = dcdx.T @ (D[:, None] * (fc[:n_het].T @ yb))
    if n_het > 2:
        direct[0] += yb[2] * (D @ u)
    return op["Px"].T @ pbar + op["Bx"].T @ nu + direct, (kn, kl)
