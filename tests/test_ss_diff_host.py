"""The dense reference of hank_ss_jvp / hank_ss_vjp (tests/ss_diff_cases.py) on the CPU: it is its own transpose, its dK/d(r, w)
agrees with finite differences of the oracle's steady state, and the plain fixed-point iterations the device runs converge to
it inside the GPU tests' bound and cap."""
import numpy as np
import pytest

import ss_diff_cases as S


@pytest.mark.parametrize("name", S.NAMES)
def test_reference_is_its_own_transpose(name):
    """<ybar, dY> + <Vbar, dV> + <Dbar, dD> = <xbar, dx> with xbar from the transposed solves (lambda, then nu), not from the
    transposed Jacobian: the two orders of the same algebra agree to 1e-12 relative."""
    c = S.case(name)
    r, op = c["ref"], c["ref"]["op"]
    G, n_hh, n_het = c["orc"].G, len(c["x"]), c["n_het"]
    rng = np.random.default_rng(3)
    dx, yb, Vb, Db = rng.standard_normal(n_hh), rng.standard_normal(n_het), rng.standard_normal(G), rng.standard_normal(G)
    lhs = yb @ (r["JY"] @ dx) + Vb @ (r["JV"] @ dx) + Db @ (r["JD"] @ dx)
    # the transposed route of the issue: g, lambda, pbar, nu, xbar
    D = c["D"]
    F = np.stack(r["f"])                                         # (n_het, G)
    g = F.T @ yb + Db
    g = g - (D @ g)
    lam = np.linalg.solve((np.eye(G) - op["Lam"] + np.outer(D, np.ones(G))).T, g)
    pbar = op["Sp"].T @ lam
    # the outputs' direct dependence: df_o = (df_o/da') da' + (df_o/dc) (a, z, 1) dx [+ c^-gamma dr for Value]
    x = c["x"]
    a, z = np.tile(c["orc"].a, c["orc"].n_e), np.repeat(c["orc"].z, c["orc"].n_a)
    p = np.asarray(c["pol"]).reshape(-1, order="F")
    cons = (1.0 + x[0]) * a + x[1] * z + (x[2] if n_hh > 2 else 0.0) - p
    gam = c["gamma"]
    u, uc = cons ** (-gam), -gam * cons ** (-gam - 1.0)
    fp = [np.ones(G), -np.ones(G), -(1.0 + x[0]) * uc, -z * uc][:n_het]          # df_o / da'
    fc = [np.zeros(G), np.ones(G), (1.0 + x[0]) * uc, z * uc][:n_het]           # df_o / dc at fixed a'
    pbar = pbar + D * sum(yb[o] * fp[o] for o in range(n_het))
    nu = np.linalg.solve((np.eye(G) - op["BV"]).T, op["PV"].T @ pbar + Vb)
    dcdx = np.stack([a, z, np.ones(G)][:n_hh], axis=1)
    direct = sum(yb[o] * ((D * fc[o]) @ dcdx) for o in range(n_het))
    if n_het > 2:
        direct[0] += yb[2] * (D @ u)
    xbar = op["Px"].T @ pbar + op["Bx"].T @ nu + direct
    rhs = xbar @ dx
    print(f"{name}: lhs {lhs:.15e} rhs {rhs:.15e}")
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs))
    JT = r["JY"].T @ yb + r["JV"].T @ Vb + r["JD"].T @ Db
    assert np.max(np.abs(xbar - JT)) <= 1e-12 * np.max(np.abs(JT))


@pytest.mark.parametrize("name", ("ks50x2", "ks30x3"))
def test_reference_against_finite_differences(name):
    """dK/d(r, w) of the dense implicit solve against central differences (h = 1e-6) of the oracle's own steady state (VFI to
    1e-13, power method to 1e-15, renormalised): 1e-3 relative — the finite differences cross kinks; this catches a missing term
    or a wrong sign, it is not a parity bound."""
    c = S.case(name)
    orc, x, h = c["orc"], c["x"], 1e-6

    def K(xx):
        V, pol, D, _ = S.steady_state(orc, xx, c["V"], c["D"])
        return float(pol.reshape(-1, order="F") @ D)

    for k in range(2):
        e = np.zeros(len(x))
        e[k] = h
        fd = (K(x + e) - K(x - e)) / (2 * h)
        ref = c["ref"]["JY"][0, k]
        print(f"{name}: dK/dx{k} implicit {ref:.8g} finite differences {fd:.8g} (relative {abs(fd - ref) / abs(ref):.2e})")
        assert abs(fd - ref) <= 1e-3 * abs(ref)


@pytest.mark.parametrize("name", S.NAMES)
def test_plain_iterations_reach_the_dense_solve(name):
    """JVP steps 1 and 4 as plain numpy iterations with the device's stopping rule (increment <= tol scale in every column, the
    distribution centred at every check): they land within 10 tol / (1 - rho) of the dense solve, in fewer steps than the cap of
    the GPU tests."""
    c = S.case(name)
    r, op, D = c["ref"], c["ref"]["op"], c["D"]
    n_hh = len(c["x"])
    dx = np.random.default_rng(5).standard_normal((n_hh, 3))

    def iterate(A, src, centre):
        v = np.zeros_like(src)
        for k in range(1, S.MAX_ITER + 1):
            vn = A @ v + src
            if centre:
                vn = vn - np.outer(D, vn.sum(axis=0))
            done = np.all(np.max(np.abs(vn - v), axis=0) <= S.TOL * np.max(np.abs(vn), axis=0))
            v = vn
            if done:
                return v, k
        return v, S.MAX_ITER + 1

    dV, kv = iterate(op["BV"], op["Bx"] @ dx, False)
    refV = r["JV"] @ dx
    errV = np.max(np.abs(dV - refV)) / np.max(np.abs(refV))
    dD, kd = iterate(op["Lam"], op["Sp"] @ (r["Jpol"] @ dx), True)
    refD = r["JD"] @ dx
    errD = np.max(np.abs(dD - refD)) / np.max(np.abs(refD))
    print(f"{name}: value loop {kv} steps, {errV:.2e} from the solve (bound {S.bound(r['rhoV']):.2e}); "
          f"distribution loop {kd} steps, {errD:.2e} (bound {S.bound(r['rhoD']):.2e}); 1'dD {np.abs(dD.sum(axis=0)).max():.2e}")
    assert kv < S.MAX_ITER and kd < S.MAX_ITER
    assert errV <= S.bound(r["rhoV"]) and errD <= S.bound(r["rhoD"])


@pytest.mark.parametrize("name", S.NAMES)
def test_numpy_loops_reach_the_dense_solves(name):
    """the loops the GPU tests count steps against (S.jvp_loops, S.vjp_loops: the device's four stopping rules on the dense
    operators) at the tolerance of those tests, 1e-9: the JVP's land on the dense solves and the VJP's on the transposed dense
    Jacobian inside S.bound(rho, 1e-9), none runs into the cap. The transposed loops see every cotangent at once and each alone."""
    c = S.case(name)
    r, tol = c["ref"], 1e-9
    G, n_hh, n_het = c["orc"].G, len(c["x"]), c["n_het"]
    rng = np.random.default_rng(9)
    dx = rng.standard_normal((n_hh, 3))
    dV, dD, (kv, kd) = S.jvp_loops(c, dx, tol)
    refV, refD = r["JV"] @ dx, r["JD"] @ dx
    errV, errD = np.max(np.abs(dV - refV)) / np.max(np.abs(refV)), np.max(np.abs(dD - refD)) / np.max(np.abs(refD))
    rho = max(r["rhoV"], r["rhoD"])
    print(f"{name}: value loop {kv} steps, {errV:.2e} (bound {S.bound(r['rhoV'], tol):.2e}); distribution loop {kd} steps, {errD:.2e} (bound {S.bound(rho, tol):.2e})")
    assert kv < S.MAX_ITER and kd < S.MAX_ITER
    assert errV <= S.bound(r["rhoV"], tol) and errD <= S.bound(rho, tol)
    yb, Vb, Db = rng.standard_normal((n_het, 3)), rng.standard_normal((G, 3)), rng.standard_normal((G, 3))
    for what, (y, v, d) in {"all": (yb, Vb, Db), "agg": (yb, None, None), "value": (None, Vb, None), "D": (None, None, Db)}.items():
        xbar, (kn, kl) = S.vjp_loops(c, y, v, d, tol)
        JT = (r["JY"].T @ y if y is not None else 0.0) + (r["JV"].T @ v if v is not None else 0.0) + (r["JD"].T @ d if d is not None else 0.0)
        err = np.max(np.abs(xbar - JT)) / np.max(np.abs(JT))
        print(f"{name} {what}: nu loop {kn} steps, lambda loop {kl} steps, xbar {err:.2e} from the transposed Jacobian (bound {S.bound(rho, tol):.2e})")
        assert kn < S.MAX_ITER and kl < S.MAX_ITER
        assert err <= S.bound(rho, tol)


def test_implicit_price_jacobian_needs_the_device(hank):
    """find_ss(price_jacobian="implicit") with the host VFI raises: there is no silent fallback to finite differences"""
    from conftest import ROOT
    m = hank.build_model_from_yaml(str(ROOT / "examples" / "krusell_smith.yaml"), overrides={"T": 20, "dimensions": {"wealth": {"n": 30}, "productivity": {"n": 2}}})
    with pytest.raises(ValueError, match="implicit"):
        hank.find_ss(m, m.ss_initial, "initial", vfi="host", price_jacobian="implicit")
    with pytest.raises(ValueError, match="price_jacobian"):
        hank.find_ss(m, m.ss_initial, "initial", vfi="host", price_jacobian="autodiff")
