"""What tests/test_jvp_het_host.py and tests/test_gpu_jvp_het.py share: the references of hank_jvp_het / hank_vjp_het_boundary.

1. `oracle_het_boundary`: the oracle loop of tests/boundary_cases.py (duals on the inputs AND on the boundary) that also returns the
   outputs >= 2. Value is the dual V_t that `Oracle.value_function` returns in that loop — the reference's own Value key
   (KrusellSmith.jl:80); UCE is z_e c^-gamma by the chain rule on the consumption dual, as in `Oracle.het_outputs`. Both are dotted
   with the dual post-transition D_t of `Oracle.transition_step` (ForwardIteration.jl:303-307);
2. the tangent map with extra outputs under boundary seeds and its transpose, in numpy, on the random records of
   tests/test_vjp_host.py with random f, f_c, S as in tests/test_vjp_het_host.py."""
import numpy as np

from oracle.oracle import SUPPORTED_N, pad_N
from test_vjp_host import _cons


# ---- 1. the oracle loop -------------------------------------------------------------------------------------------------------
def oracle_het_boundary(orc, x, V, D, gamma, n_het, y=None, dV=None, dD=None):
    """x (n_hh, P), boundary V (n_a, n_e), D (G,); seeds y (n_hh, P, N), dV, dD (n_a, n_e, N), None = zeros, one at least given.
    -> dict: agg (P, n_het) and dagg (P, n_het, N) of (savings, consumption, Value[, UCE]) — the shapes of hank_get_het_outputs;
    agg2 (P,), dagg2 (P, N) the wealth grid's aggregate; pol (P, n_a, n_e), dpol (P, n_a, n_e, N)."""
    x = np.asarray(x, dtype=np.float64)
    n_hh, P = x.shape
    n_a, n_e, a, z = orc.n_a, orc.n_e, orc.a, orc.z
    N = next(np.asarray(v).shape[-1] for v in (y, dV, dD) if v is not None)
    out = {k: [] for k in ("dagg", "dagg2", "dpol")}
    for c0 in range(0, N, SUPPORTED_N[-1]):
        n = min(N, c0 + SUPPORTED_N[-1]) - c0
        Nc = pad_N(n)
        xd = np.zeros((n_hh, P, 1 + Nc)); xd[..., 0] = x
        Vn = np.zeros((n_a, n_e, 1 + Nc)); Vn[..., 0] = V
        Dd = np.zeros((n_a, n_e, 1 + Nc)); Dd[..., 0] = np.asarray(D).reshape((n_a, n_e), order="F")
        if y is not None:
            xd[..., 1:1 + n] = y[:, :, c0:c0 + n]
        if dV is not None:
            Vn[..., 1:1 + n] = dV[:, :, c0:c0 + n]
        if dD is not None:
            Dd[..., 1:1 + n] = dD[:, :, c0:c0 + n]
        pol, val = [None] * P, [None] * P
        for t in range(P - 1, -1, -1):
            st, Vn, pol[t] = orc.value_function(Vn, xd[0, t], xd[1, t], Nc, xd[2, t] if n_hh > 2 else None)
            assert st == 0, (t, st)
            val[t] = Vn
        agg, agg2 = np.zeros((P, n_het)), np.zeros(P)
        dagg, dagg2 = np.zeros((P, n_het, n)), np.zeros((P, n))
        for t in range(P):
            Dd = orc.transition_step(pol[t], Dd, Nc)
            p0, dp, D0, dDt = pol[t][..., 0], pol[t][..., 1:1 + n], Dd[..., 0], Dd[..., 1:1 + n]
            tr, dtr = (xd[2, t, 0], xd[2, t, 1:1 + n]) if n_hh > 2 else (0.0, np.zeros(n))
            c0_ = (1.0 + xd[0, t, 0]) * a[:, None] + xd[1, t, 0] * z[None, :] + tr - p0          # KrusellSmith.jl:79
            dc = xd[0, t, 1:1 + n] * a[:, None, None] + xd[1, t, 1:1 + n] * z[None, :, None] + dtr - dp
            fs = [(p0, dp), (c0_, dc), (val[t][..., 0], val[t][..., 1:1 + n]),
                  (z[None, :] * c0_ ** (-gamma), (z[None, :] * (-gamma) * c0_ ** (-gamma - 1.0))[..., None] * dc)]
            for o, (f0, df) in enumerate(fs[:n_het]):
                agg[t, o] = np.sum(f0 * D0)
                dagg[t, o] = np.einsum("aen,ae->n", df, D0) + np.einsum("ae,aen->n", f0, dDt)
            agg2[t] = np.sum(a[:, None] * D0)
            dagg2[t] = np.einsum("a,aen->n", a, dDt)
        out["dagg"].append(dagg); out["dagg2"].append(dagg2)
        out["dpol"].append(np.stack([p[..., 1:1 + n] for p in pol]))
    res = {k: np.concatenate(v, axis=-1) for k, v in out.items()}
    res.update(agg=agg, agg2=agg2, pol=np.stack([p[..., 0] for p in pol]))
    return res


# ---- 2. both maps on a random record ------------------------------------------------------------------------------------------
def tangent_map_het_boundary(R, X, dx, dV_P, dD_0):
    """dx (3, P), dV_P, dD_0 (n_a, n_e) -> dagg (2 + NX, P): tests/test_vjp_het_host.py's tangent_map_het from non-zero dV_P and
    dD_0. The extra outputs read the dD_t the recurrence carries: dY^o_t = sum f_o,t dD_t - sum f_c,o,t D_t da'_t + the inputs'
    direct terms; consumption by its definition (a dD_0 seed moves its productivity marginal, tests/boundary_cases.py)."""
    n_a, n_e, P, a, z, Pi = R["n_a"], R["n_e"], R["P"], R["a"], R["z"], R["Pi"]
    NX = X["f"].shape[0]
    cols = np.arange(n_e)[None, :]
    dpol = np.zeros((P, n_a, n_e))
    dV = dV_P
    for t in range(P - 1, -1, -1):
        dr, dw, dtr = dx[:, t]
        rho = 1.0 / (1.0 + R["x"][0, t])
        ds = R["kc"][t] * (dV @ Pi.T) - rho * (z[None, :] * dw + dtr + R["s"][t] * dr)
        dg = R["A"][t] * ds[R["ib"][t], cols] + R["B"][t] * ds[R["ib"][t] + 1, cols]
        dpol[t] = dg
        dV = R["u"][t] * dr + R["v"][t] * ((a[:, None] * dr + z[None, :] * dw + dtr) - dg)
    dD = dD_0
    dagg = np.zeros((2 + NX, P))
    for t in range(P):
        dr, dw, dtr = dx[:, t]
        lo, w, g = R["lo"][t], R["w"][t], R["ig"][t] * R["D"][t]
        mid = np.zeros((n_a, n_e))
        cc = np.broadcast_to(cols, lo.shape)
        np.add.at(mid, (lo, cc), (1 - w) * dD - dpol[t] * g)
        np.add.at(mid, (lo + 1, cc), w * dD + dpol[t] * g)
        dD = mid @ Pi
        Dt = R["D"][t + 1]
        dagg[0, t] = np.sum(dpol[t] * Dt + R["pol"][t] * dD)
        dagg[1, t] = np.sum((a[:, None] * dr + z[None, :] * dw + dtr - dpol[t]) * Dt + _cons(R, t) * dD)
        for o in range(NX):
            Sa, Sz, S1, Sr = X["S"][o, t]
            dagg[2 + o, t] = np.sum(X["f"][o, t] * dD) - np.sum(X["fc"][o, t] * Dt * dpol[t]) + dr * (Sa + Sr) + dw * Sz + dtr * S1
    return dagg


def cotangent_map_het_boundary(R, X, yb):
    """yb (2 + NX, P) -> (xbar (3, P), Vbar_P (n_a, n_e), Dbar_0 (n_a, n_e)): Sweep A with the extra outputs' two terms, whose last
    state is the cotangent of D_0, then the unchanged Sweep B, whose last mu is the cotangent of the terminal value."""
    n_a, n_e, P, a, z, Pi = R["n_a"], R["n_e"], R["P"], R["a"], R["z"], R["Pi"]
    NX = X["f"].shape[0]
    cols = np.arange(n_e)[None, :]
    xbar = np.zeros((3, P))
    pbar = np.zeros((P, n_a, n_e))
    lam = np.zeros((n_a, n_e))
    for t in range(P - 1, -1, -1):
        Dt = R["D"][t + 1]
        lam = lam + yb[0, t] * R["pol"][t] + yb[1, t] * _cons(R, t)
        xbar[:, t] += yb[1, t] * np.array([np.sum(a[:, None] * Dt), np.sum(z[None, :] * Dt), np.sum(Dt)])
        direct = yb[0, t] - yb[1, t]
        for o in range(NX):
            Sa, Sz, S1, Sr = X["S"][o, t]
            lam = lam + yb[2 + o, t] * X["f"][o, t]
            direct = direct - yb[2 + o, t] * X["fc"][o, t]
            xbar[:, t] += yb[2 + o, t] * np.array([Sa + Sr, Sz, S1])
        U = lam @ Pi.T
        lo, w = R["lo"][t], R["w"][t]
        pbar[t] = direct * Dt + R["ig"][t] * R["D"][t] * (U[lo + 1, cols] - U[lo, cols])
        lam = (1 - w) * U[lo, cols] + w * U[lo + 1, cols]
    mu = np.zeros((n_a, n_e))
    for t in range(P):
        rho = 1.0 / (1.0 + R["x"][0, t])
        gbar = pbar[t] - R["v"][t] * mu
        xbar[:, t] += [np.sum(mu * (R["u"][t] + R["v"][t] * a[:, None])), np.sum(mu * R["v"][t] * z[None, :]), np.sum(mu * R["v"][t])]
        sbar = np.zeros((n_a, n_e))
        cc = np.broadcast_to(cols, gbar.shape)
        np.add.at(sbar, (R["ib"][t], cc), R["A"][t] * gbar)
        np.add.at(sbar, (R["ib"][t] + 1, cc), R["B"][t] * gbar)
        xbar[:, t] -= rho * np.array([np.sum(sbar * R["s"][t]), np.sum(sbar * z[None, :]), np.sum(sbar)])
        mu = (R["kc"][t] * sbar) @ Pi
    return xbar, mu, lam
