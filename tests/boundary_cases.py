"""What tests/test_boundary_host.py and tests/test_gpu_boundary.py share: the references of hank_jvp_boundary / hank_vjp_boundary.

1. `oracle_boundary`: the CPU oracle's household block with duals on the inputs AND on the boundary — `Oracle.value_function`
   backward with a dual `value_next` (the tangent of `ss_end.value`, BackwardIteration.jl:85), `Oracle.transition_step` forward with
   a dual `D_prev` (the tangent of `ss_initial.D`, ForwardIteration.jl:293), the aggregates in numpy;
2. both boundary maps on the random linearisation records of tests/test_vjp_host.py, stated in numpy: `tangent_map_boundary`
   (the recurrences of DESIGN.md section 1 from non-zero dV_P and dD_0, and consumption's aggregate as the device assembles it)
   and `cotangent_map_boundary` (Sweep A and Sweep B of DESIGN.md section 3d, keeping the two states they end with)."""
import numpy as np

from oracle.oracle import SUPPORTED_N, pad_N
from test_vjp_host import _cons


# ---- 1. the oracle loop -------------------------------------------------------------------------------------------------------
def oracle_boundary(orc, x, V, D, y=None, dV=None, dD=None):
    """x (n_hh, P), boundary V (n_a, n_e), D (G,); seeds y (n_hh, P, N), dV, dD (n_a, n_e, N), None = zeros, one at least given.
    -> dict: agg, agg2, cons (P,) — the aggregates of the policy, of the wealth grid and of consumption with the post-transition
    D_t; dagg, dagg2, dcons (P, N) their partials; pol (P, n_a, n_e), dpol (P, n_a, n_e, N)."""
    x = np.asarray(x, dtype=np.float64)
    n_hh, P = x.shape
    n_a, n_e, a, z = orc.n_a, orc.n_e, orc.a, orc.z
    N = next(np.asarray(v).shape[-1] for v in (y, dV, dD) if v is not None)
    out = {k: [] for k in ("dagg", "dagg2", "dcons", "dpol")}
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
        pol = [None] * P
        for t in range(P - 1, -1, -1):
            st, Vn, pol[t] = orc.value_function(Vn, xd[0, t], xd[1, t], Nc, xd[2, t] if n_hh > 2 else None)
            assert st == 0, (t, st)
        agg, agg2, cons = np.zeros(P), np.zeros(P), np.zeros(P)
        dagg, dagg2, dcons = np.zeros((P, n)), np.zeros((P, n)), np.zeros((P, n))
        for t in range(P):
            Dd = orc.transition_step(pol[t], Dd, Nc)
            p0, dp, D0, dDt = pol[t][..., 0], pol[t][..., 1:1 + n], Dd[..., 0], Dd[..., 1:1 + n]
            tr, dtr = (xd[2, t, 0], xd[2, t, 1:1 + n]) if n_hh > 2 else (0.0, np.zeros(n))
            # consumption: the affine map of the policy dual, c = (1 + r) a + w z_e + tr - a' (KrusellSmith.jl:79)
            c0_ = (1.0 + xd[0, t, 0]) * a[:, None] + xd[1, t, 0] * z[None, :] + tr - p0
            dc = xd[0, t, 1:1 + n] * a[:, None, None] + xd[1, t, 1:1 + n] * z[None, :, None] + dtr - dp
            agg[t], agg2[t], cons[t] = np.sum(p0 * D0), np.sum(a[:, None] * D0), np.sum(c0_ * D0)
            dagg[t] = np.einsum("aen,ae->n", dp, D0) + np.einsum("ae,aen->n", p0, dDt)
            dagg2[t] = np.einsum("a,aen->n", a, dDt)
            dcons[t] = np.einsum("aen,ae->n", dc, D0) + np.einsum("ae,aen->n", c0_, dDt)
        out["dagg"].append(dagg); out["dagg2"].append(dagg2); out["dcons"].append(dcons)
        out["dpol"].append(np.stack([p[..., 1:1 + n] for p in pol]))
    res = {k: np.concatenate(v, axis=-1) for k, v in out.items()}
    res.update(agg=agg, agg2=agg2, cons=cons, pol=np.stack([p[..., 0] for p in pol]))
    return res


def smooth_value_seeds(ec, n):
    """n smooth tangents of the terminal value of a raw economy (for finite differences: a rough V + h dV un-sorts the knots)."""
    g = ec["grid"] / ec["grid"].max()
    n_e = ec["V"].shape[1]
    return np.stack([ec["V"] * (0.3 + 0.2 * np.cos((k + 1) * g)[:, None] * (1 + 0.1 * np.arange(n_e))[None, :]) for k in range(n)], axis=-1)


# ---- 2. both maps on a random record ------------------------------------------------------------------------------------------
def tangent_map_boundary(R, dx, dV_P, dD_0):
    """dx (3, P), dV_P, dD_0 (n_a, n_e) -> (dagg (2, P) by definition, dpol (P, n_a, n_e), dC (P,) consumption's aggregate as the
    device assembles it: k_het_outputs' formula from the two reductions of the sweeps plus the seed's productivity marginal)."""
    n_a, n_e, P, a, z, Pi = R["n_a"], R["n_e"], R["P"], R["a"], R["z"], R["Pi"]
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
    dD, m = dD_0, dD_0.sum(axis=0)
    dagg, dC = np.zeros((2, P)), np.zeros(P)
    for t in range(P):
        dr, dw, dtr = dx[:, t]
        r, w, tr = R["x"][:, t]
        lo, wl, g = R["lo"][t], R["w"][t], R["ig"][t] * R["D"][t]
        mid = np.zeros((n_a, n_e))
        cc = np.broadcast_to(cols, lo.shape)
        np.add.at(mid, (lo, cc), (1 - wl) * dD - dpol[t] * g)
        np.add.at(mid, (lo + 1, cc), wl * dD + dpol[t] * g)
        dD = mid @ Pi
        Dt = R["D"][t + 1]
        dagg[0, t] = np.sum(dpol[t] * Dt + R["pol"][t] * dD)
        dagg[1, t] = np.sum((a[:, None] * dr + z[None, :] * dw + dtr - dpol[t]) * Dt + _cons(R, t) * dD)
        m = m @ Pi                                               # the productivity marginal of dD_t, without the lottery
        dAD = np.sum(a[:, None] * dD)
        dC[t] = (dr * np.sum(a[:, None] * Dt) + dw * np.sum(z[None, :] * Dt) + dtr * np.sum(Dt) + (1 + r) * dAD) - dagg[0, t] \
            + (w * np.sum(z * m) + tr * np.sum(m))
    return dagg, dpol, dC


def cotangent_map_boundary(R, yb):
    """yb (2, P) -> (xbar (3, P), pbar (P, n_a, n_e), Vbar_P (n_a, n_e), Dbar_0 (n_a, n_e)): Sweep A, whose last state is the
    cotangent of D_0, then Sweep B, whose last mu is the cotangent of the terminal value."""
    n_a, n_e, P, a, z, Pi = R["n_a"], R["n_e"], R["P"], R["a"], R["z"], R["Pi"]
    cols = np.arange(n_e)[None, :]
    xbar = np.zeros((3, P))
    pbar = np.zeros((P, n_a, n_e))
    lam = np.zeros((n_a, n_e))
    for t in range(P - 1, -1, -1):
        Dt = R["D"][t + 1]
        lam = lam + yb[0, t] * R["pol"][t] + yb[1, t] * _cons(R, t)
        xbar[:, t] += yb[1, t] * np.array([np.sum(a[:, None] * Dt), np.sum(z[None, :] * Dt), np.sum(Dt)])
        U = lam @ Pi.T
        lo, w = R["lo"][t], R["w"][t]
        pbar[t] = (yb[0, t] - yb[1, t]) * Dt + R["ig"][t] * R["D"][t] * (U[lo + 1, cols] - U[lo, cols])
        lam = (1 - w) * U[lo, cols] + w * U[lo + 1, cols]          # after t = 0: the cotangent of D_0, which hank_vjp overwrites
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
        mu = (R["kc"][t] * sbar) @ Pi                            # after t = P-1: mu_P, which hank_vjp drops
    return xbar, pbar, mu, lam
