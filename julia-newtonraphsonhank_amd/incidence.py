"""Income paths by productivity state for the household block (`HouseholdBlock.set_income_path`): who is hit.

A path is an array y (n_e, P), y[e, t] the additive income of productivity state e in period t of the budget
c + a' = (1 + r_t) a + w_t z_e + tr_t + y_t[e]. Targeted transfers, redistribution between states, a path of the productivities
themselves and the unequal incidence of a recession on earnings are all data for that one primitive; the functions here make the
data, the device knows the primitive alone."""
from __future__ import annotations

import numpy as np


def _decay(P, size, rho):
    return float(size) * float(rho) ** np.arange(int(P))


def targeted_transfer(n_e, P, states, size, rho):
    """a transfer of `size` in period 0, decaying at rate rho, paid to the productivity states `states` (indices) alone:
    y[e, t] = size rho^t for e in states, 0 elsewhere. -> y (n_e, P). Not budget-neutral: whoever pays for it is the model's."""
    y = np.zeros((int(n_e), int(P)))
    y[np.asarray(states, dtype=np.intp)] = _decay(P, size, rho)[None, :]
    return y


def redistribution(m, states, size, rho):
    """pure redistribution between states: the states `states` receive size rho^t each, the others pay a common amount such that
    sum_e m[e, t] y[e, t] = 0 in every period under the column masses m (n_e, P) — the productivity marginal of D_t, which does not
    depend on the policies; the stationary distribution of the productivity process tiled over P periods at a steady state — so no
    budget equation of the model changes. -> y (n_e, P)."""
    m = np.asarray(m, dtype=np.float64)
    if m.ndim != 2:
        raise ValueError("m must be (n_e, P): the column masses of every period (tile the stationary ones)")
    n_e, P = m.shape
    rec = np.zeros(n_e, dtype=bool)
    rec[np.asarray(states, dtype=np.intp)] = True
    if rec.all() or not rec.any():
        raise ValueError("states must name some of the productivity states, not all or none")
    give = _decay(P, size, rho)
    paid = m[rec].sum(axis=0) * give                     # what the receivers get in all, per period
    y = np.where(rec[:, None], give[None, :], -(paid / m[~rec].sum(axis=0))[None, :])
    return np.ascontiguousarray(y)


def z_path_to_income(z, z_t, w_t):
    """a path of the productivities z_t (n_e, P) around the context's constants z (n_e,) at the wages w_t (P,), as an income path:
    y[e, t] = w_t (z_t[e] - z_e)."""
    z, z_t, w_t = np.asarray(z, dtype=np.float64), np.asarray(z_t, dtype=np.float64), np.asarray(w_t, dtype=np.float64)
    if z_t.shape != (z.size, w_t.size):
        raise ValueError(f"z_t must be ({z.size}, {w_t.size}), got {z_t.shape}")
    return w_t[None, :] * (z_t - z[:, None])


def z_path_to_income_tangent(z, z_t, w_t, dz_t, dw_t):
    """the tangent of `z_path_to_income`: dy[e, t, n] = (z_t[e] - z_e) dw_t[n] + w_t dz_t[e, n]; dz_t (n_e, P, N) or None (zeros),
    dw_t (P, N) or None (zeros). The tangent map of the block is linear in dy, so the host forms it. -> dy (n_e, P, N)."""
    z, z_t, w_t = np.asarray(z, dtype=np.float64), np.asarray(z_t, dtype=np.float64), np.asarray(w_t, dtype=np.float64)
    if dz_t is None and dw_t is None:
        raise ValueError("at least one of dz_t, dw_t must be given")
    N = np.asarray(dz_t).shape[2] if dz_t is not None else np.asarray(dw_t).shape[1]
    dy = np.zeros(z_t.shape + (N,))
    if dw_t is not None:
        dy += (z_t - z[:, None])[:, :, None] * np.asarray(dw_t, dtype=np.float64)[None, :, :]
    if dz_t is not None:
        dy += w_t[None, :, None] * np.asarray(dz_t, dtype=np.float64)
    return dy


def incidence(z, pi_stat, Y_t, zeta):
    """unequal incidence of aggregate income on earnings: z_t[e] proportional to z_e^(1 + zeta log Y_t), normalised so that
    sum_e pi_stat[e] z_t[e] = sum_e pi_stat[e] z_e in every period (mean one when z has mean one). Y_t (P,) relative to its steady
    state (1 = none); zeta > 0 spreads earnings in a boom, zeta < 0 in a recession. -> z_t (n_e, P), for `z_path_to_income`."""
    z, pi_stat, Y_t = np.asarray(z, dtype=np.float64), np.asarray(pi_stat, dtype=np.float64), np.asarray(Y_t, dtype=np.float64)
    if np.any(z <= 0) or np.any(Y_t <= 0):
        raise ValueError("z and Y_t must be positive")
    raw = z[:, None] ** (1.0 + float(zeta) * np.log(Y_t))[None, :]
    return raw * (np.dot(pi_stat, z) / (pi_stat @ raw))[None, :]
