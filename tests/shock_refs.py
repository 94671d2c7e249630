"""The references of the discount-factor path (hank_set_discount_path, hank_jvp_shock, hank_vjp_shock, hank_fake_news_shock), shared by
tests/test_shock_host.py (CPU) and tests/test_gpu_shock.py.

1. `oracle_shock_sweeps`: the loop of `sweep_refs.oracle_sweeps` with two changes per period, t descending — the oracle's model
   gets beta = beta_t before `Oracle.value_function`, and the function is handed a copy of the incoming dual value whose partials
   are dV + V dbeta_t / beta_t (beta enters KrusellSmith.jl:59-62 as beta E[V']: scaling V' by (1 + eps dbeta/beta) IS the
   beta tangent); the unaugmented output is carried on. The exact dual-number reference of the level and of the beta tangent.
   Nothing under oracle/ changes: the oracle's beta is restored when the loop ends.
2. `shock_case`: the economies — the exact inputs of cases.entry_backward (both families, every gamma of cases.ENTRY_CASES, the grids
   of cases.ENTRY_GRIDS and ENTRY_WIDE) at a horizon T, with a smooth path of the household inputs and a beta path that swings 3 %.
3. `StubShockBlock`: stands in for the device context under `SteadyStateJacobian.shock_jacobian` (the pattern of
   sweep_refs._StubBlock)."""
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
