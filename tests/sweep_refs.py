"""The references the tangent and cotangent tests share, each stated once (the host modules tests/test_vjp_host.py,
test_vjp_het_host.py, test_boundary_host.py, test_jvp_het_host.py pin them; tests/test_gpu_boundary.py and test_gpu_jvp_het.py
compare the device with them).

1. `tangent_map` / `cotangent_map`: the tangent recurrences of DESIGN.md section 1 and their transpose (Sweep A and Sweep B of
   section 3d) in numpy on a random linearisation record — with extra outputs that are not affine in the policy (X, section 3a:
   dY^o_t = sum f_o,t dD_t - sum f_c,o,t D_t da'_t + dr_t (Sa + Sr) + dw_t Sz + dtr_t S1) and with seeds / cotangents on the
   boundary (dV_P, dD_0) as options;
2. `oracle_sweeps`: tests/path_refs.oracle_path_sweeps — the one loop, which the household-side paths share — at the row without a
   path: the CPU oracle's household block with duals on the inputs AND on the boundary — `Oracle.value_function`
   backward with a dual `value_next` (the tangent of `ss_end.value`, BackwardIteration.jl:85), `Oracle.transition_step` forward with
   a dual `D_prev` (the tangent of `ss_initial.D`, ForwardIteration.jl:293), the aggregates in numpy. Value is the dual V_t that
   `Oracle.value_function` returns in that loop — the reference's own Value key (KrusellSmith.jl:80); UCE is z_e c^-gamma by the
   chain rule on the consumption dual, as in `Oracle.het_outputs`; every output is dotted with the dual post-transition D_t
   (ForwardIteration.jl:303-307);
3. the stand-in blocks of the host-layer tests, which multiply by the oracle's Jacobians, and their fixtures."""
from types import SimpleNamespace

import numpy as np
import pytest

import cases as vc
import path_refs
from conftest import ROOT, ks_paths, ks_setup

NXT = 2         # extra outputs of the numpy maps


# ---- 1. both maps on a random record ------------------------------------------------------------------------------------------
def _random_record(rng, n_a=14, n_e=3, P=7, clamp=4, flat=3):
    """a linearisation record with the structure the device's has: brackets non-decreasing in wealth, a constrained prefix
    with A = B = 0, a lottery with a clamped prefix (lo = 0, w = 0, ig = 0) and a few sources clamped at the top (w = 1, ig = 0)."""
    R = {"n_a": n_a, "n_e": n_e, "P": P, "a": np.sort(rng.uniform(0, 10, n_a)), "z": rng.uniform(0.5, 2, n_e)}
    Pi = rng.uniform(0.1, 1, (n_e, n_e))
    R["Pi"] = Pi / Pi.sum(1, keepdims=True)
    sh = (P, n_a, n_e)
    for k in ("s", "kc", "A", "B", "u", "v", "pol", "ig"):
        R[k] = rng.standard_normal(sh)
    R["ib"] = np.sort(rng.integers(0, n_a - 1, sh), axis=1)
    R["A"][:, :flat] = 0.0; R["B"][:, :flat] = 0.0
    R["lo"] = rng.integers(0, n_a - 1, sh)
    R["w"] = rng.uniform(0, 1, sh)
    R["lo"][:, :clamp] = 0; R["w"][:, :clamp] = 0.0; R["ig"][:, :clamp] = 0.0
    R["lo"][:, -2:] = n_a - 2; R["w"][:, -2:] = 1.0; R["ig"][:, -2:] = 0.0
    R["D"] = rng.uniform(0, 1, (P + 1, n_a, n_e))               # D_0 .. D_P: period t's post-transition D_t is D[t + 1]
    R["x"] = np.stack([rng.uniform(0.01, 0.05, P), rng.uniform(0.8, 1.2, P), rng.uniform(0, 0.1, P)])
    return R


def _cons(R, t):
    r, w, tr = R["x"][:, t]
    return (1 + r) * R["a"][:, None] + w * R["z"][None, :] + tr - R["pol"][t]


def _extra(rng, R):
    """random f, f_c (NXT, P, n_a, n_e) and S = (Sa, Sz, S1, Sr) (NXT, P, 4) for the extra outputs of record R"""
    sh = (NXT, R["P"], R["n_a"], R["n_e"])
    return {"f": rng.standard_normal(sh), "fc": rng.standard_normal(sh), "S": rng.standard_normal((NXT, R["P"], 4))}


def tangent_map(R, dx, X=None, dV_P=None, dD_0=None):
    """dx (3, P), extra outputs X (None: none), seeds dV_P, dD_0 (n_a, n_e) (None: zeros) -> (dagg (2 + NX, P) by definition,
    dpol (P, n_a, n_e), dC (P,) consumption's aggregate as the device assembles it: k_het_outputs' formula from the two reductions
    of the sweeps plus the seed's productivity marginal). The backward tangent loop (k_tan_X / k_tan_Y), then the forward
    tangent step; the extra outputs read the dD_t the recurrence carries."""
    n_a, n_e, P, a, z, Pi = R["n_a"], R["n_e"], R["P"], R["a"], R["z"], R["Pi"]
    NX = 0 if X is None else X["f"].shape[0]
    cols = np.arange(n_e)[None, :]
    dpol = np.zeros((P, n_a, n_e))
    dV = np.zeros((n_a, n_e)) if dV_P is None else dV_P
    for t in range(P - 1, -1, -1):
        dr, dw, dtr = dx[:, t]
        rho = 1.0 / (1.0 + R["x"][0, t])
        ds = R["kc"][t] * (dV @ Pi.T) - rho * (z[None, :] * dw + dtr + R["s"][t] * dr)
        dg = R["A"][t] * ds[R["ib"][t], cols] + R["B"][t] * ds[R["ib"][t] + 1, cols]
        dpol[t] = dg
        dV = R["u"][t] * dr + R["v"][t] * ((a[:, None] * dr + z[None, :] * dw + dtr) - dg)
    dD = np.zeros((n_a, n_e)) if dD_0 is None else dD_0
    m = dD.sum(axis=0)
    dagg, dC = np.zeros((2 + NX, P)), np.zeros(P)
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
        for o in range(NX):
            Sa, Sz, S1, Sr = X["S"][o, t]
            dagg[2 + o, t] = np.sum(X["f"][o, t] * dD) - np.sum(X["fc"][o, t] * Dt * dpol[t]) + dr * (Sa + Sr) + dw * Sz + dtr * S1
        m = m @ Pi                                               # the productivity marginal of dD_t, without the lottery
        dAD = np.sum(a[:, None] * dD)
        dC[t] = (dr * np.sum(a[:, None] * Dt) + dw * np.sum(z[None, :] * Dt) + dtr * np.sum(Dt) + (1 + r) * dAD) - dagg[0, t] \
            + (w * np.sum(z * m) + tr * np.sum(m))
    return dagg, dpol, dC


def cotangent_map(R, yb, X=None):
    """yb (2 + NX, P) -> (xbar (3, P), pbar (P, n_a, n_e), Vbar_P (n_a, n_e), Dbar_0 (n_a, n_e)): Sweep A with the extra outputs'
    two terms, whose last state is the cotangent of D_0 (which hank_vjp overwrites); the unchanged Sweep B, whose last mu is the
    cotangent of the terminal value (which hank_vjp drops); and the direct terms on the inputs."""
    n_a, n_e, P, a, z, Pi = R["n_a"], R["n_e"], R["P"], R["a"], R["z"], R["Pi"]
    NX = 0 if X is None else X["f"].shape[0]
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
        U = lam @ Pi.T                                           # U[r, e] = sum_e2 Pi[e, e2] lam[r, e2]
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
        mu = (R["kc"][t] * sbar) @ Pi                            # mu[i, e2] = sum_e Pi[e, e2] kc[i, e] sbar[i, e]
    return xbar, pbar, mu, lam


# ---- 2. the oracle loop -------------------------------------------------------------------------------------------------------
def oracle_sweeps(orc, x, V, D, gamma=None, n_het=2, y=None, dV=None, dD=None):
    """x (n_hh, P), boundary V (n_a, n_e), D (G,); seeds y (n_hh, P, N), dV, dD (n_a, n_e, N), None = zeros, one at least given;
    gamma is needed for n_het = 4 only.
    -> dict: agg (P, n_het) and dagg (P, n_het, N) of (savings, consumption, Value[, UCE]) with the post-transition D_t — the shapes
    of hank_get_het_outputs; cons (P,), dcons (P, N) their consumption columns; agg2 (P,), dagg2 (P, N) the wealth grid's
    aggregate; pol (P, n_a, n_e), dpol (P, n_a, n_e, N)."""
    res = path_refs.oracle_path_sweeps(path_refs.PLAIN, orc, x, V, D, None, gamma, n_het, dx=y, dV=dV, dD=dD)
    if n_het > 1:
        res.update(cons=res["agg"][:, 1], dcons=res["dagg"][:, 1])
    return res


def smooth_value_seeds(ec, n):
    """n smooth tangents of the terminal value of a raw economy (for finite differences: a rough V + h dV un-sorts the knots)."""
    g = ec["grid"] / ec["grid"].max()
    n_e = ec["V"].shape[1]
    return np.stack([ec["V"] * (0.3 + 0.2 * np.cos((k + 1) * g)[:, None] * (1 + 0.1 * np.arange(n_e))[None, :]) for k in range(n)], axis=-1)


# ---- 3. the host layers' stand-in blocks --------------------------------------------------------------------------------------
class _StubBlock:
    """stands in for the device context: jvp / vjp multiply by the oracle's J."""
    device = None

    def __init__(self, J, agg, n_hh, P):
        self.J, self.agg, self.n_hh, self.P = J, agg, n_hh, P
        self.calls = {"primal": 0, "jvp": 0, "vjp": 0}

    def clone(self, device=None):
        other = _StubBlock(self.J, self.agg, self.n_hh, self.P)
        other.device = device
        return other

    def close(self):
        pass

    def set_boundary(self, v, D):
        pass

    def primal(self, xhh):
        self.calls["primal"] += 1
        return self.agg.copy()

    def jvp(self, dxhh):
        self.calls["jvp"] += 1
        N = dxhh.shape[2]
        return self.J @ np.asarray(dxhh).reshape(self.n_hh * self.P, N, order="F")

    def vjp(self, agg_bar, n_het=1):
        self.calls["vjp"] += 1
        assert n_het == 1 and agg_bar.shape[:2] == (self.P, 1)
        M = agg_bar.shape[2]
        return (self.J.T @ agg_bar[:, 0, :]).reshape(self.n_hh, self.P, M, order="F")


@pytest.fixture(scope="module")
def stub_setup(hank, oracle_mod):
    m, ss, orc = ks_setup(30, 3, 25)
    x, Z = ks_paths(m, ss, "x1", 0.05)
    # J (P, n_hh P) of the policy variable's aggregate from unit tangents through the CPU oracle: column k + n_hh s = input k at
    # period s (the layout of dxhh)
    agg, J, _, _ = orc.block(x[2:4], vc.unit_tangents(2, m.compspec.T - 1), ss.value, ss.D)
    old = m._hip_block
    stub = _StubBlock(J, agg, 2, m.compspec.T - 1)
    m._hip_block = stub
    try:
        yield hank, m, ss, x, Z, stub
    finally:
        m._hip_block = old


class _StubBlock3:
    """stands in for the device context: three outputs (KD, C, Value); jvp / het_outputs / vjp / vjp_het multiply by the oracle's J
    (3, P, n_hh, P)."""
    device = None

    def __init__(self, J, agg, n_hh, P):
        self.J, self.agg, self.n_hh, self.P = J, agg, n_hh, P
        self.Jm = J.reshape(3 * P, n_hh * P)                     # rows (output, t); columns (input k, period s), k slowest
        self.calls = {"primal": 0, "jvp": 0, "vjp": 0, "vjp_het": 0}
        self.declared = 2

    def clone(self, device=None):
        other = _StubBlock3(self.J, self.agg, self.n_hh, self.P)
        other.device = device
        return other

    def close(self):
        pass

    def set_boundary(self, v, D):
        pass

    def set_het_outputs(self, n):
        self.declared = n

    def primal(self, xhh):
        self.calls["primal"] += 1
        return self.agg[:, 0].copy()

    def _dagg(self, dxhh):
        N = dxhh.shape[2]
        return (self.Jm @ np.asarray(dxhh).reshape(self.n_hh * self.P, N)).reshape(3, self.P, N)

    def jvp(self, dxhh):
        self.calls["jvp"] += 1
        return self._dagg(dxhh)[0]

    def het_outputs(self, n_het, dxhh=None):
        assert n_het <= self.declared
        return self.agg[:, :n_het].copy(), None if dxhh is None else np.ascontiguousarray(self._dagg(dxhh)[:n_het].transpose(1, 0, 2))

    def vjp(self, agg_bar, n_het=1):
        raise AssertionError("a model that reaches Value took hank_vjp")

    def vjp_het(self, agg_bar, n_het):
        self.calls["vjp_het"] += 1
        assert n_het == 3 and n_het <= self.declared and agg_bar.shape[:2] == (self.P, 3)
        M = agg_bar.shape[2]
        return (self.Jm.T @ np.asarray(agg_bar).transpose(1, 0, 2).reshape(3 * self.P, M)).reshape(self.n_hh, self.P, M)


@pytest.fixture(scope="module")
def stub3_setup(hank, oracle_mod, tmp_path_factory):
    """Krusell-Smith 30x3, T = 25 with heterogeneous: [KD, Value] and a market-clearing equation that reads both (a toy model:
    what matters is that the residual layer puts weight on output 2)."""
    m0, ss0, orc = ks_setup(30, 3, 25)
    x, Z = ks_paths(m0, ss0, "x1", 0.05)
    src = (ROOT / "examples" / "krusell_smith.yaml").read_text()
    line = '    - {name: "KD", description: "capital demand (aggregate household savings)"}\n'
    assert line in src and '"KS = KD"' in src
    src = src.replace(line, line + '    - {name: "Value", description: "aggregate value"}\n').replace('"KS = KD"', '"KS = KD + 0.05 * (Value - 1.0)"')
    spec = tmp_path_factory.mktemp("vjp_het") / "ks_value.yaml"
    spec.write_text(src)
    m = hank.build_model_from_yaml(str(spec), overrides={"T": 25, "dimensions": {"wealth": {"n": 30}, "productivity": {"n": 3}}})
    assert hank.vars_of_type(m, "heterogeneous") == ("KD", "Value")
    P = m.compspec.T - 1
    J = vc.oracle_jacobian_het(orc, ss0.value, ss0.D, x[2:4], 3, m.params.γ)
    agg = orc.het_outputs(x[2:4], None, ss0.value, ss0.D, 3, m.params.γ)[0].T                 # (P, 3)
    ss = SimpleNamespace(value=ss0.value, D=ss0.D, vars={**{k: 1.0 for k in m.variables}, **dict(ss0.vars)})
    stub = _StubBlock3(J, np.ascontiguousarray(agg), 2, P)
    m._hip_block = stub
    return hank, m, ss, x, Z, stub


class _StubHet(_StubBlock3):
    """_StubBlock3 with the boundary products: Jb (3, P, 2 G) the oracle loop's Jacobian in (V_P, D_0), seeds (dV, dD) stacked"""

    def __init__(self, J, agg, n_hh, P, Jb, n_a, n_e):
        super().__init__(J, agg, n_hh, P)
        self.Jb, self.n_a, self.n_e, self.G = Jb, n_a, n_e, n_a * n_e
        self.Jbm = Jb.reshape(3 * P, 2 * self.G)
        self.calls.update(jvp_het=0, vjp_het_boundary=0)

    def clone(self, device=None):
        other = _StubHet(self.J, self.agg, self.n_hh, self.P, self.Jb, self.n_a, self.n_e)
        other.device = device
        return other

    def jvp_het(self, dxhh=None, dvalue_end=None, dD_init=None, n_het=2):
        self.calls["jvp_het"] += 1
        assert n_het <= self.declared
        N = next(np.asarray(v).shape[2] if np.asarray(v).ndim == 3 else 1 for v in (dxhh, dvalue_end, dD_init) if v is not None)
        out = np.zeros((3, self.P, N))
        if dxhh is not None:
            out += self._dagg(np.asarray(dxhh).reshape(self.n_hh, self.P, N))
        b = np.zeros((2 * self.G, N))
        for k, s in enumerate((dvalue_end, dD_init)):
            if s is not None:
                b[k * self.G:(k + 1) * self.G] = np.asarray(s).reshape((self.G, N), order="F")
        out += (self.Jbm @ b).reshape(3, self.P, N)
        return np.ascontiguousarray(out[:n_het].transpose(1, 0, 2))

    def vjp_het_boundary(self, agg_bar, n_het, value_end=True, D_init=True):
        self.calls["vjp_het_boundary"] += 1
        assert n_het == 3 and n_het <= self.declared
        M = agg_bar.shape[2]
        yb = np.asarray(agg_bar).transpose(1, 0, 2).reshape(3 * self.P, M)
        b = self.Jbm.T @ yb
        sh = (self.n_a, self.n_e, M)
        return (self.Jm.T @ yb).reshape(self.n_hh, self.P, M), b[:self.G].reshape(sh, order="F"), b[self.G:].reshape(sh, order="F")


@pytest.fixture(scope="module")
def stub_het_setup(stub3_setup, oracle_mod):
    hank, m, ss, x, Z, stub = stub3_setup
    _, ss0, orc = ks_setup(30, 3, 25)
    n_a, n_e = np.asarray(ss0.value).shape
    G = n_a * n_e
    U = np.eye(G).reshape((n_a, n_e, G), order="F")
    Zs = np.zeros_like(U)
    ref = oracle_sweeps(orc, x[2:4], np.asarray(ss0.value), np.asarray(ss0.D), m.params.γ, 3, dV=np.concatenate([U, Zs], axis=2),
                        dD=np.concatenate([Zs, U], axis=2))
    mine = _StubHet(stub.J, stub.agg, 2, stub.P, np.ascontiguousarray(ref["dagg"].transpose(1, 0, 2)), n_a, n_e)
    mine.declared = 3
    m._hip_block = mine
    yield hank, m, ss, x, Z, mine
    m._hip_block = stub
