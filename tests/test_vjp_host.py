"""The transposed household block without a GPU: (1) the recurrences hank_vjp implements (csrc/hank_adjoint.h, DESIGN.md
section 3d) are the exact transpose of the tangent recurrences of DESIGN.md section 1 — both maps stated in numpy here and
compared on random linearisation records (two outputs, three inputs, a clamped prefix); (2) the host layers above the device
(`LinearizedFunction.vjp`, `as_linear_operator`, `VJP`, `DeviceGroup.vjp`) with a stand-in block that multiplies by the CPU
oracle's Jacobian of the household block at 30x3, T = 25; (3) the raw-grid economies of tests/cases.py hold, on the oracle's policy, the
data-dependent edges tests/test_gpu_vjp_variants.py runs hank_vjp through: proven present without a GPU."""
import numpy as np
import pytest

import cases as vc
from conftest import ks_paths, ks_setup


# ---- (1) both maps in numpy ---------------------------------------------------------------------------------------------------
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


def tangent_map(R, dx):
    """dx (3, P) -> (dagg (2, P), dpol (P, n_a, n_e)): the backward tangent loop (k_tan_X / k_tan_Y), then the forward tangent step of DESIGN.md section 1."""
    n_a, n_e, P, a, z, Pi = R["n_a"], R["n_e"], R["P"], R["a"], R["z"], R["Pi"]
    cols = np.arange(n_e)[None, :]
    dpol = np.zeros((P, n_a, n_e))
    dV = np.zeros((n_a, n_e))
    for t in range(P - 1, -1, -1):
        dr, dw, dtr = dx[:, t]
        rho = 1.0 / (1.0 + R["x"][0, t])
        ds = R["kc"][t] * (dV @ Pi.T) - rho * (z[None, :] * dw + dtr + R["s"][t] * dr)
        dg = R["A"][t] * ds[R["ib"][t], cols] + R["B"][t] * ds[R["ib"][t] + 1, cols]
        dpol[t] = dg
        dV = R["u"][t] * dr + R["v"][t] * ((a[:, None] * dr + z[None, :] * dw + dtr) - dg)
    dD = np.zeros((n_a, n_e))
    dagg = np.zeros((2, P))
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
    return dagg, dpol


def cotangent_map(R, yb):
    """yb (2, P) -> (xbar (3, P), pbar (P, n_a, n_e)): Sweep A, then Sweep B."""
    n_a, n_e, P, a, z, Pi = R["n_a"], R["n_e"], R["P"], R["a"], R["z"], R["Pi"]
    cols = np.arange(n_e)[None, :]
    xbar = np.zeros((3, P))
    pbar = np.zeros((P, n_a, n_e))
    lam = np.zeros((n_a, n_e))
    for t in range(P - 1, -1, -1):
        Dt = R["D"][t + 1]
        lam = lam + yb[0, t] * R["pol"][t] + yb[1, t] * _cons(R, t)
        xbar[:, t] += yb[1, t] * np.array([np.sum(a[:, None] * Dt), np.sum(z[None, :] * Dt), np.sum(Dt)])
        U = lam @ Pi.T                                           # U[r, e] = sum_e2 Pi[e, e2] lam[r, e2]
        lo, w = R["lo"][t], R["w"][t]
        pbar[t] = (yb[0, t] - yb[1, t]) * Dt + R["ig"][t] * R["D"][t] * (U[lo + 1, cols] - U[lo, cols])
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
    return xbar, pbar


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_reverse_recurrences_are_the_transpose_of_the_tangent_recurrences(seed):
    rng = np.random.default_rng(seed)
    R = _random_record(rng)
    P = R["P"]
    J = np.zeros((2 * P, 3 * P))                                 # rows (output, t), columns (input, s)
    for k in range(3):
        for s in range(P):
            dx = np.zeros((3, P)); dx[k, s] = 1.0
            J[:, k * P + s] = tangent_map(R, dx)[0].reshape(-1)
    assert np.abs(J).max() > 1e-3
    for _ in range(4):
        yb = rng.standard_normal((2, P))
        xbar, _ = cotangent_map(R, yb)
        want = J.T @ yb.reshape(-1)
        assert np.max(np.abs(xbar.reshape(-1) - want)) <= 1e-13 * max(1.0, np.abs(want).max())
    # the policy variable alone: consumption's cotangent off
    yb = np.stack([rng.standard_normal(P), np.zeros(P)])
    assert np.allclose(cotangent_map(R, yb)[0].reshape(-1), J[:P].T @ yb[0], rtol=0, atol=1e-13 * np.abs(J).max() * P)


def test_policy_cotangent_pairs_with_the_policy_partials():
    """the policy variable's aggregate depends on the inputs through the policy partials alone, so <pbar, dpol> = <ybar, dagg>
    (what tests/test_gpu_vjp.py checks on the device with policy_cotangent_seq and dpolicy_seq)."""
    rng = np.random.default_rng(7)
    R = _random_record(rng)
    P = R["P"]
    dagg, dpol = tangent_map(R, rng.standard_normal((3, P)))
    yb = np.stack([rng.standard_normal(P), np.zeros(P)])
    _, pbar = cotangent_map(R, yb)
    assert abs(np.sum(pbar * dpol) - np.sum(yb[0] * dagg[0])) <= 1e-13 * np.sum(np.abs(pbar * dpol))


# ---- (2) the host layers with a stand-in block ------------------------------------------------------------------------------
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


def test_linearized_function_vjp_is_the_transpose_of_jvp(stub_setup):
    hank, m, ss, x, Z, stub = stub_setup
    lin = hank.LinearizedFunction(x.reshape(-1, order="F"), {"Z": Z}, m, ss, ss)
    n = lin.x.size
    rng = np.random.default_rng(1)
    y, yb = rng.standard_normal((n, 3)), rng.standard_normal((n, 5))
    Jy, JTyb = lin.jvp(y), lin.vjp(yb)
    assert JTyb.shape == (n, 5) and stub.calls["vjp"] == 1
    lhs, rhs = yb.T @ Jy, JTyb.T @ y
    assert np.max(np.abs(lhs - rhs)) <= 1e-11 * np.abs(lhs).max()
    # a single cotangent; the dense matrices; the LinearOperator's four products; VJP next to JVP
    assert np.allclose(lin.vjp(yb[:, 0]), JTyb[:, 0], rtol=0, atol=1e-13 * np.abs(JTyb).max())
    Jd, JTd = lin.jvp(np.eye(n)), lin.vjp(np.eye(n))
    assert np.max(np.abs(JTd - Jd.T)) <= 1e-12 + 1e-10 * np.abs(Jd).max()
    op = lin.as_linear_operator()
    assert op.shape == (n, n)
    assert np.array_equal(op.matmat(y), Jy) and np.array_equal(op.rmatmat(yb), JTyb)
    assert np.array_equal(op.matvec(y[:, 0]), lin.jvp(y[:, 0])) and np.array_equal(op.rmatvec(yb[:, 0]), lin.vjp(yb[:, 0]))
    assert np.array_equal(hank.VJP(lin, lin.x, yb), JTyb)
    with pytest.raises(ValueError):
        hank.VJP(lin, lin.x + 1.0, yb)
    # a cotangent that puts no weight on the aggregate does not reach the device
    before = stub.calls["vjp"]
    lin.vjp(np.zeros(n))
    assert stub.calls["vjp"] == before


def test_vjp_restores_its_record_like_jvp(stub_setup):
    hank, m, ss, x, Z, stub = stub_setup
    lin = hank.LinearizedFunction(x.reshape(-1, order="F"), {"Z": Z}, m, ss, ss)
    other = hank.LinearizedFunction(x.reshape(-1, order="F") * 1.0001, {"Z": Z}, m, ss, ss)       # takes the context's record
    assert other._generation != lin._generation
    before = stub.calls["primal"]
    lin.vjp(np.ones(lin.x.size))
    assert stub.calls["primal"] == before + 1 and lin._generation == stub._generation


def test_outputs_that_are_not_affine_in_the_policy_are_refused(stub_setup):
    hank, m, ss, x, Z, stub = stub_setup
    lin = hank.LinearizedFunction(x.reshape(-1, order="F"), {"Z": Z}, m, ss, ss)
    lin._n_out = 3
    with pytest.raises(NotImplementedError, match="not affine"):
        lin.vjp(np.ones(lin.x.size))


def test_device_group_shards_cotangent_columns_like_tangent_columns(stub_setup):
    from hank_amd.parallel import DeviceGroup
    hank, m, ss, x, Z, stub = stub_setup
    grp = DeviceGroup(stub, [None, 1, 2])
    try:
        yb = np.random.default_rng(2).standard_normal((stub.P, 1, 7))
        got = grp.vjp(yb, 1)
        assert got.shape == (2, stub.P, 7) and np.array_equal(got, stub.vjp(yb, 1))
        assert [b.calls["vjp"] for b in grp.blocks[1:]] == [1, 1]
        assert grp.vjp(yb[:, :, :2], 1).shape == (2, stub.P, 2)                  # fewer columns than devices
    finally:
        grp.close()


# ---- (3) the edge economies' preconditions ----------------------------------------------------------------------------------
def test_edge_economies_hold_their_edges_on_the_oracles_policy(oracle_mod):
    """each economy of cases.EDGE_GRIDS, on the CPU oracle's policy: a clamped prefix of 8 rows or more that is no multiple of
    the row-block count nb = ceil(n_a / R) at any tested width (and, over the economies, on both sides of nb); 8 or more sources
    clamped at the top; runs of rows in one bracket of length >= 5, odd and even. Prints what it measured (run with -s)."""
    sides = {"clo_lt_nb": False, "clo_gt_nb": False}
    for name in vc.EDGE_GRIDS:
        ec = vc.raw_economy(name)
        assert np.all(np.diff(ec["grid"]) > 0)
        got = vc.check_edges(name, ec["grid"], ec["orc"].block(ec["x"], None, ec["V"], ec["D"])[2])
        sides = {k: sides[k] or got[k] for k in sides}
    assert sides == {"clo_lt_nb": True, "clo_gt_nb": True}, sides
    assert [vc.adj_rows_per_block(M) for M in (1, 2, 3, 4, 5, 6, 8, 9, 16, 18, 32, 33)] == [64, 64, 16, 32, 8, 16, 16, 8, 8, 8, 8, 8]


def test_forward_edge_economies_hold_their_edges_on_the_oracles_policy(oracle_mod):
    """each economy of cases.FWD_EDGE_ECONOMIES, on the CPU oracle's policy, holds what tests/test_gpu_fwd_edges.py runs the forward
    families through: `deep-prefix` a clamped prefix over three members or more and past row 128, a target row with more than 64
    sources; `swing` a period with every column clamped, a clamp-free period after a clamped one, a clamp-free period after a
    clamp-free one, a returning clamp, more than 64 sources on one target; `collapse` a whole column clamped. On all six economies
    of the forward module every member-period needs at most XUCAP = 64 work units (a condition on the inputs: beyond it the
    persistent sweeps hand the context to the launches). Prints what it measured (run with -s)."""
    fe = {}
    for name in vc.FWD_ECONOMIES:
        ec = vc.raw_economy(name)
        assert np.all(np.diff(ec["grid"]) > 0)
        pol = ec["orc"].block(ec["x"], None, ec["V"], ec["D"])[2]               # (status 0, or `block` raises)
        assert np.all(np.isfinite(pol)) and np.all(np.diff(pol, axis=1) >= 0), name
        f = fe[name] = vc.forward_edges(ec["grid"], pol)
        assert np.array_equal(f["clo"], vc.edge_stats(ec["grid"], pol)[0])
        print(f"{name} ({ec['grid'].size} rows): clo per column {f['clo'].T.tolist()}, members {f['members'].max(axis=1).tolist()}, "
              f"most sources on one target per period {f['sources'].max(axis=1).tolist()}, all clamped {f['all_clamped'].astype(int).tolist()}, "
              f"reopened {f['reopened'].astype(int).tolist()}, quiet {f['quiet'].astype(int).tolist()}, units per member-period at most "
              f"{f['units'].max()} ({f['column_units']} in one column), longest unit {f['longest']} lanes")
        assert f["units"].max() <= vc.XUCAP and f["column_units"] < vc.XUCAP, (name, f["units"])
    f = fe["deep-prefix"]
    assert f["members"].max() >= 3 and f["past128"].any() and f["sources"].max() > 64
    f = fe["swing"]
    anyclo = (f["clo"] > 0).any(axis=1)
    assert f["all_clamped"].any() and f["reopened"].any() and f["quiet"].any() and f["sources"].max() > 64
    t_open = int(np.flatnonzero(f["reopened"])[0])
    assert anyclo[t_open:].any(), "the clamp does not return"
    f = fe["collapse"]
    assert np.any(f["clo"] == vc.raw_economy("collapse")["grid"].size)
    # the economies of the transposed sweeps never leave member 0 or wave 0, and never change which columns are clamped
    for name in vc.EDGE_GRIDS:
        assert fe[name]["members"].max() == 1 and not fe[name]["past128"].any() and not fe[name]["all_clamped"].any(), name
        assert not fe[name]["reopened"].any() and not fe[name]["quiet"].any(), name
