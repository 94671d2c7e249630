"""hank_vjp_het without a GPU: (1) the transposed map with cotangents on outputs that are not affine in the policy
(csrc/hank_adjoint.h): Y^o_t = sum f_o,t D_t adds a weight f_o,t on the distribution, a direct term
-f_c,o,t D_t on the policy and (Sa + Sr, Sz, S1)_o,t on the inputs. Both maps are stated in numpy on the random records of
tests/test_vjp_host.py, with random f, f_c, S for two extra outputs, and compared; (2) the host layers above the device
(`LinearizedFunction.vjp_het`, `as_linear_operator`, `VJP`, `DeviceGroup.vjp_het`) with a stand-in block that multiplies by the CPU
oracle's three-output Jacobian of the household block at 30x3, T = 25."""
from types import SimpleNamespace

import numpy as np
import pytest

import cases as vc
from conftest import ROOT, ks_paths, ks_setup
from test_vjp_host import _cons, _random_record

NXT = 2         # extra outputs of the numpy maps


# ---- (1) both maps in numpy ---------------------------------------------------------------------------------------------------
def _extra(rng, R):
    """random f, f_c (NXT, P, n_a, n_e) and S = (Sa, Sz, S1, Sr) (NXT, P, 4) for the extra outputs of record R"""
    sh = (NXT, R["P"], R["n_a"], R["n_e"])
    return {"f": rng.standard_normal(sh), "fc": rng.standard_normal(sh), "S": rng.standard_normal((NXT, R["P"], 4))}


def tangent_map_het(R, X, dx):
    """dx (3, P) -> dagg (2 + NXT, P): the tangent recurrences of DESIGN.md section 1 with the outputs of section 3a,
    dY^o_t = sum f_o,t dD_t - sum f_c,o,t D_t da'_t + dr_t (Sa + Sr) + dw_t Sz + dtr_t S1 for o >= 2."""
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
    dagg = np.zeros((2 + NXT, P))
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
        for o in range(NXT):
            Sa, Sz, S1, Sr = X["S"][o, t]
            dagg[2 + o, t] = np.sum(X["f"][o, t] * dD) - np.sum(X["fc"][o, t] * Dt * dpol[t]) + dr * (Sa + Sr) + dw * Sz + dtr * S1
    return dagg


def cotangent_map_het(R, X, yb):
    """yb (2 + NXT, P) -> (xbar (3, P), pbar (P, n_a, n_e)): Sweep A with the extra outputs' two terms, the unchanged Sweep B,
    and the direct terms on the inputs."""
    n_a, n_e, P, a, z, Pi = R["n_a"], R["n_e"], R["P"], R["a"], R["z"], R["Pi"]
    cols = np.arange(n_e)[None, :]
    xbar = np.zeros((3, P))
    pbar = np.zeros((P, n_a, n_e))
    lam = np.zeros((n_a, n_e))
    for t in range(P - 1, -1, -1):
        Dt = R["D"][t + 1]
        lam = lam + yb[0, t] * R["pol"][t] + yb[1, t] * _cons(R, t)
        xbar[:, t] += yb[1, t] * np.array([np.sum(a[:, None] * Dt), np.sum(z[None, :] * Dt), np.sum(Dt)])
        direct = yb[0, t] - yb[1, t]
        for o in range(NXT):
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
    return xbar, pbar


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_reverse_recurrences_with_extra_outputs_are_the_transpose_of_the_tangent_recurrences(seed):
    from test_vjp_host import cotangent_map
    rng = np.random.default_rng(seed)
    R = _random_record(rng)
    X = _extra(rng, R)
    P, NO = R["P"], 2 + NXT
    J = np.zeros((NO * P, 3 * P))                                # rows (output, t), columns (input, s)
    for k in range(3):
        for s in range(P):
            dx = np.zeros((3, P)); dx[k, s] = 1.0
            J[:, k * P + s] = tangent_map_het(R, X, dx).reshape(-1)
    assert np.abs(J[2 * P:]).max() > 1e-3
    scale = max(1.0, np.abs(J).max())
    for only in (None, 2, 3):                                    # every output; then one extra output alone (a swapped index shows)
        yb = rng.standard_normal((NO, P))
        if only is not None:
            yb[np.arange(NO) != only] = 0.0
        xbar, _ = cotangent_map_het(R, X, yb)
        want = J.T @ yb.reshape(-1)
        err = np.max(np.abs(xbar.reshape(-1) - want))
        print(f"seed {seed}, cotangents on {only}: max err {err:.3e} at scale {np.abs(want).max():.3e}")
        assert err <= 1e-13 * max(scale, np.abs(want).max())
    # nothing on the extra outputs: the two-output map of tests/test_vjp_host.py, bit for bit
    yb = rng.standard_normal((NO, P)); yb[2:] = 0.0
    xb0, pb0 = cotangent_map(R, yb[:2])
    xb1, pb1 = cotangent_map_het(R, X, yb)
    assert np.array_equal(xb0, xb1) and np.array_equal(pb0, pb1)


def test_policy_cotangent_with_extra_outputs_pairs_with_the_policy_partials():
    """<pbar, dpol> collects everything that reaches the outputs through the policy partials: with the inputs' direct terms
    removed from both sides the pairing holds for the extra outputs too (the store tests/test_gpu_vjp_het.py reads with
    policy_cotangent_seq)."""
    from test_vjp_host import tangent_map
    rng = np.random.default_rng(7)
    R = _random_record(rng)
    X = _extra(rng, R)
    X["S"][:] = 0.0                                              # (no direct dependence on the inputs)
    P = R["P"]
    dx = rng.standard_normal((3, P))
    dagg, dpol = tangent_map_het(R, X, dx), tangent_map(R, dx)[1]
    yb = rng.standard_normal((2 + NXT, P)); yb[1] = 0.0          # (consumption depends on the inputs directly)
    _, pbar = cotangent_map_het(R, X, yb)
    assert abs(np.sum(pbar * dpol) - np.sum(yb * dagg)) <= 1e-13 * np.sum(np.abs(pbar * dpol))


# ---- (2) the host layers with a stand-in block ------------------------------------------------------------------------------
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


def test_oracle_jacobian_of_the_first_two_outputs_is_the_two_output_one(hank, oracle_mod):
    m, ss, orc = ks_setup(30, 3, 25)
    x, _ = ks_paths(m, ss, "x1", 0.05)
    J3 = vc.oracle_jacobian_het(orc, ss.value, ss.D, x[2:4], 3, m.params.γ)
    assert np.array_equal(J3[:2], vc.oracle_jacobian(orc, ss.value, ss.D, x[2:4])) and np.abs(J3[2]).max() > 1e-3


def test_linearized_function_vjp_het_is_the_transpose_of_jvp(stub3_setup):
    hank, m, ss, x, Z, stub = stub3_setup
    lin = hank.LinearizedFunction(x.reshape(-1, order="F"), {"Z": Z}, m, ss, ss)
    assert lin._n_out == 3 and lin._out_idx == [0, 2] and stub.declared == 3
    n = lin.x.size
    rng = np.random.default_rng(1)
    y, yb = rng.standard_normal((n, 3)), rng.standard_normal((n, 5))
    Jy, JTyb = lin.jvp(y), lin.vjp_het(yb)
    assert JTyb.shape == (n, 5) and stub.calls["vjp_het"] == 1
    lhs, rhs = yb.T @ Jy, JTyb.T @ y
    assert np.max(np.abs(lhs - rhs)) <= 1e-11 * np.abs(lhs).max()
    assert np.abs(lin._Ragg[:, lin._Ragg.shape[1] // 2:]).max() > 0          # the residual layer does read Value
    assert np.allclose(lin.vjp_het(yb[:, 0]), JTyb[:, 0], rtol=0, atol=1e-13 * np.abs(JTyb).max())
    Jd, JTd = lin.jvp(np.eye(n)), lin.vjp_het(np.eye(n))
    assert np.max(np.abs(JTd - Jd.T)) <= 1e-12 + 1e-10 * np.abs(Jd).max()
    # vjp keeps its refusal; the LinearOperator and VJP take vjp_het for this model
    with pytest.raises(NotImplementedError, match="not affine"):
        lin.vjp(yb)
    op = lin.as_linear_operator()
    assert np.array_equal(op.rmatmat(yb), JTyb) and np.array_equal(op.rmatvec(yb[:, 0]), lin.vjp_het(yb[:, 0]))
    assert np.array_equal(hank.VJP(lin, lin.x, yb), JTyb)
    assert np.array_equal(hank.VJP(hank.make_fullFunction({"Z": Z}, m, ss, ss), lin.x, yb[:, :2]), JTyb[:, :2])
    before = stub.calls["vjp_het"]
    lin.vjp_het(np.zeros(n))                                      # no weight on any aggregate: nothing reaches the device
    assert stub.calls["vjp_het"] == before


def test_vjp_het_goes_through_vjp_for_a_model_with_at_most_two_outputs(hank, oracle_mod):
    from test_vjp_host import _StubBlock
    m, ss, orc = ks_setup(30, 3, 25)
    x, Z = ks_paths(m, ss, "x1", 0.05)
    agg, J, _, _ = orc.block(x[2:4], vc.unit_tangents(2, m.compspec.T - 1), ss.value, ss.D)
    old = m._hip_block
    stub = _StubBlock(J, agg, 2, m.compspec.T - 1)                # (it has no vjp_het at all)
    m._hip_block = stub
    try:
        lin = hank.LinearizedFunction(x.reshape(-1, order="F"), {"Z": Z}, m, ss, ss)
        yb = np.random.default_rng(3).standard_normal((lin.x.size, 4))
        assert np.array_equal(lin.vjp_het(yb), lin.vjp(yb)) and stub.calls["vjp"] == 2
    finally:
        m._hip_block = old


def test_device_group_shards_vjp_het_columns(stub3_setup):
    from hank_amd.parallel import DeviceGroup
    hank, m, ss, x, Z, stub = stub3_setup
    stub.set_het_outputs(3)
    grp = DeviceGroup(stub, [None, 1, 2])
    try:
        for b in grp.blocks[1:]:
            b.set_het_outputs(3)
        yb = np.random.default_rng(2).standard_normal((stub.P, 3, 7))
        got = grp.vjp_het(yb, 3)
        assert got.shape == (2, stub.P, 7) and np.array_equal(got, stub.vjp_het(yb, 3))
        assert [b.calls["vjp_het"] for b in grp.blocks[1:]] == [1, 1]
        assert grp.vjp_het(yb[:, :, :2], 3).shape == (2, stub.P, 2)              # fewer columns than devices
    finally:
        grp.close()


def test_abi_lists_the_new_entries(hank):
    import hank_amd
    assert {"hank_vjp_het", "hank_vjp_het_dev"} <= set(hank_amd.hip.ABI_SYMBOLS)
    assert hasattr(hank_amd.hip.HouseholdBlock, "vjp_het") and hasattr(hank_amd.hip.HouseholdBlock, "vjp_het_dev")
