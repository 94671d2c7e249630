"""hank_jvp_het / hank_vjp_het_boundary without a GPU: (a) the oracle loop the GPU module pins them against
(tests/sweep_refs.py) equals `Oracle.het_outputs` with zero seeds and matches central differences of it in (x, V, D) with
seeds; (b) the tangent map with extra outputs under boundary seeds and its transpose, stated in numpy on the random records of
tests/sweep_refs.py, are each other's transpose; (c) the host layers above the device (`LinearizedFunction.het_in_sweep`,
`.jvp_boundary`, `.vjp_boundary`, `DeviceGroup.jvp_het` / `.vjp_het_boundary`) with a stand-in block that multiplies by the oracle
loop's Jacobians of the three-output household block at 30x3, T = 25."""
import numpy as np
import pytest

import cases as vc
import sweep_refs as hbc
from sweep_refs import NXT, _extra, _random_record, cotangent_map, stub3_setup, stub_het_setup, tangent_map  # noqa: F401  (the setups: fixtures)


# ---- (a) the oracle loop ------------------------------------------------------------------------------------------------------
def _seeds(ec, n=3):
    """n directions on a raw economy: inputs, a smooth terminal-value tangent, a random initial-distribution tangent"""
    rng = np.random.default_rng(3)
    n_a, n_e = ec["V"].shape
    y = rng.standard_normal(ec["x"].shape + (n,)) * 1e-2
    return y, hbc.smooth_value_seeds(ec, n), rng.standard_normal((n_a, n_e, n)) / (n_a * n_e)


@pytest.mark.parametrize("name", ["dense-bottom", "both"])
def test_oracle_loop_with_zero_seeds_is_the_oracles_het_outputs(oracle_mod, name):
    ec = vc.raw_economy(name)
    y, dV, dD = _seeds(ec)
    gamma = ec["args"][4]
    agg, dagg = ec["orc"].het_outputs(ec["x"], y, ec["V"], ec["D"], 3, gamma)
    for got in (hbc.oracle_sweeps(ec["orc"], ec["x"], ec["V"], ec["D"], gamma, 3, y=y),
                hbc.oracle_sweeps(ec["orc"], ec["x"], ec["V"], ec["D"], gamma, 3, y=y, dV=0 * dV, dD=0 * dD)):
        for o in range(3):
            vc.close(got["agg"][:, o], agg[o], what=f"{name} output {o}"); vc.close(got["dagg"][:, o, :], dagg[o], what=f"{name} output {o} partials")
    # the first two outputs are the loop asked for two
    two = hbc.oracle_sweeps(ec["orc"], ec["x"], ec["V"], ec["D"], y=y, dV=dV, dD=dD)
    got = hbc.oracle_sweeps(ec["orc"], ec["x"], ec["V"], ec["D"], gamma, 3, y=y, dV=dV, dD=dD)
    assert np.array_equal(got["dagg"][:, 0, :], two["dagg"][:, 0]) and np.array_equal(got["dagg"][:, 1, :], two["dcons"]) and np.array_equal(got["dpol"], two["dpol"])


def test_oracle_loop_uce_with_zero_seeds_is_the_oracles_het_outputs_one_asset_hank(oracle_mod):
    m, ss, x, orc = vc.economy("hank", 2.0)
    x = np.ascontiguousarray(x[:, :6])
    y = np.random.default_rng(4).standard_normal(x.shape + (3,)) * 1e-2
    agg, dagg = orc.het_outputs(x, y, ss.value, ss.D, 4, m.params.γ)
    got = hbc.oracle_sweeps(orc, x, np.asarray(ss.value), np.asarray(ss.D), m.params.γ, 4, y=y)
    for o in range(4):
        vc.close(got["agg"][:, o], agg[o], what=f"hank output {o}"); vc.close(got["dagg"][:, o, :], dagg[o], what=f"hank output {o} partials")


@pytest.mark.parametrize("name", ["dense-bottom", "both"])
def test_oracle_loop_with_seeds_matches_central_differences(oracle_mod, name):
    """the step and the bound of tests/test_boundary_host.py (h = 1e-6, 1e-6 of the largest entry), output by output; each kind of
    seed reaches Value by at least 1e-2 of its largest entry"""
    ec = vc.raw_economy(name)
    orc, x, V, D, gamma = ec["orc"], ec["x"], ec["V"], ec["D"], ec["args"][4]
    n_a, n_e = V.shape
    y, dV, dD = _seeds(ec)
    d1 = hbc.oracle_sweeps(orc, x, V, D, gamma, 3, y=y, dV=dV, dD=dD)["dagg"]
    h = 1e-6
    fd = np.zeros_like(d1)
    for k in range(y.shape[2]):
        D2 = D.reshape((n_a, n_e), order="F")
        ap = orc.het_outputs(x + h * y[..., k], None, V + h * dV[..., k], (D2 + h * dD[..., k]).reshape(-1, order="F"), 3, gamma)[0]
        am = orc.het_outputs(x - h * y[..., k], None, V - h * dV[..., k], (D2 - h * dD[..., k]).reshape(-1, order="F"), 3, gamma)[0]
        fd[:, :, k] = ((ap - am) / (2 * h)).T
    for o in range(3):
        err = np.max(np.abs(fd[:, o] - d1[:, o])) / np.max(np.abs(d1[:, o]))
        print(f"{name} output {o}: dual loop vs central differences {err:.3e} of the largest entry")
        assert err <= 1e-6
    parts = {k: np.abs(hbc.oracle_sweeps(orc, x, V, D, gamma, 3, **{k: v})["dagg"][:, 2]).max() for k, v in (("y", y), ("dV", dV), ("dD", dD))}
    print(name, parts)
    assert min(parts.values()) >= 1e-2 * np.max(np.abs(d1[:, 2])), parts


# ---- (b) both maps in numpy ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_het_boundary_maps_are_each_others_transpose(seed):
    rng = np.random.default_rng(seed)
    R = _random_record(rng)
    X = _extra(rng, R)
    P, n_a, n_e = R["P"], R["n_a"], R["n_e"]
    G, NO = n_a * n_e, 2 + NXT
    zero = np.zeros((n_a, n_e))
    # zero seeds given: the map without seeds, bit for bit
    dx = rng.standard_normal((3, P))
    assert np.array_equal(tangent_map(R, dx, X, zero, zero)[0], tangent_map(R, dx, X)[0])
    # J (NO P, 3 P + 2 G): columns = unit seeds on the inputs, on dV_P, on dD_0
    J = np.zeros((NO * P, 3 * P + 2 * G))
    for k in range(3 * P):
        dx = np.zeros(3 * P); dx[k] = 1.0
        J[:, k] = tangent_map(R, dx.reshape(3, P), X, zero, zero)[0].reshape(-1)
    for k in range(2 * G):
        u = np.zeros(2 * G); u[k] = 1.0
        J[:, 3 * P + k] = tangent_map(R, np.zeros((3, P)), X, u[:G].reshape(n_a, n_e), u[G:].reshape(n_a, n_e))[0].reshape(-1)
    assert np.abs(J[2 * P:, 3 * P:3 * P + G]).max() > 1e-3 and np.abs(J[2 * P:, 3 * P + G:]).max() > 1e-3
    scale = max(1.0, np.abs(J).max())
    for only in (None, 2, 3):
        yb = rng.standard_normal((NO, P))
        if only is not None:
            yb[np.arange(NO) != only] = 0.0
        xbar, _, Vbar, Dbar = cotangent_map(R, yb, X)
        want = J.T @ yb.reshape(-1)
        got = np.concatenate([xbar.reshape(-1), Vbar.reshape(-1), Dbar.reshape(-1)])
        err = np.max(np.abs(got - want))
        print(f"seed {seed}, cotangents on {only}: max err {err:.3e} at scale {np.abs(want).max():.3e}")
        assert err <= 1e-13 * max(scale, np.abs(want).max())


# ---- (c) the host layers with a stand-in block ----------------------------------------------------------------------------------
def test_linearized_function_het_in_sweep_takes_one_jvp_het(stub_het_setup):
    hank, m, ss, x, Z, stub = stub_het_setup
    lin = hank.LinearizedFunction(x.reshape(-1, order="F"), {"Z": Z}, m, ss, ss)
    assert hank.LinearizedFunction.het_in_sweep is False and lin._n_out == 3
    y = np.random.default_rng(1).standard_normal((lin.x.size, 3))
    default = lin.jvp(y)
    assert stub.calls["jvp_het"] == 0
    before = stub.calls["jvp"]
    lin.het_in_sweep = True
    got = lin.jvp(y)
    assert stub.calls["jvp_het"] == 1 and stub.calls["jvp"] == before
    assert np.max(np.abs(got - default)) <= 1e-13 * np.abs(default).max()
    assert np.max(np.abs(lin.jvp(y[:, 0]) - default[:, 0])) <= 1e-13 * np.abs(default).max()


def test_linearized_function_vjp_boundary_is_the_transpose_of_jvp_boundary(stub_het_setup):
    hank, m, ss, x, Z, stub = stub_het_setup
    lin = hank.LinearizedFunction(x.reshape(-1, order="F"), {"Z": Z}, m, ss, ss)
    rng = np.random.default_rng(2)
    dV, dD = rng.standard_normal((stub.n_a, stub.n_e, 4)), rng.standard_normal((stub.n_a, stub.n_e, 4))
    Jb = lin.jvp_boundary(dV, dD)
    assert Jb.shape == (len(lin.Fx), 4) and np.abs(Jb).max() > 1e-6
    assert np.allclose(lin.jvp_boundary(dV, None) + lin.jvp_boundary(None, dD), Jb, rtol=0, atol=1e-12 * np.abs(Jb).max())
    assert np.allclose(lin.jvp_boundary(dV[:, :, 1], dD[:, :, 1]), Jb[:, 1], rtol=0, atol=1e-13 * np.abs(Jb).max())
    with pytest.raises(ValueError):
        lin.jvp_boundary()
    yb = rng.standard_normal((len(lin.Fx), 5))
    Vb, Db = lin.vjp_boundary(yb)
    assert Vb.shape == Db.shape == (stub.n_a, stub.n_e, 5)
    lhs, rhs = yb.T @ Jb, np.einsum("aem,aek->mk", Vb, dV) + np.einsum("aem,aek->mk", Db, dD)
    assert np.max(np.abs(lhs - rhs)) <= 1e-11 * np.abs(lhs).max()
    v1, d1 = lin.vjp_boundary(yb[:, 0])
    assert v1.shape == (stub.n_a, stub.n_e) and np.allclose(v1, Vb[:, :, 0], rtol=0, atol=1e-13 * np.abs(Vb).max())
    # Value carries weight to the boundary: dropping output 2 changes the answer
    assert np.abs(stub.Jb[2]).max() > 1e-3 and np.abs(lin._Ragg[:, lin._Ragg.shape[1] // 2:]).max() > 0


def test_device_group_shards_jvp_het_and_vjp_het_boundary_columns(stub_het_setup):
    from hank_amd.parallel import DeviceGroup
    hank, m, ss, x, Z, stub = stub_het_setup
    grp = DeviceGroup(stub, [None, 1, 2])
    try:
        for b in grp.blocks[1:]:
            b.set_het_outputs(3)
        rng = np.random.default_rng(2)
        y = rng.standard_normal((2, stub.P, 7))
        dV, dD = rng.standard_normal((stub.n_a, stub.n_e, 7)), rng.standard_normal((stub.n_a, stub.n_e, 7))
        got = grp.jvp_het(y, dV, dD, n_het=3)
        assert got.shape == (stub.P, 3, 7) and np.allclose(got, stub.jvp_het(y, dV, dD, n_het=3), rtol=0, atol=1e-12 * np.abs(got).max())
        assert [b.calls["jvp_het"] for b in grp.blocks[1:]] == [1, 1]
        assert grp.jvp_het(None, dV[:, :, :2], None, n_het=3).shape == (stub.P, 3, 2)          # fewer columns than devices
        yb = rng.standard_normal((stub.P, 3, 7))
        parts, whole = grp.vjp_het_boundary(yb, 3), stub.vjp_het_boundary(yb, 3)
        assert all(u.shape == v.shape and np.allclose(u, v, rtol=0, atol=1e-12 * np.abs(v).max()) for u, v in zip(parts, whole))
        assert grp.vjp_het_boundary(yb[:, :, :2], 3)[1].shape == (stub.n_a, stub.n_e, 2)
    finally:
        grp.close()


def test_abi_lists_the_new_entries(hank):
    import hank_amd
    assert {"hank_jvp_het", "hank_jvp_het_dev", "hank_vjp_het_boundary", "hank_vjp_het_boundary_dev"} <= set(hank_amd.hip.ABI_SYMBOLS)
    for attr in ("jvp_het", "jvp_het_dev", "vjp_het_boundary", "vjp_het_boundary_dev"):
        assert hasattr(hank_amd.hip.HouseholdBlock, attr)
    assert hasattr(hank_amd.LinearizedFunction, "jvp_boundary") and hasattr(hank_amd.LinearizedFunction, "vjp_boundary")
