"""hank_jvp_het / hank_vjp_het_boundary without a GPU: (a) the oracle loop the GPU module pins them against
(tests/het_boundary_cases.py) equals `Oracle.het_outputs` with zero seeds and matches central differences of it in (x, V, D) with
seeds; (b) the tangent map with extra outputs under boundary seeds and its transpose, stated in numpy on the random records of
tests/test_vjp_host.py, are each other's transpose; (c) the host layers above the device (`LinearizedFunction.het_in_sweep`,
`.jvp_boundary`, `.vjp_boundary`, `DeviceGroup.jvp_het` / `.vjp_het_boundary`) with a stand-in block that multiplies by the oracle
loop's Jacobians of the three-output household block at 30x3, T = 25."""
import numpy as np
import pytest

import boundary_cases as bc
import cases as vc
import het_boundary_cases as hbc
from test_vjp_het_host import NXT, _StubBlock3, _extra, stub3_setup, tangent_map_het  # noqa: F401  (stub3_setup: a fixture)
from test_vjp_host import _random_record


# ---- (a) the oracle loop ------------------------------------------------------------------------------------------------------
def _seeds(ec, n=3):
    """n directions on a raw economy: inputs, a smooth terminal-value tangent, a random initial-distribution tangent"""
    rng = np.random.default_rng(3)
    n_a, n_e = ec["V"].shape
    y = rng.standard_normal(ec["x"].shape + (n,)) * 1e-2
    return y, bc.smooth_value_seeds(ec, n), rng.standard_normal((n_a, n_e, n)) / (n_a * n_e)


@pytest.mark.parametrize("name", ["dense-bottom", "both"])
def test_oracle_loop_with_zero_seeds_is_the_oracles_het_outputs(oracle_mod, name):
    ec = vc.raw_economy(name)
    y, dV, dD = _seeds(ec)
    gamma = ec["args"][4]
    agg, dagg = ec["orc"].het_outputs(ec["x"], y, ec["V"], ec["D"], 3, gamma)
    for got in (hbc.oracle_het_boundary(ec["orc"], ec["x"], ec["V"], ec["D"], gamma, 3, y=y),
                hbc.oracle_het_boundary(ec["orc"], ec["x"], ec["V"], ec["D"], gamma, 3, y=y, dV=0 * dV, dD=0 * dD)):
        for o in range(3):
            vc.close(got["agg"][:, o], agg[o], what=f"{name} output {o}"); vc.close(got["dagg"][:, o, :], dagg[o], what=f"{name} output {o} partials")
    # the first two outputs are the loop of tests/boundary_cases.py
    two = bc.oracle_boundary(ec["orc"], ec["x"], ec["V"], ec["D"], y=y, dV=dV, dD=dD)
    got = hbc.oracle_het_boundary(ec["orc"], ec["x"], ec["V"], ec["D"], gamma, 3, y=y, dV=dV, dD=dD)
    assert np.array_equal(got["dagg"][:, 0, :], two["dagg"]) and np.array_equal(got["dagg"][:, 1, :], two["dcons"]) and np.array_equal(got["dpol"], two["dpol"])


def test_oracle_loop_uce_with_zero_seeds_is_the_oracles_het_outputs_one_asset_hank(oracle_mod):
    m, ss, x, orc = vc.economy("hank", 2.0)
    x = np.ascontiguousarray(x[:, :6])
    y = np.random.default_rng(4).standard_normal(x.shape + (3,)) * 1e-2
    agg, dagg = orc.het_outputs(x, y, ss.value, ss.D, 4, m.params.γ)
    got = hbc.oracle_het_boundary(orc, x, np.asarray(ss.value), np.asarray(ss.D), m.params.γ, 4, y=y)
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
    d1 = hbc.oracle_het_boundary(orc, x, V, D, gamma, 3, y=y, dV=dV, dD=dD)["dagg"]
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
    parts = {k: np.abs(hbc.oracle_het_boundary(orc, x, V, D, gamma, 3, **{k: v})["dagg"][:, 2]).max() for k, v in (("y", y), ("dV", dV), ("dD", dD))}
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
    # zero seeds: the map of tests/test_vjp_het_host.py, bit for bit
    dx = rng.standard_normal((3, P))
    assert np.array_equal(hbc.tangent_map_het_boundary(R, X, dx, zero, zero), tangent_map_het(R, X, dx))
    # J (NO P, 3 P + 2 G): columns = unit seeds on the inputs, on dV_P, on dD_0
    J = np.zeros((NO * P, 3 * P + 2 * G))
    for k in range(3 * P):
        dx = np.zeros(3 * P); dx[k] = 1.0
        J[:, k] = hbc.tangent_map_het_boundary(R, X, dx.reshape(3, P), zero, zero).reshape(-1)
    for k in range(2 * G):
        u = np.zeros(2 * G); u[k] = 1.0
        J[:, 3 * P + k] = hbc.tangent_map_het_boundary(R, X, np.zeros((3, P)), u[:G].reshape(n_a, n_e), u[G:].reshape(n_a, n_e)).reshape(-1)
    assert np.abs(J[2 * P:, 3 * P:3 * P + G]).max() > 1e-3 and np.abs(J[2 * P:, 3 * P + G:]).max() > 1e-3
    scale = max(1.0, np.abs(J).max())
    for only in (None, 2, 3):
        yb = rng.standard_normal((NO, P))
        if only is not None:
            yb[np.arange(NO) != only] = 0.0
        xbar, Vbar, Dbar = hbc.cotangent_map_het_boundary(R, X, yb)
        want = J.T @ yb.reshape(-1)
        got = np.concatenate([xbar.reshape(-1), Vbar.reshape(-1), Dbar.reshape(-1)])
        err = np.max(np.abs(got - want))
        print(f"seed {seed}, cotangents on {only}: max err {err:.3e} at scale {np.abs(want).max():.3e}")
        assert err <= 1e-13 * max(scale, np.abs(want).max())


# ---- (c) the host layers with a stand-in block ----------------------------------------------------------------------------------
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
    from conftest import ks_setup
    hank, m, ss, x, Z, stub = stub3_setup
    _, ss0, orc = ks_setup(30, 3, 25)
    n_a, n_e = np.asarray(ss0.value).shape
    G = n_a * n_e
    U = np.eye(G).reshape((n_a, n_e, G), order="F")
    Zs = np.zeros_like(U)
    ref = hbc.oracle_het_boundary(orc, x[2:4], np.asarray(ss0.value), np.asarray(ss0.D), m.params.γ, 3, dV=np.concatenate([U, Zs], axis=2),
                                  dD=np.concatenate([Zs, U], axis=2))
    mine = _StubHet(stub.J, stub.agg, 2, stub.P, np.ascontiguousarray(ref["dagg"].transpose(1, 0, 2)), n_a, n_e)
    mine.declared = 3
    m._hip_block = mine
    yield hank, m, ss, x, Z, mine
    m._hip_block = stub


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
