"""hank_vjp_het without a GPU: (1) the transposed map with cotangents on outputs that are not affine in the policy
(csrc/hank_adjoint.h): Y^o_t = sum f_o,t D_t adds a weight f_o,t on the distribution, a direct term
-f_c,o,t D_t on the policy and (Sa + Sr, Sz, S1)_o,t on the inputs. Both maps are stated in numpy on the random records of
tests/sweep_refs.py, with random f, f_c, S for two extra outputs, and compared; (2) the host layers above the device
(`LinearizedFunction.vjp_het`, `as_linear_operator`, `VJP`, `DeviceGroup.vjp_het`) with a stand-in block that multiplies by the CPU
oracle's three-output Jacobian of the household block at 30x3, T = 25."""
import numpy as np
import pytest

import cases as vc
from conftest import ks_paths, ks_setup
from sweep_refs import NXT, _StubBlock, _extra, _random_record, cotangent_map, stub3_setup, tangent_map  # noqa: F401  (stub3_setup: a fixture)


# ---- (1) both maps in numpy (tests/sweep_refs.py) ------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_reverse_recurrences_with_extra_outputs_are_the_transpose_of_the_tangent_recurrences(seed):
    rng = np.random.default_rng(seed)
    R = _random_record(rng)
    X = _extra(rng, R)
    P, NO = R["P"], 2 + NXT
    J = np.zeros((NO * P, 3 * P))                                # rows (output, t), columns (input, s)
    for k in range(3):
        for s in range(P):
            dx = np.zeros((3, P)); dx[k, s] = 1.0
            J[:, k * P + s] = tangent_map(R, dx, X)[0].reshape(-1)
    assert np.abs(J[2 * P:]).max() > 1e-3
    scale = max(1.0, np.abs(J).max())
    for only in (None, 2, 3):                                    # every output; then one extra output alone (a swapped index shows)
        yb = rng.standard_normal((NO, P))
        if only is not None:
            yb[np.arange(NO) != only] = 0.0
        xbar = cotangent_map(R, yb, X)[0]
        want = J.T @ yb.reshape(-1)
        err = np.max(np.abs(xbar.reshape(-1) - want))
        print(f"seed {seed}, cotangents on {only}: max err {err:.3e} at scale {np.abs(want).max():.3e}")
        assert err <= 1e-13 * max(scale, np.abs(want).max())
    # nothing on the extra outputs: the two-output map, bit for bit
    yb = rng.standard_normal((NO, P)); yb[2:] = 0.0
    xb0, pb0 = cotangent_map(R, yb[:2])[:2]
    xb1, pb1 = cotangent_map(R, yb, X)[:2]
    assert np.array_equal(xb0, xb1) and np.array_equal(pb0, pb1)


def test_policy_cotangent_with_extra_outputs_pairs_with_the_policy_partials():
    """<pbar, dpol> collects everything that reaches the outputs through the policy partials: with the inputs' direct terms
    removed from both sides the pairing holds for the extra outputs too (the store tests/test_gpu_vjp_het.py reads with
    policy_cotangent_seq)."""
    rng = np.random.default_rng(7)
    R = _random_record(rng)
    X = _extra(rng, R)
    X["S"][:] = 0.0                                              # (no direct dependence on the inputs)
    P = R["P"]
    dx = rng.standard_normal((3, P))
    dagg, dpol = tangent_map(R, dx, X)[0], tangent_map(R, dx)[1]
    yb = rng.standard_normal((2 + NXT, P)); yb[1] = 0.0          # (consumption depends on the inputs directly)
    pbar = cotangent_map(R, yb, X)[1]
    assert abs(np.sum(pbar * dpol) - np.sum(yb * dagg)) <= 1e-13 * np.sum(np.abs(pbar * dpol))


# ---- (2) the host layers with a stand-in block ------------------------------------------------------------------------------
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
