"""The transposed household block without a GPU: (1) the recurrences hank_vjp implements (csrc/hank_adjoint.h, DESIGN.md
section 3d) are the exact transpose of the tangent recurrences of DESIGN.md section 1 — both maps stated in numpy here and
compared on random linearisation records (tests/sweep_refs.py) (two outputs, three inputs, a clamped prefix); (2) the host layers above the device
(`LinearizedFunction.vjp`, `as_linear_operator`, `VJP`, `DeviceGroup.vjp`) with a stand-in block that multiplies by the CPU
oracle's Jacobian of the household block at 30x3, T = 25; (3) the raw-grid economies of tests/cases.py hold, on the oracle's policy, the
data-dependent edges tests/test_gpu_vjp_variants.py runs hank_vjp through: proven present without a GPU."""
import numpy as np
import pytest

import cases as vc
from sweep_refs import _random_record, cotangent_map, stub_setup, tangent_map  # noqa: F401  (stub_setup: a fixture)


# ---- (1) both maps in numpy (tests/sweep_refs.py) ------------------------------------------------------------------------------
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
        xbar = cotangent_map(R, yb)[0]
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
    dagg, dpol, _ = tangent_map(R, rng.standard_normal((3, P)))
    yb = np.stack([rng.standard_normal(P), np.zeros(P)])
    pbar = cotangent_map(R, yb)[1]
    assert abs(np.sum(pbar * dpol) - np.sum(yb[0] * dagg[0])) <= 1e-13 * np.sum(np.abs(pbar * dpol))


# ---- (2) the host layers with a stand-in block ------------------------------------------------------------------------------
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
