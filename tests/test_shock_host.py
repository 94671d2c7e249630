"""CPU tests of the discount-factor path's references and host layers (no GPU):
1. tests/path_refs.oracle_path_sweeps at tests/shock_refs.KIND — the oracle loop with beta = beta_t and the value's partials augmented by V dbeta_t / beta_t —
   against a central difference of ITS OWN level in the entries beta_0 and beta_{P-1} (step 1e-6, agreement 1e-6 relative): the
   construction the GPU tests compare with is pinned without a device;
2. tests/path_refs.jacobians at tests/shock_refs.KIND — the dense pair every width of tests/test_gpu_shock_geometry.py is compared with — against
   the sweeps with random seeds in the inputs and in beta together, and the raw grids' edges on the oracle's policy under a path;
3. SteadyStateJacobian.shock_jacobian's recursion on a stand-in block;
4. examples/solve_hank.py's arguments."""
import numpy as np
import pytest

import cases
import path_checks as C
import path_refs
import shock_refs as R
from cases import close

STEP = 1e-6
K = R.KIND


@pytest.mark.parametrize("family,name,n_a,n_e,T", [("ks", "gamma2", 33, 2, 4), ("hank", "gamma1.5", 33, 2, 4), ("ks", "gamma1", 33, 2, 2),
                                                  ("hank", "gamma3", 130, 3, 12)])
def test_the_reference_s_beta_tangent_is_the_derivative_of_its_own_level(oracle_mod, family, name, n_a, n_e, T):
    c = R.shock_case(family, name, n_a, n_e, T)
    P, nh = T - 1, c["n_het"]
    entries = sorted({0, P - 1})
    dbeta = np.zeros((P, len(entries)))
    for k, t in enumerate(entries):
        dbeta[t, k] = 1.0
    ref = path_refs.oracle_path_sweeps(K, c["orc"], c["x"], c["V"], c["D"], c["path"], c["gamma"], nh, dpath=dbeta)
    assert c["orc"].m.beta == c["beta"]                          # the oracle's own beta is restored
    for k, t in enumerate(entries):
        lv = []
        for sgn in (1.0, -1.0):
            b = c["path"].copy()
            b[t] += sgn * STEP
            lv.append(path_refs.oracle_path_sweeps(K, c["orc"], c["x"], c["V"], c["D"], b, c["gamma"], nh))
        what = f"{family} {name} {n_a}x{n_e} T={T} beta_{t}"
        fd_agg = (lv[0]["agg"] - lv[1]["agg"]) / (2 * STEP)
        fd_pol = (lv[0]["pol"] - lv[1]["pol"]) / (2 * STEP)
        assert np.abs(fd_agg).max() > 1e-3, what
        for o in range(nh):
            close(ref["dagg"][:, o, k], fd_agg[:, o], rel=1e-6, ab=0.0, what=f"{what} output {o}")
        close(ref["dpol"][..., k], fd_pol, rel=1e-6, ab=0.0, what=f"{what} policy")
        # beta_t moves no policy after t
        assert not np.any(ref["dpol"][t + 1:, ..., k])


def test_a_constant_path_is_the_oracle_s_own_block(oracle_mod):
    c = R.shock_case("ks", "gamma2", 33, 2, 4)
    ref = path_refs.oracle_path_sweeps(K, c["orc"], c["x"], c["V"], c["D"], np.full(3, c["beta"]), c["gamma"], 3)
    agg, _, pol, _ = c["orc"].block(c["x"], None, c["V"], c["D"])
    close(ref["agg"][:, 0], agg, what="constant path: aggregate")
    close(ref["pol"], pol, what="constant path: policy")


LINEAR_ECONOMIES = [("shape", 65, 3, 12), ("shape", 40, 11, 10), ("shape", 40, 1, 10), ("raw", "both")]


@pytest.mark.parametrize("econ", LINEAR_ECONOMIES, ids=lambda e: "-".join(str(q) for q in e))
def test_the_dense_pair_reproduces_the_sweeps_with_both_seeds(oracle_mod, econ):
    """path_refs.jacobians' (Jx, Jb) — and the grid aggregate's pair — against path_refs.oracle_path_sweeps with random y and dbeta together:
    the map is linear, so the two agree to rounding (1e-13 of the largest entry; measured <= 1.2e-15)"""
    c = R.geometry_case(*econ)
    r = C.dense_pair_reproduces_sweeps(K, c, f"{econ}", 1e-13)
    J2x, J2b = path_refs.grid_jacobians(*r.args)
    close(np.einsum("tks,ksn->tn", J2x, r.dx) + J2b @ r.dp, r.ref["dagg2"], rel=1e-13, ab=0.0, what=f"{econ} grid aggregate")


@pytest.mark.parametrize("name", R.EDGE_ECONOMIES)
def test_the_raw_grids_keep_their_edges_under_a_path(oracle_mod, name):
    """conditions on the inputs of tests/test_gpu_shock_geometry.py section D: under beta_path(beta, 9) the oracle's policy holds
    a deep clamped prefix, sources capped at the top and long runs of rows in one bracket (measured: clo up to 61 / 3 / 73, top up to
    1 / 43 / 19, runs up to 52 / 2 / 60 for dense-bottom / short-top / both; deep-prefix: 265 clamped rows; swing: 123 sources on one
    target row)"""
    c = R.geometry_case("raw", name)
    assert c["path"].shape == (cases.EDGE_P,)
    pol = path_refs.oracle_path_sweeps(K, c["orc"], c["x"], c["V"], c["D"], c["path"], c["gamma"], c["n_het"])["pol"]
    assert np.all(np.isfinite(pol))
    R.check_path_edges(name, c["grid"], pol)


def test_shock_jacobian_is_the_toeplitz_recursion_per_output(hank):
    C.jacobian_is_the_toeplitz_recursion(hank, K, (), 3, 2)


def test_the_example_parses_the_discount_shock():
    from examples.solve_hank import parse_args
    a = parse_args(["--discount-shock", "0.002", "0.8"])
    assert a.discount_shock == [0.002, 0.8] and not a.gradient
    a = parse_args(["--discount-shock", "0.002", "0.8", "--gradient", "--n-a", "130", "--n-e", "3", "--T", "40"])
    assert a.discount_shock == [0.002, 0.8] and a.gradient and (a.n_a, a.n_e, a.T) == (130, 3, 40)
    assert parse_args([]).discount_shock is None
    with pytest.raises(SystemExit):
        parse_args(["--discount-shock", "0.002"])
