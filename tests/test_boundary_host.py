"""Tangents and cotangents on the boundary (V_P = `ss_end.value`, D_0 = `ss_initial.D`) without a GPU: (a) the oracle loop the
GPU module pins hank_jvp_boundary against (tests/sweep_refs.py: `Oracle.value_function` backward with a dual `value_next`,
`Oracle.transition_step` forward with a dual `D_prev`, the aggregates in numpy) equals `Oracle.block` with zero seeds and matches
central differences of `Oracle.block` in (x, V, D) with seeds; (b) both boundary maps stated in numpy on the random linearisation
records of tests/sweep_refs.py are each other's transpose, the productivity-marginal term of consumption included."""
import numpy as np
import pytest

import cases as vc
import sweep_refs as bc
from sweep_refs import _random_record, cotangent_map, tangent_map


# ---- (a) the oracle loop ------------------------------------------------------------------------------------------------------
def _seeds(ec, n=3):
    """n directions on a raw economy: inputs, a smooth terminal-value tangent, a random initial-distribution tangent"""
    rng = np.random.default_rng(3)
    n_a, n_e = ec["V"].shape
    y = rng.standard_normal(ec["x"].shape + (n,)) * 1e-2
    return y, bc.smooth_value_seeds(ec, n), rng.standard_normal((n_a, n_e, n)) / (n_a * n_e)


@pytest.mark.parametrize("name", ["dense-bottom", "both"])
def test_oracle_loop_with_zero_seeds_is_the_oracles_block(oracle_mod, name):
    """measured: 6e-14 absolute on the aggregate, 9e-16 relative on the partials"""
    ec = vc.raw_economy(name)
    y, dV, dD = _seeds(ec)
    agg, dagg, pol, dpol = ec["orc"].block(ec["x"], y, ec["V"], ec["D"])
    for got in (bc.oracle_sweeps(ec["orc"], ec["x"], ec["V"], ec["D"], y=y),
                bc.oracle_sweeps(ec["orc"], ec["x"], ec["V"], ec["D"], y=y, dV=0 * dV, dD=0 * dD)):
        vc.close(got["agg"][:, 0], agg, what=name + " agg"); vc.close(got["dagg"][:, 0], dagg, what=name + " dagg")
        vc.close(got["pol"], pol, what=name + " policy"); vc.close(got["dpol"], dpol, what=name + " dpolicy")
    # consumption and the grid aggregate against the two-variable block
    agg_h, dagg_h = ec["orc"].block_het(ec["x"], y, ec["V"], ec["D"])
    vc.close(got["cons"], agg_h[1], what=name + " consumption"); vc.close(got["dcons"], dagg_h[1], what=name + " dconsumption")


@pytest.mark.parametrize("name", ["dense-bottom", "both"])
def test_oracle_loop_with_seeds_matches_central_differences(oracle_mod, name):
    """h = 1e-6: measured 1.2e-8 and 3.9e-10 of the largest entry on the two economies; the bound is 1e-6, two orders above the
    worse. The dx-only, dV-only and dD-only parts each reach at least 1e-2 of the largest entry, four orders above the bound: a
    loop that dropped one would be seen (measured: the three are within a factor of 20 of each other)."""
    ec = vc.raw_economy(name)
    orc, x, V, D = ec["orc"], ec["x"], ec["V"], ec["D"]
    n_a, n_e = V.shape
    y, dV, dD = _seeds(ec)
    d1 = bc.oracle_sweeps(orc, x, V, D, y=y, dV=dV, dD=dD)["dagg"][:, 0]
    h = 1e-6
    fd = np.zeros_like(d1)
    for k in range(y.shape[2]):
        D2 = D.reshape((n_a, n_e), order="F")
        ap = orc.block(x + h * y[..., k], None, V + h * dV[..., k], (D2 + h * dD[..., k]).reshape(-1, order="F"))[0]
        am = orc.block(x - h * y[..., k], None, V - h * dV[..., k], (D2 - h * dD[..., k]).reshape(-1, order="F"))[0]
        fd[:, k] = (ap - am) / (2 * h)
    err = np.max(np.abs(fd - d1)) / np.max(np.abs(d1))
    print(f"{name}: dual loop vs central differences {err:.3e} of the largest entry")
    assert err <= 1e-6
    parts = {k: np.abs(bc.oracle_sweeps(orc, x, V, D, **{k: v})["dagg"][:, 0]).max() for k, v in (("y", y), ("dV", dV), ("dD", dD))}
    print(name, parts)
    assert min(parts.values()) >= 1e-2 * np.max(np.abs(d1)), parts
    # linear in the seeds
    sup = sum(bc.oracle_sweeps(orc, x, V, D, **{k: v})["dagg"][:, 0] for k, v in (("y", y), ("dV", dV), ("dD", dD)))
    vc.close(sup, d1, what=name + " superposition")


# ---- (b) both boundary maps in numpy ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_boundary_maps_are_each_others_transpose(seed):
    rng = np.random.default_rng(seed)
    R = _random_record(rng)
    P, n_a, n_e = R["P"], R["n_a"], R["n_e"]
    G = n_a * n_e
    zero = np.zeros((n_a, n_e))
    # zero seeds given: the maps without seeds
    dx = rng.standard_normal((3, P))
    d0, p0, c0 = tangent_map(R, dx, None, zero, zero)
    dref, pref, _ = tangent_map(R, dx)
    assert np.array_equal(d0, dref) and np.array_equal(p0, pref)
    assert np.max(np.abs(c0 - dref[1])) <= 1e-13 * np.abs(dref).max()
    # J_b (2 P, 2 G): columns = unit seeds on dV_P, then on dD_0; consumption as the device assembles it equals its definition
    J = np.zeros((2 * P, 2 * G))
    for k in range(2 * G):
        u = np.zeros(2 * G); u[k] = 1.0
        dagg, _, dC = tangent_map(R, np.zeros((3, P)), None, u[:G].reshape(n_a, n_e), u[G:].reshape(n_a, n_e))
        assert np.max(np.abs(dC - dagg[1])) <= 1e-13 * max(1.0, np.abs(dagg).max()), k
        J[:, k] = dagg.reshape(-1)
    assert np.abs(J[:, :G]).max() > 1e-3 and np.abs(J[:, G:]).max() > 1e-3
    # a dD_0 seed that moves total mass and the productivity marginal: the term k_het_outputs leaves out is not small
    dD = rng.uniform(0, 1, (n_a, n_e))
    dagg, _, dC = tangent_map(R, np.zeros((3, P)), None, zero, dD)
    m = dD.sum(axis=0) @ R["Pi"]
    assert abs(R["x"][1, 0] * np.sum(R["z"] * m) + R["x"][2, 0] * np.sum(m)) > 1e-2 * np.abs(dagg[1]).max()
    assert np.max(np.abs(dC - dagg[1])) <= 1e-13 * np.abs(dagg).max()
    for _ in range(4):
        yb = rng.standard_normal((2, P))
        xbar, pbar, Vbar, Dbar = cotangent_map(R, yb)
        xref, pbref = cotangent_map(R, yb)[:2]                   # (the map that keeps its two last states is the only one now)
        assert np.array_equal(xbar, xref) and np.array_equal(pbar, pbref)
        want = J.T @ yb.reshape(-1)
        got = np.concatenate([Vbar.reshape(-1), Dbar.reshape(-1)])
        assert np.max(np.abs(got - want)) <= 1e-13 * max(1.0, np.abs(want).max())
    # the policy variable alone
    yb = np.stack([rng.standard_normal(P), np.zeros(P)])
    _, _, Vbar, Dbar = cotangent_map(R, yb)
    assert np.allclose(np.concatenate([Vbar.reshape(-1), Dbar.reshape(-1)]), J[:P].T @ yb[0], rtol=0, atol=1e-13 * np.abs(J).max() * P)
