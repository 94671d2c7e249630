"""The oracle against the self-consistency checks the reference itself relies on:
 1 steady-state residual; 2 F(x_ss)≈0 through the full pipeline; 4 AD vs finite differences;
 5 residual length; 6 column-stochastic lottery / mass conservation; plus dual-specific checks
 (chunk independence, linearity in the tangent)."""
import numpy as np
import pytest

from conftest import ks_paths, ks_setup


def test_ss_residual_and_full_pipeline_at_ss(ks_small):
    m, ss, orc = ks_small
    P = m.compspec.T - 1
    # item 1: residuals_fn on the tiled SS column (test_SteadyState.jl:61-84)
    xMat = np.tile(np.array([ss.vars[k] for k in m.variables])[:, None], (1, 2))
    assert np.linalg.norm(m.residuals_fn(xMat, m.params)) < 10 * m.compspec.ε
    # hand-written equilibrium identities (test_SteadyState.jl:46-59)
    α, δ = m.params.α, m.params.δ
    v = ss.vars
    assert abs(v["Y"] - v["Z"] * v["KS"] ** α) < 1e-5
    assert abs(v["r"] + δ - α * v["Z"] * v["KS"] ** (α - 1)) < 1e-5
    assert abs(v["w"] - (1 - α) * v["Z"] * v["KS"] ** α) < 1e-5
    assert abs(v["KS"] - v["KD"]) < 1e-5
    # item 2: F(x_ss) ~ 0 through Backward -> Forward -> Residuals with a constant SS path
    x0, _ = ks_paths(m, ss, "x0")
    F, _ = orc.ks_jvp(x0, np.zeros((4, P, 1)), np.ones(P), α, δ, v["KS"], ss.value, ss.D)
    assert F.shape == (4 * P,)          # item 5 (test_Model.jl:84-92)
    assert np.max(np.abs(F)) < 10 * m.compspec.ε


def test_mass_conservation_and_stochastic_lottery(ks_small):
    m, ss, orc = ks_small
    P = m.compspec.T - 1
    x, _ = ks_paths(m, ss, "x1", 0.05)
    N = 2
    xr = np.zeros((P, 1 + N)); xw = np.zeros((P, 1 + N))
    xr[:, 0], xw[:, 0] = x[2], x[3]
    rng = np.random.default_rng(1)
    xr[:, 1:], xw[:, 1:] = rng.standard_normal((P, N)), rng.standard_normal((P, N))
    st, pol = orc.backward_iteration(xr, xw, ss.value, N)
    assert st == 0
    agg, Dseq = orc.forward_iteration(pol, ss.D, N, return_D=True)
    # item 6 (ForwardIteration.jl:28-35): D_t stays a probability vector, its partials sum to zero
    np.testing.assert_allclose(Dseq[..., 0].sum(axis=(1, 2)), 1.0, atol=1e-12)
    assert np.max(np.abs(Dseq[..., 1:].sum(axis=(1, 2)))) < 1e-10
    assert Dseq[..., 0].min() >= 0.0
    # policies are monotone in wealth and respect the borrowing constraint
    assert np.all(np.diff(pol[..., 0], axis=1) >= 0)
    assert pol[..., 0].min() >= m.params.borrow_cons


@pytest.mark.parametrize("kind,shock", [("x0", 0.0), ("x1", 0.05)])
def test_ad_vs_central_differences(ks_small, kind, shock):
    """item 4 (SteadyState.jl:296-356): dual-number JVP vs finite differences of the Float64 path."""
    m, ss, orc = ks_small
    P = m.compspec.T - 1
    α, δ = m.params.α, m.params.δ
    x, Z = ks_paths(m, ss, kind, shock)
    rng = np.random.default_rng(2)
    y = rng.standard_normal((4, P, 2))
    _, J = orc.ks_jvp(x, y, Z, α, δ, ss.vars["KS"], ss.value, ss.D)
    f = lambda xx: orc.ks_jvp(xx, np.zeros((4, P, 1)), Z, α, δ, ss.vars["KS"], ss.value, ss.D)[0]
    for k in range(2):
        h = 1e-6
        fd = (f(x + h * y[:, :, k]) - f(x - h * y[:, :, k])) / (2 * h)
        # the map is piecewise smooth (kinks at bracket changes): FD agrees to O(h) relative
        assert np.max(np.abs(fd - J[:, k])) < 2e-4 * np.max(np.abs(J[:, k]))


def test_chunk_independence_and_linearity(ks_small):
    """partials are independent of the chunk they travel in (N=1 vs N=3 vs padded N=4) and linear."""
    m, ss, orc = ks_small
    P = m.compspec.T - 1
    α, δ = m.params.α, m.params.δ
    x, Z = ks_paths(m, ss, "x1", 0.05)
    rng = np.random.default_rng(3)
    y = rng.standard_normal((4, P, 3))
    F3, J3 = orc.ks_jvp(x, y, Z, α, δ, ss.vars["KS"], ss.value, ss.D)
    for k in range(3):
        F1, J1 = orc.ks_jvp(x, y[:, :, k], Z, α, δ, ss.vars["KS"], ss.value, ss.D)
        assert np.array_equal(F1, F3)
        assert np.array_equal(J1[:, 0], J3[:, k])
    comb = 0.3 * y[:, :, 0] - 1.7 * y[:, :, 1]
    _, Jc = orc.ks_jvp(x, comb, Z, α, δ, ss.vars["KS"], ss.value, ss.D)
    ref = 0.3 * J3[:, 0] - 1.7 * J3[:, 1]
    np.testing.assert_allclose(Jc[:, 0], ref, rtol=0, atol=1e-10 * np.abs(ref).max())


def test_oracle_reports_julia_errors(ks_small):
    """unsorted knots -> Interpolations error; negative base under a fractional power -> DomainError."""
    m, ss, orc = ks_small
    bad = np.array(ss.value, copy=True)
    bad[10, :] *= 1e-4                            # a spike in consumption: knots no longer sorted
    st, _, _ = orc.value_function(bad, [ss.vars["r"]], [ss.vars["w"]], 1)
    assert st == 3
    from oracle.oracle import Oracle
    wd, pd_ = m.heterogeneity["wealth"], m.heterogeneity["productivity"]
    o2 = Oracle(wd.grid, pd_.grid, pd_.transition, m.params.β, 2.5, m.params.borrow_cons)
    st, _, _ = o2.value_function(-np.abs(ss.value), [ss.vars["r"]], [ss.vars["w"]], 1)
    assert st in (3, 4)


# ---- the references of the GPU suite (Oracle.block, block_het, het_outputs) against the functions they wrap ----
def _seeded_by_hand(x, y):
    """the two passes of N = 33 as Oracle.block makes them: 32 partials, then one (N = 1 is a compiled width)."""
    from oracle.oracle import pad_N
    for c0, c1 in ((0, 32), (32, y.shape[2])):
        Nc = pad_N(c1 - c0)
        xd = np.zeros(x.shape + (1 + Nc,))
        xd[..., 0] = x
        xd[..., 1:1 + c1 - c0] = y[:, :, c0:c1]
        yield c1 - c0, Nc, xd


@pytest.fixture(scope="module")
def ks_30x3():
    m, ss, orc = ks_setup(30, 3, 25)
    return m, ss, orc, np.ascontiguousarray(ks_paths(m, ss, "x1", 0.05)[0][2:4])


def test_block_is_household_block_on_the_seeded_passes(ks_30x3):
    """N = 33: one full pass of 32 partials and one of a single partial; bit for bit what household_block returns on the same
    two duals, and with y=None the value column of those passes."""
    m, ss, orc, x = ks_30x3
    y = np.random.default_rng(4).standard_normal((2, 24, 33))
    agg, dagg, pol, dpol = orc.block(x, y, ss.value, ss.D)
    assert agg.shape == (24,) and dagg.shape == (24, 33) and pol.shape == (24, 30, 3) and dpol.shape == (24, 30, 3, 33)
    c0 = 0
    for n, Nc, xd in _seeded_by_hand(x, y):
        st, oa, op = orc.household_block(xd[0], xd[1], ss.value, ss.D, Nc)
        assert st == 0
        assert np.array_equal(agg, oa[:, 0]) and np.array_equal(pol, op[..., 0])
        assert np.array_equal(dagg[:, c0:c0 + n], oa[:, 1:1 + n]) and np.array_equal(dpol[..., c0:c0 + n], op[..., 1:1 + n])
        c0 += n
    a0, d0, p0, dp0 = orc.block(x, None, ss.value, ss.D)
    assert np.array_equal(a0, agg) and np.array_equal(p0, pol) and d0.shape == (24, 0) and dp0.shape == (24, 30, 3, 0)
    with pytest.raises(RuntimeError, match="oracle status 3"):          # a non-zero status raises
        bad = np.array(ss.value, copy=True)
        bad[10, :] *= 1e-4
        orc.block(x, None, bad, ss.D)


def test_block_het_is_household_block_het_on_the_seeded_pass(ks_30x3):
    from oracle.oracle import pad_N
    m, ss, orc, x = ks_30x3
    N = 3
    y = np.random.default_rng(5).standard_normal((2, 24, N))
    xd = np.zeros((2, 24, 1 + pad_N(N)))
    xd[..., 0] = x
    xd[..., 1:] = y
    st, oa, _, _ = orc.household_block_het(xd[0], xd[1], ss.value, ss.D, pad_N(N))
    assert st == 0
    agg, dagg = orc.block_het(x, y, ss.value, ss.D)
    assert agg.shape == (2, 24) and dagg.shape == (2, 24, N)
    assert np.array_equal(agg, oa[..., 0]) and np.array_equal(dagg, oa[..., 1:])
    assert np.array_equal(orc.block_het(x, None, ss.value, ss.D)[0], agg)


def test_het_outputs_rows_and_the_value_rows_central_difference(ks_30x3):
    """n_het = 3: rows 0 and 1 are block_het's bit for bit; row 2 (Value) agrees with a central difference of its own value
    along the first direction, h = 1e-6: measured 2.7e-10 of the largest partial on the CPU oracle (truncation O(h^2) against
    rounding eps/h, smallest at this h), bound 3e-9, a decade above."""
    m, ss, orc, x = ks_30x3
    y = np.random.default_rng(5).standard_normal((2, 24, 3))
    agg, dagg = orc.het_outputs(x, y, ss.value, ss.D, 3, m.params.γ)
    assert agg.shape == (3, 24) and dagg.shape == (3, 24, 3)
    a2, d2 = orc.block_het(x, y, ss.value, ss.D)
    assert np.array_equal(agg[:2], a2) and np.array_equal(dagg[:2], d2)
    h, d = 1e-6, y[:, :, 0]
    up, dn = (orc.het_outputs(x + s * h * d, None, ss.value, ss.D, 3, m.params.γ)[0][2] for s in (1.0, -1.0))
    err = np.max(np.abs((up - dn) / (2 * h) - dagg[2][:, 0])) / np.max(np.abs(dagg[2][:, 0]))
    print(f"Value row: central difference vs partial, relative to the largest partial: {err:.3e}")
    assert err <= 3e-9
