"""hank_vjp_het: the transposed sweeps with cotangents on the heterogeneous outputs that are not affine in the policy (Value, UCE;
csrc/hank_adjoint.h) on the MI355X. The reference is the CPU oracle's Jacobian J (n_het, P, n_hh, P) from unit
tangents through Oracle.het_outputs (at most 32 columns per pass), transposed — never another run of the device: (1) Krusell-Smith
with Value, (2) the sticky-wage one-asset HANK with Value and UCE, each with every output and with one extra output alone (a swapped
output index shows), records by the launches and by the persistent sweeps, batch widths 1, 5, 32, 33; (3) the 1024-thread block;
(4) the pow path of the outputs' f; (5) the raw-grid economies with a deep clamped prefix, x̄ against the oracle and Sweep A's p̄
against a numpy pullback (the only check of the clamped prefix's store: those rows carry A = B = 0, so x̄ cannot see it); (6) the
context's state rules; (7) the host layers. Tolerance: cases.close (rel 1e-10 + abs 1e-12 on the largest entry of the reference)
unless stated."""
import numpy as np
import pytest

import cases
from cases import block as _block, close as _close, jacobian_het as _jac, jt as _jt
from conftest import ks_paths, ks_setup

pytestmark = pytest.mark.gpu

WIDTHS = (1, 5, 32, 33)


def _ks_case():
    m, ss, orc = ks_setup(130, 3, 40)
    x = np.ascontiguousarray(ks_paths(m, ss, "x1", 0.05)[0][2:4])
    return m, ss, x, _jac("ks", orc, ss.value, ss.D, x, 3, m.params.γ)


def _wages_case():
    m, ss = cases.hank_economy(80, 3, 40, "one_asset_hank_wages.yaml")
    x = cases.hank_x(ss, m.compspec.T - 1)
    return m, ss, x, _jac("wages", cases.oracle_of(m), ss.value, ss.D, x, 4, m.params.γ)


def _only(yb, outputs):
    """yb with every output but `outputs` zeroed"""
    out = np.zeros_like(yb)
    out[:, list(outputs), :] = yb[:, list(outputs), :]
    return out


def _against_oracle(hb, J, n_het, widths, alone, what, seed=0):
    """hb.vjp_het at every width against J' yb: cotangents on every output, then on each output of `alone` alone"""
    P = J.shape[1]
    for M in widths:
        yb = np.random.default_rng(100 * seed + 10 * M + n_het).standard_normal((P, n_het, M))
        got = hb.vjp_het(yb, n_het)
        assert got.shape == (J.shape[2], P, M)
        _close(got, _jt(J[:n_het], yb), what=f"{what} M={M}")
        for o in alone:
            y1 = _only(yb, [o])
            _close(hb.vjp_het(y1, n_het), _jt(J[:n_het], y1), what=f"{what} M={M}, output {o} alone")


# ---- 1, 2. against the oracle's Jacobian, transposed ----------------------------------------------------------------------
@pytest.mark.parametrize("schedule", ["launch", "xcd"])
def test_vjp_het_is_the_oracle_jacobian_transposed_krusell_smith_130x3_value(hank, oracle_mod, schedule):
    m, ss, x, J = _ks_case()
    hb = _block(hank, m, schedule)
    try:
        hb.set_boundary(ss.value, ss.D)
        hb.set_het_outputs(3)
        hb.primal(x)
        assert hb.stats()["schedule"] == (0 if schedule == "launch" else 1)
        _against_oracle(hb, J, 3, WIDTHS, (2,), f"ks {schedule}")
    finally:
        hb.close()


@pytest.mark.parametrize("schedule", ["launch", "xcd"])
def test_vjp_het_is_the_oracle_jacobian_transposed_sticky_wage_hank_80x3_value_and_uce(hank, oracle_mod, schedule):
    m, ss, x, J = _wages_case()
    hb = _block(hank, m, schedule)
    try:
        assert hb.n_hh == 3
        hb.set_boundary(ss.value, ss.D)
        hb.set_het_outputs(4)
        hb.primal(x)
        _against_oracle(hb, J, 4, WIDTHS, (3, 2), f"wages {schedule}")
        _against_oracle(hb, J, 3, (5, 32), (), f"wages {schedule} n_het=3")        # NX = 1 on a record that holds two outputs
    finally:
        hb.close()


# ---- 3. the 1024-thread block ---------------------------------------------------------------------------------------------
def test_vjp_het_at_sixteen_productivity_states(hank, oracle_mod):
    m, V, D, xhh, orc = cases.shape(40, 16, 10)
    J = _jac(("shape", 40, 16, 10), orc, V, D, xhh, 3, m.params.γ)
    hb = _block(hank, m, "launch")
    try:
        assert hb.n_e == 16
        hb.set_boundary(V, D)
        hb.set_het_outputs(3)
        hb.primal(xhh)
        _against_oracle(hb, J, 3, (1, 5, 32), (2,), "40x16")
    finally:
        hb.close()


# ---- 4. the pow path of hx_f ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,n_het", [("ks", 3), ("hank", 4)])
def test_vjp_het_at_a_curvature_that_takes_pow(hank, oracle_mod, family, n_het):
    m, ss, xhh, orc = cases.economy(family, 1.5)
    J = _jac(("economy", family, 1.5), orc, ss.value, ss.D, xhh, n_het, 1.5)
    hb = _block(hank, m, "launch")
    try:
        hb.set_boundary(ss.value, ss.D)
        hb.set_het_outputs(n_het)
        hb.primal(xhh)
        _against_oracle(hb, J, n_het, (6,), tuple(range(2, n_het)), f"{family} gamma=1.5")
    finally:
        hb.close()


# ---- 5. clamped prefix, top clamp, long segments ----------------------------------------------------------------------------
def pullback_het(grid, Pi, pol, D0, Dseq, lam_w, direct):
    """cases.forward_iteration_pullback generalised to outputs Y_t = sum f_t D_t: lam_w (n_a, n_e, P) = sum_o yb_o,t f_o,t is what
    period t adds to the distribution's cotangent (yb pol for the policy variable alone), direct (n_a, n_e, P) the outputs' direct
    weight on the policy per unit of D_t (yb there; -yb f_c for an output that is not affine in it). -> Δpolicy (n_a, n_e, P)."""
    n_a, n_e, P = pol.shape
    cols = np.arange(n_e)[None, :]
    dD = np.zeros((n_a, n_e))
    out = np.zeros((n_a, n_e, P))
    for t in range(P - 1, -1, -1):
        Dt, Dprev = Dseq[:, :, t], (Dseq[:, :, t - 1] if t > 0 else D0)
        dD = dD + lam_w[:, :, t]
        out[:, :, t] += direct[:, :, t] * Dt
        u = dD @ Pi.T
        m0 = np.searchsorted(grid, pol[:, :, t], side="left")
        interior = (m0 > 0) & (m0 < n_a)
        hi, lo = np.clip(m0, 1, n_a - 1), np.clip(m0, 1, n_a - 1) - 1
        gap = grid[hi] - grid[lo]
        out[:, :, t] += np.where(interior, Dprev * (u[hi, cols] - u[lo, cols]) / gap, 0.0)
        w = (pol[:, :, t] - grid[lo]) / gap
        dD = np.where(m0 == 0, u[0, cols], np.where(m0 >= n_a, u[n_a - 1, cols], (1 - w) * u[lo, cols] + w * u[hi, cols]))
    return out


def _ks_weights(hb, x, gamma, yb):
    """lam_w and direct of pullback_het for Krusell-Smith's three outputs (KD, C, Value = (1+r) c^-gamma) and one cotangent
    column yb (P, 3), from the device's policy, the inputs and the grid"""
    pol = hb.policy_seq()                                                   # (n_a, n_e, P)
    r, w = x[0][None, None, :], x[1][None, None, :]
    cons = (1.0 + r) * hb.a_grid[:, None, None] + w * hb.z_grid[None, :, None] - pol
    f = (1.0 + r) * cons ** (-gamma)
    fc = -gamma * f / cons
    y0, y1, y2 = (yb[:, o][None, None, :] for o in range(3))
    return y0 * pol + y1 * cons + y2 * f, y0 - y1 - y2 * fc


@pytest.mark.parametrize("name", list(cases.EDGE_GRIDS))
def test_vjp_het_on_clamped_prefix_top_clamp_and_long_segments(hank, oracle_mod, name):
    ec = cases.raw_economy(name)
    grid, V, D, x, orc = ec["grid"], ec["V"], ec["D"], ec["x"], ec["orc"]
    gamma = ec["args"][4]
    P = x.shape[1]
    J = _jac(("raw", name), orc, V, D, x, 3, gamma)
    rng = np.random.default_rng(43)
    hb = cases.raw_block(hank, ec["args"], "launch")
    try:
        hb.set_boundary(V, D)
        hb.set_het_outputs(3)
        hb.primal(x)
        cases.check_edges(name, grid, hb.policy_seq().transpose(2, 0, 1))
        pol, Dseq = hb.policy_seq(), hb.dist_seq()
        D0 = np.asarray(D).reshape(hb.n_a, hb.n_e, order="F")
        for M in cases.EDGE_WIDTHS:
            for alone in (None, 2):
                what = f"{name} M={M}" + ("" if alone is None else f", output {alone} alone")
                yb = rng.standard_normal((P, 3, M))
                if alone is not None:
                    yb = _only(yb, [alone])
                _close(hb.vjp_het(yb, 3), _jt(J, yb), what=what)
                pbar = hb.policy_cotangent_seq(M)
                for k in sorted({0, M - 1}):
                    lam_w, direct = _ks_weights(hb, x, gamma, yb[:, :, k])
                    _close(pbar[..., k], pullback_het(hb.a_grid, hb.Pi, pol, D0, Dseq, lam_w, direct), rel=1e-11, ab=0.0, what=f"{what} pbar column {k}")
    finally:
        hb.close()


# ---- 6. state -------------------------------------------------------------------------------------------------------------
def test_state_rules(hank, oracle_mod):
    import torch
    from hank_amd.hip import HANK_ERR_BAD_ARG, HANK_ERR_NOT_READY
    m, ss, x, J = _ks_case()
    P = x.shape[1]
    rng = np.random.default_rng(2)
    yb = rng.standard_normal((P, 3, 32))
    hb = _block(hank, m, "launch")
    try:
        def code(fn):
            with pytest.raises(hank.HankHIPError) as e:
                fn()
            return e.value.code
        hb.set_boundary(ss.value, ss.D)
        hb.primal(x)
        assert code(lambda: hb.vjp_het(yb, 3)) == HANK_ERR_NOT_READY                  # three outputs before the declaration
        assert code(lambda: hb.vjp_het(np.zeros((P, 4, 2)), 4)) == HANK_ERR_BAD_ARG   # UCE on Krusell-Smith
        assert code(lambda: hb.vjp_het(np.zeros((P, 1, 0)), 1)) == HANK_ERR_BAD_ARG   # M = 0
        # n_het <= 2: hank_vjp's path, its bits
        for n_het in (1, 2):
            a, pa = hb.vjp_het(yb[:, :n_het, :], n_het), hb.policy_cotangent_seq(32)
            b, pb = hb.vjp(yb[:, :n_het, :], n_het), hb.policy_cotangent_seq(32)
            assert np.array_equal(a, b) and np.array_equal(pa, pb)
        hb.set_het_outputs(3)
        # the tangent readers are served the same bits before and after
        y = rng.standard_normal((2, P, 4))
        hb.jvp(y)
        dpol0, het0 = hb.dpolicy_seq(4), hb.het_outputs(3, y)
        alloc0 = hb.stats()["tangent_workspaces_allocated"]
        xb = hb.vjp_het(yb, 3)
        assert hb.stats()["tangent_workspaces_allocated"] == alloc0                   # the width's workspace is hank_vjp's
        _close(xb, _jt(J, yb))
        pb = hb.policy_cotangent_seq(32)
        assert np.array_equal(hb.dpolicy_seq(4), dpol0)
        het1 = hb.het_outputs(3, y)                                                   # (between two vjp_het calls)
        assert np.array_equal(het1[0], het0[0]) and np.array_equal(het1[1], het0[1])
        # the same input, the same bits; zero in, exact zeros out
        assert np.array_equal(hb.vjp_het(yb, 3), xb) and np.array_equal(hb.policy_cotangent_seq(32), pb)
        z = hb.vjp_het(np.zeros_like(yb), 3)
        assert not z.any() and not hb.policy_cotangent_seq(32).any()
        t = hb.last_vjp_timings()
        assert t["sweep_a"]["ms"] > 0 and t["sweep_b"]["ms"] > 0 and t["sweep_a"]["launches"] == P
        # hank_vjp on the same workspace in between, and its refusal, are as before
        _close(hb.vjp(yb[:, :2, :], 2), _jt(J[:2], yb[:, :2, :]))
        with pytest.raises(hank.HankHIPError, match="not affine"):
            hb.vjp(yb, 3)
        assert np.array_equal(hb.vjp_het(yb, 3), xb)
        # the device-pointer form: bit for bit
        d_in = torch.from_numpy(np.asfortranarray(yb).reshape(-1, order="F").copy()).cuda()
        d_out = torch.empty(2 * P * 32, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        hb.vjp_het_dev(3, d_in.data_ptr(), 32, d_out.data_ptr())
        hb.sync()
        assert np.array_equal(d_out.cpu().numpy().reshape((2, P, 32), order="F"), xb)
        # a stale f / f_c record: another path, its own Jacobian
        x2 = np.ascontiguousarray(x * np.array([[1.1], [0.99]]))
        J2 = _jac("ks-x2", ks_setup(130, 3, 40)[2], ss.value, ss.D, x2, 3, m.params.γ)
        assert np.abs(J2 - J).max() > 1e-4 * np.abs(J).max()
        hb.primal(x2)
        assert code(lambda: hb.policy_cotangent_seq(32)) == HANK_ERR_NOT_READY
        _close(hb.vjp_het(yb, 3), _jt(J2, yb), what="after a primal at another path")
        hb.primal(x)
        assert np.array_equal(hb.vjp_het(yb, 3), xb)
        # a new boundary
        hb.set_boundary(ss.value * 1.0001, ss.D)
        assert code(lambda: hb.vjp_het(yb, 3)) == HANK_ERR_NOT_READY
        assert code(lambda: hb.policy_cotangent_seq(32)) == HANK_ERR_NOT_READY
    finally:
        hb.close()


# ---- 7. host layers -------------------------------------------------------------------------------------------------------
def test_linearized_function_sticky_wage_hank(hank, oracle_mod):
    m, ss = cases.hank_economy(80, 3, 40, "one_asset_hank_wages.yaml")
    P = m.compspec.T - 1
    keys = hank.vars_of_type(m, "endogenous")
    x0 = np.tile(np.array([ss.vars[k] for k in keys]), P) * (1 + 1e-4 * np.random.default_rng(0).standard_normal(len(keys) * P))
    lin = hank.LinearizedFunction(x0, {"ei": 0.0025 * 0.6 ** np.arange(P)}, m, ss, ss)
    assert lin._n_out == 4
    n = lin.x.size
    rng = np.random.default_rng(1)
    y, yb = rng.standard_normal((n, 3)), rng.standard_normal((n, 4))
    JTyb = lin.vjp_het(yb)
    lhs, rhs = yb.T @ lin.jvp(y), JTyb.T @ y
    print(f"<ybar, J y> vs <J' ybar, y>: {np.max(np.abs(lhs - rhs)) / np.abs(lhs).max():.3e}")
    assert np.max(np.abs(lhs - rhs)) <= 1e-11 * np.abs(lhs).max()
    assert np.array_equal(lin.as_linear_operator().rmatmat(yb), JTyb)
    assert np.array_equal(hank.VJP(lin, lin.x, yb), JTyb)


def test_linearized_function_goods_market_hank_takes_hank_vjp(hank, oracle_mod):
    m, ss = cases.hank_economy(80, 3, 40, "one_asset_hank_goods.yaml")
    P = m.compspec.T - 1
    keys = hank.vars_of_type(m, "endogenous")
    x0 = np.tile(np.array([ss.vars[k] for k in keys]), P) * (1 + 1e-4 * np.random.default_rng(0).standard_normal(len(keys) * P))
    lin = hank.LinearizedFunction(x0, {"ei": 0.0025 * 0.6 ** np.arange(P)}, m, ss, ss)
    assert lin._n_out == 2
    yb = np.random.default_rng(1).standard_normal((lin.x.size, 4))
    assert np.array_equal(lin.vjp_het(yb), lin.vjp(yb))
