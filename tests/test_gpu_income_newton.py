"""One end-to-end run of the income path through the host layers (one-asset HANK 130x3, T = 40): NewtonRaphsonHANK with `income_path`
converges on the nonlinear transition under a budget-neutral transfer to the lowest productivity state, and for a small transfer the
converged deviation agrees with the first-order response -J̅⁻¹ (∂F/∂y) vec(y) assembled from SteadyStateJacobian.income_jacobian
(hank_fake_news_income) to within 1e-2 of the deviation's largest entry — a smallness-of-shock condition (the gap is second order in
the transfer), not a parity claim. `LinearizedFunction.vjp_income` is the transpose of `jvp_income`."""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

SIZE, RHO = 1e-3, 0.8


def test_newton_under_an_income_path_and_the_linear_response(hank, oracle_mod):
    from hank_amd import incidence
    from hank_amd.SteadyStateJacobian import income_jacobian
    m, ss = cases.hank_economy(130, 3, 40)
    P = m.compspec.T - 1
    n_a, n_e = np.asarray(ss.value).shape
    keys = hank.vars_of_type(m, "endogenous")
    x0 = np.tile(np.array([ss.vars[k] for k in keys]), P)
    exog = {"ei": np.zeros(P)}
    mass = np.asarray(ss.D).reshape((n_a, n_e), order="F").sum(axis=0)
    y = incidence.redistribution(np.tile(mass[:, None], (1, P)), [0], SIZE, RHO)
    assert np.abs(mass @ y).max() < 1e-18
    hb = hank.household_block(m)
    try:
        J = hank.getSteadyStateJacobian(ss, m)
        lin0 = hank.LinearizedFunction(x0, exog, m, ss, ss)
        assert np.linalg.norm(lin0.Fx) < 1e-8                      # the steady state solves the system without a shock
        Jy = income_jacobian(lin0.hb, lin0._n_out)
        dF = lin0.residual_income_jacobian(Jy)                     # (n, n_e P), column e + n_e s
        unit = np.eye(n_e * P)[:, :4].reshape((n_e, P, 4), order="F")
        cols = lin0.jvp_income(unit)                               # ∂F/∂y's first columns, by hank_jvp_income at the same record
        cases.close(dF[:, :4], cols, what="∂F/∂y from income_jacobian against hank_jvp_income")
        rng = np.random.default_rng(0)
        yb, dy = rng.standard_normal((len(x0), 3)), rng.standard_normal((n_e, P, 3))
        lhs, rhs = np.einsum("rm,rn->mn", yb, lin0.jvp_income(dy)), np.einsum("etm,etn->mn", lin0.vjp_income(yb), dy)
        scale = np.einsum("rm,rn->mn", np.abs(yb), np.abs(lin0.jvp_income(dy)))
        assert np.all(np.abs(lhs - rhs) <= 1e-10 * scale), np.max(np.abs(lhs - rhs) / scale)
        dx_lin = -np.linalg.solve(np.asarray(J), dF @ y.reshape(-1, order="F"))
        x = hank.NewtonRaphsonHANK(x0, J, exog, m, ss, ss, ε=1e-9, income_path=y)
        lin = hank.LinearizedFunction(x, exog, m, ss, ss, income_path=y)
        res = float(np.linalg.norm(lin.Fx))
        dev = x - x0
        gap, top = float(np.max(np.abs(dev - dx_lin))), float(np.max(np.abs(dev)))
        print(f"residual {res:.3e}; deviation's largest entry {top:.3e}; nonlinear minus linear {gap:.3e} ({gap / top:.3e} of it); "
              f"Newton iterations {hank.NewtonRaphsonHANK.iterations}")
        assert res < 1e-8
        assert top > 1e-7 and gap <= 1e-2 * top
        assert np.array_equal(lin.hb.income_path, y)
        # a linearisation without a path on the same context clears it and restores its own record
        assert np.linalg.norm(hank.LinearizedFunction(x0, exog, m, ss, ss).Fx) < 1e-8 and lin.hb.income_path is None
        with pytest.raises(ValueError):
            hank.LinearizedFunction(x0, exog, m, ss, ss, income_path=y, discount_path=np.full(P, m.params.β))
    finally:
        hb.set_income_path(None)
