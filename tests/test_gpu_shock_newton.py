"""One end-to-end run of the discount-factor path through the host layers (one-asset HANK 130x3, T = 40): NewtonRaphsonHANK with
`discount_path` converges on the nonlinear transition, and for a small shock the converged deviation agrees with the first-order
response -J̅⁻¹ (∂F/∂beta) dbeta assembled from SteadyStateJacobian.shock_jacobian (hank_fake_news_shock) to within 1e-2 of the
deviation's largest entry — a smallness-of-shock condition (the gap is second order in the shock), not a parity claim."""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

SIZE, RHO = 1e-4, 0.8


def test_newton_under_a_discount_path_and_the_linear_response(hank, oracle_mod):
    from hank_amd.SteadyStateJacobian import shock_jacobian
    m, ss = cases.hank_economy(130, 3, 40)
    P = m.compspec.T - 1
    keys = hank.vars_of_type(m, "endogenous")
    x0 = np.tile(np.array([ss.vars[k] for k in keys]), P)
    exog = {"ei": np.zeros(P)}
    dbeta = m.params.β * SIZE * RHO ** np.arange(P)
    hb = hank.household_block(m)
    try:
        J = hank.getSteadyStateJacobian(ss, m)
        lin0 = hank.LinearizedFunction(x0, exog, m, ss, ss)
        assert np.linalg.norm(lin0.Fx) < 1e-8                      # the steady state solves the system without a shock
        Jb = shock_jacobian(lin0.hb, lin0._n_out)
        dF = lin0.residual_shock_jacobian(Jb)
        close_cols = lin0.jvp_shock(np.eye(P)[:, :3])              # ∂F/∂beta's first columns, by hank_jvp_shock at the same record
        cases.close(dF[:, :3], close_cols, what="∂F/∂beta from shock_jacobian against hank_jvp_shock")
        dx_lin = -np.linalg.solve(np.asarray(J), dF @ dbeta)
        x = hank.NewtonRaphsonHANK(x0, J, exog, m, ss, ss, ε=1e-9, discount_path=m.params.β + dbeta)
        lin = hank.LinearizedFunction(x, exog, m, ss, ss, discount_path=m.params.β + dbeta)
        res = float(np.linalg.norm(lin.Fx))
        dev = x - x0
        gap, top = float(np.max(np.abs(dev - dx_lin))), float(np.max(np.abs(dev)))
        print(f"residual {res:.3e}; deviation's largest entry {top:.3e}; nonlinear minus linear {gap:.3e} ({gap / top:.3e} of it); "
              f"Newton iterations {hank.NewtonRaphsonHANK.iterations}")
        assert res < 1e-8
        assert top > 1e-7 and gap <= 1e-2 * top
        assert np.array_equal(lin.hb.discount_path, m.params.β + dbeta)
        # a linearisation without a path on the same context clears it and restores its own record
        assert np.linalg.norm(hank.LinearizedFunction(x0, exog, m, ss, ss).Fx) < 1e-8 and lin.hb.discount_path is None
    finally:
        hb.set_discount_path(None)
