"""One end-to-end run of the borrowing-limit path through the host layers (one-asset HANK 130x3, T = 40, at a steady state whose limit
lies inside the wealth grid: examples/solve_hank.py's `_crunch_setup`): NewtonRaphsonHANK with `borrow_path` converges on the nonlinear
transition, and for a small shock the converged deviation agrees with the first-order response -J̅⁻¹ (∂F/∂amin) damin assembled from
SteadyStateJacobian.borrow_jacobian (hank_fake_news_borrow) to within 1e-2 of the deviation's largest entry — a smallness-of-shock
condition (the gap is second order in the shock), not a parity claim, the bound of tests/test_gpu_shock_newton.py.

The gradient of ½‖F‖² with respect to the path from ONE hank_vjp_borrow against a central difference of the DEVICE's own level, step
h = 1e-6, to 1e-5 of the gradient's largest entry: the difference's truncation is O(h²) of a smooth merit (the limits sit strictly inside
a bracket, and the test asserts that the recorded constrained set is the same at amin ± h), and its rounding is eps·½‖F‖²/h, some
1e-18 at ‖F‖ ≈ 1e-4, against a gradient of the order of ‖F‖ itself."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZE, RHO, STEP = 1e-4, 0.8, 1e-6


def test_newton_under_a_borrowing_limit_path_the_linear_response_and_the_gradient(hank, oracle_mod):
    import cases
    from examples.solve_hank import _crunch_setup
    from hank_amd.SteadyStateJacobian import borrow_jacobian
    h, m, ss, keys, x0, exog, damin, a, k = _crunch_setup(130, 3, 40, SIZE, RHO, "one_asset_hank.yaml")
    P, bc = m.compspec.T - 1, m.params.borrow_cons
    assert k >= 3 and a[k - 1] < bc < bc + SIZE < a[k]                  # grid points below the limit; the path stays inside its bracket
    hb = hank.household_block(m)
    try:
        J = hank.getSteadyStateJacobian(ss, m)
        lin0 = hank.LinearizedFunction(x0, exog, m, ss, ss)
        assert np.linalg.norm(lin0.Fx) < 1e-8                      # the steady state solves the system without a shock
        Ja = borrow_jacobian(lin0.hb, lin0._n_out)
        dF = lin0.residual_borrow_jacobian(Ja)
        assert np.abs(dF).max() > 1e-3                             # (points below the limit: the derivative is not the kink's zero)
        cases.close(dF[:, :3], lin0.jvp_borrow(np.eye(P)[:, :3]), what="∂F/∂amin from borrow_jacobian against hank_jvp_borrow")
        dx_lin = -np.linalg.solve(np.asarray(J), dF @ damin)
        x = hank.NewtonRaphsonHANK(x0, J, exog, m, ss, ss, ε=1e-9, borrow_path=bc + damin)
        lin = hank.LinearizedFunction(x, exog, m, ss, ss, borrow_path=bc + damin)
        res = float(np.linalg.norm(lin.Fx))
        dev = x - x0
        gap, top = float(np.max(np.abs(dev - dx_lin))), float(np.max(np.abs(dev)))
        print(f"residual {res:.3e}; deviation's largest entry {top:.3e}; nonlinear minus linear {gap:.3e} ({gap / top:.3e} of it); "
              f"Newton iterations {hank.NewtonRaphsonHANK.iterations}")
        assert res < 1e-8
        assert top > 1e-7 and gap <= 1e-2 * top
        assert np.array_equal(lin.hb.borrow_path, bc + damin)
        # the gradient at the starting point, where F != 0 under the path, against the device's own level
        path = bc + damin
        at = hank.LinearizedFunction(x0, exog, m, ss, ss, borrow_path=path)
        g = at.vjp_borrow(at.Fx)
        cases.close(g, at.jvp_borrow(np.eye(P)).T @ at.Fx, what="hank_vjp_borrow against the columns of hank_jvp_borrow")
        C0 = hb.policy_seq() == path[None, None, :]
        for t in (0, 1, P - 1):
            f = []
            for sgn in (1.0, -1.0):
                p = path.copy()
                p[t] += sgn * STEP
                F = hank.LinearizedFunction(x0, exog, m, ss, ss, borrow_path=p).Fx
                assert np.array_equal(hb.policy_seq() == p[None, None, :], C0), t      # the same constrained set: a condition on the inputs
                f.append(0.5 * float(F @ F))
            fd = (f[0] - f[1]) / (2 * STEP)
            print(f"amin_bar[{t}] = {g[t]:.10e}, central difference {fd:.10e}")
            assert abs(g[t] - fd) <= 1e-5 * np.abs(g).max(), (t, g[t], fd)
        assert np.abs(g).max() > 1e-7
        # a linearisation without a path on the same context clears it and restores its own record
        assert np.linalg.norm(hank.LinearizedFunction(x0, exog, m, ss, ss).Fx) < 1e-8 and lin.hb.borrow_path is None
    finally:
        hb.set_borrow_path(None)
