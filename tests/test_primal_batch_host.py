"""The host side of hank_primal_batch, without a device: the step rule `backtrack` as a pure function, NewtonRaphsonHANK's
step="backtrack" loop on a toy map through a fake `residuals_batch`, and the binding's array layouts against a fake library that
reads and writes the C ABI's offsets ((n_hh, P, K), (P, n_het, K), (G, P, K), column-major)."""
import ctypes as C

import numpy as np
import pytest


def test_backtrack_accepts_the_full_step_that_halves_the_norm(hank):
    from hank_amd.NewtonRaphson import backtrack
    assert backtrack([0.25, 0.5, 0.7], 1.0) == 0          # ‖F‖ halves: ‖F‖² quarters


def test_backtrack_finds_the_first_passing_trial(hank):
    from hank_amd.NewtonRaphson import backtrack
    c1 = 1e-4
    assert backtrack([4.0, 1.5, 0.9, 0.1], 1.0, c1) == 2
    # the bound is Armijo's, (1 - 2 c1 2^-j) f0², per trial: a trial just above its own bound fails, just below passes
    f0 = 2.0
    edge = lambda j, eps: (1.0 - 2.0 * c1 * 2.0 ** -j) * f0 + eps          # noqa: E731
    assert backtrack([edge(0, 1e-9), edge(1, -1e-9)], f0, c1) == 1
    assert backtrack([edge(0, 1e-9), edge(1, 1e-9), edge(2, 0.0)], f0, c1) == 2


def test_backtrack_falls_back_to_the_smallest_norm_below_f0(hank):
    from hank_amd.NewtonRaphson import backtrack
    c1 = 0.4           # a demanding rule: trial j must reach (1 - 0.8 2^-j) f0²
    assert backtrack([0.9, 0.7, 0.85], 1.0, c1) == 1      # bounds 0.2, 0.6, 0.8: none passes; the smallest is trial 1, below f0²


def test_backtrack_raises_when_nothing_decreases(hank):
    from hank_amd.NewtonRaphson import StepRuleError, backtrack
    with pytest.raises(StepRuleError):
        backtrack([1.0, 1.2, 3.0], 1.0)
    with pytest.raises(StepRuleError):
        backtrack([np.inf, np.nan], 1.0)


def test_backtrack_skips_entries_that_are_not_finite(hank):
    from hank_amd.NewtonRaphson import backtrack
    assert backtrack([np.inf, np.nan, 0.5], 1.0) == 2
    assert backtrack([np.inf, 0.99999, np.inf], 1.0, 0.4) == 1      # (the fallback skips them too)


def test_newton_backtrack_converges_where_the_full_step_diverges(hank, monkeypatch):
    """F(x) = (atan x1, atan x2) from x0 = (3, -2.5): Newton's full step overshoots further every time (|x| > 1.39 diverges),
    halved steps converge. y_Iteration and residuals_batch are replaced by the map's own exact ones."""
    import hank_amd.NewtonRaphson as NR

    F = np.arctan
    calls = {"batch": 0, "cols": []}

    def fake_y(J, x, y0, *a, **kw):
        fake_y.last_Fx = F(x)
        return F(x) * (1.0 + x * x)                        # J(x)⁻¹ F(x), J = diag(1 / (1 + x²))

    def fake_batch(xs, *a, **kw):
        calls["batch"] += 1
        calls["cols"].append(xs.shape[1])
        return F(xs)

    monkeypatch.setattr(NR, "y_Iteration", fake_y)
    monkeypatch.setattr(NR, "residuals_batch", fake_batch)
    x0 = np.array([3.0, -2.5])
    with np.errstate(over="ignore", invalid="ignore"):
        x_full = NR.NewtonRaphsonHANK(x0, None, {}, None, None, None, ε=1e-12)
    assert not np.all(np.abs(x_full) < 1.0), x_full                     # the full step has left for infinity
    x = NR.NewtonRaphsonHANK(x0, None, {}, None, None, None, ε=1e-12, step="backtrack", n_trial=6)
    sizes, norms = NR.NewtonRaphsonHANK.step_sizes, NR.NewtonRaphsonHANK.residual_norms
    assert np.max(np.abs(x)) < 1e-12
    assert sizes[0] < 1.0 and all(a in [2.0 ** -j for j in range(6)] for a in sizes)
    assert all(b <= a for a, b in zip(norms, norms[1:])), norms
    assert calls["batch"] <= len(sizes) and set(calls["cols"]) == {6}   # ONE batch of n_trial columns per outer iteration
    with pytest.raises(ValueError):
        NR.NewtonRaphsonHANK(x0, None, {}, None, None, None, step="armijo")


class _FakeLib:
    """hank_primal_batch of the C ABI on host memory: agg[t + P (o + n_het k)] = 1000 k + 100 o + t + xhh[0 + n_hh (t + P k)],
    policy[g + G (t + P k)] = k + 0.001 (g + G t), status[k] = 0"""

    def __init__(self, n_hh, P, G):
        self.n_hh, self.P, self.G = n_hh, P, G

    def hank_primal_batch(self, ctx, n_het, xp, K, ap, pp, sp):
        for k in range(K):
            for t in range(self.P):
                for o in range(n_het):
                    ap[t + self.P * (o + n_het * k)] = 1000.0 * k + 100.0 * o + t + xp[self.n_hh * (t + self.P * k)]
                if pp:
                    for g in range(self.G):
                        pp[g + self.G * (t + self.P * k)] = k + 0.001 * (g + self.G * t)
            sp[k] = 0
        return 0


def test_the_bindings_layouts_are_the_c_abis(hank):
    hb = object.__new__(hank.HouseholdBlock)
    hb.n_hh, hb.P, hb.n_a, hb.n_e, hb.G = 3, 4, 5, 2, 10
    hb._ctx, hb._lib = C.c_void_p(), _FakeLib(3, 4, 10)
    K, n_het = 3, 2
    x = np.random.default_rng(0).standard_normal((3, 4, K))
    for xin in (x, np.ascontiguousarray(x), np.asfortranarray(x)):                 # any memory order comes in as (n_hh, P, K) column-major
        aggs, status, pol = hb.primal_batch(xin, n_het=n_het, policy=True)
        assert aggs.shape == (4, n_het, K) and aggs.strides == (8, 32, 64) and status.dtype == np.int32 and status.shape == (K,)
        assert pol.shape == (5, 2, 4, K) and pol.strides == (8, 40, 80, 320)
        for k in range(K):
            for o in range(n_het):
                assert np.array_equal(aggs[:, o, k], 1000.0 * k + 100.0 * o + np.arange(4) + x[0, :, k])
            g = np.arange(10).reshape((5, 2), order="F")
            for t in range(4):
                assert np.array_equal(pol[:, :, t, k], k + 0.001 * (g + 10 * t))
    one = hb.primal_batch(x[:, :, 1])                                              # one path (n_hh, P): a batch of one, no policies
    assert len(one) == 2 and one[0].shape == (4, 1, 1) and np.array_equal(one[0][:, 0, 0], np.arange(4) + x[0, :, 1])
    hb._ctx = None                                                                  # (nothing to destroy)
