"""The device's verdict on work already enqueued has one owner in the host library: the caller says whose
work the error word speaks about. An error on the record (hank_primal*, hank_jvp, hank_check, and what an asynchronous sweep left
pending) takes the record AND the tangent batch with it, whichever form of the entry ran; an error of a call's own work (the
granular steps, hank_vfi) leaves both exactly as they were; the fixed points' fallback goes through the sweeps' decision.
Economy of the suite's error tests: KS 50x2, T = 100, x at the steady state, N = 3; the bad boundary scales one row of the
terminal value, which un-sorts the EGM knots of the last period ("period 99")."""
import numpy as np
import pytest
import torch

from cases import block
from conftest import ks_paths, ks_setup

pytestmark = pytest.mark.gpu
P, N = 99, 3


def economy():
    m, ss, _ = ks_setup(50, 2, 100)
    x, _ = ks_paths(m, ss, "x0")
    bad = np.array(ss.value, copy=True)
    bad[7, :] *= 1e-4
    y = np.random.default_rng(3).standard_normal((2, P, N))
    return m, ss, x[2:4], y, bad


def on_device(a):
    return torch.from_numpy(np.asfortranarray(a).reshape(-1, order="F").copy()).to(torch.device("cuda", 0))


def refused(hank, call):
    with pytest.raises(hank.HankHIPError) as ei:
        call()
    assert ei.value.code == hank.hip.HANK_ERR_NOT_READY, ei.value


@pytest.mark.parametrize("sched", ["launch", None])
def test_a_failed_asynchronous_dual_pass_leaves_no_batch(hank, sched):
    """hank_primal_jvp_dev at a boundary that raises HANK_ERR_KNOTS: hank_check reports it, and the partials of the failed primal
    are nobody's — hank_get_dpolicy_seq and hank_get_grid_aggregates answer HANK_ERR_NOT_READY, as after the host-pointer
    hank_primal_jvp. (Before the verdict had one owner the _dev sequence kept the batch current and dpolicy_seq answered HANK_OK.)

    No other test drives a Dual pass at a model error, so the tangent halves' indexing was read first. Unsorted knots cannot take
    the bracket index out of [0, n_a - 2]: egm_Y (hank_kernels.h) ends every branch with i = 0 (x < s[0]), i = n - 2 (x > s[n-1])
    or `i = lo < 0 ? 0 : (lo > n - 2 ? n - 2 : lo)` behind a bisection whose probes `mid` lie strictly between lo >= -1 and hi <= n
    and whose gallops stop at `q >= n` / `q < 0`; the guess is clamped first (`p = guess < n - 1 ? guess : n - 2`).
    launch schedule: tan_back_body (k_fused_back) reads `bi = R.ib[off]` — that i — and gathers `col[bi * N]`, `col[(bi + 1) * N]`
    of an [n_a][N] column. Persistent schedule: k_xdual_back loads the rows `rb + q`, `rb + q + 1` with
    `q = guess < 0 ? 0 : (guess < na - 1 ? guess : na - 2)` and `rb + o.ib`, `rb + o.ib + 1` with o.ib that same i. The forward
    halves read the lottery's segment offsets, which k_lottery fills for every r in [0, n] with source indices in [0, n] whether or
    not the policy is monotone (each r is crossed by some step prev < r <= cur, or by the last source's tail), so every gather
    `j < st[r]` stays inside the column. The Float64 halves run at this boundary in test_knots_error_from_the_sweep and
    test_forced_persistent_sweeps_error_surface."""
    m, ss, x, y, bad = economy()
    d_x, d_y = on_device(x), on_device(y)
    hb = block(hank, m, sched)
    hb.set_boundary(bad, ss.D)
    hb.primal_jvp_dev(d_x.data_ptr(), d_y.data_ptr(), N)
    with pytest.raises(hank.KnotsNotSortedError, match="period 99"):
        hb.check()
    refused(hank, lambda: hb.dpolicy_seq(N))
    refused(hank, lambda: hb.grid_aggregates(N))
    hb.check()                                           # reported once
    hb.set_boundary(ss.value, ss.D)
    agg = hb.primal(x)                                   # the context works
    assert np.all(np.isfinite(agg)) and hb.jvp(y).shape == (P, N) and hb.dpolicy_seq(N).shape == (50, 2, P, N)
    assert hb.stats()["fallbacks"] == 0
    hb.close()
    # the host-pointer form on a fresh context: the same two refusals
    hb = block(hank, m, sched)
    hb.set_boundary(bad, ss.D)
    with pytest.raises(hank.KnotsNotSortedError, match="period 99"):
        hb.primal_jvp(x, y)
    refused(hank, lambda: hb.dpolicy_seq(N))
    refused(hank, lambda: hb.grid_aggregates(N))
    hb.set_boundary(ss.value, ss.D)
    assert np.array_equal(hb.primal(x), agg)
    hb.close()


def test_a_calls_own_error_leaves_the_record_and_the_batch_alone(hank):
    """a granular step and a value iteration that raise, between a hank_jvp and its readers: the policy partials are the kept array
    bit for bit and hank_jvp runs again, with the same bits, without a new hank_primal."""
    m, ss, x, y, bad = economy()
    r, w = ss.vars["r"], ss.vars["w"]
    hb = block(hank, m, None)
    hb.set_boundary(ss.value, ss.D)
    hb.primal(x)
    d0 = hb.jvp(y)
    dpol0 = hb.dpolicy_seq(N)
    with pytest.raises(hank.KnotsNotSortedError, match="sorted"):
        hb.backward_step(bad, [r, w])
    assert np.array_equal(hb.dpolicy_seq(N), dpol0)
    assert np.array_equal(hb.jvp(y), d0)
    with pytest.raises((hank.DomainError, hank.KnotsNotSortedError)):
        hb.vfi(np.ones((50, 2)), [0.01, -50.0], 1e-11)
    assert np.array_equal(hb.dpolicy_seq(N), dpol0)
    assert np.array_equal(hb.jvp(y), d0)
    assert hb.calls["primal"] == 1 and hb.stats()["fallbacks"] == 0
    hb.close()


def test_a_pending_sweep_error_is_reported_by_the_next_call_scoped_entry(hank):
    """hank_primal_dev at the bad boundary, never checked: the granular step that follows reports the SWEEP's error (its message
    names the period) instead of overwriting the error word, the error counts against the record, and it is reported once."""
    m, ss, x, y, bad = economy()
    r, w = ss.vars["r"], ss.vars["w"]
    d_x = on_device(x)
    hb = block(hank, m, None)
    hb.set_boundary(bad, ss.D)
    hb.primal_dev(d_x.data_ptr())
    with pytest.raises(hank.KnotsNotSortedError, match="period 99"):
        hb.backward_step(ss.value, [r, w])
    refused(hank, lambda: hb.jvp(y))
    v, pol = hb.backward_step(ss.value, [r, w])
    assert np.all(np.isfinite(v)) and np.all(np.isfinite(pol))
    hb.close()


def test_forced_schedule_fixed_point_fails_loudly(hank):
    """the fixed points' fallback is the sweeps' decision: where the schedule was forced, a persistent value iteration whose group
    did not form is reported and the context stays where it was (the other half of test_steady_state_fixed_points_fall_back)."""
    m, ss, _ = ks_setup(130, 3, 20)
    xv = dict(ss.vars)
    hb = block(hank, m, "xcd", HANK_XFAULT="placement:fixedpoint")
    with pytest.raises(hank.HankHIPError, match="persistent value iteration") as ei:
        hb.vfi(np.ones((130, 3)), [xv["r"], xv["w"]], 1e-11)
    assert ei.value.code == hank.hip.HANK_ERR_SWEEP
    st = hb.stats()
    assert st["fallbacks"] == 0 and st["schedule"] == 1
    hb.close()


def test_a_fixed_point_that_falls_back_still_reports_the_lottery_error(hank):
    """hank_stationary_dist builds the lottery of the caller's policy in FRONT of its persistent launch, and only that kernel raises
    "not monotone". When the launch's group does not form (HANK_XFAULT=placement:fixedpoint) the context moves to the launches, which
    do not build the lottery again: the error taken with the launch's verdict is still the call's answer, as on a context that is on
    the launches from the start. The policy: the steady state's, with row 60 replaced by row 10 (a lower bracket than row 59's)."""
    m, ss, _ = ks_setup(130, 3, 20)
    grid = m.heterogeneity["wealth"].grid
    pol = np.array(ss.policies["KD"], copy=True)
    pol[60, :] = pol[10, :]
    assert np.all(np.searchsorted(grid, pol[60]) < np.searchsorted(grid, pol[59]))       # (the brackets, not just the values, step down)
    for sched, env, fallbacks in (("launch", {}, 0), (None, {"HANK_XFAULT": "placement:fixedpoint"}, 1)):
        hb = block(hank, m, sched, **env)
        with pytest.raises(hank.HankHIPError, match="not monotone") as ei:
            hb.stationary_dist(pol, max_iter=50)         # (two checks: a lottery that is no transition need not converge)
        assert ei.value.code == hank.hip.HANK_ERR_NONMONOTONE
        assert hb.stats()["fallbacks"] == fallbacks
        D, _ = hb.stationary_dist(ss.policies["KD"])         # reported once: the context serves the next call
        assert abs(D.sum() - 1.0) < 1e-12
        hb.close()
