"""hank_ss_jvp / hank_ss_vjp on the MI355X: derivatives of the steady state's household objects (V_ss, a'_ss, D_ss and the
aggregates) in the household prices, against the dense reference of tests/ss_diff_cases.py (the CPU oracle's operators and direct
solves, pinned by tests/test_ss_diff_host.py). (1) JVP parity; (2) VJP parity; (3) the transpose identity between the two device
entries (never counted as parity); (4) state rules; (5) the cap, bits, records of both schedules; (6) find_ss with the implicit
price Jacobian.

Tolerance, derived: a loop stopped on relative increments <= tol sits within 10 tol / (1 - rho) of its limit (S.bound), on top of
the suite's rel 1e-10 + abs 1e-12 (cases.close); tol = 1e-13, rho = rho(B_V) for value and policy, max(rho(B_V), |lambda_2(Lam)|)
for the distribution, the aggregates and everything transposed. Every loop runs under max_iter = 20 000."""
import ctypes

import numpy as np
import pytest

import cases
import ss_diff_cases as S
from conftest import ROOT

pytestmark = pytest.mark.gpu


def _ctx(hank, name, schedule=None, primal=True, declare=True):
    c = S.case(name)
    hb = cases.raw_block(hank, c["args"], schedule)
    hb.set_boundary(c["V"], c["D"])
    if declare:
        hb.set_het_outputs(c["n_het"])
    if primal:
        hb.primal(np.tile(c["x"][:, None], (1, hb.P)))
    return hb, c


def _rel(c, dist):
    r = c["ref"]
    return 1e-10 + S.bound(max(r["rhoV"], r["rhoD"]) if dist else r["rhoV"])


def _flat(a):
    """(n_a, n_e, N) -> (G, N), pt = e n_a + a"""
    return a.reshape((-1, a.shape[2]), order="F")


# ---- 1. JVP parity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 3, 4, 33])
@pytest.mark.parametrize("name", S.NAMES)
def test_ss_jvp_matches_the_dense_solve(hank, oracle_mod, name, N):
    """every economy, one and two directions per lane, the gather and the source-stationary forward form (N = 33: one wave per
    row), every count of outputs the family allows: dagg, dV, dpol, dD, and 1'dD"""
    hb, c = _ctx(hank, name)
    try:
        r, n_hh = c["ref"], len(c["x"])
        dx = np.random.default_rng(100 + N).standard_normal((n_hh, N))
        for n_het in range(1, c["n_het"] + 1):
            dagg, dV, dpol, dD, iters = hb.ss_jvp(dx, n_het=n_het, tol=S.TOL, max_iter=S.MAX_ITER)
            what = f"{name} N={N} n_het={n_het} (steps {iters})"
            cases.close(_flat(dV), r["JV"] @ dx, rel=_rel(c, False), what=what + " dV")
            cases.close(_flat(dpol), r["Jpol"] @ dx, rel=_rel(c, False), what=what + " dpol")
            cases.close(_flat(dD), r["JD"] @ dx, rel=_rel(c, True), what=what + " dD")
            cases.close(dagg, r["JY"][:n_het] @ dx, rel=_rel(c, True), what=what + " dagg")
            one = np.abs(_flat(dD).sum(axis=0)).max()
            print(f"{what}: 1'dD {one:.3e}")
            assert one <= 1e-12 + _rel(c, True) * np.abs(r["JD"] @ dx).max()
            assert 0 < iters[0] < S.MAX_ITER and 0 < iters[1] < S.MAX_ITER
    finally:
        hb.close()


# ---- 2. VJP parity ----------------------------------------------------------------------------------------------------------------
VJP_MODES = {"agg": (True, False, False), "value": (False, True, False), "D": (False, False, True), "all": (True, True, True)}


def _cots(c, M, seed=0):
    rng = np.random.default_rng(200 + M + seed)
    G = c["orc"].G
    return rng.standard_normal((c["n_het"], M)), rng.standard_normal((G, M)), rng.standard_normal((G, M))


@pytest.mark.parametrize("M", [1, 4, 33])
@pytest.mark.parametrize("name", S.NAMES)
def test_ss_vjp_matches_the_transposed_dense_jacobian(hank, oracle_mod, name, M):
    """agg_bar alone, value_bar alone, D_bar alone and all three, against J' of the assembled dense Jacobian; `clamp` has more
    clamped source rows than one row block of the M = 1 geometry owns"""
    hb, c = _ctx(hank, name)
    try:
        r, n_het = c["ref"], c["n_het"]
        yb, Vb, Db = _cots(c, M)
        for mode, (wy, wv, wd) in VJP_MODES.items():
            xbar, iters = hb.ss_vjp(yb if wy else None, Vb if wv else None, Db if wd else None, n_het=n_het, tol=S.TOL, max_iter=S.MAX_ITER)
            ref = (r["JY"].T @ yb if wy else 0.0) + (r["JV"].T @ Vb if wv else 0.0) + (r["JD"].T @ Db if wd else 0.0)
            cases.close(xbar, ref, rel=_rel(c, True), what=f"{name} M={M} {mode} (steps {iters}) xhh_bar")
            assert iters[0] < S.MAX_ITER and iters[1] < S.MAX_ITER
        if n_het > 2:      # fewer outputs than the family has
            xbar, _ = hb.ss_vjp(yb[:2], None, None, n_het=2, tol=S.TOL, max_iter=S.MAX_ITER)
            cases.close(xbar, r["JY"][:2].T @ yb[:2], rel=_rel(c, True), what=f"{name} M={M} n_het=2 xhh_bar")
    finally:
        hb.close()


# ---- 3. the transpose identity (two device products: never parity) --------------------------------------------------------------------
@pytest.mark.parametrize("name", S.NAMES)
def test_the_two_entries_are_transposes(hank, oracle_mod, name):
    hb, c = _ctx(hank, name)
    try:
        n_het, n_hh = c["n_het"], len(c["x"])
        rng = np.random.default_rng(7)
        dx = rng.standard_normal((n_hh, 4))
        yb, Vb, Db = _cots(c, 3, seed=1)
        dagg, dV, dpol, dD, _ = hb.ss_jvp(dx, n_het=n_het, tol=S.TOL, max_iter=S.MAX_ITER)
        xbar, _ = hb.ss_vjp(yb, Vb, Db, n_het=n_het, tol=S.TOL, max_iter=S.MAX_ITER)
        lhs = yb.T @ dagg + Vb.T @ _flat(dV) + Db.T @ _flat(dD)      # (3, 4)
        rhs = xbar.T @ dx
        cases.close(lhs, rhs, rel=_rel(c, True), what=f"{name} <ybar, dY> + <Vbar, dV> + <Dbar, dD> against <xbar, dx>")
    finally:
        hb.close()


# ---- 4. state rules ---------------------------------------------------------------------------------------------------------------
def _raw_jvp(hank, hb, n_het, N=1, max_iter=S.MAX_ITER):
    lib = hank.hip.load_library()
    dx = np.ones((hb.n_hh, N), order="F")
    out = np.empty((max(n_het, 1), N), order="F")
    it, res = (ctypes.c_int32 * 2)(), (ctypes.c_double * 2)()
    p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))      # noqa: E731
    return lib.hank_ss_jvp(hb._ctx, n_het, p(dx), N, S.TOL, max_iter, None, None, None, p(out), it, res), it, res


def _raw_vjp(hank, hb, n_het, yb, M=1):
    lib = hank.hip.load_library()
    out = np.empty((hb.n_hh, M), order="F")
    it, res = (ctypes.c_int32 * 2)(), (ctypes.c_double * 2)()
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))      # noqa: E731
    return lib.hank_ss_vjp(hb._ctx, n_het, p(yb), None, None, M, S.TOL, S.MAX_ITER, p(out), it, res)


def test_state_rules(hank, oracle_mod):
    """HANK_ERR_NOT_READY before a primal, after a primal at a path that varies, after a device-pointer primal and after a new
    boundary; HANK_ERR_BAD_ARG for all-NULL cotangents and a count above the family's; HANK_ERR_NOT_READY above the declared count"""
    import torch
    hb, c = _ctx(hank, "ks50x2", primal=False)
    try:
        NOT_READY, BAD_ARG = hank.hip.HANK_ERR_NOT_READY, hank.hip.HANK_ERR_BAD_ARG
        x = np.tile(c["x"][:, None], (1, hb.P))
        y1 = np.ones((3, 1), order="F")
        assert _raw_jvp(hank, hb, 2)[0] == NOT_READY and _raw_vjp(hank, hb, 2, y1[:2].copy(order="F")) == NOT_READY      # no primal
        xt = x.copy()
        xt[0, 3] *= 1.01
        hb.primal(xt)
        assert _raw_jvp(hank, hb, 2)[0] == NOT_READY and _raw_vjp(hank, hb, 2, y1[:2].copy(order="F")) == NOT_READY      # a path that varies
        hb.primal(x)
        assert _raw_jvp(hank, hb, 2)[0] == hank.hip.HANK_OK
        dx_t = torch.tensor(np.asfortranarray(x).reshape(-1, order="F"), device="cuda", dtype=torch.float64)
        hb.primal_dev(dx_t.data_ptr())
        hb.sync()
        assert _raw_jvp(hank, hb, 2)[0] == NOT_READY and _raw_vjp(hank, hb, 2, y1[:2].copy(order="F")) == NOT_READY      # a device-pointer primal
        hb.primal(x)
        assert _raw_vjp(hank, hb, 2, y1[:2].copy(order="F")) == hank.hip.HANK_OK
        assert _raw_vjp(hank, hb, 2, None) == BAD_ARG                                          # all three cotangents NULL
        assert _raw_jvp(hank, hb, 4)[0] == BAD_ARG and _raw_vjp(hank, hb, 4, np.ones((4, 1), order="F")) == BAD_ARG   # Krusell-Smith has three outputs
        assert _raw_jvp(hank, hb, 0)[0] == BAD_ARG
        hb.set_boundary(c["V"] * 1.001, c["D"])
        assert _raw_jvp(hank, hb, 2)[0] == NOT_READY and _raw_vjp(hank, hb, 2, y1[:2].copy(order="F")) == NOT_READY      # a new boundary
        assert "hank_primal must be called before hank_ss_vjp" in hank.hip.load_library().hank_last_error(hb._ctx).decode()
    finally:
        hb.close()
    hb, c = _ctx(hank, "ks50x2", declare=False)
    try:
        assert _raw_jvp(hank, hb, 3)[0] == hank.hip.HANK_ERR_NOT_READY           # three outputs asked for, two declared
        assert _raw_jvp(hank, hb, 2)[0] == hank.hip.HANK_OK
    finally:
        hb.close()


def test_last_ss_timings_follow_the_loops(hank, oracle_mod):
    """(-1, -1) on a fresh context after `primal`; both loops' times after ss_jvp and after ss_vjp; a call rejected at its
    arguments leaves the last values standing"""
    hb, c = _ctx(hank, "ks50x2")
    try:
        assert hb.last_ss_timings() == (-1.0, -1.0)
        hb.ss_jvp(np.ones((hb.n_hh, 1)), tol=S.TOL, max_iter=S.MAX_ITER)
        tj = hb.last_ss_timings()
        assert tj[0] > 0 and tj[1] > 0, tj
        hb.ss_vjp(np.ones((2, 1)), tol=S.TOL, max_iter=S.MAX_ITER)
        tv = hb.last_ss_timings()
        assert tv[0] > 0 and tv[1] > 0, tv
        assert _raw_jvp(hank, hb, 2, N=0)[0] == hank.hip.HANK_ERR_BAD_ARG
        assert hb.last_ss_timings() == tv
    finally:
        hb.close()


def test_calls_leave_the_context_alone(hank, oracle_mod):
    """the current tangent batch, the current cotangent batch, the memo and sweep counters, the family of the last tangent sweep:
    all as before; hank_fake_news returns the same bits before and after"""
    hb, c = _ctx(hank, "ks50x2")
    try:
        rng = np.random.default_rng(11)
        F0, Dv0 = hb.fake_news()
        y = rng.standard_normal((hb.n_hh, hb.P, 3)) * 1e-2
        hb.jvp(y)
        hb.vjp(rng.standard_normal((hb.P, 2)))
        dpol0, pbar0, st0, info0 = hb.dpolicy_seq(3), hb.policy_cotangent_seq(2), hb.stats(), hb.info()
        hb.ss_jvp(rng.standard_normal((hb.n_hh, 3)), n_het=3, tol=S.TOL, max_iter=S.MAX_ITER)
        hb.ss_vjp(rng.standard_normal((3, 2)), rng.standard_normal((hb.G, 2)), rng.standard_normal((hb.G, 2)), n_het=3, tol=S.TOL, max_iter=S.MAX_ITER)
        st1, info1 = hb.stats(), hb.info()
        assert np.array_equal(hb.dpolicy_seq(3), dpol0) and np.array_equal(hb.policy_cotangent_seq(2), pbar0)
        assert st1["primal_memo_hits"] == st0["primal_memo_hits"] and st1["primal_sweeps"] == st0["primal_sweeps"]
        assert st1["tangent_workspaces_allocated"] == st0["tangent_workspaces_allocated"] and st1["schedule"] == st0["schedule"]
        assert info1["last_tangent_family"] == info0["last_tangent_family"]
        F1, Dv1 = hb.fake_news()
        assert np.array_equal(F0, F1) and np.array_equal(Dv0, Dv1)
    finally:
        hb.close()


# ---- 5. the cap, bits, records of both schedules ------------------------------------------------------------------------------------
def test_iteration_cap_is_not_an_error(hank, oracle_mod):
    hb, c = _ctx(hank, "ks30x3")
    try:
        rc, it, res = _raw_jvp(hank, hb, 2, N=2, max_iter=5)
        assert rc == hank.hip.HANK_OK and it[0] == 5 and it[1] == 5
        print(f"after 5 steps: increment ratios {res[0]:.3e}, {res[1]:.3e}")
        assert res[0] > S.TOL and res[1] > S.TOL and np.isfinite(res[0]) and np.isfinite(res[1])
        with pytest.raises(hank.hip.SteadyStateLoopError):
            hb.ss_jvp(np.ones((hb.n_hh, 2)), tol=S.TOL, max_iter=5)
        with pytest.raises(hank.hip.SteadyStateLoopError):
            hb.ss_vjp(np.ones((2, 2)), tol=S.TOL, max_iter=5)
        assert hb.last_ss["iters"] == (5, 5)
    finally:
        hb.close()


@pytest.mark.parametrize("name", ["hank30x3", "clamp"])
def test_two_identical_calls_give_identical_bits(hank, oracle_mod, name):
    hb, c = _ctx(hank, name)
    try:
        n_het, n_hh = c["n_het"], len(c["x"])
        for width in (3, 4):
            dx = np.random.default_rng(width).standard_normal((n_hh, width))
            yb, Vb, Db = _cots(c, width)
            a, b = hb.ss_jvp(dx, n_het=n_het, max_iter=S.MAX_ITER), hb.ss_jvp(dx, n_het=n_het, max_iter=S.MAX_ITER)
            assert all(np.array_equal(p, q) for p, q in zip(a[:4], b[:4])) and a[4] == b[4]
            p, q = hb.ss_vjp(yb, Vb, Db, n_het=n_het, max_iter=S.MAX_ITER), hb.ss_vjp(yb, Vb, Db, n_het=n_het, max_iter=S.MAX_ITER)
            assert np.array_equal(p[0], q[0]) and p[1] == q[1]
    finally:
        hb.close()


def test_a_record_written_by_any_family_serves(hank, oracle_mod):
    """the record of HANK_SCHEDULE=launch and the record of the default schedule: results inside the bound of each other"""
    out = {}
    for sched in ("launch", None):
        hb, c = _ctx(hank, "ks50x2", schedule=sched)
        try:
            dx = np.random.default_rng(21).standard_normal((2, 4))
            yb, Vb, Db = _cots(c, 4)
            out[sched] = hb.ss_jvp(dx, n_het=3, max_iter=S.MAX_ITER)[:4] + (hb.ss_vjp(yb, Vb, Db, n_het=3, max_iter=S.MAX_ITER)[0],)
        finally:
            hb.close()
    for k, what in enumerate(("dagg", "dV", "dpol", "dD", "xhh_bar")):
        cases.close(out[None][k], out["launch"][k], rel=_rel(c, True), what=f"default schedule's record against the launch schedule's: {what}")


# ---- 6. the price Newton of the steady state -----------------------------------------------------------------------------------------
def test_find_ss_with_the_implicit_price_jacobian(hank, oracle_mod):
    """Krusell-Smith 50x2 from the YAML guesses: converges; its solution's residual, evaluated by the unchanged "fd" assembler, is
    within compspec.eps; fewer VFI steps than "fd" """
    ov = {"T": 100, "dimensions": {"wealth": {"n": 50}, "productivity": {"n": 2}}}

    def solve(pj):
        m = hank.build_model_from_yaml(str(ROOT / "examples" / "krusell_smith.yaml"), overrides=ov)
        return m, hank.find_ss(m, m.ss_initial, "initial", vfi="device", price_jacobian=pj)

    m, ss = solve("implicit")
    _, ss_fd = solve("fd")
    print(f"implicit: {ss.solve_info}\nfd:       {ss_fd.solve_info}")
    assert ss.solve_info["residual_norm"] <= m.compspec.ε and ss.solve_info["newton_iterations"] < 100
    asm = hank.SSAssembler(m, m.ss_initial, None, "device")
    z = hank.Residuals(asm(np.array([ss.vars[k] for k in asm.free_keys])), m)
    print(f"residual of the implicit solution under the fd assembler: {np.linalg.norm(z):.3e} (eps {m.compspec.ε:.1e})")
    assert np.linalg.norm(z) <= m.compspec.ε
    assert ss.solve_info["vfi_steps"] < ss_fd.solve_info["vfi_steps"]
    for k in m.variables:
        assert abs(ss.vars[k] - ss_fd.vars[k]) <= 1e-6 * max(1.0, abs(ss_fd.vars[k])), k
