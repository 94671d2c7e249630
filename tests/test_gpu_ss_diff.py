"""hank_ss_jvp / hank_ss_vjp on the MI355X: derivatives of the steady state's household objects (V_ss, a'_ss, D_ss and the
aggregates) in the household prices, against the dense reference of tests/ss_diff_cases.py (the CPU oracle's operators and direct
solves, pinned by tests/test_ss_diff_host.py). (1) JVP parity; (2) VJP parity; (3) the transpose identity between the two device
entries (never counted as parity); (4) state rules; (5) the cap, bits, records of both schedules; (5b) the device-pointer entries,
bit for bit against the host forms; (5c) the step at which each loop stops, against numpy iterations on the dense operators, and the
state behind the stop word; (6) find_ss with the implicit price Jacobian. (1) and (2) run every lane geometry of the two entries
(the table under "the widths"), n_e = 5 and 16, and gamma = 0.5, 1, 2, 3.

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


# ---- the widths ---------------------------------------------------------------------------------------------------------------------
# The first four economies keep the widths they had, the new ones run four each, and three economies — `clamp` (190 rows: several
# row blocks at every RB), `hank30x3` (three inputs, up to two extra outputs) and `ks40x16` (1024-thread blocks) — run every lane
# geometry: tests/test_geom_host.py pins what each width reaches (SS_JVP_TABLE, SS_VJP_TABLE).
#   JVP N   2: double2, NC 1, RB 64        7: double, NC 8, gather form, 7 of 8 lanes        16: double2, NC 8, full wave
#           9: double, NC 16, the first source-stationary width, RB 4, block map on        18: double2, NC 16, 9 of 16 lanes
#          32: double2, NC 16 full, the last width with the block map on        34: double2, NC 32, RB 2, block map off
#          65: double, NC 64, two blocks in y, one live lane in the second        130: the same on double2 lanes
#   VJP M   2: double2, NC 1, R 64        3: double, NC 4, R 16, 3 of 4 lanes        7: double, NC 8, R = RB = 8, two slot trips
#          16: double2, NC 8 full        32: double2, NC 16, R 8, RB 4, with ks40x16 the largest LDS tile
#          34: double2, NC 16, two blocks in y, one live lane in the second
GEOMETRY_NAMES = ("clamp", "hank30x3", "ks40x16")
JVP_GEOMETRY_WIDTHS = (2, 7, 16, 9, 18, 32, 34, 65, 130)
VJP_GEOMETRY_WIDTHS = (2, 3, 7, 16, 32, 34)


def _widths(old, new, geometry):
    """[(name, width)]: economy by economy, no pair twice"""
    pairs = [(n, w) for n in S.OLD_NAMES for w in old] + [(n, w) for n in S.NEW_NAMES for w in new]
    return pairs + [(n, w) for n in GEOMETRY_NAMES for w in geometry if (n, w) not in pairs]


# ---- 1. JVP parity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N", _widths((1, 3, 4, 33), (1, 4, 18, 33), JVP_GEOMETRY_WIDTHS))
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


@pytest.mark.parametrize("name,M", _widths((1, 4, 33), (1, 4, 7, 32), VJP_GEOMETRY_WIDTHS))
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


# ---- 5b. the device-pointer entries ------------------------------------------------------------------------------------------------
def _dp(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _host_jvp(hank, hb, dx, n_het, want=(True, True, True)):
    """hank_ss_jvp with any of its three exports NULL -> [dagg, dV, dpol, dD] ((G, N) column-major; None where not wanted), iters"""
    N = dx.shape[1]
    dxf = np.asfortranarray(dx)
    outs = [np.full((hb.G, N), np.nan, order="F") if w else None for w in want]
    dagg = np.full((n_het, N), np.nan, order="F")
    it, res = (ctypes.c_int32 * 2)(), (ctypes.c_double * 2)()
    rc = hank.hip.load_library().hank_ss_jvp(hb._ctx, n_het, _dp(dxf), N, S.TOL, S.MAX_ITER, _dp(outs[0]), _dp(outs[1]), _dp(outs[2]), _dp(dagg), it, res)
    assert rc == hank.hip.HANK_OK
    return [dagg] + outs, (it[0], it[1])


def _dev_jvp(hb, dx, n_het, want=(True, True, True)):
    """`ss_jvp_dev` on torch tensors, the same shapes and the same NaN fill"""
    import torch
    N = dx.shape[1]
    t_dx = torch.from_numpy(np.asfortranarray(dx).reshape(-1, order="F").copy()).cuda()
    t_out = [torch.full((hb.G * N,), float("nan"), dtype=torch.float64, device="cuda") if w else None for w in want]
    t_agg = torch.full((n_het * N,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    iters = hb.ss_jvp_dev(t_dx.data_ptr(), N, t_agg.data_ptr(), *(0 if t is None else t.data_ptr() for t in t_out), n_het=n_het, tol=S.TOL, max_iter=S.MAX_ITER)
    back = lambda t, rows: None if t is None else t.cpu().numpy().reshape((rows, N), order="F")      # noqa: E731
    return [back(t_agg, n_het)] + [back(t, hb.G) for t in t_out], iters


def _same_bits(a, b, what):
    for k, (p, q) in enumerate(zip(a, b)):
        assert (p is None) == (q is None), (what, k)
        if p is not None:
            assert not np.isnan(p).any(), (what, k, "an output was left unwritten")
            assert np.array_equal(p, q), f"{what}: output {k} differs in {np.count_nonzero(p != q)} entries, by up to {np.max(np.abs(p - q)):.3e}"


WANTS = ((True, True, True), (False, True, True), (True, False, True), (True, True, False), (False, False, False))


@pytest.mark.parametrize("name", ["hank30x3", "clamp"])
def test_ss_jvp_dev_gives_the_host_form_s_bits(hank, oracle_mod, name):
    """one odd and one even width: every output of hank_ss_jvp_dev (exports straight to the caller's buffers, inputs by device
    copies) equals hank_ss_jvp's bit for bit; with each export NULL in turn and all three NULL, in both forms, dagg and the
    remaining exports keep their bits; the wrapper of the host form agrees with the raw call"""
    hb, c = _ctx(hank, name)
    try:
        n_het, n_hh = c["n_het"], len(c["x"])
        for N in (3, 4):
            dx = np.random.default_rng(300 + N).standard_normal((n_hh, N))
            full, it0 = _host_jvp(hank, hb, dx, n_het)
            wrapped = hb.ss_jvp(dx, n_het=n_het, tol=S.TOL, max_iter=S.MAX_ITER)
            _same_bits(full, [wrapped[0]] + [_flat(a) for a in wrapped[1:4]], f"{name} N={N} raw host call against HouseholdBlock.ss_jvp")
            assert tuple(it0) == wrapped[4]
            for want in WANTS:
                expect = [full[0]] + [f if w else None for f, w in zip(full[1:], want)]
                host, ith = _host_jvp(hank, hb, dx, n_het, want)
                _same_bits(host, expect, f"{name} N={N} host form, exports wanted {want}")
                dev, itd = _dev_jvp(hb, dx, n_het, want)
                _same_bits(dev, expect, f"{name} N={N} device-pointer form, exports wanted {want}")
                assert tuple(ith) == tuple(itd) == tuple(it0) and hb.last_ss["iters"] == tuple(it0)
    finally:
        hb.close()


def _dev_vjp(hb, yb, Vb, Db, n_het):
    import torch
    M = next(v.shape[1] for v in (yb, Vb, Db) if v is not None)
    up = lambda a: None if a is None else torch.from_numpy(np.asfortranarray(a).reshape(-1, order="F").copy()).cuda()      # noqa: E731
    ts = [up(a) for a in (yb, Vb, Db)]
    t_out = torch.full((hb.n_hh * M,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    iters = hb.ss_vjp_dev(*(0 if t is None else t.data_ptr() for t in ts), M, t_out.data_ptr(), n_het=n_het, tol=S.TOL, max_iter=S.MAX_ITER)
    return t_out.cpu().numpy().reshape((hb.n_hh, M), order="F"), iters


@pytest.mark.parametrize("name", ["hank30x3", "clamp"])
def test_ss_vjp_dev_gives_the_host_form_s_bits(hank, oracle_mod, name):
    """one odd and one even width, every mode of cotangents: hank_ss_vjp_dev's xhh_bar equals hank_ss_vjp's bit for bit. With
    value_bar and D_bar both given the two pass through ONE staging buffer, ordered by the stream alone: that call is also the sum
    of the two single-cotangent calls (inside `close`: each call stops its loops on its own)."""
    hb, c = _ctx(hank, name)
    try:
        n_het = c["n_het"]
        for M in (3, 4):
            yb, Vb, Db = _cots(c, M, seed=5)
            got = {}
            for mode, (y, v, d) in {"agg": (yb, None, None), "value": (None, Vb, None), "D": (None, None, Db), "value+D": (None, Vb, Db), "all": (yb, Vb, Db)}.items():
                host, ith = hb.ss_vjp(y, v, d, n_het=n_het, tol=S.TOL, max_iter=S.MAX_ITER)
                dev, itd = _dev_vjp(hb, y, v, d, n_het)
                _same_bits([dev], [host], f"{name} M={M} {mode}: device-pointer form against the host form")
                assert ith == itd and hb.last_ss["iters"] == ith
                got[mode] = dev
            cases.close(got["value+D"], got["value"] + got["D"], rel=_rel(c, True), what=f"{name} M={M} value_bar and D_bar together against the two alone")
            cases.close(got["all"], got["agg"] + got["value"] + got["D"], rel=_rel(c, True), what=f"{name} M={M} all three together against each alone")
            ref = c["ref"]["JV"].T @ Vb + c["ref"]["JD"].T @ Db
            cases.close(got["value+D"], ref, rel=_rel(c, True), what=f"{name} M={M} value_bar and D_bar together against the dense Jacobian")
    finally:
        hb.close()


def test_dev_calls_leave_the_context_alone(hank, oracle_mod):
    """the assertions of test_calls_leave_the_context_alone after the device-pointer forms"""
    hb, c = _ctx(hank, "ks50x2")
    try:
        rng = np.random.default_rng(12)
        F0, Dv0 = hb.fake_news()
        hb.jvp(rng.standard_normal((hb.n_hh, hb.P, 3)) * 1e-2)
        hb.vjp(rng.standard_normal((hb.P, 2)))
        dpol0, pbar0, st0, info0 = hb.dpolicy_seq(3), hb.policy_cotangent_seq(2), hb.stats(), hb.info()
        _dev_jvp(hb, rng.standard_normal((hb.n_hh, 3)), 3)
        _dev_vjp(hb, rng.standard_normal((3, 2)), rng.standard_normal((hb.G, 2)), rng.standard_normal((hb.G, 2)), 3)
        st1, info1 = hb.stats(), hb.info()
        assert np.array_equal(hb.dpolicy_seq(3), dpol0) and np.array_equal(hb.policy_cotangent_seq(2), pbar0)
        assert st1["primal_memo_hits"] == st0["primal_memo_hits"] and st1["primal_sweeps"] == st0["primal_sweeps"]
        assert st1["tangent_workspaces_allocated"] == st0["tangent_workspaces_allocated"] and st1["schedule"] == st0["schedule"]
        assert info1["last_tangent_family"] == info0["last_tangent_family"]
        F1, Dv1 = hb.fake_news()
        assert np.array_equal(F0, F1) and np.array_equal(Dv0, Dv1)
    finally:
        hb.close()


# ---- 5c. the stop rule and the frozen state -------------------------------------------------------------------------------------------
# tol = 1e-9: the increments sit far above rounding, so the step at which a loop's rule first holds is a property of the operators.
# The increment ratio moves by about 2.5 % per step (rho ~ 0.975), so rounding can tip at most the step at the threshold: +-1, the
# margin tests/test_gpu_steady_state.py gives its step counts. The value loop's numpy iteration starts where the device's does, at
# the knots' tangent ds = 0 (S.value_loop_start: from closed forms, not from the device); from dV = 0 it would stop 11 (`clamp`) and
# 51 (`ks30x3`) steps earlier than the device, whose trajectory is another one.
STOP_TOL = 1e-9


@pytest.mark.parametrize("name", ["ks30x3", "clamp"])
def test_loops_stop_where_the_rule_says_and_the_state_freezes(hank, oracle_mod, name):
    """N = M = 3. (1) `iters` of the value, distribution, nu and lambda loops against the steps plain numpy iterations on the dense
    operators take under the same rules (S.jvp_loops, S.vjp_loops: nothing of them comes from the device). (2) A first call under
    max_iter = MAX_ITER has launches of a chunk queued behind the stop word; a second call capped at the first's larger `iters`
    has none in that loop: the same bits in every output, so whatever runs behind the stop word leaves the state alone."""
    hb, c = _ctx(hank, name)
    try:
        n_het, n_hh = c["n_het"], len(c["x"])
        dx = np.random.default_rng(400).standard_normal((n_hh, 3))
        yb, Vb, Db = _cots(c, 3, seed=9)
        a = hb.ss_jvp(dx, n_het=n_het, tol=STOP_TOL, max_iter=S.MAX_ITER)
        _, _, kj = S.jvp_loops(c, dx, STOP_TOL)
        print(f"{name} JVP: device (value, distribution) steps {a[4]}, numpy {kj}")
        p = hb.ss_vjp(yb, Vb, Db, n_het=n_het, tol=STOP_TOL, max_iter=S.MAX_ITER)
        _, kv = S.vjp_loops(c, yb, Vb, Db, STOP_TOL)
        print(f"{name} VJP: device (nu, lambda) steps {p[1]}, numpy {kv}")
        assert all(0 < k < S.MAX_ITER for k in kj + kv)
        assert abs(a[4][0] - kj[0]) <= 1 and abs(a[4][1] - kj[1]) <= 1, (a[4], kj)
        assert abs(p[1][0] - kv[0]) <= 1 and abs(p[1][1] - kv[1]) <= 1, (p[1], kv)
        b = hb.ss_jvp(dx, n_het=n_het, tol=STOP_TOL, max_iter=max(a[4]), check=False)
        assert b[4] == a[4]
        _same_bits(b[:4], a[:4], f"{name} JVP capped at {max(a[4])} steps against the call under the cap {S.MAX_ITER}")
        q = hb.ss_vjp(yb, Vb, Db, n_het=n_het, tol=STOP_TOL, max_iter=max(p[1]), check=False)
        assert q[1] == p[1]
        _same_bits([q[0]], [p[0]], f"{name} VJP capped at {max(p[1])} steps against the call under the cap {S.MAX_ITER}")
    finally:
        hb.close()


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
