"""hank_vjp (csrc/hank_adjoint.h) where tests/test_gpu_vjp.py does not take it. The reference is always the CPU
oracle's Jacobian from unit tangents, transposed (x̄), or the numpy restatement of the reference's ForwardIteration_pullback (p̄,
Sweep A alone): never another run of hank_vjp. Comparisons between runs are stated as what they are (batch invariance, the record
writers against each other, diet on against off) and come on top of the oracle check.

A. every lane geometry build_cotwork derives from the batch width M: all nine (V, NC) pairs, R = 64, 32, 16 and 8 rows per block,
   idle column lanes, a partial last y-block, several y-blocks, at n_a = R - 1, R, R + 1 and 2 R + 1 for R = 64 (multiples of and
   one off the smaller R as well);
B. n_e = 1, 2, 5, 7, 11, 12, 16: 64 n_e threads per block, the cross-wave reduction on both sides of n_e = 6, the largest dynamic
   LDS the family asks for (59 392 bytes: n_e = 16, M = 32);
C. every curvature and record layout of the variant suite (pow_crra's branches, kc and v read or rebuilt);
D. records written by every entry point and family, revisited through the primal memo, and after hank_fake_news;
E. raw-grid economies whose policy holds a deep clamped prefix (the 1/nb share-out of k_adj_dist), many sources capped at the
   top, and long runs of rows in one bracket (the two-rows-per-trip walk of k_adj_egm): tests/test_vjp_host.py proves those edges
   present on the oracle's policy. The launch family's hank_jvp is held to the same bound on the same case, so a miss of the
   VJP alone is a kernel finding and a miss of both an ill-conditioned grid;
F. the benched size with both aggregates and an odd width (VT = double), by projection on oracle columns.

Tolerance: the suite's rel 1e-10 + abs 1e-12 on the largest entry of the reference (cases.close), 1e-10 of the summed
magnitudes for the projection, 1e-12 of the summed magnitudes for the pairing, 1e-13 of the largest entry for one column in
different batches, 1e-12 for the same record written by another family or with the other layout."""
import numpy as np
import pytest

import cases as vc
from cases import close, jt

pytestmark = pytest.mark.gpu

_J = {}


def _jac(key, orc, V, D, x):
    """the oracle's Jacobian of a case, once per session"""
    if key not in _J:
        _J[key] = vc.oracle_jacobian(orc, V, D, x)
    return _J[key]


def _same_column(a, b, what):
    err, scale = np.max(np.abs(a - b)), np.abs(b).max()
    print(f"{what}: max diff {err:.3e} vs scale {scale:.3e}")
    assert err <= 1e-13 * scale, f"{what}: max diff {err:.3e} vs scale {scale:.3e}"


def _pullback_columns(hb, D0, yb, M, what):
    """policy_cotangent_seq of the current n_het = 1 batch against the reference pullback, first and last column"""
    pbar = hb.policy_cotangent_seq(M)
    pol, Dseq = hb.policy_seq(), hb.dist_seq()
    D0 = np.asarray(D0).reshape(hb.n_a, hb.n_e, order="F")
    for k in sorted({0, M - 1}):
        close(pbar[..., k], vc.forward_iteration_pullback(hb.a_grid, hb.Pi, pol, D0, Dseq, yb[:, 0, k]), what=f"{what} pbar column {k}")
    return pbar


# ---- A. lane geometries ---------------------------------------------------------------------------------------------------
GEOM_M = (1, 2, 3, 4, 6, 8, 16, 17, 34, 64, 97, 256)


@pytest.mark.parametrize("n_het", [1, 2])
@pytest.mark.parametrize("n_a", [63, 64, 65, 129])
def test_every_lane_geometry_against_the_oracle(hank, oracle_mod, n_a, n_het):
    m, V, D, xhh, orc = vc.shape(n_a, 3, 12)
    P = xhh.shape[1]
    J = _jac(("shape", n_a, 3, 12), orc, V, D, xhh)
    assert np.abs(J).max() > 1e-3
    yb = np.random.default_rng(100 * n_a + n_het).standard_normal((P, n_het, max(GEOM_M)))
    hb = vc.block(hank, m, "launch")
    try:
        hb.set_boundary(V, D)
        hb.primal(xhh)
        assert hb.stats()["schedule"] == 0
        for M in GEOM_M:
            what = f"{n_a}x3 n_het={n_het} M={M}"
            got = hb.vjp(yb[:, :, :M], n_het)
            assert got.shape == (2, P, M)
            close(got, jt(J[:n_het], yb[:, :, :M]), what=what)
            if n_het == 1 and M in (1, 2, 4, 6, 34):
                _pullback_columns(hb, D, yb[:, :, :M], M, what)
        # one column alone (VT = double, R = 64), in an odd batch (R = 8) and in an even one (VT = double2)
        alone, odd, even = hb.vjp(yb[:, :, 7:8], n_het)[:, :, 0], hb.vjp(yb[:, :, :33], n_het)[:, :, 7], hb.vjp(yb[:, :, :34], n_het)[:, :, 7]
        _same_column(alone, odd, "alone vs in 33")
        _same_column(even, odd, "in 34 vs in 33")
        _same_column(alone, even, "alone vs in 34")
    finally:
        hb.close()


# ---- B. n_e -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", ["launch", "xcd"])
@pytest.mark.parametrize("n_e", [1, 2, 5, 7, 11, 12, 16])
def test_every_block_size_against_the_oracle(hank, oracle_mod, n_e, schedule):
    """64 n_e threads per block; sums 0..5 of k_adj_egm are reduced by wave q mod n_e (n_e < 6: several per wave; n_e > 6: idle
    waves); n_e = 16 is the 1024-thread block, and its M = 32 the 59 392 bytes of dynamic LDS."""
    if n_e == 1:
        args, V, D, xhh, orc = vc.shape_one_column(40, 10)
        hb = vc.raw_block(hank, args, schedule)
    else:
        m, V, D, xhh, orc = vc.shape(40, n_e, 10)
        hb = vc.block(hank, m, schedule)
    P = xhh.shape[1]
    J = _jac(("shape", 40, n_e, 10), orc, V, D, xhh)
    assert np.abs(J).max() > 1e-3
    try:
        assert hb.n_e == n_e and hb.n_hh == 2
        hb.set_boundary(V, D)
        hb.primal(xhh)
        assert hb.stats()["schedule"] == (0 if schedule == "launch" else 1) and hb.stats()["fallbacks"] == 0
        for M in (1, 5, 32):
            yb = np.random.default_rng(10 * M + n_e).standard_normal((P, 2, M))
            close(hb.vjp(yb, 2), jt(J, yb), what=f"40x{n_e} {schedule} M={M}")
    finally:
        hb.close()


# ---- C. curvature x record layout ----------------------------------------------------------------------------------------
MATRIX = [(fam, case) for fam in ("ks", "hank") for case in vc.CASES if not (fam == "hank" and case == "gamma0.5")]


@pytest.mark.parametrize("family,case", MATRIX)
def test_every_curvature_and_record_layout_against_the_oracle(hank, oracle_mod, family, case):
    """(the one-asset HANK calibration has no steady state at gamma = 0.5: tests/test_gpu_variants.py)"""
    gamma, diet_env, diet = vc.CASES[case]
    m, ss, xhh, orc = vc.economy(family, gamma)
    P = xhh.shape[1]
    J = _jac(("economy", family, gamma), orc, ss.value, ss.D, xhh)
    ybs = {(n_het, M): np.random.default_rng(10 * M + n_het).standard_normal((P, n_het, M)) for n_het in (1, 2) for M in (1, 6, 33)}

    def run(sched, env):
        hb = vc.block(hank, m, sched, HANK_RECORD_DIET=env)
        try:
            hb.set_boundary(ss.value, ss.D)
            assert hb.info()["record_diet"] == (diet if env == diet_env else 1), (sched, hb.info())
            hb.primal(xhh)
            assert hb.stats()["schedule"] == (0 if sched == "launch" else 1) and hb.stats()["fallbacks"] == 0
            return {key: hb.vjp(yb, key[0]) for key, yb in ybs.items()}
        finally:
            hb.close()
    for sched in ("launch", "xcd"):
        got = run(sched, diet_env)
        for (n_het, M), yb in ybs.items():
            close(got[n_het, M], jt(J[:n_het], yb), what=f"{family} {case} {sched} n_het={n_het} M={M}")
        if diet_env == "0":
            # the same curvature with the diet on: kc and v rebuilt through the cancellation in cm (~1e-13)
            on = run(sched, None)
            for key in ybs:
                close(got[key], on[key], 1e-12, what=f"{family} {case} {sched} diet off vs on {key}")


# ---- D. record writers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["ks", "hank"])
def test_every_record_writer_serves_the_same_cotangents(hank, oracle_mod, family):
    """the record hank_vjp reads, written by hank_primal, by the Dual pass of each family (persistent: N = 5, host and device
    pointers; launches: N = 40; on-chip wide: N = 96), found again through the primal memo, and read after hank_fake_news (at the
    steady state: it needs a constant path). hank_vjp reads no lwg (it is not built for it) and leaves the tangent batch current."""
    import torch
    from hank_amd.BackwardIteration import household_inputs
    from hank_amd.GeneralStructures import vars_of_type
    m, ss, xhh, orc = vc.economy(family, 2.0)
    n_hh, P = xhh.shape
    x_ss = np.tile(np.array([ss.vars[k] for k in vars_of_type(m, "endogenous")]), P)
    exog = {k: np.full(P, float(ss.vars[k])) for k in vars_of_type(m, "exogenous")}
    xss = np.ascontiguousarray(household_inputs(x_ss, exog, m)[0])
    assert xss.shape == xhh.shape
    J = {"x": _jac(("economy", family, 2.0), orc, ss.value, ss.D, xhh), "ss": _jac(("economy-ss", family, 2.0), orc, ss.value, ss.D, xss)}
    rng = np.random.default_rng(31)
    y = rng.standard_normal((n_hh, P, 96))
    yb = rng.standard_normal((P, 2, 6))
    # the launch schedule's record
    hl = vc.block(hank, m, "launch")
    try:
        hl.set_boundary(ss.value, ss.D)
        ref = {}
        for at, x in (("x", xhh), ("ss", xss)):
            hl.primal(x)
            ref[at] = hl.vjp(yb, 2)
            close(ref[at], jt(J[at], yb), what=f"{family} launch record at {at}")
    finally:
        hl.close()
    hb = vc.block(hank, m, None)
    try:
        hb.set_boundary(ss.value, ss.D)

        def dual(N, fam):
            hb.primal_jvp(xhh, np.ascontiguousarray(y[:, :, :N]))
            assert hb.info()["last_tangent_family_name"] == fam, (N, hb.info())
            return N

        def dual_dev(N):
            d_x = torch.from_numpy(np.asfortranarray(xhh).reshape(-1, order="F").copy()).cuda()
            d_y = torch.from_numpy(np.asfortranarray(y[:, :, :N]).reshape(-1, order="F").copy()).cuda()
            d_a, d_d = torch.empty(P, dtype=torch.float64, device="cuda"), torch.empty(P * N, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            hb.primal_jvp_dev(d_x.data_ptr(), d_y.data_ptr(), N, d_a.data_ptr(), d_d.data_ptr())
            hb.sync(); hb.check()
            assert hb.info()["last_tangent_family_name"] == "xcd-persistent", hb.info()
            return N

        def memo():                                     # the host-pointer Dual entry at the x on record: only its tangent sweeps run
            hb.primal_jvp(xhh, np.ascontiguousarray(y[:, :, :5]))
            hits, sweeps = hb.stats()["primal_memo_hits"], hb.stats()["primal_sweeps"]
            hb.primal_jvp(xhh, np.ascontiguousarray(y[:, :, 5:10]))
            assert hb.stats()["primal_memo_hits"] == hits + 1 and hb.stats()["primal_sweeps"] == sweeps
            return 5

        def after_fake_news():
            hb.primal(xss)
            hb.fake_news()
            return 0
        writers = [("hank_primal", "x", lambda: (hb.primal(xhh), 0)[1]),
                   ("Dual pass N=5", "x", lambda: dual(5, "xcd-persistent")),
                   ("Dual pass N=40", "x", lambda: dual(40, "launch-per-period")),
                   ("Dual pass N=96", "x", lambda: dual(96, "on-chip-wide")),
                   ("device-pointer Dual pass N=5", "x", lambda: dual_dev(5)),
                   ("primal memo", "x", memo),
                   ("after hank_fake_news", "ss", after_fake_news)]
        for name, at, write in writers:
            what = f"{family} {name}"
            hb.primal(xhh * 1.01)                       # another record in between: every writer writes
            N = write()
            lwg = hb.info()["lwg_builds"]
            got = hb.vjp(yb, 2)
            assert hb.info()["lwg_builds"] == lwg, what
            close(got, jt(J[at], yb), what=what + " vs oracle")
            close(got, ref[at], 1e-12, what=what + " vs the launch schedule's record")
            if N == 0:                                  # no tangent batch yet: one at this record
                N = 5
                hb.jvp(np.ascontiguousarray(y[:, :, :N]))
            dpol = hb.dpolicy_seq(N)
            lwg = hb.info()["lwg_builds"]
            assert np.array_equal(hb.vjp(yb, 2), got), what + ": the same record and cotangents, the same bits"
            assert hb.info()["lwg_builds"] == lwg, what
            assert np.array_equal(hb.dpolicy_seq(N), dpol), what + ": the tangent batch stays current"
        assert hb.stats()["fallbacks"] == 0
    finally:
        hb.close()


# ---- E. clamp and long-segment economies ------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", ["launch", "xcd"])
@pytest.mark.parametrize("name", list(vc.EDGE_GRIDS))
def test_clamped_prefix_top_clamp_and_long_segments(hank, oracle_mod, name, schedule):
    ec = vc.raw_economy(name)
    grid, V, D, x, orc = ec["grid"], ec["V"], ec["D"], ec["x"], ec["orc"]
    P = x.shape[1]
    J = _jac(("raw", name), orc, V, D, x)
    assert np.abs(J).max() > 1e-3
    rng = np.random.default_rng(41)
    hb = vc.raw_block(hank, ec["args"], schedule)
    try:
        hb.set_boundary(V, D)
        hb.primal(x)
        assert hb.stats()["schedule"] == (0 if schedule == "launch" else 1) and hb.stats()["fallbacks"] == 0
        vc.check_edges(name, grid, hb.policy_seq().transpose(2, 0, 1))        # the device's policy holds the edges too
        # conditioning: the tangent sweeps on the same case at the same bound
        y = rng.standard_normal((2, P, 33))
        close(hb.jvp(y), np.einsum("tks,ksn->tn", J[0], y), what=f"{name} {schedule} hank_jvp")
        for M in vc.EDGE_WIDTHS:
            for n_het in (1, 2):
                what = f"{name} {schedule} n_het={n_het} M={M}"
                yb = rng.standard_normal((P, n_het, M))
                close(hb.vjp(yb, n_het), jt(J[:n_het], yb), what=what)
                if n_het == 1:
                    pbar = _pullback_columns(hb, D, yb, M, what)
                    # <pbar, dpol> = <ybar, dagg> for a JVP batch at the same record
                    dagg = hb.jvp(y[:, :, :M])
                    dpol = hb.dpolicy_seq(M)
                    lhs, rhs = np.einsum("aetm,aetn->mn", pbar, dpol), np.einsum("tm,tn->mn", yb[:, 0, :], dagg)
                    terms = np.einsum("aetm,aetn->mn", np.abs(pbar), np.abs(dpol))
                    print(f"{what} pairing: max |lhs - rhs| / sum|terms| = {np.max(np.abs(lhs - rhs) / terms):.3e}")
                    assert np.all(np.abs(lhs - rhs) <= 1e-12 * terms), what
    finally:
        hb.close()


# ---- F. full size ---------------------------------------------------------------------------------------------------------
def test_full_size_2000x11_T300_both_aggregates_M33_by_projection_on_oracle_columns(hank, oracle_mod):
    m, ss, xhh, y, Jy = vc.fullsize_oracle_columns()            # Jy (2, P, 32): both aggregates
    hb = hank.household_block(m)
    hb.set_boundary(ss.value, ss.D)
    P, M = 299, 33
    yb = np.random.default_rng(2).standard_normal((P, 2, M))
    hb.primal(xhh)
    xbar = hb.vjp(yb, 2)                                        # (2, P, M)
    lhs = np.einsum("tom,otn->mn", yb, Jy)
    rhs = np.einsum("ktm,ktn->mn", xbar, y)
    scale = np.einsum("tom,otn->mn", np.abs(yb), np.abs(Jy))
    print(f"projection: max |lhs - rhs| / scale = {np.max(np.abs(lhs - rhs) / scale):.3e}")
    assert np.all(np.abs(lhs - rhs) <= 1e-10 * scale)
    t = hb.last_vjp_timings()
    assert t["sweep_a"]["ms"] > 0 and t["sweep_b"]["ms"] > 0 and t["sweep_a"]["launches"] == P
