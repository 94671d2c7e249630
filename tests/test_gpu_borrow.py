"""The borrowing-limit path on the device (hank_set_borrow_path, hank_jvp_borrow, hank_vjp_borrow, hank_fake_news_borrow) through the
C ABI, against tests/path_refs.oracle_path_sweeps at tests/borrow_refs.KIND — one unchanged CPU oracle per limit, the constrained set from an oracle whose
limit lies far below the grid, KrusellSmith.jl:76-80 restated on duals — which tests/test_borrow_host.py pins against the
constant-limit oracle's bits and against a central difference of its own level.

Shapes: the grids of cases.ENTRY_GRIDS — (33, 2): two primal blocks, the second holding one row; (130, 3) — both families, every gamma
of cases.ENTRY_CASES with its record diet, horizons T = 2, 3, 4 and 12, widths 1, 3 and 33. The path (borrow_refs.borrow_path) holds a
limit strictly inside a bracket, one on a grid point, a[0] and a value below it, and tightens and relaxes. Tolerance: cases.close (rel
1e-10 + abs 1e-12) against the oracle; bits where the header promises bits; the transposed identity at 1e-10 of the summed magnitudes."""
import numpy as np
import pytest

import borrow_refs as R
import cases
import fake_news_refs as FR
import path_checks as C
import path_refs
import ss_diff_cases as S
from cases import close, jt
from path_checks import NOT_READY, grid_cases

pytestmark = pytest.mark.gpu

K = R.KIND


def _groups(c):
    """all three bases: the constrained households' consumption (the rows at or below the highest limit), the top half's consumption,
    the lower half's savings, and the mass at or below the highest limit"""
    n_a, n_e = c["V"].shape
    a = np.asarray(c["args"][0])
    W = np.zeros((n_a, n_e, 4))
    W[a <= R.LIMIT_HI, :, 0] = 1.0
    W[n_a // 2:, :, 1] = 1.0
    W[: n_a // 2, :, 2] = 1.0
    W[a <= R.LIMIT_HI, :, 3] = 1.0
    return W.reshape((n_a * n_e, 4), order="F"), np.array([2, 2, 1, 0], dtype=np.int32)


# ---- 1. the level -------------------------------------------------------------------------------------------------------------------
@grid_cases
def test_primal_at_a_path_matches_the_oracle_under_every_schedule(hank, oracle_mod, family, name, n_a, n_e):
    for T in R.HORIZONS:
        c = R.borrow_case(family, name, n_a, n_e, T)
        P, nh, what = T - 1, c["n_het"], f"{family} {name} {n_a}x{n_e} T={T}"
        ref = path_refs.oracle_path_sweeps(*C.ref_args(K, c))
        got = {}
        for sched in ("launch", "xcd", "wide"):
            hb = C.ctx(hank, K, c, sched)
            try:
                before = hb.stats()
                agg0 = hb.primal(c["x"])
                got[sched] = (agg0, hb.het_outputs(nh)[0], hb.policy_seq(), hb.dist_seq())
                st, tm = hb.stats(), hb.last_timings()
                assert st["fallbacks"] == 0 and st["sweep_launches"] == before["sweep_launches"] and st["schedule"] == before["schedule"], (what, sched, st)
                assert tm["primal_backward"]["launches"] == P + 2, (what, sched, tm)
            finally:
                hb.close()
        agg0, agg, pol, dist = got["launch"]
        close(agg0, ref["agg"][:, 0], what=f"{what} aggregate")
        for o in range(nh):
            close(agg[:, o], ref["agg"][:, o], what=f"{what} output {o}")
        close(pol.transpose(2, 0, 1), ref["pol"], what=f"{what} policy")
        close(dist.transpose(2, 0, 1), ref["Dseq"], what=f"{what} distribution")
        assert np.array_equal(pol.transpose(2, 0, 1) == c["amin"][:, None, None], ref["pol"] == c["amin"][:, None, None]), what
        for sched in ("xcd", "wide"):
            assert all(np.array_equal(g, l) for g, l in zip(got[sched], got["launch"])), (what, sched)
        assert np.abs(ref["pol"] - path_refs.oracle_path_sweeps(*C.ref_args(K, c, False))["pol"]).max() > 1e-3, what      # (the path moves the policy)


@grid_cases
def test_a_path_at_the_model_s_limit_gives_the_bits_of_no_path(hank, oracle_mod, family, name, n_a, n_e):
    """the bits of no path are the launch family's (a path keeps every sweep on the launches, and the families do not agree bit for
    bit at twelve periods): a context under HANK_SCHEDULE=launch without a path is the yardstick, and a context under either schedule
    with the neutral path gives its bits"""
    for T in (2, 12):
        c = R.borrow_case(family, name, n_a, n_e, T)
        C.neutral_path_gives_the_bits_of_no_path(hank, K, c, (family, name, n_a, n_e, T), het=c["n_het"], default_too=True)


# ---- 2. hank_jvp_borrow ---------------------------------------------------------------------------------------------------------------
def _borrow_against_oracle(hb, c, tag, dx, da, path):
    J = path_refs.jacobians(*C.ref_args(K, c, path))
    N = next(v.shape[-1] for v in (dx, da) if v is not None)
    nh = c["n_het"]
    ref = path_refs.linear(J, dx, da)
    dpol = path_refs.linear_policies(*C.ref_args(K, c, path), dx=dx, dp=da)
    close(hb.jvp_borrow(dx, da), ref[:, 0, :], what=f"{tag} dagg")
    got = hb.dpolicy_seq(N).transpose(2, 0, 1, 3)
    close(got, dpol, what=f"{tag} dpolicy")
    _, dagg = hb.het_outputs(nh, np.zeros((hb.n_hh, hb.P, N)) if dx is None else dx)
    for o in range(nh):
        close(dagg[:, o, :], ref[:, o, :], what=f"{tag} output {o}")
    return got, dagg


def _jvp_borrow_case(hank, c, tag, widths=R.WIDTHS, t_only=True, schedule=None, paths=(True, False)):
    P = c["x"].shape[1]
    for path in paths:
        hb = C.ctx(hank, K, c, schedule, path=path)
        try:
            hb.primal(c["x"])
            tg = f"{tag} {'path' if path else 'no path'}"
            for N in widths:
                dx, da = path_refs.seeds(K, c, N, 11 + N)
                _borrow_against_oracle(hb, c, f"{tg} N={N} inputs and amin", dx, da, path)
                _borrow_against_oracle(hb, c, f"{tg} N={N} amin alone", None, da, path)
                _borrow_against_oracle(hb, c, f"{tg} N={N} inputs alone", dx, None, path)
            if t_only:
                for t in sorted({0, P - 1}):
                    _, da = path_refs.seeds(K, c, 3, 13, t_only=t)
                    _borrow_against_oracle(hb, c, f"{tg} N=3 amin_{t} alone", None, da, path)
            if path:      # convention (i): a seed in a period with amin_t <= a[0] moves nothing, exactly
                for t, k in enumerate(c["kinds"]):
                    if k in ("first", "below"):
                        _, da = path_refs.seeds(K, c, 3, 17, t_only=t)
                        dagg = hb.jvp_borrow(None, da)
                        assert not np.any(dagg) and not np.any(hb.dpolicy_seq(3)), (tg, t, k)
                        assert not np.any(hb.het_outputs(c["n_het"], np.zeros((hb.n_hh, P, 3)))[1]), (tg, t, k)
            tm = hb.last_timings()
            assert tm["tangent_backward"]["launches"] == 2 * P + 3 and tm["tangent_forward"]["launches"] == P + 3, (tg, tm)
            assert hb.info()["last_tangent_family_name"] == cases.FAMILY["launch"] and hb.stats()["fallbacks"] == 0
        finally:
            hb.close()


@grid_cases
def test_jvp_borrow_matches_the_oracle(hank, oracle_mod, family, name, n_a, n_e):
    for T in R.HORIZONS:
        _jvp_borrow_case(hank, R.borrow_case(family, name, n_a, n_e, T), f"{family} {name} {n_a}x{n_e} T={T}")


@pytest.mark.parametrize("schedule", ["xcd", "wide"])
def test_jvp_borrow_at_a_record_written_by_another_family(hank, oracle_mod, schedule):
    """without a path the primal runs on the context's schedule; the seed rebuilds the constrained set from that record. The model's
    limit is moved inside the grid, or the set would be empty"""
    c0 = R.borrow_case("hank", "gamma2", 130, 3, 12)
    c = R.with_limit(c0, R.limits(np.asarray(c0["args"][0]))["inside"])
    hb = C.ctx(hank, K, c, schedule, path=False)
    try:
        hb.primal(c["x"])
        dx, da = path_refs.seeds(K, c, 33, 5)
        got, _ = _borrow_against_oracle(hb, c, f"record by {schedule}", dx, da, False)
        assert np.any(got[0] != 0)
    finally:
        hb.close()


@grid_cases
def test_jvp_borrow_without_a_seed_in_the_limit_is_hank_jvp_bit_for_bit(hank, oracle_mod, family, name, n_a, n_e):
    for T in (2, 4):
        C.no_seed_in_the_path_is_hank_jvp_bit_for_bit(hank, K, R.borrow_case(family, name, n_a, n_e, T), (family, name, n_a, n_e, T), R.WIDTHS, signbits=True)


# ---- 3. hank_vjp_borrow ----------------------------------------------------------------------------------------------------------------
def _vjp_borrow_case(hank, c, tag, widths=R.WIDTHS, schedule=None, paths=(True, False)):
    P, nh = c["x"].shape[1], c["n_het"]
    rng = np.random.default_rng(P)
    for path in paths:
        hb = C.ctx(hank, K, c, schedule, path=path)
        try:
            hb.primal(c["x"])
            Jx, Ja = path_refs.jacobians(*C.ref_args(K, c, path))
            dx, da = path_refs.seeds(K, c, 3, 21)
            hb.jvp_borrow(dx, da)
            _, Jd = hb.het_outputs(nh, dx)                                        # (P, n_het, N)
            for M in widths:
                for n_het in sorted({1, 2, nh}):
                    what = f"{tag} path={path} M={M} n_het={n_het}"
                    yb = rng.standard_normal((P, n_het, M))
                    xbar, abar = hb.vjp_borrow(yb, n_het)
                    assert np.array_equal(xbar, hb.vjp_het(yb, n_het)), what
                    x2, a2 = hb.vjp_borrow(yb, n_het)
                    assert np.array_equal(x2, xbar) and np.array_equal(a2, abar), what
                    close(abar, path_refs.path_bar(Ja, yb), what=f"{what} amin_bar")
                    close(xbar, jt(Jx[:n_het], yb), what=f"{what} xhh_bar")
                    C.transposed_identity(what, K, yb, Jd, xbar, dx, abar, da, moves=False)
                    if path:      # convention (i): exact zeros
                        assert not np.any(abar[[t for t, k in enumerate(c["kinds"]) if k in ("first", "below")]]), what
            tv = hb.last_vjp_timings()
            assert tv["sweep_b"]["launches"] == 2 * P + 3, tv
        finally:
            hb.close()


@grid_cases
def test_vjp_borrow_is_the_transpose_of_jvp_borrow(hank, oracle_mod, family, name, n_a, n_e):
    for T in R.HORIZONS:
        _vjp_borrow_case(hank, R.borrow_case(family, name, n_a, n_e, T), f"{family} {name} {n_a}x{n_e} T={T}")


def test_vjp_borrow_at_every_block_shape_of_the_reduction(hank, oracle_mod):
    """k_brw_abar is launched with RO = AdjGeom::R of the batch width and MC = shk_mc(M) columns across the lanes — k_shk_bbar's pairs:
    one width per pair, and the tails of a last column block"""
    pair = lambda M: (cases.adj_rows_per_block(M), cases.shk_mc(M))                 # noqa: E731
    every = {pair(M) for M in range(1, 257)}
    widths = {}
    for M in (1, 2, 3, 4, 5, 6, 8, 16, 17, 32, 34, 64, 65, 66, 97, 130, 256):
        widths.setdefault(pair(M), M)
    assert set(widths) == every, sorted(every - set(widths))
    c = R.borrow_case("ks", "gamma2", 130, 3, 4)
    _vjp_borrow_case(hank, c, "ks gamma2 130x3 T=4", widths=tuple(sorted(set(widths.values()) | {65, 130})), paths=(True,))


# ---- 4. a raw grid with a deep interior constrained prefix ------------------------------------------------------------------------------
def test_a_raw_grid_with_a_deep_constrained_prefix(hank, oracle_mod):
    """"deep-prefix": 700 rows, dense at the bottom; the limit sits 568 rows into the grid, so period 0's constrained set is an
    interior prefix of more than 400 rows in every column — hundreds of sources on one target row of the forward sweep, many row blocks
    of the seed and of the reduction"""
    c = R.raw_case("deep-prefix")
    ref = path_refs.oracle_path_sweeps(*C.ref_args(K, c))
    assert ref["C"][0].sum(axis=0).min() > 64 and ref["C"][0].sum(axis=0).min() > 2 * cases.adj_rows_per_block(1)
    hb = C.ctx(hank, K, c, None)
    try:
        agg = hb.primal(c["x"])
        close(agg, ref["agg"][:, 0], what="raw deep-prefix aggregate")
        close(hb.policy_seq().transpose(2, 0, 1), ref["pol"], what="raw deep-prefix policy")
    finally:
        hb.close()
    _jvp_borrow_case(hank, c, "raw deep-prefix", widths=(3, 33), t_only=False, paths=(True,))
    _vjp_borrow_case(hank, c, "raw deep-prefix", widths=(1, 33), paths=(True,))


# ---- 5. hank_fake_news_borrow -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("econ", ["ks30x3", "hank30x3"])
@pytest.mark.parametrize("T", [2, 3, 12])
def test_borrow_jacobian_matches_the_reference_at_a_steady_record(hank, oracle_mod, econ, T):
    """on a fresh context, as its first fake-news call; the model's limit lies inside the grid, three or four points below it"""
    from hank_amd.SteadyStateJacobian import borrow_jacobian
    c = R.steady_case(econ)
    P, nh = T - 1, c["n_het"]
    args = c["args"][:6] + (T,) + c["args"][7:]
    hb = cases.raw_block(hank, args, None)
    try:
        hb.set_boundary(c["V"], c["D"])
        hb.set_het_outputs(nh)
        x = np.tile(c["x"][:, None], (1, P))
        hb.primal(x)
        J = borrow_jacobian(hb, nh)                                          # (n_het, P, P)
        _, Ja = path_refs.jacobians(K, args, x, c["V"], c["D"], np.full(P, c["bc"]), c["gamma"], nh)
        for o in range(nh):
            assert np.abs(Ja[:, o]).max() > 1e-3
            close(J[o], Ja[:, o, :], what=f"{econ} T={T} J_amin of output {o}")
        F, Dv = hb.fake_news_borrow(nh)
        assert Dv[0, 0] > 0 and abs(Dv[0, 0] + Dv[0, 1]) <= 1e-12 * abs(Dv[0, 0])      # da' = 1 on C under D_ss; c = .. - a': no direct term
        for n in range(1, nh):
            assert np.array_equal(borrow_jacobian(hb, n), J[:n])
        hb.jvp_borrow(None, np.eye(P))                                       # the device's own unit columns
        _, cols = hb.het_outputs(nh, np.zeros((hb.n_hh, P, P)))
        for o in range(nh):
            close(J[o], cols[:, o, :], what=f"{econ} T={T} J_amin of output {o} against the unit columns")
        hb.set_borrow_path(np.full(P, c["bc"]))
        hb.primal(x)
        C.raises(NOT_READY, hb.fake_news_borrow, nh)
    finally:
        hb.close()


# ---- 6. the record's readers at a path -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,name,n_a,n_e", [("ks", "gamma2", 33, 2), ("hank", "gamma1.5", 130, 3), ("hank", "gamma1", 33, 2)])
def test_the_record_s_readers_work_at_a_path(hank, oracle_mod, family, name, n_a, n_e):
    c = R.borrow_case(family, name, n_a, n_e, 12)
    P, nh = 11, c["n_het"]
    grp = _groups(c)
    hb = C.ctx(hank, K, c, None)
    try:
        hb.set_group_outputs(*grp)
        hb.primal(c["x"])
        dx, _ = path_refs.seeds(K, c, 3, 7)
        ref = path_refs.oracle_path_sweeps(*C.ref_args(K, c), dx=dx, groups=grp)
        Jx, _ = path_refs.jacobians(*C.ref_args(K, c))
        what = f"{family} {name} {n_a}x{n_e}"
        close(hb.jvp_het(dx, n_het=nh), ref["dagg"], what=f"{what} hank_jvp_het")
        hb.jvp(dx)
        g, dg = hb.group_outputs(dx)
        close(g, ref["grp"], what=f"{what} group levels")
        close(dg, ref["dgrp"], what=f"{what} group tangents")
        assert all(np.abs(ref["grp"][:, k]).max() > 0 and np.abs(ref["dgrp"][:, k]).max() > 0 for k in range(4))
        yb = np.random.default_rng(3).standard_normal((P, nh, 3))
        close(hb.vjp_het(yb, nh), jt(Jx, yb), what=f"{what} hank_vjp_het")
        gb = np.random.default_rng(4).standard_normal((P, 4, 3))
        xbar = hb.vjp_group(gb)
        lhs = np.einsum("tkm,tkn->mn", gb, dg)                                    # the device's own tangents: the transposed identity
        rhs = np.einsum("ktm,ktn->mn", xbar, dx)
        scale = np.einsum("tkm,tkn->mn", np.abs(gb), np.abs(dg))
        print(f"{what} hank_vjp_group: max |lhs - rhs| / scale = {np.max(np.abs(lhs - rhs) / scale):.3e}")
        assert np.all(np.abs(lhs - rhs) <= 1e-10 * scale), (what, np.max(np.abs(lhs - rhs) / scale))
        step = [hb.backward_step(c["V"], c["x"][:, 0]), hb.backward_step_dual(c["V"], np.ones(c["V"].shape + (2,)), c["x"][:, 0], np.ones((hb.n_hh, 2)))]
    finally:
        hb.close()
    hb = C.ctx(hank, K, c, None, path=False)                                         # the step entries keep the model's constant: no path's bits
    try:
        same = [hb.backward_step(c["V"], c["x"][:, 0]), hb.backward_step_dual(c["V"], np.ones(c["V"].shape + (2,)), c["x"][:, 0], np.ones((hb.n_hh, 2)))]
        for got, want in zip(step, same):
            assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want)), what
        st, Vo, Ko = c["orc"].value_function(c["V"], c["x"][0, 0], c["x"][1, 0], 1, c["x"][2, 0] if hb.n_hh > 2 else None)
        assert st == 0
        close(step[0][1], Ko[..., 0], what=f"{what} hank_backward_step's policy at the model's limit")
    finally:
        hb.close()


# ---- 7. refusals, exclusions, invalidation ---------------------------------------------------------------------------------------------------
def test_entries_defined_at_one_limit_are_refused_while_a_path_is_set(hank, oracle_mod):
    c = S.case("ks30x3")
    P, nh = S.T_SHORT - 1, c["n_het"]
    hb = cases.raw_block(hank, c["args"], None)
    try:
        hb.set_boundary(c["V"], c["D"])
        hb.set_het_outputs(nh)
        hb.set_group_outputs(np.ones((hb.G, 1)), np.array([1], dtype=np.int32))
        x = FR.constant_path(c, P)
        dx = np.full((hb.n_hh, P, 2), 1e-3)
        yb = np.ones((P, 2, 2))
        calls = {
            "primal_batch": lambda: hb.primal_batch(x[:, :, None], 1),
            "ss_batch": lambda: hb.ss_batch(c["x"], 1e-8, 1, vfi_max_iter=50, dist_max_iter=50),
            "vfi": lambda: hb.vfi(np.ones((hb.n_a, hb.n_e)), c["x"], 1e-8, 50),
            "ss_jvp": lambda: hb.ss_jvp(np.ones(hb.n_hh), nh, 1e-6, 500, check=False),
            "ss_vjp": lambda: hb.ss_vjp(np.ones(nh), n_het=nh, tol=1e-6, max_iter=500, check=False),
            "fake_news": hb.fake_news,
            "fake_news_het": lambda: hb.fake_news_het(nh),
            "fake_news_group": hb.fake_news_group,
            "fake_news_shock": lambda: hb.fake_news_shock(nh),
            "fake_news_income": lambda: hb.fake_news_income(2),
            "fake_news_borrow": lambda: hb.fake_news_borrow(nh),
        }
        a = np.asarray(c["args"][0])
        amin = np.full(P, 0.5 * (a[1] + a[2]))
        hb.set_borrow_path(amin)
        hb.primal(x)
        dagg = hb.jvp(dx)
        for k, f in calls.items():
            C.raises(NOT_READY, f)
            assert np.array_equal(hb.jvp(dx), dagg), k                              # the record is still valid
        # each pair of setters, and the other kinds' entries under this path
        for f in (lambda: hb.jvp_shock(dx, None), lambda: hb.vjp_shock(yb, 2), lambda: hb.jvp_income(dx, None), lambda: hb.vjp_income(yb, 2)):
            C.raises(NOT_READY, f)
        C.raises(NOT_READY, hb.set_discount_path, np.full(P, c["args"][3]))
        C.raises(NOT_READY, hb.set_income_path, np.zeros((hb.n_e, P)))
        assert np.array_equal(hb.borrow_path, amin) and hb.discount_path is None and hb.income_path is None
        assert np.array_equal(hb.jvp(dx), dagg)
        hb.set_borrow_path(None)
        C.raises(NOT_READY, hb.jvp, dx)                                           # clearing drops the record too
        hb.primal(x)
        for k, f in calls.items():
            f()
        for setter, path in ((hb.set_discount_path, np.full(P, c["args"][3])), (hb.set_income_path, np.zeros((hb.n_e, P)))):
            setter(path)
            C.raises(NOT_READY, hb.set_borrow_path, amin)
            hb.primal(x)
            C.raises(NOT_READY, hb.jvp_borrow, dx, None)
            C.raises(NOT_READY, hb.vjp_borrow, yb, 2)
            assert hb.borrow_path is None
            setter(None)
    finally:
        hb.close()


def test_a_bad_path_changes_nothing_and_a_new_path_drops_the_record(hank, oracle_mod):
    c = R.borrow_case("ks", "gamma2", 33, 2, 4)
    top = float(np.asarray(c["args"][0])[-1])
    am = c["amin"].copy()
    am[0] += 1e-3
    C.bad_path_and_new_path(hank, K, c, bad=(np.nan, np.inf, -np.inf, np.nextafter(top, np.inf)), at=1, new=am, vjp=lambda hb: hb.vjp_borrow(np.ones((3, 1, 1)), 1),
                            own_entry=True)


def test_a_second_path_and_a_second_boundary_on_cached_graphs_and_the_dev_forms(hank, oracle_mod):
    """the graphs of a width hold the address of the path's values, not the values: a second path and a second boundary are served by
    the graphs the first captured. The _dev forms give the host forms' bits."""
    import torch
    c = R.borrow_case("hank", "gamma2", 33, 2, 4)
    P, nh, N = 3, c["n_het"], 3
    hb = C.ctx(hank, K, c, None)
    try:
        dx, da = path_refs.seeds(K, c, N, 2)
        yb = np.random.default_rng(1).standard_normal((P, 2, N))
        am2 = c["amin"][::-1].copy()
        V2 = c["V"] * 1.01
        for amin, V in ((c["amin"], c["V"]), (am2, c["V"]), (am2, V2)):
            hb.set_boundary(V, c["D"])
            hb.set_borrow_path(amin)
            hb.primal(c["x"])
            J = path_refs.jacobians(K, c["args"], c["x"], V, c["D"], amin, c["gamma"], nh)
            dagg = hb.jvp_borrow(dx, da)
            close(dagg, path_refs.linear(J, dx, da)[:, 0, :], what="hank_jvp_borrow on the cached graphs")
            xbar, abar = hb.vjp_borrow(yb, 2)
            close(abar, path_refs.path_bar(J[1], yb), what="hank_vjp_borrow on the cached graphs")
            dev = lambda v: torch.tensor(np.asfortranarray(v).ravel(order="F"), device="cuda")      # noqa: E731
            d_dx, d_da, d_out = dev(dx), dev(da), torch.empty(P * N, dtype=torch.float64, device="cuda")
            hb.jvp_borrow_dev(d_dx.data_ptr(), d_da.data_ptr(), N, d_out.data_ptr())
            hb.sync()
            assert np.array_equal(d_out.cpu().numpy().reshape((P, N), order="F"), dagg)
            d_yb, d_x, d_a = dev(yb), torch.empty(hb.n_hh * P * N, dtype=torch.float64, device="cuda"), torch.empty(P * N, dtype=torch.float64, device="cuda")
            hb.vjp_borrow_dev(2, d_yb.data_ptr(), N, d_x.data_ptr(), d_a.data_ptr())
            hb.sync()
            assert np.array_equal(d_a.cpu().numpy().reshape((P, N), order="F"), abar)
            assert np.array_equal(d_x.cpu().numpy().reshape((hb.n_hh, P, N), order="F"), xbar)
    finally:
        hb.close()


def test_clone_carries_the_path_and_the_memo_does_not_serve_another(hank, oracle_mod):
    c = R.borrow_case("hank", "gamma2", 33, 2, 4)
    ref = lambda k, p, dx: path_refs.oracle_path_sweeps(K, c["args"], c["x"], c["V"], c["D"], p, c["gamma"], 2, dx=dx)      # noqa: E731
    C.memo_and_clone(hank, K, c, c["amin"][::-1].copy(), ref, hits=False)
