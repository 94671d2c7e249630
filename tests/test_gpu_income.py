"""The income path by productivity state on the device (hank_set_income_path, hank_jvp_income, hank_vjp_income, hank_fake_news_income,
hank_get_het_outputs_income) through the C ABI, against tests/path_refs.oracle_path_sweeps at tests/income_refs.KIND — the CPU oracle's EGM step run once per
productivity state with the dual transfer (tr_t + y_t[e], dtr_t + dy_t[e]) and the columns assembled, which tests/test_income_host.py
pins against a central difference of its own level.

Shapes: the grids of cases.ENTRY_GRIDS — (33, 2): two primal blocks, the second holding one row; (130, 3) — both families, every gamma
of cases.ENTRY_CASES with its record diet (gamma = 1 and 2 rebuild kc from s and v from u: where a missed + y shows), horizons T = 2,
3, 4 and 12 (P = 1: only the -rho dy term of the seed; P = 2 separates y_0 and y_{P-1}), widths 1, 3 and 33, N = 96 once at
cases.ENTRY_WIDE (n_e = 11), a raw grid with deep clamps and "swing", where every column is clamped in one period and consumption
moves one for one with y. The path alternates in sign across e, decays in t and is 2 % of the smallest w z_e. Tolerance: cases.close
(rel 1e-10 + abs 1e-12) against the oracle; bits where the header promises bits; the transposed identity at 1e-10 of the summed
magnitudes."""
import numpy as np
import pytest

import cases
import fake_news_refs as FR
import income_refs as R
import path_checks as C
import path_refs
import ss_diff_cases as S
from cases import close, jt
from hank_amd.hip import _p
from path_checks import BAD_ARG, NOT_READY, grid_cases

pytestmark = pytest.mark.gpu

K = R.KIND


# ---- 1. the level -------------------------------------------------------------------------------------------------------------------
def _level(hank, c, what, schedules=("launch", "xcd")):
    ref = path_refs.oracle_path_sweeps(*C.ref_args(K, c))
    P = c["x"].shape[1]
    got = {}
    for sched in schedules:
        hb = C.ctx(hank, K, c, sched)
        try:
            before = hb.stats()
            agg0 = hb.primal(c["x"])
            agg, none = hb.het_outputs(2)
            assert none is None
            got[sched] = (agg0, agg, hb.policy_seq(), hb.dist_seq())
            st, tm = hb.stats(), hb.last_timings()
            assert st["fallbacks"] == 0 and st["sweep_launches"] == before["sweep_launches"], (what, sched, st)
            assert st["schedule"] == before["schedule"], (what, sched, st)
            assert tm["primal_backward"]["launches"] == P + 2 and tm["primal_backward"]["ms"] > 0, (what, sched, tm)
        finally:
            hb.close()
    agg0, agg, pol, dist = got[schedules[0]]
    close(agg0, ref["agg"][:, 0], what=f"{what} aggregate")
    for o in range(2):
        close(agg[:, o], ref["agg"][:, o], what=f"{what} output {o}")
    close(pol.transpose(2, 0, 1), ref["pol"], what=f"{what} policy")
    close(dist.transpose(2, 0, 1), ref["Dseq"], what=f"{what} distribution")
    for sched in schedules[1:]:
        assert all(np.array_equal(g, l) for g, l in zip(got[sched], got[schedules[0]])), (what, sched)
    return ref


@grid_cases
def test_primal_at_a_path_matches_the_oracle_under_every_schedule(hank, oracle_mod, family, name, n_a, n_e):
    for T in R.HORIZONS:
        c = R.income_case(family, name, n_a, n_e, T)
        what = f"{family} {name} {n_a}x{n_e} T={T}"
        ref = _level(hank, c, what)
        assert np.abs(ref["pol"] - path_refs.oracle_path_sweeps(*C.ref_args(K, c, False))["pol"]).max() > 1e-3, what      # (the path moves the policy)


@grid_cases
def test_a_path_of_zeros_gives_the_bits_of_no_path(hank, oracle_mod, family, name, n_a, n_e):
    for T in R.HORIZONS:
        C.neutral_path_gives_the_bits_of_no_path(hank, K, R.income_case(family, name, n_a, n_e, T), (family, name, n_a, n_e, T), het=2)


# ---- 2. hank_jvp_income ---------------------------------------------------------------------------------------------------------------
def _income_against_oracle(hb, c, tag, dx, dy, path):
    a = C.ref_args(K, c, path)
    N = next(v.shape[-1] for v in (dx, dy) if v is not None)
    ref = path_refs.linear(path_refs.jacobians(*a), dx, dy)
    dpol = path_refs.linear_policies(*a, dx=dx, dp=dy)
    close(hb.jvp_income(dx, dy), ref[:, 0, :], what=f"{tag} dagg")
    close(hb.dpolicy_seq(N).transpose(2, 0, 1, 3), dpol, what=f"{tag} dpolicy")
    _, dagg = hb.het_outputs(2, dx, dy=np.zeros((hb.n_e, hb.P, N)) if dy is None else dy)
    for o in range(2):
        assert np.abs(ref[:, o, :]).max() > 1e-6, (tag, o)
        close(dagg[:, o, :], ref[:, o, :], what=f"{tag} output {o}")


def _jvp_income_case(hank, c, tag, widths=R.WIDTHS, t_only=True, schedule=None):
    P = c["x"].shape[1]
    for path in (True, False):
        hb = C.ctx(hank, K, c, schedule, path=path)
        try:
            hb.primal(c["x"])
            tg = f"{tag} {'path' if path else 'no path'}"
            # the sweeps themselves once, against the linear reference every width uses
            dx, dy = path_refs.seeds(K, c, 3, 10)
            own = path_refs.oracle_path_sweeps(*C.ref_args(K, c, path), dx=dx, dpath=dy)
            lin = path_refs.linear(path_refs.jacobians(*C.ref_args(K, c, path)), dx, dy)
            close(lin, own["dagg"], rel=1e-12, ab=0.0, what=f"{tg} the reference is linear")
            for N in widths:
                dx, dy = path_refs.seeds(K, c, N, 11 + N)
                _income_against_oracle(hb, c, f"{tg} N={N} inputs and y", dx, dy, path)
                _income_against_oracle(hb, c, f"{tg} N={N} y alone", None, dy, path)
                _income_against_oracle(hb, c, f"{tg} N={N} inputs alone", dx, None, path)
            if t_only:
                for t in sorted({0, P - 1}):
                    dx, dy = path_refs.seeds(K, c, 3, 13, t_only=t)
                    _income_against_oracle(hb, c, f"{tg} N=3 y_{t} alone", None, dy, path)
            tm = hb.last_timings()
            assert tm["tangent_backward"]["launches"] == 2 * P + 3 and tm["tangent_forward"]["launches"] == P + 3, (tg, tm)
            assert hb.info()["last_tangent_family_name"] == cases.FAMILY["launch"] and hb.stats()["fallbacks"] == 0
        finally:
            hb.close()


@grid_cases
def test_jvp_income_matches_the_oracle(hank, oracle_mod, family, name, n_a, n_e):
    for T in R.HORIZONS:
        _jvp_income_case(hank, R.income_case(family, name, n_a, n_e, T), f"{family} {name} {n_a}x{n_e} T={T}")


def test_jvp_income_at_eleven_states_and_96_directions(hank, oracle_mod):
    c = R.income_case("ks", "gamma2", *cases.ENTRY_WIDE, 12)
    _level(hank, c, "ks gamma2 40x11 T=12")
    _jvp_income_case(hank, c, "ks gamma2 40x11 T=12", widths=(96,), t_only=False)


def test_jvp_income_where_the_seed_s_staging_does_not_fit(hank, oracle_mod):
    """k_inc_seed_back stages Pi and two dy slices, n_e n_e + 2 n_e N doubles, in LDS up to 48 KiB and reads global memory beyond: at
    n_e = 11 that is from N = 274 on"""
    c = R.income_case("ks", "gamma2", *cases.ENTRY_WIDE, 4)
    n_e = c["y"].shape[0]
    assert 8 * (n_e * n_e + 2 * n_e * 273) <= 48 * 1024 < 8 * (n_e * n_e + 2 * n_e * 288)
    _jvp_income_case(hank, c, "ks gamma2 40x11 T=4", widths=(273, 288), t_only=False)


@grid_cases
def test_jvp_income_without_an_income_seed_is_hank_jvp_bit_for_bit(hank, oracle_mod, family, name, n_a, n_e):
    for T in (2, 4):
        C.no_seed_in_the_path_is_hank_jvp_bit_for_bit(hank, K, R.income_case(family, name, n_a, n_e, T), (family, name, n_a, n_e, T), R.WIDTHS, direct=True)


# ---- 3. hank_vjp_income ----------------------------------------------------------------------------------------------------------------
def _vjp_income_case(hank, c, tag, widths=R.WIDTHS, schedule=None):
    P = c["x"].shape[1]
    rng = np.random.default_rng(P)
    for path in (True, False):
        hb = C.ctx(hank, K, c, schedule, path=path)
        try:
            hb.primal(c["x"])
            Jx, Jy = path_refs.jacobians(*C.ref_args(K, c, path))
            dx, dy = path_refs.seeds(K, c, 3, 21)
            hb.jvp_income(dx, dy)
            _, Jd = hb.het_outputs(2, dx, dy=dy)                                  # (P, 2, N)
            for M in widths:
                for n_het in (1, 2):
                    what = f"{tag} path={path} M={M} n_het={n_het}"
                    yb = rng.standard_normal((P, n_het, M))
                    xbar, ybar = hb.vjp_income(yb, n_het)
                    assert np.array_equal(xbar, hb.vjp(yb, n_het)), what
                    x2, y2 = hb.vjp_income(yb, n_het)
                    assert np.array_equal(x2, xbar) and np.array_equal(y2, ybar), what
                    close(ybar, path_refs.path_bar(Jy, yb), what=f"{what} y_bar")
                    close(xbar, jt(Jx[:n_het], yb), what=f"{what} xhh_bar")
                    C.transposed_identity(what, K, yb, Jd, xbar, dx, ybar, dy)
            tv = hb.last_vjp_timings()
            assert tv["sweep_b"]["launches"] == 2 * P + 3, tv
        finally:
            hb.close()


@grid_cases
def test_vjp_income_is_the_transpose_of_jvp_income(hank, oracle_mod, family, name, n_a, n_e):
    for T in R.HORIZONS:
        _vjp_income_case(hank, R.income_case(family, name, n_a, n_e, T), f"{family} {name} {n_a}x{n_e} T={T}")


def test_vjp_income_at_eleven_states(hank, oracle_mod):
    _vjp_income_case(hank, R.income_case("ks", "gamma2", *cases.ENTRY_WIDE, 12), "ks gamma2 40x11 T=12", widths=(3, 96))


# ---- 4. clamped columns ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("econ", ["both", "swing"])
def test_raw_grids_with_clamped_columns(hank, oracle_mod, econ):
    """"both": clamped prefixes of 39..58 rows and sources capped at the top; "swing": every column clamped in period 1, none in period
    2. At a clamped row the policy does not move (da' = 0) and consumption moves one for one with y: the direct term carries it."""
    c = R.raw_case(econ)
    ref = _level(hank, c, f"raw {econ}")
    clamped = ref["pol"] <= c["grid"][0]
    assert clamped.any(axis=1).any(), econ
    if econ == "swing":
        assert clamped[1].any(axis=0).all() and not clamped[2].any(), econ
    P, n_e = c["x"].shape[1], c["y"].shape[0]
    dy = np.eye(n_e * P).reshape((n_e, P, n_e * P), order="F")
    dpol = path_refs.linear_policies(*C.ref_args(K, c), dp=dy)                        # [t, a, e, (e', s)]
    for t, a, e in zip(*np.nonzero(clamped)):
        assert not np.any(dpol[t, a, e]), (econ, t, a, e)
    _jvp_income_case(hank, c, f"raw {econ}", widths=(3, 33), t_only=False)
    _vjp_income_case(hank, c, f"raw {econ}", widths=(1, 33))


# ---- 5. hank_fake_news_income ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("econ", ["ks30x3", "hank30x3"])
def test_income_jacobian_matches_the_reference_at_a_steady_record(hank, oracle_mod, econ):
    from hank_amd.SteadyStateJacobian import income_jacobian
    c = S.case(econ)
    T = 12
    P = T - 1
    hb = cases.raw_block(hank, c["args"][:6] + (T,) + c["args"][7:], None)
    try:
        hb.set_boundary(c["V"], c["D"])
        x = FR.constant_path(c, P)
        hb.primal(x)
        J = income_jacobian(hb, 2)                                           # (2, P, n_e, P)
        _, Jy = path_refs.jacobians(K, c["orc"], x, c["V"], c["D"], None)
        mass = path_refs.oracle_path_sweeps(K, c["orc"], x, c["V"], c["D"])["mass"]
        for o in range(2):
            assert np.abs(Jy[:, o]).max() > 1e-3
            close(J[o], Jy[:, o], what=f"{econ} J_y of output {o}")
        F, Dv = hb.fake_news_income(2)
        F1, Dv1 = hb.fake_news_income(1)
        assert np.array_equal(F1[..., 0], F[..., 0]) and np.array_equal(Dv1[..., 0], Dv[..., 0])
        # consumption's direct term: c = .. + y - a', so the policy parts of Dv cancel between the two outputs and m_ss[e] is left at lag 0
        close(Dv[0, :, 0] + Dv[0, :, 1], mass[0], what=f"{econ} direct term")
        assert np.abs(Dv[1:, :, 0] + Dv[1:, :, 1]).max() <= 1e-13 * np.abs(Dv).max(), econ
        out = np.empty(P * P * hb.n_e * 3)
        assert hb._lib.hank_fake_news_income(hb._ctx, 3, _p(out), _p(out)) == BAD_ARG
        hb.jvp_income(None, np.eye(hb.n_e * P).reshape((hb.n_e, P, hb.n_e * P), order="F"))      # the device's own unit columns
        _, cols = hb.het_outputs(2, None, dy=np.eye(hb.n_e * P).reshape((hb.n_e, P, hb.n_e * P), order="F"))
        for o in range(2):
            close(J[o], cols[:, o, :].reshape(P, P, hb.n_e).transpose(0, 2, 1), what=f"{econ} J_y of output {o} against the unit columns")
        hb.set_income_path(np.zeros((hb.n_e, P)))
        hb.primal(x)
        C.raises(NOT_READY, hb.fake_news_income, 2)
    finally:
        hb.close()


def test_fake_news_with_fewer_states_than_inputs_on_a_fresh_context(hank, oracle_mod):
    """n_e = 2 < n_hh = 3, and the income (or the beta) entry as the FIRST fake-news call of its context: the shared workspace is sized
    by the widest batch so far, and the record kernels write every output's direct sums over the n_hh inputs whatever the batch is"""
    from hank_amd.SteadyStateJacobian import income_jacobian, shock_jacobian
    c = R.two_state_hank()
    P = c["args"][6] - 1
    x = np.tile(c["x"][:, None], (1, P))
    _, Jy = path_refs.jacobians(K, c["orc"], x, c["V"], c["D"], None)
    het = None
    for first in ("income", "shock", "het"):
        hb = cases.raw_block(hank, c["args"], None)
        try:
            assert hb.n_e == 2 and hb.n_hh == 3
            hb.set_boundary(c["V"], c["D"])
            hb.primal(x)
            calls = {"income": lambda: income_jacobian(hb, 2), "shock": lambda: shock_jacobian(hb, 2), "het": lambda: hb.fake_news_het(2)}
            got = {first: calls[first]()}
            for k in calls:
                if k != first:
                    got[k] = calls[k]()
            for o in range(2):
                close(got["income"][o], Jy[:, o], what=f"hank 30x2, {first} first: J_y of output {o}")
            hb.jvp_shock(None, np.eye(P))
            _, cols = hb.het_outputs(2, np.zeros((3, P, P)))
            for o in range(2):
                close(got["shock"][o], cols[:, o, :], what=f"hank 30x2, {first} first: J_beta of output {o}")
            if het is None:
                het = got["het"]
            assert all(np.array_equal(g, h) for g, h in zip(got["het"], het)), first      # (the order of the calls moves no bit)
        finally:
            hb.close()


def test_a_batch_with_income_directions_carries_them(hank, oracle_mod):
    """consumption has a direct term in dy: hank_get_het_outputs adds it from the batch's own dy, and the readers that rebuild c from
    the inputs refuse the batch's tangents — with or without a path set — until hank_jvp makes another"""
    c = R.income_case("hank", "gamma2", 33, 2, 4)
    P, N = 3, 3
    dx, dy = path_refs.seeds(K, c, N, 4)
    cons_group = (np.ones((33 * 2, 2)), np.array([1, 2], dtype=np.int32))
    for path in (False, True):
        hb = C.ctx(hank, K, c, None, path=path)
        try:
            hb.set_het_outputs(4)
            hb.set_group_outputs(*cons_group)
            hb.primal(c["x"])
            ref = path_refs.linear(path_refs.jacobians(*C.ref_args(K, c, path)), dx, dy)
            hb.jvp_income(dx, dy)
            _, own = hb.het_outputs(2, dx)                                       # the batch's own dy
            _, given = hb.het_outputs(2, dx, dy=dy)
            assert np.array_equal(own, given), path
            close(own[:, 1, :], ref[:, 1, :], what=f"path={path}: consumption's tangent from the batch's own dy")
            C.raises(NOT_READY, hb.het_outputs, 3, dx)
            C.raises(NOT_READY, hb.group_outputs, dx)
            hb.het_outputs(2)                                                    # the levels of outputs 0 and 1 are always served
            if not path:
                hb.het_outputs(3)                                                # ... and every level and tangent where c is rebuilt rightly
                hb.group_outputs()
                hb.jvp_income(dx, None)                                          # no income directions: hank_jvp's batch
                hb.het_outputs(3, dx)
                hb.group_outputs(dx)
                hb.jvp_income(dx, dy)
                C.raises(NOT_READY, hb.het_outputs, 3, dx)
                hb.jvp(dx)
                _, plain = hb.het_outputs(3, dx)
                close(plain[:, 1, :], path_refs.linear(path_refs.jacobians(*C.ref_args(K, c, path)), dx, None)[:, 1, :], what="after hank_jvp: no direct term")
                hb.group_outputs(dx)
        finally:
            hb.close()


# ---- 6. refusals and invalidation ---------------------------------------------------------------------------------------------------------
def test_entries_that_rebuild_consumption_are_refused_while_a_path_is_set(hank, oracle_mod):
    c = S.case("ks30x3")
    P, nh = S.T_SHORT - 1, c["n_het"]
    hb = cases.raw_block(hank, c["args"], None)
    try:
        hb.set_boundary(c["V"], c["D"])
        hb.set_het_outputs(nh)
        G, N = hb.G, 2
        x = FR.constant_path(c, P)
        dx = np.full((hb.n_hh, P, N), 1e-3)
        dV = np.zeros((hb.n_a, hb.n_e, N))
        yb = np.ones((P, 2, N))
        cons_group = (np.ones((G, 1)), np.array([hb.GROUP_CONS], dtype=np.int32))
        mass_groups = (np.ones((G, 2)), np.array([hb.GROUP_MASS, hb.GROUP_POLICY], dtype=np.int32))
        calls = {
            "het_outputs(3)": lambda: hb.het_outputs(nh),
            "jvp_het": lambda: hb.jvp_het(dx, n_het=2),
            "vjp_het": lambda: hb.vjp_het(yb, 2),
            "vjp_het_boundary": lambda: hb.vjp_het_boundary(yb, 2),
            "vjp_group": lambda: hb.vjp_group(np.ones((P, 2, N))),
            "jvp_boundary": lambda: hb.jvp_boundary(dx, dV, None),
            "vjp_boundary": lambda: hb.vjp_boundary(yb, 2),
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
            "set_discount_path": lambda: hb.set_discount_path(np.full(P, c["args"][3])),
        }
        y = R.income_path(hb.z_grid, x)
        hb.set_group_outputs(*mass_groups)
        hb.set_income_path(y)
        hb.primal(x)
        dagg = hb.jvp(dx)
        for k, f in calls.items():
            C.raises(NOT_READY, f)
            assert np.array_equal(hb.jvp(dx), dagg), k                              # the record is still valid
        assert np.array_equal(hb.income_path, y) and hb.discount_path is None
        grp, dgrp = hb.group_outputs(dx)                                          # the mass and policy bases read the record
        close(dgrp[:, 1, :], dagg, what="the policy base over every point is the aggregate's tangent")
        close(grp[:, 0], np.ones(P), what="the mass base over every point is one")
        hb.set_group_outputs(*cons_group)
        C.raises(NOT_READY, hb.group_outputs)
        assert np.array_equal(hb.jvp(dx), dagg)
        hb.backward_step(c["V"], c["x"])                                          # the step entries ignore the path
        hb.set_income_path(None)
        C.raises(NOT_READY, hb.jvp, dx)                                           # clearing drops the record too
        hb.primal(x)
        hb.set_group_outputs(*mass_groups)
        del calls["set_discount_path"]
        for k, f in calls.items():
            f()
        hb.set_discount_path(np.full(P, c["args"][3]))
        C.raises(NOT_READY, hb.set_income_path, y)                                 # the two paths exclude each other
        hb.primal(x)
        C.raises(NOT_READY, hb.jvp_income, dx, None)
        C.raises(NOT_READY, hb.vjp_income, yb, 2)
    finally:
        hb.close()


def test_a_bad_path_changes_nothing_and_a_new_path_drops_the_record(hank, oracle_mod):
    c = R.income_case("ks", "gamma2", 33, 2, 4)
    C.bad_path_and_new_path(hank, K, c, bad=(np.nan, np.inf, -np.inf), at=(1, 1), new=c["y"] * 1.001, vjp=lambda hb: hb.vjp_income(np.ones((3, 1))), own_entry=True)


def test_the_primal_memo_does_not_serve_another_path_and_clone_carries_the_path(hank, oracle_mod):
    c = R.income_case("hank", "gamma2", 33, 2, 4)
    C.memo_and_clone(hank, K, c, -c["y"], lambda k, p, dx: path_refs.oracle_path_sweeps(K, c["orc"], c["x"], c["V"], c["D"], p, dx=dx), hits=True)


def test_a_forced_persistent_schedule_runs_the_launches_at_a_path(hank, oracle_mod):
    c = R.income_case("ks", "gamma2", 130, 3, 12)
    hb = C.ctx(hank, K, c, "xcd")
    try:
        hb.primal(c["x"])
        dx, dy = path_refs.seeds(K, c, 33, 3)
        ref = path_refs.linear(path_refs.jacobians(*C.ref_args(K, c)), dx, None)
        close(hb.jvp(dx), ref[:, 0, :], what="hank_jvp at a path under HANK_SCHEDULE=xcd")
        assert hb.info()["last_tangent_family_name"] == cases.FAMILY["launch"], hb.info()
        agg, dagg = hb.primal_jvp(c["x"] * 1.0, dx)
        close(dagg, ref[:, 0, :], what="hank_primal_jvp at a path under HANK_SCHEDULE=xcd")
        st = hb.stats()
        assert st["fallbacks"] == 0 and st["sweep_launches"] == 0 and st["schedule"] == 1, st
        tm = hb.last_timings()
        assert tm["primal_backward"]["launches"] == 13 and tm["tangent_backward"]["launches"] == 13, tm
    finally:
        hb.close()
