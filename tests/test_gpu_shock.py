"""The discount-factor path on the device (hank_set_discount_path, hank_jvp_shock, hank_vjp_shock, hank_fake_news_shock) through the C
ABI, against tests/path_refs.oracle_path_sweeps at tests/shock_refs.KIND — the CPU oracle's loop with beta = beta_t per period and the value's partials
augmented by V dbeta_t / beta_t, which tests/test_shock_host.py pins against a central difference of its own level.

Shapes: the grids of cases.ENTRY_GRIDS — (33, 2): two primal blocks, the second holding one row; (130, 3) — both families, every gamma
of cases.ENTRY_CASES (gamma = 1 and 2 with the record diet on, where the persistent and wide tangent sweeps rebuild kc from the MODEL's
beta; general gammas and the diet switched off), horizons T = 2, 3, 4 and 12 (P = 1 makes beta_0 and beta_{P-1} the same entry, P = 2
separates them), widths 1, 3 and 33, and N = 96 once at cases.ENTRY_WIDE. Tolerance: cases.close (rel 1e-10 + abs 1e-12) against the
oracle; bits where the header promises bits; the transposed identity under the projection bound of tests/test_gpu_vjp_variants.py
(1e-10 of the summed magnitudes); hank_fake_news_shock under cases.close, as tests/test_gpu_fake_news_dense.py. Every other width, n_e,
the raw grids with deep clamps and the oracle's own beta_bar are in tests/test_gpu_shock_geometry.py."""
import numpy as np
import pytest

import cases
import fake_news_refs as FR
import path_checks as C
import path_refs
import shock_refs as R
import ss_diff_cases as S
from cases import close
from path_checks import NOT_READY, grid_cases

pytestmark = pytest.mark.gpu

K = R.KIND
_REF = {}


def _ref(c, key, **kw):
    """path_refs.oracle_path_sweeps of case c, once per session and key; path: the beta path (None: the model's constant)"""
    k = (id(c), key)
    if k not in _REF:
        P = c["x"].shape[1]
        path = kw.pop("path", c["path"])
        _REF[k] = path_refs.oracle_path_sweeps(K, c["orc"], c["x"], c["V"], c["D"], np.full(P, c["beta"]) if path is None else path, c["gamma"], c["n_het"], **kw)
    return _REF[k]


def _groups(c):
    """two groups: the lower half of the wealth grid's savings, and consumption under smooth positive weights"""
    n_a, n_e = c["V"].shape
    W = np.zeros((n_a, n_e, 2))
    W[: n_a // 2, :, 0] = 1.0
    W[:, :, 1] = (0.5 + np.linspace(0.0, 1.0, n_a))[:, None] * (1.0 + 0.25 * np.arange(n_e))[None, :]
    return W.reshape((n_a * n_e, 2), order="F"), np.array([1, 2], dtype=np.int32)


# ---- 1. the level -------------------------------------------------------------------------------------------------------------------
@grid_cases
def test_primal_at_a_path_matches_the_oracle_under_every_schedule(hank, oracle_mod, family, name, n_a, n_e):
    for T in R.HORIZONS:
        c = R.shock_case(family, name, n_a, n_e, T)
        ref = _ref(c, "level")
        what = f"{family} {name} {n_a}x{n_e} T={T}"
        got = {}
        for sched in ("launch", "xcd", "wide"):
            hb = C.ctx(hank, K, c, sched)
            try:
                before = hb.stats()
                agg0 = hb.primal(c["x"])
                agg, _ = hb.het_outputs(c["n_het"])
                got[sched] = (agg0, agg, hb.policy_seq())
                st, tm = hb.stats(), hb.last_timings()
                assert st["fallbacks"] == 0 and st["sweep_launches"] == before["sweep_launches"], (what, sched, st)
                assert st["schedule"] == before["schedule"], (what, sched, st)
                assert tm["primal_backward"]["launches"] == T + 1 and tm["primal_backward"]["ms"] > 0, (what, sched, tm)
            finally:
                hb.close()
        agg0, agg, pol = got["launch"]
        close(agg0, ref["agg"][:, 0], what=f"{what} aggregate")
        for o in range(c["n_het"]):
            close(agg[:, o], ref["agg"][:, o], what=f"{what} output {o}")
        close(pol.transpose(2, 0, 1), ref["pol"], what=f"{what} policy")
        assert np.abs(ref["pol"] - _ref(c, "level-const", path=None)["pol"]).max() > 1e-3, what      # (the path moves the policy)
        for sched in ("xcd", "wide"):
            assert all(np.array_equal(g, l) for g, l in zip(got[sched], got["launch"])), (what, sched)


@grid_cases
def test_a_constant_path_gives_the_bits_of_no_path(hank, oracle_mod, family, name, n_a, n_e):
    for T in R.HORIZONS:
        C.neutral_path_gives_the_bits_of_no_path(hank, K, R.shock_case(family, name, n_a, n_e, T), (family, name, n_a, n_e, T))


# ---- 2. hank_jvp at a beta-path record ----------------------------------------------------------------------------------------------
def _jvp_at_path(hank, c, sched, N, what):
    y, _ = path_refs.seeds(K, c, N, 7)
    ref = _ref(c, ("inputs", N), dx=y)
    hb = C.ctx(hank, K, c, sched)
    try:
        hb.primal(c["x"])
        close(hb.jvp(y), ref["dagg"][:, 0, :], what=f"{what} hank_jvp")
        close(hb.dpolicy_seq(N).transpose(2, 0, 1, 3), ref["dpol"], what=f"{what} dpolicy")
        _, dagg = hb.het_outputs(c["n_het"], y)
        for o in range(c["n_het"]):
            close(dagg[:, o, :], ref["dagg"][:, o, :], what=f"{what} output {o}")
        assert hb.info()["last_tangent_family_name"] == cases.FAMILY["launch"] and hb.stats()["fallbacks"] == 0, (what, hb.info(), hb.stats())
        agg, dagg2 = hb.primal_jvp(c["x"] * 1.0, y)      # the Dual pass's entry at a path: the launches too
        close(dagg2, ref["dagg"][:, 0, :], what=f"{what} hank_primal_jvp")
        close(agg, ref["agg"][:, 0], what=f"{what} hank_primal_jvp value")
        assert hb.stats()["sweep_launches"] == 0, (what, hb.stats())      # no persistent sweep ran on this context
    finally:
        hb.close()


@grid_cases
def test_jvp_reads_the_record_of_a_path_under_every_schedule(hank, oracle_mod, family, name, n_a, n_e):
    """a persistent or wide tangent sweep at this record would rebuild kc with the model's beta (diet_kc)"""
    for T in R.HORIZONS:
        c = R.shock_case(family, name, n_a, n_e, T)
        for sched in ("launch", "xcd", "wide"):
            _jvp_at_path(hank, c, sched, 33, f"{family} {name} {n_a}x{n_e} T={T} {sched} N=33")


def test_jvp_at_the_width_of_the_wide_family(hank, oracle_mod):
    c = R.shock_case("ks", "gamma2", *cases.ENTRY_WIDE, 12)
    _jvp_at_path(hank, c, None, 96, "ks gamma2 40x11 T=12 default schedule N=96")


# ---- 3. hank_jvp_shock ----------------------------------------------------------------------------------------------------------------
def _shock_against_oracle(hb, c, tag, N, y, db, seed_key, path):
    ref = _ref(c, (seed_key, N, path is None), dx=y, dpath=db, groups=_groups(c), path=path)
    P, n_hh = c["x"].shape[1], c["x"].shape[0]
    yz = np.zeros((n_hh, P, N)) if y is None else y
    close(hb.jvp_shock(y, db), ref["dagg"][:, 0, :], what=f"{tag} dagg")
    close(hb.dpolicy_seq(N).transpose(2, 0, 1, 3), ref["dpol"], what=f"{tag} dpolicy")
    _, dagg = hb.het_outputs(c["n_het"], yz)
    for o in range(c["n_het"]):
        assert np.abs(ref["dagg"][:, o, :]).max() > 1e-6, (tag, o)
        close(dagg[:, o, :], ref["dagg"][:, o, :], what=f"{tag} output {o}")
    grp, dgrp = hb.group_outputs(yz)
    close(grp, ref["grp"], what=f"{tag} groups")
    close(dgrp, ref["dgrp"], what=f"{tag} groups' tangents")
    _, d2 = hb.grid_aggregates(N)
    close(d2, ref["dagg2"], what=f"{tag} grid aggregate")


@grid_cases
def test_jvp_shock_matches_the_oracle(hank, oracle_mod, family, name, n_a, n_e):
    for T in R.HORIZONS:
        c = R.shock_case(family, name, n_a, n_e, T)
        P = T - 1
        for path in (c["path"], None):
            hb = C.ctx(hank, K, c, None, path=path is not None)
            try:
                hb.set_group_outputs(*_groups(c))
                hb.primal(c["x"])
                tag = f"{family} {name} {n_a}x{n_e} T={T} {'path' if path is not None else 'constant beta'}"
                for N in (1, 33):
                    y, db = path_refs.seeds(K, c, N, 11)
                    _shock_against_oracle(hb, c, f"{tag} N={N} inputs and beta", N, y, db, "both", path)
                y, db = path_refs.seeds(K, c, 3, 12)
                _shock_against_oracle(hb, c, f"{tag} N=3 beta alone", 3, None, db, "beta", path)
                for t_only in sorted({0, P - 1}):
                    y, db = path_refs.seeds(K, c, 3, 13, t_only=t_only)
                    _shock_against_oracle(hb, c, f"{tag} N=3 beta_{t_only} alone", 3, y, db, ("only", t_only), path)
                tm = hb.last_timings()
                assert tm["tangent_backward"]["launches"] == 2 * P + 3 and tm["tangent_forward"]["launches"] == P + 3, (tag, tm)
                assert hb.info()["last_tangent_family_name"] == cases.FAMILY["launch"] and hb.stats()["fallbacks"] == 0
            finally:
                hb.close()


@grid_cases
def test_jvp_shock_without_a_beta_seed_is_hank_jvp_bit_for_bit(hank, oracle_mod, family, name, n_a, n_e):
    for T in (2, 4):
        C.no_seed_in_the_path_is_hank_jvp_bit_for_bit(hank, K, R.shock_case(family, name, n_a, n_e, T), (family, name, n_a, n_e, T), R.WIDTHS)


# ---- 4. hank_vjp_shock ------------------------------------------------------------------------------------------------------------------
@grid_cases
def test_vjp_shock_is_the_transpose_of_jvp_shock(hank, oracle_mod, family, name, n_a, n_e):
    for T in R.HORIZONS:
        c = R.shock_case(family, name, n_a, n_e, T)
        P, nh, N = T - 1, c["n_het"], 3
        rng = np.random.default_rng(T)
        for with_path in (True, False):
            hb = C.ctx(hank, K, c, None, path=with_path)
            try:
                hb.primal(c["x"])
                y, db = path_refs.seeds(K, c, N, 21)
                hb.jvp_shock(y, db)
                _, Jy = hb.het_outputs(nh, y)                                  # (P, n_het, N)
                for M in R.WIDTHS:
                    for n_het in range(1, nh + 1):
                        what = f"{family} {name} {n_a}x{n_e} T={T} path={with_path} M={M} n_het={n_het}"
                        yb = rng.standard_normal((P, n_het, M))
                        xbar, bbar = hb.vjp_shock(yb, n_het)
                        assert np.array_equal(xbar, hb.vjp_het(yb, n_het)), what
                        x2, b2 = hb.vjp_shock(yb, n_het)
                        assert np.array_equal(x2, xbar) and np.array_equal(b2, bbar), what
                        C.transposed_identity(what, K, yb, Jy, xbar, y, bbar, db)
                tv = hb.last_vjp_timings()
                assert tv["sweep_b"]["launches"] == 2 * P + 3, tv
            finally:
                hb.close()


# ---- 5. hank_fake_news_shock ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("econ", ["ks30x3", "hank30x3"])
@pytest.mark.parametrize("T", [3, 12])
def test_shock_jacobian_matches_the_unit_columns(hank, oracle_mod, econ, T):
    from hank_amd.SteadyStateJacobian import shock_jacobian
    c = S.case(econ)
    P, nh = T - 1, c["n_het"]
    hb = cases.raw_block(hank, c["args"][:6] + (T,) + c["args"][7:], None)
    try:
        hb.set_boundary(c["V"], c["D"])
        hb.set_het_outputs(nh)
        hb.primal(FR.constant_path(c, P))
        J = shock_jacobian(hb, nh)                                           # (n_het, P, P)
        hb.jvp_shock(None, np.eye(P))
        _, cols = hb.het_outputs(nh, np.zeros((hb.n_hh, P, P)))                # (P, n_het, P): [t, o, s]
        for o in range(nh):
            assert np.abs(cols[:, o, :]).max() > 1e-3
            close(J[o], cols[:, o, :], what=f"{econ} T={T} J_beta of output {o}")
        for n in range(1, nh):
            assert np.array_equal(shock_jacobian(hb, n), J[:n])
        hb.set_discount_path(np.full(P, c["args"][3]))
        C.raises(NOT_READY, hb.fake_news_shock, nh)
    finally:
        hb.close()


# ---- 6. refusals and invalidation ---------------------------------------------------------------------------------------------------------
def test_entries_defined_at_one_beta_are_refused_while_a_path_is_set(hank, oracle_mod):
    c = S.case("ks30x3")
    P, nh = S.T_SHORT - 1, c["n_het"]
    hb = cases.raw_block(hank, c["args"], None)
    try:
        hb.set_boundary(c["V"], c["D"])
        hb.set_het_outputs(nh)
        G = hb.G
        W = np.ones((G, 1))
        hb.set_group_outputs(W, np.array([1], dtype=np.int32))
        x = FR.constant_path(c, P)
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
        }
        hb.set_discount_path(np.full(P, c["args"][3] * 0.999))
        hb.primal(x)
        for k, f in calls.items():
            C.raises(NOT_READY, f)
        hb.set_discount_path(None)
        C.raises(NOT_READY, hb.jvp, np.zeros((hb.n_hh, P, 1)))                   # clearing drops the record too
        hb.primal(x)
        for k, f in calls.items():
            f()
    finally:
        hb.close()


def test_a_bad_path_changes_nothing_and_a_new_path_drops_the_record(hank, oracle_mod):
    c = R.shock_case("ks", "gamma2", 33, 2, 4)
    C.bad_path_and_new_path(hank, K, c, bad=(0.0, -0.9, np.nan, np.inf), at=1, new=c["path"] * 1.001, vjp=lambda hb: hb.vjp(np.ones((3, 1))), own_entry=False)


def test_the_primal_memo_does_not_serve_another_path_and_clone_carries_the_path(hank, oracle_mod):
    c = R.shock_case("hank", "gamma2", 33, 2, 4)
    C.memo_and_clone(hank, K, c, c["path"][::-1].copy(), lambda k, p, y: _ref(c, ("memo", k), dx=y, path=p), hits=True)
