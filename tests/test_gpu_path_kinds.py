"""Both path kinds — the discount-factor path and the income path — living in ONE context and in ONE workspace of a width.

The suites of the two kinds (tests/test_gpu_shock.py, tests/test_gpu_income.py) alternate the kinds on one context only at DIFFERENT
widths (hank_fake_news_shock runs one direction, hank_fake_news_income n_e), so a buffer or a graph that the kinds shared inside one
tangent or cotangent workspace, or a primal graph that outlived a change of kind, would go unseen there. Here every call is made
twice: among calls of the other kind on a shared context, and as the first path call of a fresh context. The device code is
deterministic and the kinds own separate buffers and graphs, so the two must agree BIT FOR BIT.

Economies: the suite's smallest — Krusell-Smith 30x3 and the one-asset HANK 30x3 of tests/ss_diff_cases.py at their short horizon
(T = 12), the HANK 30x2 of tests/income_refs.two_state_hank for the Toeplitz entries. Widths 3 and 4: one and two directions per lane.
The level under a path is held against the oracle loops of tests/shock_refs.py and tests/income_refs.py at cases.close; the transposed
identity at the figure of tests/test_gpu_shock.py and tests/test_gpu_income.py, 1e-10 of the summed magnitudes."""
import numpy as np
import pytest

import cases
import income_refs as IR
import path_refs
import shock_refs as SR
import ss_diff_cases as S
from cases import close

pytestmark = pytest.mark.gpu

ECONS = ("ks30x3", "hank30x3")
WIDTHS = (3, 4)
_CASE, _TAN = {}, {}


def _case(econ):
    """S.case(econ) with a path of the household inputs that moves (the deviations of shock_refs.shock_case), a beta path and an
    income path, cached"""
    if econ not in _CASE:
        c = S.case(econ)
        P = S.T_SHORT - 1
        t = np.arange(P)
        dev = np.stack([0.1 * 0.8 ** t, 0.01 * 0.7 ** t, -0.02 * 0.9 ** t])[:len(c["x"])]
        x = np.ascontiguousarray(np.asarray(c["x"])[:, None] * (1.0 + dev))
        _CASE[econ] = dict(args=c["args"], orc=c["orc"], V=c["V"], D=c["D"], x=x, gamma=c["gamma"], beta=float(c["args"][3]),
                           path=SR.beta_path(float(c["args"][3]), P), y=IR.income_path(c["orc"].z, x))
    return _CASE[econ]


def _ctx(hank, c, schedule=None):
    hb = cases.raw_block(hank, c["args"], schedule)
    hb.set_boundary(c["V"], c["D"])
    return hb


def _seeds(c, N):
    """dx (n_hh, P, N), dbeta (P, N), dy (n_e, P, N)"""
    rng = np.random.default_rng(100 + N)
    n_hh, P = c["x"].shape
    return rng.standard_normal((n_hh, P, N)) * 1e-2, rng.standard_normal((P, N)) * 1e-2, rng.standard_normal((c["y"].shape[0], P, N)) * 1e-2


def _jvp(hb, kind, dx, d):
    """one tangent call of a kind and everything its batch serves: (dagg, dpolicy_seq, het_outputs(2)'s tangents)"""
    N = dx.shape[-1]
    if kind == "shock":
        return hb.jvp_shock(dx, d), hb.dpolicy_seq(N), hb.het_outputs(2, dx)[1]
    return hb.jvp_income(dx, d), hb.dpolicy_seq(N), hb.het_outputs(2, dx, dy=d)[1]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(u, v) for u, v in zip(a, b))


def _fresh_tangents(hank, econ, N):
    """{kind: _jvp of that kind as the FIRST path call of a fresh context}, once per session"""
    if (econ, N) not in _TAN:
        c = _case(econ)
        dx, db, dy = _seeds(c, N)
        out = {}
        for kind, d in (("shock", db), ("income", dy)):
            hb = _ctx(hank, c)
            try:
                hb.primal(c["x"])
                out[kind] = _jvp(hb, kind, dx, d)
            finally:
                hb.close()
        _TAN[(econ, N)] = out
    return _TAN[(econ, N)]


# ---- (a) tangent sweeps, both kinds at one width ------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", WIDTHS)
@pytest.mark.parametrize("econ", ECONS)
def test_tangent_sweeps_of_both_kinds_share_a_width(hank, oracle_mod, econ, N):
    c = _case(econ)
    dx, db, dy = _seeds(c, N)
    fresh = _fresh_tangents(hank, econ, N)
    hb = _ctx(hank, c)
    try:
        hb.primal(c["x"])
        first = _jvp(hb, "shock", dx, db)
        second = _jvp(hb, "income", dx, dy)
        third = _jvp(hb, "shock", dx, db)
        P = c["x"].shape[1]
        tm = hb.last_timings()
        assert tm["tangent_backward"]["launches"] == 2 * P + 3 and tm["tangent_forward"]["launches"] == P + 3, tm
    finally:
        hb.close()
    assert all(np.abs(v[0]).max() > 1e-6 for v in (first, second)), (econ, N)
    assert not np.array_equal(first[0], second[0]), (econ, N)      # (the kinds' seeds differ: the calls are not one call)
    assert _same(third, first), (econ, N, "the shock call after an income call at the same width")
    assert _same(first, fresh["shock"]) and _same(third, fresh["shock"]), (econ, N, "shock against a fresh context")
    assert _same(second, fresh["income"]), (econ, N, "income against a fresh context")


# ---- (b) transposed sweeps, both kinds at one width ---------------------------------------------------------------------------------
@pytest.mark.parametrize("M", WIDTHS)
@pytest.mark.parametrize("econ", ECONS)
def test_transposed_sweeps_of_both_kinds_share_a_width(hank, oracle_mod, econ, M):
    c = _case(econ)
    P, n_het = c["x"].shape[1], 2
    yb = np.random.default_rng(M).standard_normal((P, n_het, M))
    alone = {}
    for kind in ("shock", "income"):      # a context that runs ONE kind
        hb = _ctx(hank, c)
        try:
            hb.primal(c["x"])
            alone[kind] = hb.vjp_shock(yb, n_het) if kind == "shock" else hb.vjp_income(yb, n_het)
        finally:
            hb.close()
    hb = _ctx(hank, c)
    try:
        hb.primal(c["x"])
        xs, bbar = hb.vjp_shock(yb, n_het)
        xi, ybar = hb.vjp_income(yb, n_het)
        xs2, bbar2 = hb.vjp_shock(yb, n_het)
        xv = hb.vjp(yb, n_het)
        tv = hb.last_vjp_timings()
        assert tv["sweep_b"]["launches"] == P + 1, tv      # (hank_vjp's own Sweep B after both kinds')
    finally:
        hb.close()
    assert np.array_equal(xs, xv) and np.array_equal(xi, xv) and np.array_equal(xs2, xv), (econ, M)
    assert np.array_equal(bbar2, bbar), (econ, M)
    assert _same((xs, bbar), alone["shock"]) and _same((xi, ybar), alone["income"]), (econ, M)
    assert np.abs(bbar).max() > 1e-6 and np.abs(ybar).max() > 1e-6, (econ, M)
    # the transpose identity against (a)'s tangents of the same width, at the suite's figure for hank_vjp_shock / hank_vjp_income
    dx, db, dy = _seeds(c, M)
    fresh = _fresh_tangents(hank, econ, M)
    for kind, xbar, lin in (("shock", xs, np.einsum("tm,tn->mn", bbar, db)), ("income", xi, np.einsum("etm,etn->mn", ybar, dy))):
        Jd = fresh[kind][2]                                                 # (P, 2, N)
        lhs = np.einsum("tom,ton->mn", yb, Jd[:, :n_het, :])
        rhs = np.einsum("ktm,ktn->mn", xbar, dx) + lin
        scale = np.einsum("tom,ton->mn", np.abs(yb), np.abs(Jd[:, :n_het, :]))
        print(f"{econ} M={M} {kind}: max |lhs - rhs| / scale = {np.max(np.abs(lhs - rhs) / scale):.3e}")
        assert np.all(np.abs(lhs - rhs) <= 1e-10 * scale), (econ, M, kind)


# ---- (c) switching kinds on one context ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("econ", ECONS)
def test_switching_kinds_on_one_context(hank, oracle_mod, econ):
    """a context on the per-period launches (its own primal graphs are captured when it is created): each kind's backward primal graph
    is ONE capture more at the kind's first primal under a path, none after, whatever was set and cleared in between"""
    c = _case(econ)
    orc, x, V, D = c["orc"], c["x"], c["V"], c["D"]
    hb = _ctx(hank, c, "launch")
    try:
        def primal():
            before = hb.stats()["graphs_captured"]
            agg = hb.primal(x)
            return (agg, hb.policy_seq()), hb.stats()["graphs_captured"] - before

        first, grew = primal()
        assert grew == 0, grew
        ref_beta = path_refs.oracle_path_sweeps(SR.KIND, orc, x, V, D, c["path"], c["gamma"], 2)
        ref_y = path_refs.oracle_path_sweeps(IR.KIND, orc, x, V, D, c["y"])
        grown = []
        for _ in range(2):      # (the second round: both kinds' graphs are there)
            hb.set_discount_path(c["path"])
            at_beta, g1 = primal()
            _, g2 = primal()
            hb.set_discount_path(None)
            hb.set_income_path(c["y"])
            at_y, g3 = primal()
            _, g4 = primal()
            hb.set_income_path(None)
            last, g5 = primal()
            grown.append((g1, g2, g3, g4, g5))
            assert _same(last, first), econ
            close(at_beta[0], ref_beta["agg"][:, 0], what=f"{econ} aggregate at the beta path")
            close(at_beta[1].transpose(2, 0, 1), ref_beta["pol"], what=f"{econ} policy at the beta path")
            close(at_y[0], ref_y["agg"][:, 0], what=f"{econ} aggregate at the income path")
            close(at_y[1].transpose(2, 0, 1), ref_y["pol"], what=f"{econ} policy at the income path")
            assert np.abs(at_beta[1] - first[1]).max() > 1e-3 and np.abs(at_y[1] - first[1]).max() > 1e-3, econ      # (the paths move the policy)
        assert grown == [(1, 0, 1, 0, 0), (0, 0, 0, 0, 0)], grown
        tm = hb.last_timings()
        assert tm["primal_backward"]["launches"] == x.shape[1] + 2, tm
    finally:
        hb.close()


# ---- (d) Toeplitz entries, both kinds in one context --------------------------------------------------------------------------------
def test_toeplitz_entries_of_both_kinds_share_a_context(hank, oracle_mod):
    """fake_news reuses the workspace's dpol and the kinds' staging buffers: hank_fake_news_income and hank_jvp_income share the
    workspace of width n_e = 2, hank_fake_news_shock and hank_jvp_shock that of width 1"""
    c = IR.two_state_hank()
    P = c["args"][6] - 1
    x = np.tile(c["x"][:, None], (1, P))
    rng = np.random.default_rng(7)
    dx = {N: rng.standard_normal((3, P, N)) * 1e-2 for N in (1, 2)}
    db, dy = rng.standard_normal((P, 1)) * 1e-2, rng.standard_normal((2, P, 2)) * 1e-2
    calls = {"fn_income": lambda hb: hb.fake_news_income(2), "fn_shock": lambda hb: hb.fake_news_shock(2),
             "jvp_income": lambda hb: _jvp(hb, "income", dx[2], dy), "jvp_shock": lambda hb: _jvp(hb, "shock", dx[1], db)}

    def run(names):
        hb = _ctx(hank, c)
        try:
            assert hb.n_e == 2 and hb.n_hh == 3
            hb.primal(x)
            return {k: calls[k](hb) for k in names}
        finally:
            hb.close()

    fresh = {k: run([k])[k] for k in calls}
    assert all(np.abs(v[0]).max() > 1e-6 for v in fresh.values())
    for order in (("fn_income", "fn_shock"), ("fn_shock", "fn_income")):
        got = run(order + ("jvp_income", "jvp_shock"))
        for k in calls:
            assert _same(got[k], fresh[k]), (order, k)
