"""tests/ld_refs.py on the CPU, at the shapes tests/test_gpu_entrywise.py runs on the device: the float64 run of the restatement and
the C oracle (another operation order, libm's pow: the oracle's second, independent witness) lie inside the running error bound
at EVERY entry of every output; the bound is not vacuous (conditions on the inputs); `within` sees a one-entry error of 1e-11
relative that `close` cannot. Figures of the committed run: profiles/entrywise.log."""
import numpy as np
import pytest

import cases
import ld_refs
from cases import ENTRY_BACKWARD, ENTRY_CASES, ENTRY_FORWARD, close, within

BACKWARD = ENTRY_BACKWARD
ARRAYS = ("V", "policy", "dV", "dpolicy")


def _back(family, name, n_a, n_e):
    gamma, _, diet = ENTRY_CASES[name]
    c = cases.entry_backward(family, gamma, n_a, n_e)
    return c, diet, cases.entry_refs(c, diet), f"{family} {name} {n_a}x{n_e}"


@pytest.mark.parametrize("family,name,n_a,n_e", BACKWARD)
def test_backward_float64_run_within_bound(family, name, n_a, n_e):
    c, diet, refs, what = _back(family, name, n_a, n_e)
    for k, ((x, dx), R) in enumerate(zip(c["steps"], refs)):
        F = ld_refs.egm_step(np.float64, c["a"], c["z"], c["Pi"], c["beta"], c["gamma"], c["bc"], c["V"], c["dV"], x, dx, diet)
        for q in ARRAYS:
            assert F[q].v.dtype == np.float64 and R[q].v.dtype == np.longdouble
            within(F[q].v, R[q].v, R[q].bound(), f"float64 {what} prices{k} {q}", R["ambiguous"])
        for q in ("constrained", "below", "above"):
            assert np.array_equal(F[q] | R["ambiguous"], R[q] | R["ambiguous"]), (what, k, q)


def _oracle_flat_top_residue(c, R):
    """One operation of the ORACLE that the kernels do not perform. Above the last knot the reference evaluates the interpolant at
    the clamped query, which is the Dual knot itself (Interpolations' Flat(); oracle/hank_oracle.c interp_flat): f = (k_n - k_n-1) /
    (k_n - k_n-1) has the value 1 and the partial (1/h) dp + (-(h / (h h))) dp with dp = ds_n - ds_n-1, zero in exact arithmetic.
    1/h, h h and the quotient round once each, so the two factors cancel to 3 u / h at most; the two products and their sum round
    once each: |f'| <= 6 u |dp| / h, and the policy's partial is f' (a_n - a_n-1). The kernels write an exact zero there (the
    bound of ld_refs is zero); this residue is what the oracle's check adds on those rows, and on no others. -> (n_a, n_e, N)"""
    a, s, ds = c["a"], R["s"].v, R["ds"].v
    res = 6.0 * ld_refs.U53 * np.abs(ds[-1] - ds[-2]) / (s[-1] - s[-2])[:, None] * (a[-1] - a[-2])        # (n_e, N)
    return np.where(R["above"][..., None], res.astype(np.float64)[None], 0.0) * ld_refs.ROUND_UP


@pytest.mark.parametrize("family,name,n_a,n_e", BACKWARD)
def test_backward_oracle_within_bound(oracle_mod, family, name, n_a, n_e):
    c, _, refs, what = _back(family, name, n_a, n_e)
    orc = oracle_mod.Oracle(c["a"], c["z"], c["Pi"], c["beta"], c["gamma"], c["bc"])
    N = c["dV"].shape[2]
    for k, ((x, dx), R) in enumerate(zip(c["steps"], refs)):
        tr = np.r_[x[2], dx[2]] if family == "hank" else None
        st, oV, oP = orc.value_function(np.concatenate([c["V"][..., None], c["dV"]], -1), np.r_[x[0], dx[0]], np.r_[x[1], dx[1]], N, tr)
        assert st == 0
        noise = _oracle_flat_top_residue(c, R)
        extra = {"V": 0.0, "policy": 0.0, "dpolicy": noise, "dV": np.abs(R["v"].v).astype(np.float64)[..., None] * noise}
        for q, o in (("V", oV[..., 0]), ("policy", oP[..., 0]), ("dV", oV[..., 1:]), ("dpolicy", oP[..., 1:])):
            within(o, R[q].v, R[q].bound() + extra[q], f"oracle {what} prices{k} {q}", R["ambiguous"])
        con = R["constrained"] & ~R["ambiguous"]
        assert np.all(oP[..., 0][con] == c["bc"]) and np.all(oP[..., 1:][con] == 0.0)


@pytest.mark.parametrize("family,name,n_a,n_e", BACKWARD)
def test_backward_bound_is_not_vacuous(family, name, n_a, n_e):
    """conditions on the inputs: the bound on V below 1e-12 |V| at every entry; over the case's prices a constrained row, a row
    below the first knot and one above the last; exact outcomes carry a zero bound"""
    c, _, refs, what = _back(family, name, n_a, n_e)
    for R in refs:
        rel = R["V"].bound() / np.abs(R["V"].v).astype(np.float64)
        print(f"{what}: bound on V at most {rel.max():.2e} |V|, V over {float(R['V'].v.max() / R['V'].v.min()):.1f}x")
        assert rel.max() <= 1e-12
        flat = R["constrained"] | R["below"] | R["above"]
        assert np.all(R["policy"].e[flat] == 0.0) and np.all(R["dpolicy"].e[flat] == 0.0) and np.all(R["dpolicy"].v[flat] == 0.0)
        assert np.all(R["policy"].v[R["constrained"]] == c["bc"])
    assert any(R["constrained"].any() for R in refs) and any(R["below"].any() for R in refs) and any(R["above"].any() for R in refs)
    if family == "hank":                 # the limit sits above the first grid point: `max` binds on interpolated policies too
        assert any((R["constrained"] & ~R["below"]).any() for R in refs), what


@pytest.mark.parametrize("n_e", [2, 3, 4, 11])
def test_a_transposed_Pi_shows(n_e):
    """the entry-wise cases' transition matrix is row-stochastic and not symmetric: the restatement run with Pi' leaves the bound
    in the EGM step (value and partials) and in the distribution step"""
    Pi = cases.entry_Pi(n_e)
    assert np.all(Pi > 0) and np.allclose(Pi.sum(axis=1), 1.0, rtol=0, atol=4e-16) and np.abs(Pi - Pi.T).max() > 0.01
    if n_e in (2, 11):
        c, diet, refs, _ = _back("ks", "gamma2", *((33, 2) if n_e == 2 else (40, 11)))
        (x, dx), R = c["steps"][0], refs[0]
        F = ld_refs.egm_step(np.float64, c["a"], c["z"], c["Pi"].T, c["beta"], c["gamma"], c["bc"], c["V"], c["dV"], x, dx, diet)
        for q in ("V", "dV"):
            with pytest.raises(AssertionError):
                within(F[q].v, R[q].v, R[q].bound(), f"Pi transposed {q}", R["ambiguous"])
    if n_e in (2, 4):
        name = "33x2" if n_e == 2 else "257x4"
        c, R = cases.entry_forward(name), cases.entry_forward_ref(name)
        F = ld_refs.forward_step(np.float64, c["a"], c["Pi"].T, c["policy"], c["dpolicy"], c["D"], c["dD"])
        with pytest.raises(AssertionError, match="max err/bound"):
            within(F["D"].v, R["D"].v, R["D"].bound(), "Pi transposed D", R["ambiguous"])


@pytest.mark.parametrize("family", ["ks", "hank"])
@pytest.mark.parametrize("gamma", [1.0, 2.0])
def test_record_diet_moves_the_coefficients_by_rounding(family, gamma):
    """csrc/hank_kernels.h, RECORD DIET: kc rebuilt from s (cm through a cancellation) and v from u "move by rounding (1e-13)".
    The float64 rebuilt coefficients lie inside their own running bound around the long double TEXTBOOK ones; the figure is printed."""
    c = cases.entry_backward(family, gamma, 130, 3)
    for k, (x, dx) in enumerate(c["steps"]):
        R = ld_refs.egm_step(np.longdouble, c["a"], c["z"], c["Pi"], c["beta"], gamma, c["bc"], c["V"], c["dV"], x, dx, 0)
        B = ld_refs.egm_step(np.longdouble, c["a"], c["z"], c["Pi"], c["beta"], gamma, c["bc"], c["V"], c["dV"], x, dx, 1)
        F = ld_refs.egm_step(np.float64, c["a"], c["z"], c["Pi"], c["beta"], gamma, c["bc"], c["V"], c["dV"], x, dx, 1)
        for q in ("kc", "v"):
            within(F[q].v, R[q].v, B[q].bound(), f"float64 diet vs textbook {family} gamma{gamma:g} 130x3 prices{k} {q}")
            moved = np.max(np.abs(F[q].v - R[q].v) / np.abs(R[q].v))
            print(f"record diet {family} gamma{gamma:g} prices{k} {q}: moved by at most {float(moved):.2e} relative")
            assert moved <= 1e-13


def _oracle_step(oracle_mod, c):
    orc = oracle_mod.Oracle(*c["args"][:6])
    N = c["dpolicy"].shape[2]
    return orc.transition_step(np.concatenate([c["policy"][..., None], c["dpolicy"]], -1), np.concatenate([c["D"][..., None], c["dD"]], -1), N)


@pytest.mark.parametrize("name", ENTRY_FORWARD)
def test_forward_float64_run_and_oracle_within_bound(oracle_mod, name):
    c, R = cases.entry_forward(name), cases.entry_forward_ref(name)
    F = ld_refs.forward_step(np.float64, c["a"], c["Pi"], c["policy"], c["dpolicy"], c["D"], c["dD"])
    for q in ("D", "dD", "agg", "dagg", "total"):
        within(F[q].v, R[q].v, R[q].bound(), f"float64 forward {name} {q}", R["ambiguous"] if q in ("D", "dD") else None)
    oD = _oracle_step(oracle_mod, c)
    within(oD[..., 0], R["D"].v, R["D"].bound(), f"oracle forward {name} D", R["ambiguous"])
    within(oD[..., 1:], R["dD"].v, R["dD"].bound(), f"oracle forward {name} dD", R["ambiguous"])
    if name == "golden-own":              # the committed vectors are the oracle's output: the same bits
        assert np.array_equal(oD, np.load(cases.ROOT / "tests" / "golden" / "forward_step_edge_30x3_N3.npz")["D_new"])


@pytest.mark.parametrize("name", ENTRY_FORWARD)
def test_forward_bound_is_not_vacuous(name):
    """the bound on D_new at most 1e-12 of the unweighted mass of the sources that touch the row, at every entry; D_prev with
    entries below 1e-20; clamps at both ends, exact grid hits, a non-monotone policy; a row no source touches is exactly zero"""
    c, R = cases.entry_forward(name), cases.entry_forward_ref(name)
    b, mass = R["D"].bound(), R["mass"]
    assert np.all(b <= 1e-12 * mass)
    print(f"forward {name}: bound / mass at most {np.max(b[mass > 0] / mass[mass > 0]):.2e}; D_prev {c['D'].min():.1e} .. {c['D'].max():.1e}, "
          f"D_new {float(R['D'].v[R['D'].v > 0].min()):.1e} .. {float(R['D'].v.max()):.1e}, empty rows {int((mass == 0).sum())}")
    assert np.all(R["D"].v[mass == 0] == 0.0)
    assert (c["D"].min() < 1e-20 or name == "golden-own") and abs(c["D"].sum() - 1.0) < 1e-15
    a, p = c["a"], c["policy"]
    assert (p <= a[0]).any() and (p > a[-1]).any() and np.isin(p, a[1:-1]).any() and np.any(np.diff(p, axis=0) < 0)
    assert abs(float(R["total"].v) - 1.0) <= 1e-14


def test_within_sees_what_close_cannot():
    """on data only: one small entry of a float64 output moved by 1e-11 relative — the top-row V, a tail entry of D"""
    c, diet, refs, _ = _back("ks", "gamma2-nodiet", 130, 3)
    x, dx = c["steps"][0]
    V = ld_refs.egm_step(np.float64, c["a"], c["z"], c["Pi"], c["beta"], c["gamma"], c["bc"], c["V"], c["dV"], x, dx, diet)["V"].v.copy()
    R = refs[0]["V"]
    assert V[-1, 0] < 0.05 * V.max()
    within(V, R.v, R.bound(), "V as computed")
    V[-1, 0] *= 1.0 + 1e-11
    close(V, R.v.astype(np.float64), what="V, top row moved")
    with pytest.raises(AssertionError, match="max err/bound"):
        within(V, R.v, R.bound(), "V, top row moved")
    f, Rf = cases.entry_forward("257x4"), cases.entry_forward_ref("257x4")["D"]
    D = ld_refs.forward_step(np.float64, f["a"], f["Pi"], f["policy"], f["dpolicy"], f["D"], f["dD"])["D"].v.copy()
    k = np.unravel_index(np.argmin(np.where(D > 0, D, np.inf)), D.shape)
    assert 0 < D[k] < 1e-12 * D.max()
    within(D, Rf.v, Rf.bound(), "D as computed")
    D[k] *= 1.0 + 1e-11
    close(D, Rf.v.astype(np.float64), what="D, a tail entry moved")
    with pytest.raises(AssertionError, match="max err/bound"):
        within(D, Rf.v, Rf.bound(), "D, a tail entry moved")


def test_within_rejects_nan_shape_and_too_many_skips():
    ref, b = np.ones((4, 3), dtype=np.longdouble), np.full((4, 3), 1e-15)
    within(np.ones((4, 3)), ref, b, "equal")
    with pytest.raises(AssertionError, match="NaN"):
        within(np.full((4, 3), np.nan), ref, b, "nan")
    with pytest.raises(AssertionError):
        within(np.ones((4, 1)), ref, b, "shape")
    with pytest.raises(AssertionError, match="ambiguous"):
        within(np.ones((4, 3)), ref, b, "skips", skip=np.eye(4, 3, dtype=bool))
    with pytest.raises(AssertionError, match="max err/bound"):      # a zero bound is an exact outcome
        within(np.ones((4, 3)) + 2.0 ** -52, ref, np.zeros((4, 3)), "exact")


def test_tracked_rules():
    """the bound's rules on small data: a sum's bound covers every order; a power of two is free; a gather moves the bound"""
    rng = np.random.default_rng(5)
    x = rng.standard_normal(1000) * 10.0 ** rng.uniform(-8, 8, 1000)
    t = ld_refs.Tracked(x.astype(np.longdouble)).sum()
    for order in (np.arange(1000), np.arange(1000)[::-1], rng.permutation(1000)):
        s = 0.0
        for v in x[order]:
            s += v
        assert abs(np.longdouble(s) - t.v) <= t.bound()
    assert abs(np.longdouble(np.sum(x)) - t.v) <= t.bound()
    y = ld_refs.Tracked(np.asarray([3.0]), 1e-17)
    assert y.scaled(-2.0).e[0] == 2e-17 and (-y).e[0] == 1e-17 and y[0].e == 1e-17
    assert (y * 2.0).e[0] > 2e-17
    q = ld_refs.Tracked(np.asarray([3.0], dtype=np.longdouble)).rcp()
    assert abs(q.e[0] - 2 * 2.0 ** -52 / 3.0) < 1e-30 and abs(np.longdouble(1.0 / 3.0) - q.v[0]) <= q.e[0]


def test_distribution_push_compounds_and_holds_the_oracle(oracle_mod):
    """the sweeps' reference on the CPU: D_0 pushed in long double through the oracle's policy sequence; the oracle's own D_t and
    its aggregate lie inside the compounding bound at every period and entry"""
    m, V, D0, xhh, orc = cases.shape(130, 3, 12)
    _, _, opol, _ = orc.block(xhh, None, V, D0)
    oagg, oD = orc.forward_iteration(np.stack([opol, np.zeros_like(opol)], axis=-1), D0, 1, return_D=True)
    grid, Pi = m.heterogeneity["wealth"].grid, np.asarray(m.heterogeneity["productivity"].transition)
    push = cases.push_distribution(grid, Pi, np.ascontiguousarray(opol.transpose(1, 2, 0)), D0)
    rel = []
    for t, R in enumerate(push):
        within(oD[t, ..., 0], R["D"].v, R["D"].bound(), f"oracle push 130x3 t={t} D", R["ambiguous"])
        within(oagg[t, 0], R["agg"].v, R["agg"].bound(), f"oracle push 130x3 t={t} agg")
        rel.append(float(np.max(R["D"].bound() / np.maximum(R["mass"], 1e-300))))
    assert rel[-1] > rel[0] and rel[-1] <= 1e-12, rel
