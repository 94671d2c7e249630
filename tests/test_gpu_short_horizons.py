"""Horizons of one, two and three periods (T = 2, 3, 4; hank_create accepts T >= 2) through every entry and every kernel family.
The other GPU modules start at P = 4 or 5; the period arithmetic of the sweeps differs from the generic case exactly below that:
k_xfwd asks for work units one and two periods ahead (request_units(t + 2), min(t + 1, P - 1)), the persistent backward sweeps
preload `DEEP` periods ahead and count P + 1 episodes, k_wide_fwd writes the aggregate of period t two periods later (outn[t - 2],
the epilogue's `if (P >= 2) outn[P - 2]`), the launch family's fused graphs run k <= P iterations with tp = -1 tails, and the
adjoint chain's first and last step are the same launch at P = 1 (k_bnd_vend's `P == 1 ? 1 : 0`).

Shapes (each at T = 2, 3, 4): Krusell-Smith 130x3 (three members of the persistent family, the last short) and 65x11 (the bench's
768-thread block, two members) of cases.shape; the raw grid `deep-prefix` (700x3, twelve members) with its path cut to the first
P periods; the one-asset HANK 80x3 (three household inputs, four outputs) at its steady state as boundary. Measured on the oracle's
policy: cut this short, `deep-prefix` clamps no row at the bottom (its prefix builds up over the nine periods behind V_T; at P = 1,
2, 3 clo = 0 in every column and period) and keeps 85 to 93 sources on the top row of column 2 in the last period, a work unit of
more than 64 lanes. The mass on the virtual rows comes from a fifth shape, `swing` (600x3) on periods 1 .. P of its path: at P = 2,
3 the first period clamps 130 to 161 rows of EVERY column (members 0 to 2, anyopen == 0, 22 to 34 % of the mass on row 0) and the
last period clamps none, so all virtual mass re-enters through row 0's lottery; at P = 1 the only period after V_T clamps nothing
on any of the raw grids, whatever the prices.

The reference is always the CPU oracle (oracle/hank_oracle.c) — its household block, its loop with duals on the boundary
(tests/sweep_refs.py), its Jacobian from unit tangents, transposed — or the dense operators of tests/ss_diff_cases.py and
tests/fake_news_refs.py; a device product is compared with another device product only for bits, for the launches' 1e-12 and for the
dot-product identity. Tolerance: cases.close (rel 1e-10 + abs 1e-12) unless stated. Under a forced schedule the family that served
and `fallbacks == 0` are asserted: a fallback would hide a persistent sweep's bug behind the launches' numbers.

P = 1 of hank_fake_news[_het] is covered here (test_fake_news_matches_the_dense_reference); hank_ss_jvp / hank_ss_vjp refuse it
(include/hank_hip.h), which test_steady_state_derivatives_refuse_one_period asserts."""
import numpy as np
import pytest

import cases
import fake_news_refs as R
import ss_diff_cases as S
import sweep_refs
from cases import close

pytestmark = pytest.mark.gpu

HORIZONS = (2, 3, 4)
NAMES = ("ks130x3", "ks65x11", "deep-prefix", "swing", "hank80x3")
CONTEXTS = [("launch", {}), ("xcd", {}), ("xcd", {"HANK_RECORD_DIET": 0}), ("wide", {"HANK_WIDE_R": 2}), ("wide", {"HANK_WIDE_R": 4}), (None, {})]
NX = (1, 5, 16, 32)          # the persistent family: D = 1, 1, 2, 4 and both lane widths
NW = (2, 5)                  # the wide family
NWIDE = 96                   # the default schedule sends it to the on-chip wide sweeps
WIDTHS = {"launch": tuple(sorted(set(NX + NW))) + (NWIDE,), "xcd": NX, "wide": NW, None: tuple(sorted(set(NX + NW))) + (NWIDE,)}
THREE = ("launch", "xcd", "wide")
_SHAPES = {}


def short_shape(name, T):
    """-> (HouseholdBlock's arguments at T, V (n_a, n_e), D (G,), x (n_hh, T - 1), oracle, the family's count of outputs), cached"""
    if (name, T) not in _SHAPES:
        P = T - 1
        if name.startswith("ks"):
            m, V, D, x, orc = cases.shape(*{"ks130x3": (130, 3), "ks65x11": (65, 11)}[name], T)
            out = (cases.model_args(m), V, D, x, orc, 3)
        elif name in ("deep-prefix", "swing"):
            ec = cases.raw_economy(name)
            first = 0 if name == "deep-prefix" else 1
            x = np.ascontiguousarray(ec["x"][:, first:first + P])
            pol = ec["orc"].block(x, None, ec["V"], ec["D"])[2]
            clo, top = (pol <= ec["grid"][0]).sum(axis=1), (pol >= ec["grid"][-1]).sum(axis=1)          # (P, n_e)
            if name == "deep-prefix":
                assert top[-1].max() > 64, (top, "a target row with more sources than a work unit has lanes")
            elif P > 1:
                assert np.all(clo[0] > 2 * cases.XRW) and not clo[-1].any(), (clo, "every column clamped over three members, then none")
            out = (ec["args"][:6] + (T,) + ec["args"][7:], ec["V"], ec["D"], x, ec["orc"], 3)
        else:
            m, ss = cases.hank_economy(80, 3, 40)
            args = cases.model_args(m)
            out = (args[:6] + (T,) + args[7:], np.asarray(ss.value), np.asarray(ss.D), cases.hank_x(ss, P), cases.oracle_of(m), 4)
        assert out[0][6] == T and out[3].shape[1] == P
        _SHAPES[name, T] = out
    return _SHAPES[name, T]


def _ctx(hank, name, T, schedule=None, **env):
    args, V, D, x, orc, n_het = short_shape(name, T)
    hb = cases.raw_block(hank, args, schedule, **env)
    assert hb.P == T - 1
    hb.set_boundary(V, D)
    hb.set_het_outputs(n_het)
    return hb


def _served(hb, sched, what):
    """the family of the last tangent sweep under a forced schedule, and no fallback"""
    assert hb.info()["last_tangent_family_name"] == cases.FAMILY[sched], (what, hb.info())
    assert hb.stats()["fallbacks"] == 0, (what, hb.stats())


short = pytest.mark.parametrize("T", HORIZONS)
named = pytest.mark.parametrize("name", NAMES)


# ---- 1. the sweeps ----------------------------------------------------------------------------------------------------------------
@short
@named
def test_both_entry_points_of_every_family(hank, oracle_mod, name, T):
    """cases.against_oracle_and_launches: the Dual pass and hank_primal + hank_jvp, each from a record of another x, at every width
    of every context — aggregates, policy, partials, D_t and dagg against the oracle and the launches, the family, no fallback, a
    second hank_jvp's bits"""
    args, V, D, x, orc, _ = short_shape(name, T)
    for sched, env, st, info in cases.against_oracle_and_launches(hank, (args, V, D, x, orc), CONTEXTS, WIDTHS):
        assert st["fallbacks"] == 0, (name, T, sched, env, st)
        if sched is None or sched == "wide":
            assert info["wide_supported"] == 1, (name, T, info)


# ---- 2. heterogeneous outputs -----------------------------------------------------------------------------------------------------
_HET = {}


def _seeds(name, T, N):
    """N directions in the manner of tests/test_gpu_jvp_het.py: inputs, terminal value (of the value's scale), initial distribution"""
    _, V, D, x, _, _ = short_shape(name, T)
    rng = np.random.default_rng(100 * T + N)
    n_a, n_e = V.shape
    y = rng.standard_normal(x.shape + (N,)) * 1e-2
    dV = rng.standard_normal((n_a, n_e, N)) * np.abs(V)[:, :, None]
    dD = rng.uniform(0.0, 1.0, (n_a, n_e, N)) * (1.0 + np.arange(n_e))[None, :, None] / (n_a * n_e)
    return y, dV, dD


def _het_refs(name, T, N):
    """Oracle.het_outputs at the inputs' directions, and the oracle loop with the boundary's seeds as well, once per case"""
    if (name, T, N) not in _HET:
        args, V, D, x, orc, n_het = short_shape(name, T)
        y, dV, dD = _seeds(name, T, N)
        plain = orc.het_outputs(x, y, V, D, n_het, args[4])
        cons = orc.block_het(x, y, V, D)
        close(plain[0][:2], cons[0], what=f"{name} T={T}: the oracle's two routes to savings and consumption")
        close(plain[1][:2], cons[1], what=f"{name} T={T}: ... and to their partials")
        seeded = sweep_refs.oracle_sweeps(orc, x, V, D, args[4], n_het, y=y, dV=dV, dD=dD)
        assert all(np.abs(seeded["dagg"][:, o]).max() > 1e-6 for o in range(n_het)), (name, T)
        _HET[name, T, N] = (plain, seeded)
    return _HET[name, T, N]


@short
@named
def test_heterogeneous_outputs_and_their_tangents(hank, oracle_mod, name, T):
    """hank_get_het_outputs after a tangent sweep of each family (the Dual pass at N = 2, hank_primal + hank_jvp at N = 5), and
    hank_jvp_het without and with seeds on V_T and D_0, for every output of the family"""
    args, V, D, x, orc, n_het = short_shape(name, T)
    for sched in THREE:
        hb = _ctx(hank, name, T, sched)
        try:
            for entry, N in (("dual", 2), ("tan", 5)):
                y, dV, dD = _seeds(name, T, N)
                (oagg, odagg), seeded = _het_refs(name, T, N)
                what = f"{name} T={T} {sched} {entry} N={N}"
                if entry == "dual":
                    hb.primal(x * 1.01); hb.primal_jvp(x, y)
                else:
                    hb.primal(x * 1.01); hb.primal(x); hb.jvp(y)
                _served(hb, sched, what)
                agg, dagg = hb.het_outputs(n_het, y)
                assert agg.shape == (T - 1, n_het) and dagg.shape == (T - 1, n_het, N)
                for o in range(n_het):
                    close(agg[:, o], oagg[o], what=f"{what} output {o}")
                    close(dagg[:, o, :], odagg[o], what=f"{what} output {o} partials")
                got = hb.jvp_het(y, n_het=n_het)
                got_b = hb.jvp_het(y, dV, dD, n_het=n_het)
                assert got.shape == got_b.shape == (T - 1, n_het, N)
                for o in range(n_het):
                    close(got[:, o, :], odagg[o], what=f"{what} jvp_het output {o}")
                    close(got_b[:, o, :], seeded["dagg"][:, o, :], what=f"{what} jvp_het with boundary seeds, output {o}")
                close(hb.dpolicy_seq(N).transpose(2, 0, 1, 3), seeded["dpol"], what=f"{what} jvp_het with boundary seeds, dpolicy")
            assert hb.stats()["fallbacks"] == 0
        finally:
            hb.close()


# ---- 3. the transposed sweeps -----------------------------------------------------------------------------------------------------
_JAC = {}
FULL_BOUNDARY_G = 800        # up to this many grid points the boundary's Jacobian is taken whole (G unit seeds on V_T, G on D_0)


def _jacobians(name, T):
    """-> (J2 (2, P, n_hh, P), Jh (n_het, P, n_hh, P), Sv, Sd (n_a, n_e, K), Jb (n_het, P, K)): the oracle's Jacobians in the inputs
    from unit tangents, and its loop's columns J_b s for K boundary seeds s = (Sv, Sd) — every unit seed where G <= FULL_BOUNDARY_G
    (130x3, 65x11, 80x3: the exported cotangents are then compared entry by entry), else three random seeds on V_T alone and three
    on D_0 alone (700x3, 600x3: 2 G unit seeds are 4200 columns of 2100 points each)"""
    if (name, T) not in _JAC:
        args, V, D, x, orc, n_het = short_shape(name, T)
        n_a, n_e = V.shape
        G = n_a * n_e
        J2 = cases.oracle_jacobian(orc, V, D, x)
        Jh = cases.jacobian_het(("short", name, T), orc, V, D, x, n_het, args[4])
        close(Jh[:2], J2, what=f"{name} T={T}: the oracle's two Jacobians of savings and consumption")
        if G <= FULL_BOUNDARY_G:
            U = np.eye(G).reshape((n_a, n_e, G), order="F")
            Sv, Sd = np.concatenate([U, np.zeros_like(U)], axis=2), np.concatenate([np.zeros_like(U), U], axis=2)
        else:
            _, dV, dD = _seeds(name, T, 6)
            Sv, Sd = dV.copy(), dD.copy()
            Sv[:, :, 3:] = 0.0; Sd[:, :, :3] = 0.0
        Jb = sweep_refs.oracle_sweeps(orc, x, V, D, args[4], n_het, dV=Sv, dD=Sd)["dagg"].transpose(1, 0, 2)
        assert np.all(np.abs(Jb).max(axis=(1, 2)) > 1e-6), (name, T)
        _JAC[name, T] = (J2, Jh, Sv, Sd, np.ascontiguousarray(Jb))
    return _JAC[name, T]


def _boundary(Vb, Db, yb, Sv, Sd, Jb, what):
    """the exported boundary cotangents against the oracle: <Vbar, s_V> + <Dbar, s_D> = <ybar, J_b s> for every seed s; with unit
    seeds (one of the two terms is then a single entry) that is each entry of value_end_bar and of D_init_bar"""
    n_het = yb.shape[1]
    want = np.einsum("tom,otk->mk", yb, Jb[:n_het])
    got = np.einsum("aem,aek->mk", Vb, Sv) + np.einsum("aem,aek->mk", Db, Sd)
    half = Sv.shape[2] // 2
    close(got[:, :half], want[:, :half], what=what + " value_end_bar")
    close(got[:, half:], want[:, half:], what=what + " D_init_bar")


@short
@named
def test_transposed_sweeps(hank, oracle_mod, name, T):
    """hank_vjp, hank_vjp_het, hank_vjp_boundary and hank_vjp_het_boundary at M = 1, 3, 4 on a record of the launches and of the
    persistent sweeps, against the oracle's Jacobians transposed; <ybar, J y> = <J'ybar, y> against the context's own hank_jvp_het
    at 1e-10 of the products' scale (the sum of the products' absolute values). At P = 1 the adjoint chain's first and last step
    are one launch: both exported boundary cotangents are compared with the oracle's there as everywhere."""
    args, V, D, x, orc, n_het = short_shape(name, T)
    J2, Jh, Sv, Sd, Jb = _jacobians(name, T)
    n_hh, P = x.shape
    rng = np.random.default_rng(7 * T)
    y = rng.standard_normal((n_hh, P, 3)) * 1e-2
    for sched in ("launch", "xcd"):
        hb = _ctx(hank, name, T, sched)
        try:
            hb.primal(x * 1.01); hb.primal(x)
            assert hb.stats()["schedule"] == (0 if sched == "launch" else 1)
            Jy = hb.jvp_het(y, n_het=n_het)                                 # (P, n_het, 3)
            for M in (1, 3, 4):
                what = f"{name} T={T} {sched} M={M}"
                yb = rng.standard_normal((P, n_het, M))
                for k in (1, 2):
                    xb = hb.vjp(yb[:, :k], k)
                    assert xb.shape == (n_hh, P, M)
                    close(xb, cases.jt(J2[:k], yb[:, :k]), what=f"{what} vjp n_het={k}")
                    xb2, Vb, Db = hb.vjp_boundary(yb[:, :k], k)
                    assert np.array_equal(xb2, xb), what + ": vjp_boundary's xhh_bar bits"
                    _boundary(Vb, Db, yb[:, :k], Sv, Sd, Jb, f"{what} vjp_boundary n_het={k}")
                xh = hb.vjp_het(yb, n_het)
                close(xh, cases.jt(Jh, yb), what=what + " vjp_het")
                assert np.all(np.isfinite(hb.policy_cotangent_seq(M)))
                xh2, Vb, Db = hb.vjp_het_boundary(yb, n_het)
                assert np.array_equal(xh2, xh), what + ": vjp_het_boundary's xhh_bar bits"
                _boundary(Vb, Db, yb, Sv, Sd, Jb, what + " vjp_het_boundary")
                lhs, rhs = np.einsum("tom,ton->mn", yb, Jy), np.einsum("ksm,ksn->mn", xh, y)
                scale = max(np.einsum("tom,ton->mn", np.abs(yb), np.abs(Jy)).max(), np.einsum("ksm,ksn->mn", np.abs(xh), np.abs(y)).max())
                close(lhs, rhs, rel=0.0, ab=1e-10 * scale, what=what + " <ybar, J y> against <J'ybar, y>")
            assert hb.stats()["fallbacks"] == 0 and hb.stats()["schedule"] == (0 if sched == "launch" else 1)
        finally:
            hb.close()


# ---- 4. hank_primal_batch ---------------------------------------------------------------------------------------------------------
@short
@named
def test_primal_batch_is_the_launches_primal_bit_for_bit(hank, oracle_mod, name, T):
    """K = 3 paths: every scenario's output 0 and policy equal hank_primal of a launch context at its path bit for bit (and the
    oracle under `close`); the context's own recorded primal — policy, D_t, a hank_jvp at it — is left alone"""
    args, V, D, x, orc, n_het = short_shape(name, T)
    xs = np.stack([x, x * 1.01, x * 0.99], axis=2)
    y = _seeds(name, T, 5)[0]
    hl = _ctx(hank, name, T, "launch")
    hb = _ctx(hank, name, T)
    try:
        hb.primal(x * 1.005)
        before = (hb.policy_seq(), hb.dist_seq(), hb.jvp(y))
        aggs, status, pols = hb.primal_batch(xs, n_het=1, policy=True)
        assert aggs.shape == (T - 1, 1, 3) and pols.shape == V.shape + (T - 1, 3) and not status.any()
        for k in range(3):
            what = f"{name} T={T} scenario {k}"
            agg = hl.primal(xs[:, :, k])
            assert np.array_equal(aggs[:, 0, k], agg), what + ": output 0 bits vs the launches"
            assert np.array_equal(pols[..., k], hl.policy_seq()), what + ": policy bits vs the launches"
            oagg, _, opol, _ = orc.block(xs[:, :, k], None, V, D)
            close(aggs[:, 0, k], oagg, what=what + " vs oracle"); close(pols[..., k].transpose(2, 0, 1), opol, what=what + " policy vs oracle")
        assert np.array_equal(hb.policy_seq(), before[0]) and np.array_equal(hb.dist_seq(), before[1]) and np.array_equal(hb.jvp(y), before[2])
        assert hb.stats()["fallbacks"] == 0
    finally:
        hb.close(); hl.close()


# ---- 5. fake news -----------------------------------------------------------------------------------------------------------------
_FN = {}


def _stationary(hank, name, P, schedule=None):
    """tests/test_gpu_fake_news_dense.py's context: the polished (V, D) of ss_diff_cases.case as both boundaries, `primal` at the
    constant path, T = P + 1"""
    c = S.case(name)
    hb = cases.raw_block(hank, c["args"][:6] + (P + 1,) + c["args"][7:], schedule)
    hb.set_boundary(c["V"], c["D"])
    hb.set_het_outputs(c["n_het"])
    agg = hb.primal(R.constant_path(c, P))
    assert hb.P == P and agg.shape == (P,)
    return hb, c


def _slabs(got, ref, what):
    """tests/test_gpu_fake_news_dense.py's bound: `close` once per (input, output) slab"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    for o in range(ref.shape[-1]):
        for k in range(ref.shape[-2]):
            assert np.any(ref[..., k, o] != 0.0), (what, k, o)
            close(got[..., k, o], ref[..., k, o], what=f"{what} input {k} output {o}")


@pytest.mark.parametrize("P", (1, 2, 3))
@pytest.mark.parametrize("name", ("ks30x3", "hank30x3"))
def test_fake_news_matches_the_dense_reference(hank, oracle_mod, name, P):
    """hank_fake_news and hank_fake_news_het(n) for every n of the family: every entry of F (P, P, n_hh[, n]) and Dv (P, n_hh[, n])
    against fake_news_refs.dense_fake_news, on a record of the default schedule and of the launches. At P = 1 both are one lag:
    F[0, 0] = f . S_p P_x and Dv[0] the same-period effect."""
    if (name, P) not in _FN:
        c = S.case(name)
        _FN[name, P] = R.dense_fake_news(c, P, c["n_het"])
    Fr, Dvr = _FN[name, P]
    for sched in (None, "launch"):
        hb, c = _stationary(hank, name, P, sched)
        try:
            what = f"{name} P={P} schedule {sched or 'default'}"
            for n in range(1, c["n_het"] + 1):
                F, Dv = hb.fake_news_het(n)
                assert F.shape == (P, P, hb.n_hh, n) and Dv.shape == (P, hb.n_hh, n)
                _slabs(F, Fr[..., :n], f"{what} fake_news_het({n}) F")
                _slabs(Dv, Dvr[..., :n], f"{what} fake_news_het({n}) Dv")
            F0, Dv0 = hb.fake_news()
            _slabs(F0[..., None], Fr[..., :1], what + " fake_news() F")
            _slabs(Dv0[..., None], Dvr[..., :1], what + " fake_news() Dv")
            assert np.array_equal(F0, F[..., 0]) and np.array_equal(Dv0, Dv[..., 0])
            assert hb.stats()["fallbacks"] == 0
        finally:
            hb.close()


# ---- 6. derivatives through the steady state --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("ks30x3", "hank30x3"))
def test_steady_state_derivatives_refuse_one_period(hank, oracle_mod, name):
    """T = 2: HANK_ERR_BAD_ARG naming the horizon from both entries, before anything is launched; the context serves a primal
    afterwards"""
    hb, c = _stationary(hank, name, 1)
    try:
        n_hh, G = len(c["x"]), c["orc"].G
        calls = {"hank_ss_jvp": lambda: hb.ss_jvp(np.ones((n_hh, 2)), n_het=2, tol=S.TOL, max_iter=S.MAX_ITER),
                 "hank_ss_vjp": lambda: hb.ss_vjp(np.ones((2, 2)), np.ones((G, 2)), np.ones((G, 2)), n_het=2, tol=S.TOL, max_iter=S.MAX_ITER)}
        before = hb.stats()["sweep_launches"]
        for who, call in calls.items():
            with pytest.raises(hank.HankHIPError, match="at least two periods") as e:
                call()
            assert e.value.code == hank.hip.HANK_ERR_BAD_ARG and who in str(e.value), (who, e.value)
        assert hb.stats()["sweep_launches"] == before
        x = R.constant_path(c, 1) * 1.01
        agg = hb.primal(x)
        oagg, _, opol, _ = c["orc"].block(x, None, c["V"], c["D"])
        close(agg, oagg, what=f"{name}: primal after the refusals"); close(hb.policy_seq().transpose(2, 0, 1), opol, what=f"{name}: its policy")
    finally:
        hb.close()


@pytest.mark.parametrize("name", ("ks30x3", "hank30x3"))
def test_steady_state_derivatives_at_two_periods(hank, oracle_mod, name):
    """T = 3, the shortest record both entries take (the value loop spans periods 0 and 1): hank_ss_jvp at N = 3 and hank_ss_vjp at
    M = 3 with every cotangent, against the dense solves at tests/test_gpu_ss_diff.py's bound — 10 tol / (1 - rho) on top of
    `close`'s rel 1e-10, rho = rho(B_V) for value and policy, max(rho(B_V), |lambda_2(Lam)|) for the rest"""
    hb, c = _stationary(hank, name, 2)
    try:
        r, n_hh, n_het, G = c["ref"], len(c["x"]), c["n_het"], c["orc"].G
        rel_v, rel_d = 1e-10 + S.bound(r["rhoV"]), 1e-10 + S.bound(max(r["rhoV"], r["rhoD"]))
        rng = np.random.default_rng(11)
        dx = rng.standard_normal((n_hh, 3))
        dagg, dV, dpol, dD, iters = hb.ss_jvp(dx, n_het=n_het, tol=S.TOL, max_iter=S.MAX_ITER)
        what = f"{name} T=3 (steps {iters})"
        flat = lambda a: a.reshape((G, a.shape[2]), order="F")          # noqa: E731
        close(flat(dV), r["JV"] @ dx, rel=rel_v, what=what + " dV"); close(flat(dpol), r["Jpol"] @ dx, rel=rel_v, what=what + " dpol")
        close(flat(dD), r["JD"] @ dx, rel=rel_d, what=what + " dD"); close(dagg, r["JY"] @ dx, rel=rel_d, what=what + " dagg")
        assert 0 < iters[0] < S.MAX_ITER and 0 < iters[1] < S.MAX_ITER
        yb, Vb, Db = rng.standard_normal((n_het, 3)), rng.standard_normal((G, 3)), rng.standard_normal((G, 3))
        xbar, iters = hb.ss_vjp(yb, Vb, Db, n_het=n_het, tol=S.TOL, max_iter=S.MAX_ITER)
        close(xbar, r["JY"].T @ yb + r["JV"].T @ Vb + r["JD"].T @ Db, rel=rel_d, what=f"{name} T=3 (steps {iters}) xhh_bar")
        assert iters[0] < S.MAX_ITER and iters[1] < S.MAX_ITER
    finally:
        hb.close()


# ---- 7. the readers ---------------------------------------------------------------------------------------------------------------
@short
@named
def test_readers_return_the_short_record(hank, oracle_mod, name, T):
    """every reader after a Dual pass (N = 5) and a hank_vjp (M = 3) on a context of the persistent sweeps: P-sized arrays, the
    policy, its partials, D_t and the grid's aggregate the oracle's, the lottery the policy's bracket and weight, Sweep A's policy
    cotangent the reference's pullback, and work units in every period"""
    args, V, D, x, orc, n_het = short_shape(name, T)
    n_a, n_e = V.shape
    P, N, M = T - 1, 5, 3
    y = _seeds(name, T, N)[0]
    _, _, opol, odpol = orc.block(x, y, V, D)
    oD = cases.oracle_dist_seq(orc, opol, D)
    hb = _ctx(hank, name, T, "xcd")
    try:
        hb.primal(x * 1.01); hb.primal_jvp(x, y)
        _served(hb, "xcd", f"{name} T={T}")
        what = f"{name} T={T} reader"
        pol, dpol, Dq = hb.policy_seq(), hb.dpolicy_seq(N), hb.dist_seq()
        assert pol.shape == (n_a, n_e, P) and dpol.shape == (n_a, n_e, P, N) and Dq.shape == (n_a, n_e, P)
        close(pol.transpose(2, 0, 1), opol, what=what + " policy_seq"); close(dpol.transpose(2, 0, 1, 3), odpol, what=what + " dpolicy_seq")
        close(Dq.transpose(2, 0, 1), oD, what=what + " dist_seq")
        ad, dad = hb.grid_aggregates(N)
        assert ad.shape == (P,) and dad.shape == (P, N) and np.all(np.isfinite(dad))
        close(ad, np.einsum("i,tie->t", hb.a_grid, oD), what=what + " grid_aggregates")
        rec = hb.lottery_record()
        a = hb.a_grid
        assert all(rec[k].shape == (n_a, n_e, P) for k in ("lo", "lw", "ig", "lq")) and rec["iga"].shape == (n_a,)
        assert rec["lo"].min() >= 0 and rec["lo"].max() <= n_a - 2 and rec["lw"].min() >= 0.0 and rec["lw"].max() <= 1.0
        assert np.all(np.isfinite(rec["ig"])) and np.all(np.isfinite(rec["lq"]["w"])) and np.all(np.isfinite(rec["iga"]))
        close((1.0 - rec["lw"]) * a[rec["lo"]] + rec["lw"] * a[rec["lo"] + 1], np.clip(pol, a[0], a[-1]), what=what + " lottery_record: the policy from lo and lw")
        src, units = hb.forward_units()
        assert src.shape == (P, -(-n_a // cases.XRW)) and units.shape == src.shape + (cases.XUCAP, 2)
        nu = (src >> 18) & 0x7f
        assert np.all(nu <= cases.XUCAP) and np.all(nu.sum(axis=1) >= 1), (name, T, nu)      # (a member above every policy has none)
        yb = np.random.default_rng(T).standard_normal((P, 1, M))
        hb.vjp(yb, 1)
        pbar = hb.policy_cotangent_seq(M)
        assert pbar.shape == (n_a, n_e, P, M)
        D0 = np.asarray(D).reshape((n_a, n_e), order="F")
        for k in (0, M - 1):
            close(pbar[..., k], cases.forward_iteration_pullback(a, hb.Pi, pol, D0, Dq, yb[:, 0, k]), what=f"{what} policy_cotangent_seq column {k}")
        assert hb.stats()["fallbacks"] == 0
    finally:
        hb.close()
