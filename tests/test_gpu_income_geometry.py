"""The income-path entries (hank_jvp_income, hank_vjp_income, hank_fake_news_income, hank_get_het_outputs_income and their _dev forms;
csrc/hank_income.h) where tests/test_gpu_income.py does not take them: every block shape of k_inc_ybar, every n_e up to the bound the
seed kernel unrolls to, every lane geometry of the direction widths, the raw grids with deep clamps and more than 256 rows, the
device-pointer forms, and the state the entries share with hank_vjp and keep across a new path or boundary. The reference is always the
CPU oracle's dense pair (Jx, Jy) of tests/path_refs.jacobians at tests/income_refs.KIND — unit tangents through the oracle's loop at the path,
which tests/test_income_host.py pins against the loop with random seeds — never another device run: the tangent map is linear, so
    dagg = Jx dx + Jy dy,    xhh_bar = jt(Jx[:n_het], yb),    y_bar[e, s, m] = sum_{t,o} Jy[t, o, e, s] yb[t, o, m]
hold at every width, and the policy's partials are path_refs.linear_policies' over the full width. Comparisons between two device runs
are stated as what they are (bits against hank_vjp, one column in different batches, the transposed identity, host against device
pointers) and come on top of the oracle check.

A. hank_vjp_income at every cotangent geometry: k_inc_ybar's eight (RO, MC) pairs — (64,1), (64,2), (16,4), (32,4), (8,8), (16,8),
   (8,16), (8,32); tests/test_income_host.py restates the launch arithmetic — on 63, 64, 65 and 129 rows (a multiple of RO, one off it
   on either side, several blocks); every even M (the double2 state read as plain doubles at stride M); blockIdx.y > 0 with a full and
   a partial last column block (M = 65, 66, 97, 130, 256); with and without consumption's cotangent (the direct term m_t[e] yb1);
B. n_e = 1, 2, 5, 11, 16: the level under both schedules, the e-outer item split of k_inc_ybar, the column loops of k_inc_seed_back
   unrolled to INC_NE = 16 with every slot live and with one, a seed in period P-1 alone (dyn is null); the seed's LDS staging limit at
   n_e = 16 (N = 184 | 185);
C. hank_jvp_income at every direction geometry, with a path and without: even N (double2 lanes around the seed kernel's [e][n_a][N]
   doubles) and N >= 128, k_inc_cons' direct term up to N = 256, the grid aggregate, the policy's partials over the full width;
D. the raw-grid economies of tests/cases.py, section 3, under income_path — 600, 257, 192, 700 and 600 rows (k_inc_mass strides), a
   clamped prefix of 200 rows and more, a period with every column clamped: the device's policy holds the edges (tests/test_income_host.py:
   the oracle's does), its partials in the n_e P unit directions of y are exact zeros at every clamped point; hank_jvp_income at N = 33
   is held to the same bound as hank_vjp_income on the same record, so a miss of one alone is a kernel finding and a miss of both an
   ill-conditioned grid (tests/test_gpu_vjp_variants.py, E);
E. the _dev forms give the host forms' bits; a zero d_dxhh is a zero seed, a zero d_dy hank_jvp's batch, a zero d_dagg leaves the batch
   current; hank_get_het_outputs_income_dev with the caller's dy and with the batch's own;
F. state: hank_vjp_income interleaved with hank_vjp at one width (path[PATH_INCOME].g_B and g_B share st, pbar, partS, partM), a tangent
   batch that stays current across it, a second path and a second boundary on cached widths (the captured graphs hold the addresses
   of d_inc_m and of the path, not their values; the column masses are rebuilt when the record is), and no path on records written by
   the persistent and the on-chip wide family;
G. hank_fake_news_income's Toeplitz Jacobian against the oracle's Jy at horizons of two and three periods.

Tolerance: cases.close (rel 1e-10 + abs 1e-12 on the reference's largest entry, which is above 1e-6 everywhere: asserted) for every
oracle comparison, 1e-10 of the summed magnitudes for the transposed identity, 1e-13 of the largest entry for one column in different
batches (`_same_column` of tests/test_gpu_vjp_variants.py), bits where stated. Every test prints its largest error-to-bound ratio
(run with -s)."""
import numpy as np
import pytest

import cases
import fake_news_refs as FR
import income_refs as R
import path_refs
import shock_refs
import ss_diff_cases as S
from cases import jt
from test_gpu_vjp_variants import _same_column

pytestmark = pytest.mark.gpu

LAUNCH = cases.FAMILY["launch"]
GEOM_M, GEOM_N = R.GEOM_M, R.GEOM_N
_WORST = {}


def _close(sec, a, b, what):
    """cases.close on a reference above 1e-6, and the section's largest error-to-bound ratio kept for the test's last line"""
    a, b = np.asarray(a), np.asarray(b)
    assert np.abs(b).max() > 1e-6, (what, np.abs(b).max())
    cases.close(a, b, what=what)
    _WORST[sec] = max(_WORST.get(sec, 0.0), float(np.max(np.abs(a - b)) / (1e-12 + 1e-10 * np.abs(b).max())))


def _report(sec):
    print(f"section {sec}: largest error-to-bound ratio so far {_WORST.get(sec, 0.0):.3e}")


def _refs(c, y="y", D=None):
    """(the oracle's arguments, (Jx, Jy), (J2x, J2y)) of case c at its own path, at none (None) or at a given array; D: another D_0"""
    a = (c["orc"], c["x"], c["V"], c["D"] if D is None else D, c["y"] if isinstance(y, str) else y)
    return a, path_refs.jacobians(R.KIND, *a), path_refs.grid_jacobians(R.KIND, *a)


def _ctx(hank, c, schedule="launch", y="y"):
    """a context of case c with its boundary, the path set (None: no path) and the primal run"""
    hb = cases.raw_block(hank, c["args"], schedule)
    try:
        hb.set_boundary(c["V"], c["D"])
        if y is not None:
            hb.set_income_path(c["y"] if isinstance(y, str) else y)
        hb.primal(c["x"])
    except BaseException:
        hb.close()
        raise
    return hb


def _vjp_against_oracle(sec, hb, J, yb, what):
    """hank_vjp_income on yb (P, n_het, M): xhh_bar and every entry of y_bar against the oracle pair; xhh_bar's bits against hank_vjp's
    (device against device). -> (xhh_bar, y_bar)"""
    Jx, Jy = J
    n_het, M = yb.shape[1:]
    xbar, ybar = hb.vjp_income(yb, n_het)
    assert xbar.shape == (Jx.shape[2], Jx.shape[1], M) and ybar.shape == (Jy.shape[2], Jy.shape[3], M), (what, xbar.shape, ybar.shape)
    _close(sec, xbar, jt(Jx[:n_het], yb), f"{what} xhh_bar")
    _close(sec, ybar, path_refs.path_bar(Jy, yb), f"{what} y_bar")
    assert np.array_equal(xbar, hb.vjp(yb, n_het)), f"{what}: xhh_bar is hank_vjp's bit for bit"
    return xbar, ybar


def _jvp_against_oracle(sec, hb, a, J, J2, dx, dy, what, policies=True):
    """hank_jvp_income on dx (n_hh, P, N) or None and dy (n_e, P, N) or None: the aggregate, both outputs (consumption with its direct
    term), the grid aggregate and (policies) the policy's partials over the full width against the linear reference; served by the
    launches, no fallback. a: the oracle's arguments (`_refs`)"""
    N = next(v.shape[-1] for v in (dx, dy) if v is not None)
    P = a[1].shape[1]
    ref = path_refs.linear(J, dx, dy)
    dagg = hb.jvp_income(dx, dy)
    assert dagg.shape == (P, N), (what, dagg.shape)
    _close(sec, dagg, ref[:, 0, :], f"{what} dagg")
    _, dhet = hb.het_outputs(2, dx, dy=np.zeros((hb.n_e, P, N)) if dy is None else dy)
    for o in range(2):
        _close(sec, dhet[:, o, :], ref[:, o, :], f"{what} output {o}")
    _close(sec, hb.grid_aggregates(N)[1], path_refs.grid_linear(J2, dx, dy), f"{what} grid aggregate")
    if policies:
        _close(sec, hb.dpolicy_seq(N).transpose(2, 0, 1, 3), path_refs.linear_policies(R.KIND, *a, dx=dx, dp=dy), f"{what} dpolicy")
    assert hb.info()["last_tangent_family_name"] == LAUNCH and hb.stats()["fallbacks"] == 0, (what, hb.info(), hb.stats())


def _seeds(c, N, seed):
    """dx (n_hh, P, N) and dy (n_e, P, N) of unit scale (the references are linear in them)"""
    rng = np.random.default_rng(seed)
    n_hh, P = c["x"].shape
    return rng.standard_normal((n_hh, P, N)), rng.standard_normal((c["y"].shape[0], P, N))


# ---- A. hank_vjp_income at every cotangent geometry -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n_a", [63, 64, 65, 129])
def test_vjp_income_at_every_cotangent_geometry(hank, oracle_mod, n_a):
    c = R.geometry_case("shape", n_a, 3, 12)
    P = c["x"].shape[1]
    _, J, _ = _refs(c)
    yb = np.random.default_rng(100 * n_a).standard_normal((P, 2, max(GEOM_M)))
    hb = _ctx(hank, c)
    try:
        assert hb.stats()["schedule"] == 0
        ybar = {}
        for n_het in (1, 2):
            for M in GEOM_M:
                _, ybar[n_het, M] = _vjp_against_oracle("A", hb, J, np.ascontiguousarray(yb[:, :n_het, :M]), f"{n_a}x3 n_het={n_het} M={M}")
            # one column alone (RO = 64, MC = 1), in an odd batch and in an even one (double2 state); column 70 sits in blockIdx.y = 2
            # of k_inc_ybar (MC = 32) at 97 and 130
            for k, odd, even in ((7, 33, 34), (70, 97, 130)):
                alone, in_odd, in_even = (hb.vjp_income(np.ascontiguousarray(yb[:, :n_het, sl]), n_het)
                                          for sl in (slice(k, k + 1), slice(0, odd), slice(0, even)))
                for q, name in ((0, "xhh_bar"), (1, "y_bar")):
                    a, o, e = alone[q][..., 0], in_odd[q][..., k], in_even[q][..., k]
                    _same_column(a, o, f"{n_a}x3 n_het={n_het} {name} column {k}: alone vs in {odd}")
                    _same_column(e, o, f"{n_a}x3 n_het={n_het} {name} column {k}: in {even} vs in {odd}")
                    _same_column(a, e, f"{n_a}x3 n_het={n_het} {name} column {k}: alone vs in {even}")
        for M in GEOM_M:      # n_het = 1: yb1 is zeros, the direct term m_t[e] yb1 vanishes; n_het = 2 carries it
            assert not np.array_equal(ybar[1, M], ybar[2, M]), (n_a, M)
        assert hb.stats()["fallbacks"] == 0
    finally:
        hb.close()
    _report("A")


# ---- B. n_e -----------------------------------------------------------------------------------------------------------------------------
def _level(hank, c, what):
    """the level at the path under both schedules (tests/test_gpu_income._level): against the oracle, `xcd` against `launch` in bits"""
    ref = path_refs.oracle_path_sweeps(R.KIND, c["orc"], c["x"], c["V"], c["D"], c["y"])
    P = c["x"].shape[1]
    got = {}
    for sched in ("launch", "xcd"):
        hb = cases.raw_block(hank, c["args"], sched)
        try:
            hb.set_boundary(c["V"], c["D"])
            hb.set_income_path(c["y"])
            before = hb.stats()
            agg0 = hb.primal(c["x"])
            agg, none = hb.het_outputs(2)
            assert none is None
            got[sched] = (agg0, agg, hb.policy_seq(), hb.dist_seq())
            st, tm = hb.stats(), hb.last_timings()
            assert st["fallbacks"] == 0 and st["sweep_launches"] == before["sweep_launches"], (what, sched, st)
            assert st["schedule"] == before["schedule"] == (0 if sched == "launch" else 1), (what, sched, st)
            assert tm["primal_backward"]["launches"] == P + 2 and tm["primal_backward"]["ms"] > 0, (what, sched, tm)
        finally:
            hb.close()
    agg0, agg, pol, dist = got["launch"]
    _close("B", agg0, ref["agg"][:, 0], f"{what} aggregate")
    for o in range(2):
        _close("B", agg[:, o], ref["agg"][:, o], f"{what} output {o}")
    _close("B", pol.transpose(2, 0, 1), ref["pol"], f"{what} policy")
    _close("B", dist.transpose(2, 0, 1), ref["Dseq"], f"{what} distribution")
    assert all(np.array_equal(g, l) for g, l in zip(got["xcd"], got["launch"])), what


N_E = [1, 2, 5, 11, 16]      # one test per entry and n_e: the oracle runs the value function n_e times a period, the first of the three pays


@pytest.mark.parametrize("n_e", N_E)
def test_the_level_at_every_n_e(hank, oracle_mod, n_e):
    _level(hank, R.geometry_case("shape", 40, n_e, 10), f"40x{n_e}")
    _report("B")


@pytest.mark.parametrize("n_e", N_E)
def test_vjp_income_at_every_n_e(hank, oracle_mod, n_e):
    c = R.geometry_case("shape", 40, n_e, 10)
    P = c["x"].shape[1]
    _, J, _ = _refs(c)
    hb = _ctx(hank, c)
    try:
        assert hb.n_e == n_e and hb.n_hh == 2 and c["y"].shape == (n_e, P)
        for M in (1, 5, 32, 66):
            yb = np.random.default_rng(10 * M + n_e).standard_normal((P, 2, M))
            for n_het in (1, 2):
                _vjp_against_oracle("B", hb, J, np.ascontiguousarray(yb[:, :n_het, :]), f"40x{n_e} n_het={n_het} M={M}")
        assert hb.stats()["fallbacks"] == 0
    finally:
        hb.close()
    _report("B")


@pytest.mark.parametrize("n_e", N_E)
def test_jvp_income_at_every_n_e(hank, oracle_mod, n_e):
    c = R.geometry_case("shape", 40, n_e, 10)
    P = c["x"].shape[1]
    a, J, J2 = _refs(c)
    hb = _ctx(hank, c)
    try:
        assert hb.n_e == n_e and hb.n_hh == 2 and c["y"].shape == (n_e, P)
        for N in (1, 4, 33):
            dx, dy = _seeds(c, N, 20 * N + n_e)
            _jvp_against_oracle("B", hb, a, J, J2, dx, dy, f"40x{n_e} N={N} inputs and y")
            _jvp_against_oracle("B", hb, a, J, J2, None, dy, f"40x{n_e} N={N} y alone")
            last = np.zeros((1, P, 1)); last[0, P - 1] = 1.0      # no Pi v dy_{t+1} term in this seed: dyn is null at t = P-1
            _jvp_against_oracle("B", hb, a, J, J2, None, dy * last, f"40x{n_e} N={N} y_{P - 1} alone")
    finally:
        hb.close()
    _report("B")


def test_jvp_income_at_sixteen_states_where_the_seed_s_staging_ends(hank, oracle_mod):
    """k_inc_seed_back stages Pi and two dy slices, n_e n_e + 2 n_e N doubles, in LDS up to 48 KiB and reads global memory beyond: at
    the bound n_e = 16 the last width that fits is N = 184"""
    c = R.geometry_case("shape", 40, 16, 4)
    assert 8 * (256 + 32 * 184) <= 48 * 1024 < 8 * (256 + 32 * 185) and c["y"].shape[0] == 16
    a, J, J2 = _refs(c)
    hb = _ctx(hank, c)
    try:
        for N in (184, 185):
            dx, dy = _seeds(c, N, N)
            _jvp_against_oracle("B", hb, a, J, J2, dx, dy, f"40x16 T=4 N={N} inputs and y")
            _jvp_against_oracle("B", hb, a, J, J2, None, dy, f"40x16 T=4 N={N} y alone")
    finally:
        hb.close()
    _report("B")


# ---- C. hank_jvp_income at every direction geometry ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [True, False], ids=["path", "no-path"])
@pytest.mark.parametrize("n_a", [65, 129])
def test_jvp_income_at_every_direction_geometry(hank, oracle_mod, n_a, path):
    c = R.geometry_case("shape", n_a, 3, 12)
    y = "y" if path else None
    a, J, J2 = _refs(c, y)
    dx, dy = _seeds(c, max(GEOM_N), n_a)
    hb = _ctx(hank, c, y=y)
    try:
        for N in GEOM_N:
            _jvp_against_oracle("C", hb, a, J, J2, np.ascontiguousarray(dx[:, :, :N]), np.ascontiguousarray(dy[:, :, :N]), f"{n_a}x3 {y} N={N}")
        for N in (2, 130):
            _jvp_against_oracle("C", hb, a, J, J2, None, np.ascontiguousarray(dy[:, :, :N]), f"{n_a}x3 {y} N={N} y alone")
    finally:
        hb.close()
    _report("C")


# ---- D. clamp and long-segment grids ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.EDGE_ECONOMIES)
def test_clamped_prefix_top_clamp_and_long_segments_under_an_income_path(hank, oracle_mod, name):
    """The policy's partials are held to the oracle point by point on the shape grids (B, C, E, F), not here: a partial is a ratio of
    knot differences, so an ulp of a knot (1.1e-16 of a cash-on-hand near one) enters it divided by the width of the bracket the policy
    lies in, and these grids have brackets down to 4e-12: no bound of cases.close's kind follows from the formats. Measured on an MI355X
    with the 27 unit directions (largest entry 0.97 .. 0.98), max err and the bracket at that point: short-top 1.4e-13 (7.8e-3),
    swing 2.7e-12 (1.6e-4), both 2.9e-12 (1.9e-5), dense-bottom 5.8e-12 (9.5e-6), deep-prefix 1.3e-10 (4.3e-7; 1.3 times what
    cases.close would allow) — ordered as the brackets are. The figure is printed; what is asserted of the partials here is the
    exact zero at every clamped point, and the aggregates, outputs and cotangents, which weigh those points by their mass, at
    cases.close (largest error-to-bound ratio of the section: 8.5e-4)."""
    c = R.geometry_case("raw", name)
    n_e, P = c["y"].shape
    assert P == cases.EDGE_P and n_e * P == 27
    a, J, J2 = _refs(c)
    ref = path_refs.oracle_path_sweeps(R.KIND, *a)
    rng = np.random.default_rng(43)
    hb = _ctx(hank, c)
    try:
        assert hb.stats()["fallbacks"] == 0 and hb.n_a == c["grid"].size
        pol = hb.policy_seq().transpose(2, 0, 1)
        shock_refs.check_path_edges(name, c["grid"], pol)                                   # the device's policy holds the edges too
        _close("D", pol, ref["pol"], f"{name} policy")
        _close("D", hb.het_outputs(2)[0][:, 1], ref["agg"][:, 1], f"{name} consumption (holds sum_e y_t[e] m_t[e])")
        # a clamped point's policy does not move with any y_s[e']: exact zeros in the n_e P unit directions
        unit = np.eye(n_e * P).reshape((n_e, P, n_e * P), order="F")
        _jvp_against_oracle("D", hb, a, J, J2, None, unit, f"{name} the {n_e * P} unit directions of y", policies=False)
        clamped = pol <= c["grid"][0]
        assert clamped.any(axis=1).any(), name
        dpol = hb.dpolicy_seq(n_e * P).transpose(2, 0, 1, 3)
        assert not np.any(dpol[clamped]) and np.any(dpol[~clamped]), name
        err = np.abs(dpol - path_refs.linear_policies(R.KIND, *a, dp=unit))                # measured, not asserted (the docstring)
        k = tuple(int(q) for q in np.unravel_index(np.argmax(err), err.shape))
        m0 = min(max(int(np.searchsorted(c["grid"], pol[k[:3]])), 1), c["grid"].size - 1)
        print(f"{name}: the policy's partials point by point, max err {err.max():.3e} at (t, a, e, direction) = {k}, where the policy "
              f"{pol[k[:3]]:.3e} lies in a bracket {c['grid'][m0] - c['grid'][m0 - 1]:.3e} wide (first bracket of the grid: {c['grid'][1] - c['grid'][0]:.3e})")
        # conditioning: the tangent sweeps with the seed kernel on the same record at the same bound
        dx, dy = _seeds(c, 33, 47)
        _jvp_against_oracle("D", hb, a, J, J2, dx, dy, f"{name} N=33", policies=False)
        _, Jd = hb.het_outputs(2, dx, dy=dy)                                         # (P, 2, 33), the batch of the line above
        for M in cases.EDGE_WIDTHS + (66,):
            for n_het in (1, 2):
                what = f"{name} n_het={n_het} M={M}"
                yb = rng.standard_normal((P, n_het, M))
                xbar, ybar = _vjp_against_oracle("D", hb, J, yb, what)
                if M == 33:      # the transposed identity of tests/test_gpu_income.py, device against device
                    lhs = np.einsum("tom,ton->mn", yb, Jd[:, :n_het, :])
                    rhs = np.einsum("ktm,ktn->mn", xbar, dx) + np.einsum("etm,etn->mn", ybar, dy)
                    scale = np.einsum("tom,ton->mn", np.abs(yb), np.abs(Jd[:, :n_het, :]))
                    print(f"{what}: transposed identity, max |lhs - rhs| / scale = {np.max(np.abs(lhs - rhs) / scale):.3e}")
                    assert np.all(np.abs(lhs - rhs) <= 1e-10 * scale), what
        assert hb.stats()["fallbacks"] == 0
    finally:
        hb.close()
    _report("D")


# ---- E. the device-pointer forms -----------------------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.asfortranarray(a).reshape(-1, order="F").copy()).cuda()


@pytest.mark.parametrize("W", [5, 34])
def test_device_pointer_forms_equal_the_host_forms(hank, oracle_mod, W):
    import torch
    c = R.geometry_case("shape", 65, 3, 12)
    n_hh, P = c["x"].shape
    n_e = c["y"].shape[0]
    dx, dy = _seeds(c, W, W)
    yb = np.random.default_rng(W).standard_normal((P, 2, W))
    hb = _ctx(hank, c)
    try:
        dagg, dpol = hb.jvp_income(dx, dy), hb.dpolicy_seq(W)
        agg, dhet = hb.het_outputs(2, dx, dy=dy)
        _, dhet2 = hb.het_outputs(2, dx, dy=2.0 * dy)                         # the caller's dy in place of the batch's own
        assert not np.array_equal(dhet2[:, 1, :], dhet[:, 1, :]) and np.array_equal(dhet2[:, 0, :], dhet[:, 0, :])
        dagg_y, dpol_y = hb.jvp_income(None, dy), hb.dpolicy_seq(W)
        dagg_x, dpol_x, dhet_x = hb.jvp(dx), hb.dpolicy_seq(W), hb.het_outputs(2, dx)[1]
        assert not np.array_equal(dagg_y, dagg) and not np.array_equal(dagg_x, dagg)
        xbar, ybar = hb.vjp_income(yb, 2)
        hb.jvp_income(dx * 0.5, dy * 0.5)                     # another batch in between: every _dev call below runs its sweeps
        d_dx, d_dy, d_dy2, d_yb = _dev(dx), _dev(dy), _dev(2.0 * dy), _dev(yb)
        d_out = torch.zeros(P * W, dtype=torch.float64, device="cuda")
        d_agg = torch.zeros(P * 2, dtype=torch.float64, device="cuda")
        d_dhet = torch.zeros(P * 2 * W, dtype=torch.float64, device="cuda")
        d_xbar = torch.zeros(n_hh * P * W, dtype=torch.float64, device="cuda")
        d_ybar = torch.zeros(n_e * P * W, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        host = lambda d, *shape: d.cpu().numpy().reshape(shape, order="F")      # noqa: E731

        hb.jvp_income_dev(d_dx.data_ptr(), d_dy.data_ptr(), W, d_out.data_ptr())
        hb.sync(); hb.check()
        assert np.array_equal(host(d_out, P, W), dagg) and np.array_equal(hb.dpolicy_seq(W), dpol), W
        hb.het_outputs_dev(2, d_dx.data_ptr(), W, d_agg.data_ptr(), d_dhet.data_ptr(), d_dy=d_dy2.data_ptr())
        hb.sync(); hb.check()
        assert np.array_equal(host(d_agg, P, 2), agg) and np.array_equal(host(d_dhet, P, 2, W), dhet2), W
        hb.het_outputs_dev(2, d_dx.data_ptr(), W, d_agg.data_ptr(), d_dhet.data_ptr(), d_dy=d_dy.data_ptr())
        hb.sync(); hb.check()
        assert np.array_equal(host(d_agg, P, 2), agg) and np.array_equal(host(d_dhet, P, 2, W), dhet), W
        d_dhet.zero_()
        hb.het_outputs_dev(2, d_dx.data_ptr(), W, d_agg.data_ptr(), d_dhet.data_ptr(), d_dy=0)      # no d_dy: the batch's own dy
        hb.sync(); hb.check()
        assert np.array_equal(host(d_dhet, P, 2, W), dhet), W
        hb.jvp_income_dev(0, d_dy.data_ptr(), W, d_out.data_ptr())                   # a zero pointer for d_dxhh is a zero seed
        hb.sync(); hb.check()
        assert np.array_equal(host(d_out, P, W), dagg_y) and np.array_equal(hb.dpolicy_seq(W), dpol_y), W
        hb.jvp_income_dev(d_dx.data_ptr(), 0, W, d_out.data_ptr())                   # a zero pointer for d_dy: hank_jvp's batch
        hb.sync(); hb.check()
        assert np.array_equal(host(d_out, P, W), dagg_x) and np.array_equal(hb.dpolicy_seq(W), dpol_x), W
        assert np.array_equal(hb.het_outputs(2, dx)[1], dhet_x), W
        hb.jvp_income_dev(d_dx.data_ptr(), d_dy.data_ptr(), W, 0)                    # no d_dagg: the batch is current all the same
        hb.sync(); hb.check()
        assert np.array_equal(hb.het_outputs(2, dx)[1], dhet) and np.array_equal(hb.dpolicy_seq(W), dpol), W
        hb.vjp_income_dev(2, d_yb.data_ptr(), W, d_xbar.data_ptr(), d_ybar.data_ptr())
        hb.sync(); hb.check()
        assert np.array_equal(host(d_xbar, n_hh, P, W), xbar) and np.array_equal(host(d_ybar, n_e, P, W), ybar), W
        # ... and the host forms' figures are the oracle's
        a, J, J2 = _refs(c)
        _jvp_against_oracle("E", hb, a, J, J2, dx, dy, f"65x3 N={W}")
        _vjp_against_oracle("E", hb, J, yb, f"65x3 M={W}")
        assert hb.stats()["fallbacks"] == 0
    finally:
        hb.close()
    _report("E")


# ---- F. state ----------------------------------------------------------------------------------------------------------------------------
def test_vjp_income_shares_its_state_with_vjp_and_follows_a_new_path_and_a_new_boundary(hank, oracle_mod):
    c = R.geometry_case("shape", 65, 3, 12)
    P = c["x"].shape[1]
    a, J, J2 = _refs(c)
    yb = np.random.default_rng(5).standard_normal((P, 2, 66))
    y34, y33, y66 = (np.ascontiguousarray(yb[:, :, :M]) for M in (34, 33, 66))
    hb = _ctx(hank, c)
    try:
        # 1. path[PATH_INCOME].g_B, g_B, path[PATH_INCOME].g_B at one width: the first and third calls give the same bits; another
        # width in between as well
        first = _vjp_against_oracle("F", hb, J, y34, "M=34 first")
        plain = hb.vjp(y34, 2)
        third = hb.vjp_income(y34, 2)
        assert all(np.array_equal(p, q) for p, q in zip(first, third)) and np.array_equal(plain, first[0])
        _vjp_against_oracle("F", hb, J, y33, "M=33 in between")
        again = hb.vjp_income(y34, 2)
        assert all(np.array_equal(p, q) for p, q in zip(first, again))
        at66 = _vjp_against_oracle("F", hb, J, y66, "M=66 first path")
        # 2. a tangent batch stays current across hank_vjp_income
        dx, dy = _seeds(c, 4, 6)
        _jvp_against_oracle("F", hb, a, J, J2, dx, dy, "N=4")
        dpol = hb.dpolicy_seq(4)
        hb.vjp_income(y34, 2)
        assert np.array_equal(hb.dpolicy_seq(4), dpol)
        # 3. a second path on the cached widths: the graphs read the new y_t[e]
        y2 = -c["y"]
        a2, Jr, _ = _refs(c, y2)
        assert np.abs(Jr[1] - J[1]).max() > 1e-3 * np.abs(J[1]).max()
        hb.set_income_path(y2)
        hb.primal(c["x"])
        second = {}
        for yM, old, tag in ((y34, first, "M=34"), (y66, at66, "M=66")):
            second[tag] = new = _vjp_against_oracle("F", hb, Jr, yM, f"{tag} second path")
            assert not np.array_equal(new[0], old[0]) and not np.array_equal(new[1], old[1]), tag
        cons = hb.het_outputs(2)[0][:, 1]
        _close("F", cons, path_refs.oracle_path_sweeps(R.KIND, *a2)["agg"][:, 1], "second path: consumption")
        # 4. a second boundary on the cached widths: the column masses m_t[e] are the new record's
        D2 = R.rescaled_D0(c)
        a3, Jd, _ = _refs(c, y2, D2)
        ref2, ref3 = path_refs.oracle_path_sweeps(R.KIND, *a2), path_refs.oracle_path_sweeps(R.KIND, *a3)
        assert np.abs(ref3["mass"] - ref2["mass"]).max() > 0.1
        direct = lambda m: m.T[:, :, None] * y34[None, :, 1, :]                   # noqa: E731  (n_e, P, M): m_t[e] yb1_t[m]
        assert np.abs(direct(ref3["mass"]) - direct(ref2["mass"])).max() > 1e-2 * np.abs(path_refs.path_bar(Jd[1], y34)).max()
        hb.set_boundary(c["V"], D2)
        hb.primal(c["x"])
        for yM, tag in ((y34, "M=34"), (y66, "M=66")):
            new = _vjp_against_oracle("F", hb, Jd, yM, f"{tag} second boundary")
            assert not np.array_equal(new[1], second[tag][1]), tag
        cons3 = hb.het_outputs(2)[0][:, 1]
        _close("F", cons3, ref3["agg"][:, 1], "second boundary: consumption")
        assert not np.array_equal(cons3, cons)
        assert hb.stats()["fallbacks"] == 0
    finally:
        hb.close()
    _report("F")


@pytest.mark.parametrize("schedule", ["xcd", "wide"])
def test_no_path_on_records_of_the_persistent_and_the_wide_family(hank, oracle_mod, schedule):
    """no path: the record is written by the forced family's Dual pass (and, for `xcd`, by its hank_primal first); the seed reads that
    record's kc and v, k_inc_mass its distributions"""
    c = R.geometry_case("shape", 65, 3, 12)
    P = c["x"].shape[1]
    a, J, J2 = _refs(c, None)
    N0 = 5 if schedule == "xcd" else 96
    dx0, _ = _seeds(c, N0, 8)
    yb = np.random.default_rng(9).standard_normal((P, 2, 34))
    hb = _ctx(hank, c, schedule, y=None)
    try:
        writers = [("hank_primal_jvp", lambda: hb.primal_jvp(c["x"], dx0))]
        if schedule == "xcd":
            assert hb.stats()["schedule"] == 1, hb.stats()
            writers.insert(0, ("hank_primal", lambda: hb.primal(c["x"])))
        for name, write in writers:
            hb.primal(c["x"] * 1.01)                         # another record in between: the writer writes
            write()
            if name == "hank_primal_jvp":
                assert hb.info()["last_tangent_family_name"] == cases.FAMILY[schedule], (schedule, hb.info())
            assert hb.stats()["fallbacks"] == 0, (schedule, name, hb.stats())
            _vjp_against_oracle("F", hb, J, yb, f"{schedule} record of {name}, no path, M=34")
            _vjp_against_oracle("F", hb, J, np.ascontiguousarray(yb[:, :1, :5]), f"{schedule} record of {name}, no path, M=5")
            for N in (4, 33):
                dx, dy = _seeds(c, N, 10 + N)
                _jvp_against_oracle("F", hb, a, J, J2, dx, dy, f"{schedule} record of {name}, no path, N={N}")
    finally:
        hb.close()
    _report("F")


# ---- G. hank_fake_news_income at short horizons ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("econ", ["ks30x3", "hank30x3"])
@pytest.mark.parametrize("T", [2, 3])
def test_income_jacobian_matches_the_oracle_at_short_horizons(hank, oracle_mod, econ, T):
    from hank_amd.SteadyStateJacobian import income_jacobian
    c = S.case(econ)
    P = T - 1
    x = FR.constant_path(c, P)
    _, Jy = path_refs.jacobians(R.KIND, c["orc"], x, c["V"], c["D"], None)
    hb = cases.raw_block(hank, c["args"][:6] + (T,) + c["args"][7:], None)
    try:
        hb.set_boundary(c["V"], c["D"])
        hb.primal(x)
        Jd = income_jacobian(hb, 2)                                                  # (2, P, n_e, P)
        assert Jd.shape == (2, P, hb.n_e, P)
        for o in range(2):
            _close("G", Jd[o], Jy[:, o], f"{econ} T={T} J_y of output {o}")
        assert hb.stats()["fallbacks"] == 0
    finally:
        hb.close()
    _report("G")
