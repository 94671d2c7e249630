"""The discount-path entries (hank_jvp_shock, hank_vjp_shock, hank_fake_news_shock and their _dev forms; csrc/hank_shock.h) where
tests/test_gpu_shock.py does not take them: every lane geometry of the cotangent and direction widths, every n_e, the raw grids with
deep clamps and long segments, the device-pointer forms and the state the entries share with hank_vjp_het. The reference is always the
CPU oracle's dense pair (Jx, Jb) of tests/path_refs.jacobians at tests/shock_refs.KIND — unit tangents through the oracle's loop at the path, which
tests/test_shock_host.py pins against the loop with random seeds — never another device run: the tangent map is linear, so
    dagg = Jx y + Jb dbeta,    xhh_bar = jt(Jx[:n_het], yb),    beta_bar[s, m] = sum_{t,o} Jb[t, o, s] yb[t, o, m]
hold at every width. Comparisons between two device runs are stated as what they are (bits against hank_vjp_het, one column in
different batches, the transposed identity, host against device pointers) and come on top of the oracle check.

A. hank_vjp_shock at every cotangent geometry: M = 1 .. 256 on 63, 64, 65 and 129 rows — the double2 state under k_shk_bbar's plain
   doubles at stride M (every even M), MC = 1, 2, 4, .., 64, RO = 64, 32, 16, 8, nslot = 16 (M >= 64), blockIdx.y > 0 with a full and a
   partial last column block (M = 65, 66, 97, 130, 256), k_reduce_parts at ceil(M / 64) = 2, 3, 4; n_a a multiple of RO and one off it;
B. n_e = 1, 2, 5, 11, 16: the e-outer item split of k_shk_bbar and the column loop of k_shk_seed_back;
C. hank_jvp_shock at every direction geometry: even N (double2 lanes around the seed kernel's [e][n_a][N] doubles) and N >= 128 (four
   row groups per wave in k_tan_back), the policy's partials against the oracle's loop itself, a beta-only seed;
D. the raw-grid economies of tests/cases.py, section 3 — a clamped prefix of 61, 73 and 265 rows, 43 sources capped at the top, runs of
   up to 60 rows in one bracket, a period with every column clamped — under beta_path(beta, 9): the device's policy holds the edges
   (tests/test_shock_host.py: the oracle's does); hank_jvp_shock at N = 33 is held to the same bound as hank_vjp_shock on the same
   record, so a miss of one alone is a kernel finding and a miss of both an ill-conditioned grid (tests/test_gpu_vjp_variants.py, E);
E. the _dev forms give the host forms' bits; a zero d_dxhh is a zero seed, a zero d_dagg leaves the batch current;
F. state: hank_vjp_shock interleaved with hank_vjp_het at one width (g_B and g_BS share st, pbar, partS, partM), a tangent batch that
   stays current across it, a second path on cached widths (the captured graphs hold d_beta's address, not its values), and constant
   beta on records written by the persistent and the on-chip wide family (kb is rebuilt from that family's s);
G. hank_fake_news_shock's Toeplitz Jacobian against the oracle's Jb at the constant path.

Tolerance: cases.close (rel 1e-10 + abs 1e-12 on the reference's largest entry) for every oracle comparison, 1e-10 of the summed
magnitudes for the transposed identity, 1e-13 of the largest entry for one column in different batches (`_same_column` of
tests/test_gpu_vjp_variants.py), bits where stated. Every test prints its largest error-to-bound ratio (run with -s)."""
import numpy as np
import pytest

import cases
import fake_news_refs as FR
import path_refs
import shock_refs as R
import ss_diff_cases as S
from cases import jt
from test_gpu_vjp_variants import _same_column

pytestmark = pytest.mark.gpu

LAUNCH = cases.FAMILY["launch"]
GEOM_M = (1, 2, 3, 4, 6, 8, 16, 17, 32, 34, 64, 65, 66, 97, 130, 256)
GEOM_N = (2, 4, 16, 34, 64, 66, 129, 130, 256)
_WORST = {}


def _close(sec, a, b, what):
    """cases.close, and the section's largest error-to-bound ratio kept for the test's last line"""
    a, b = np.asarray(a), np.asarray(b)
    cases.close(a, b, what=what)
    _WORST[sec] = max(_WORST.get(sec, 0.0), float(np.max(np.abs(a - b)) / (1e-12 + 1e-10 * np.abs(b).max())))


def _report(sec):
    print(f"section {sec}: largest error-to-bound ratio so far {_WORST.get(sec, 0.0):.3e}")


def _refs(c, path="path"):
    """(path in force (P,), (Jx, Jb), (J2x, J2b)) of case c: its own path, the constant one (None) or a given array"""
    P = c["x"].shape[1]
    bt = c["path"] if isinstance(path, str) else np.full(P, c["beta"]) if path is None else np.asarray(path)
    a = (c["orc"], c["x"], c["V"], c["D"], bt, c["gamma"], c["n_het"])
    return bt, path_refs.jacobians(R.KIND, *a), path_refs.grid_jacobians(R.KIND, *a)


def _ctx(hank, c, schedule="launch", path="path"):
    """a context of case c with its boundary, three outputs declared, the path set (None: constant beta) and the primal run"""
    hb = cases.raw_block(hank, c["args"], schedule)
    try:
        hb.set_boundary(c["V"], c["D"])
        hb.set_het_outputs(c["n_het"])
        if path is not None:
            hb.set_discount_path(c["path"] if isinstance(path, str) else path)
        hb.primal(c["x"])
    except BaseException:
        hb.close()
        raise
    return hb


def _vjp_against_oracle(sec, hb, J, yb, what):
    """hank_vjp_shock on yb (P, n_het, M): xhh_bar and every entry of beta_bar against the oracle pair; xhh_bar's bits against
    hank_vjp_het's (device against device). -> (xhh_bar, beta_bar)"""
    Jx, Jb = J
    n_het, M = yb.shape[1:]
    xbar, bbar = hb.vjp_shock(yb, n_het)
    assert xbar.shape == (Jx.shape[2], Jx.shape[1], M) and bbar.shape == (Jx.shape[1], M), (what, xbar.shape, bbar.shape)
    _close(sec, xbar, jt(Jx[:n_het], yb), f"{what} xhh_bar")
    _close(sec, bbar, path_refs.path_bar(Jb, yb), f"{what} beta_bar")
    assert np.array_equal(xbar, hb.vjp_het(yb, n_het)), f"{what}: xhh_bar is hank_vjp_het's bit for bit"
    return xbar, bbar


def _jvp_against_oracle(sec, hb, c, J, J2, y, db, what):
    """hank_jvp_shock on y (n_hh, P, N) or None and db (P, N) or None: the aggregate, every output and the grid aggregate against
    the linear reference; served by the launches, no fallback"""
    N = next(v.shape[-1] for v in (y, db) if v is not None)
    ref = path_refs.linear(J, y, db)
    dagg = hb.jvp_shock(y, db)
    assert dagg.shape == (c["x"].shape[1], N), (what, dagg.shape)
    _close(sec, dagg, ref[:, 0, :], f"{what} dagg")
    _, dhet = hb.het_outputs(c["n_het"], np.zeros(c["x"].shape + (N,)) if y is None else y)
    for o in range(c["n_het"]):
        _close(sec, dhet[:, o, :], ref[:, o, :], f"{what} output {o}")
    J2x, J2b = J2
    ref2 = (0.0 if y is None else np.einsum("tks,ksn->tn", J2x, y)) + (0.0 if db is None else J2b @ db)
    _close(sec, hb.grid_aggregates(N)[1], ref2, f"{what} grid aggregate")
    assert hb.info()["last_tangent_family_name"] == LAUNCH and hb.stats()["fallbacks"] == 0, (what, hb.info(), hb.stats())


def _seeds(c, N, seed):
    """y (n_hh, P, N) and dbeta (P, N) of unit scale (the references are linear in them)"""
    rng = np.random.default_rng(seed)
    n_hh, P = c["x"].shape
    return rng.standard_normal((n_hh, P, N)), rng.standard_normal((P, N))


# ---- A. hank_vjp_shock at every cotangent geometry ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_a", [63, 64, 65, 129])
def test_vjp_shock_at_every_cotangent_geometry(hank, oracle_mod, n_a):
    c = R.geometry_case("shape", n_a, 3, 12)
    P = c["x"].shape[1]
    _, J, _ = _refs(c)
    yb = np.random.default_rng(100 * n_a).standard_normal((P, c["n_het"], max(GEOM_M)))
    hb = _ctx(hank, c)
    try:
        assert hb.stats()["schedule"] == 0
        for n_het in (1, 3):
            for M in GEOM_M:
                _vjp_against_oracle("A", hb, J, np.ascontiguousarray(yb[:, :n_het, :M]), f"{n_a}x3 n_het={n_het} M={M}")
            # one column alone (double, RO = 64, MC = 1), in an odd batch and in an even one (double2 state); column 70 sits in the
            # second y-block of k_shk_bbar at 97 and 130
            for k, odd, even in ((7, 33, 34), (70, 97, 130)):
                alone, in_odd, in_even = (hb.vjp_shock(np.ascontiguousarray(yb[:, :n_het, sl]), n_het)
                                          for sl in (slice(k, k + 1), slice(0, odd), slice(0, even)))
                for q, name in ((0, "xhh_bar"), (1, "beta_bar")):
                    a, o, e = alone[q][..., 0], in_odd[q][..., k], in_even[q][..., k]
                    _same_column(a, o, f"{n_a}x3 n_het={n_het} {name} column {k}: alone vs in {odd}")
                    _same_column(e, o, f"{n_a}x3 n_het={n_het} {name} column {k}: in {even} vs in {odd}")
                    _same_column(a, e, f"{n_a}x3 n_het={n_het} {name} column {k}: alone vs in {even}")
        assert hb.stats()["fallbacks"] == 0
    finally:
        hb.close()
    _report("A")


# ---- B. n_e -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_e", [1, 2, 5, 11, 16])
def test_both_entries_at_every_n_e(hank, oracle_mod, n_e):
    c = R.geometry_case("shape", 40, n_e, 10)
    P = c["x"].shape[1]
    _, J, J2 = _refs(c)
    hb = _ctx(hank, c)
    try:
        assert hb.n_e == n_e and hb.n_hh == 2
        for M in (1, 5, 32, 66):
            yb = np.random.default_rng(10 * M + n_e).standard_normal((P, c["n_het"], M))
            for n_het in (1, 3):
                _vjp_against_oracle("B", hb, J, np.ascontiguousarray(yb[:, :n_het, :]), f"40x{n_e} n_het={n_het} M={M}")
        for N in (1, 4, 33):
            y, db = _seeds(c, N, 20 * N + n_e)
            _jvp_against_oracle("B", hb, c, J, J2, y, db, f"40x{n_e} N={N}")
    finally:
        hb.close()
    _report("B")


# ---- C. hank_jvp_shock at every direction geometry ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_a", [65, 129])
def test_jvp_shock_at_every_direction_geometry(hank, oracle_mod, n_a):
    c = R.geometry_case("shape", n_a, 3, 12)
    bt, J, J2 = _refs(c)
    y, db = _seeds(c, max(GEOM_N), n_a)
    k = cases.N_ORACLE
    loop = path_refs.oracle_path_sweeps(R.KIND, c["orc"], c["x"], c["V"], c["D"], bt, c["gamma"], c["n_het"], dx=y[:, :, :k], dpath=db[:, :k])
    assert np.abs(loop["dpol"]).max() > 1e-3
    hb = _ctx(hank, c)
    try:
        for N in GEOM_N:
            what = f"{n_a}x3 N={N}"
            _jvp_against_oracle("C", hb, c, J, J2, np.ascontiguousarray(y[:, :, :N]), np.ascontiguousarray(db[:, :N]), what)
            q = min(N, k)
            _close("C", hb.dpolicy_seq(N).transpose(2, 0, 1, 3)[..., :q], loop["dpol"][..., :q], f"{what} dpolicy against the oracle's loop")
        for N in (2, 130):
            _jvp_against_oracle("C", hb, c, J, J2, None, np.ascontiguousarray(db[:, :N]), f"{n_a}x3 N={N} beta alone")
    finally:
        hb.close()
    _report("C")


# ---- D. clamp and long-segment grids ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.EDGE_ECONOMIES)
def test_clamped_prefix_top_clamp_and_long_segments_under_a_path(hank, oracle_mod, name):
    c = R.geometry_case("raw", name)
    P = c["x"].shape[1]
    assert P == cases.EDGE_P
    _, J, J2 = _refs(c)
    rng = np.random.default_rng(43)
    hb = _ctx(hank, c)
    try:
        assert hb.stats()["fallbacks"] == 0
        R.check_path_edges(name, c["grid"], hb.policy_seq().transpose(2, 0, 1))      # the device's policy holds the edges too
        # conditioning: the tangent sweeps with the seed kernel on the same record at the same bound
        y, db = _seeds(c, 33, 47)
        _jvp_against_oracle("D", hb, c, J, J2, y, db, f"{name} N=33")
        _, Jy = hb.het_outputs(c["n_het"], y)                                        # (P, n_het, 33), the batch of the line above
        for M in cases.EDGE_WIDTHS + (66,):
            for n_het in (1, 3):
                what = f"{name} n_het={n_het} M={M}"
                yb = rng.standard_normal((P, n_het, M))
                xbar, bbar = _vjp_against_oracle("D", hb, J, yb, what)
                if M == 33:      # the transposed identity of tests/test_gpu_shock.py, device against device
                    lhs = np.einsum("tom,ton->mn", yb, Jy[:, :n_het, :])
                    rhs = np.einsum("ktm,ktn->mn", xbar, y) + np.einsum("tm,tn->mn", bbar, db)
                    scale = np.einsum("tom,ton->mn", np.abs(yb), np.abs(Jy[:, :n_het, :]))
                    print(f"{what}: transposed identity, max |lhs - rhs| / scale = {np.max(np.abs(lhs - rhs) / scale):.3e}")
                    assert np.all(np.abs(lhs - rhs) <= 1e-10 * scale), what
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
    nh = c["n_het"]
    y, db = _seeds(c, W, W)
    yb = np.random.default_rng(W).standard_normal((P, nh, W))
    hb = _ctx(hank, c)
    try:
        dagg, dpol, dhet = hb.jvp_shock(y, db), hb.dpolicy_seq(W), hb.het_outputs(nh, y)[1]
        dagg_b, dpol_b = hb.jvp_shock(None, db), hb.dpolicy_seq(W)
        assert not np.array_equal(dagg_b, dagg)
        xbar, bbar = hb.vjp_shock(yb, nh)
        hb.jvp_shock(y * 0.5, db * 0.5)                       # another batch in between: every _dev call below runs its sweeps
        d_y, d_db, d_yb = _dev(y), _dev(db), _dev(yb)
        d_out = torch.zeros(P * W, dtype=torch.float64, device="cuda")
        d_xbar = torch.zeros(n_hh * P * W, dtype=torch.float64, device="cuda")
        d_bbar = torch.zeros(P * W, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        hb.jvp_shock_dev(d_y.data_ptr(), d_db.data_ptr(), W, d_out.data_ptr())
        hb.sync(); hb.check()
        assert np.array_equal(d_out.cpu().numpy().reshape((P, W), order="F"), dagg), W
        assert np.array_equal(hb.dpolicy_seq(W), dpol), W
        hb.jvp_shock_dev(0, d_db.data_ptr(), W, d_out.data_ptr())                    # a zero pointer for d_dxhh is a zero seed
        hb.sync(); hb.check()
        assert np.array_equal(d_out.cpu().numpy().reshape((P, W), order="F"), dagg_b), W
        assert np.array_equal(hb.dpolicy_seq(W), dpol_b), W
        hb.jvp_shock_dev(d_y.data_ptr(), d_db.data_ptr(), W, 0)                      # no d_dagg: the batch is current all the same
        hb.sync(); hb.check()
        assert np.array_equal(hb.het_outputs(nh, y)[1], dhet) and np.array_equal(hb.dpolicy_seq(W), dpol), W
        hb.vjp_shock_dev(nh, d_yb.data_ptr(), W, d_xbar.data_ptr(), d_bbar.data_ptr())
        hb.sync(); hb.check()
        assert np.array_equal(d_xbar.cpu().numpy().reshape((n_hh, P, W), order="F"), xbar), W
        assert np.array_equal(d_bbar.cpu().numpy().reshape((P, W), order="F"), bbar), W
        # ... and the host forms' figures are the oracle's
        _, J, J2 = _refs(c)
        _jvp_against_oracle("E", hb, c, J, J2, y, db, f"65x3 N={W}")
        _vjp_against_oracle("E", hb, J, yb, f"65x3 M={W}")
        assert hb.stats()["fallbacks"] == 0
    finally:
        hb.close()
    _report("E")


# ---- F. state ----------------------------------------------------------------------------------------------------------------------------
def test_vjp_shock_shares_its_state_with_vjp_het_and_follows_a_new_path(hank, oracle_mod):
    c = R.geometry_case("shape", 65, 3, 12)
    P, nh = c["x"].shape[1], c["n_het"]
    _, J, J2 = _refs(c)
    yb = np.random.default_rng(5).standard_normal((P, nh, 66))
    y34, y33, y66 = (np.ascontiguousarray(yb[:, :, :M]) for M in (34, 33, 66))
    hb = _ctx(hank, c)
    try:
        # 1. g_BS, g_B, g_BS at one width: the first and third calls give the same bits; another width in between as well
        first = _vjp_against_oracle("F", hb, J, y34, "M=34 first")
        het = hb.vjp_het(y34, nh)
        third = hb.vjp_shock(y34, nh)
        assert all(np.array_equal(a, b) for a, b in zip(first, third)) and np.array_equal(het, first[0])
        _vjp_against_oracle("F", hb, J, y33, "M=33 in between")
        again = hb.vjp_shock(y34, nh)
        assert all(np.array_equal(a, b) for a, b in zip(first, again))
        at66 = _vjp_against_oracle("F", hb, J, y66, "M=66 first path")
        # 2. a tangent batch stays current across hank_vjp_shock
        y, db = _seeds(c, 4, 6)
        _jvp_against_oracle("F", hb, c, J, J2, y, db, "N=4")
        dpol = hb.dpolicy_seq(4)
        hb.vjp_shock(y34, nh)
        assert np.array_equal(hb.dpolicy_seq(4), dpol)
        # 3. a second path on the cached widths: the graphs read the new beta_t
        path2 = c["path"][::-1].copy()
        _, Jr, _ = _refs(c, path2)
        assert np.abs(Jr[1] - J[1]).max() > 1e-3 * np.abs(J[1]).max()
        hb.set_discount_path(path2)
        hb.primal(c["x"])
        for yM, old, tag in ((y34, first, "M=34"), (y66, at66, "M=66")):
            new = _vjp_against_oracle("F", hb, Jr, yM, f"{tag} second path")
            assert not np.array_equal(new[0], old[0]) and not np.array_equal(new[1], old[1]), tag
        assert hb.stats()["fallbacks"] == 0
    finally:
        hb.close()
    _report("F")


@pytest.mark.parametrize("schedule", ["xcd", "wide"])
def test_constant_beta_on_records_of_the_persistent_and_the_wide_family(hank, oracle_mod, schedule):
    """no path: the record is written by the forced family's Dual pass (and, for `xcd`, by its hank_primal first); kb of the seed and
    of beta_bar is rebuilt from that record's s"""
    c = R.geometry_case("shape", 65, 3, 12)
    P, nh = c["x"].shape[1], c["n_het"]
    _, J, J2 = _refs(c, None)
    N0 = 5 if schedule == "xcd" else 96
    y0, _ = _seeds(c, N0, 8)
    yb = np.random.default_rng(9).standard_normal((P, nh, 34))
    hb = _ctx(hank, c, schedule, path=None)
    try:
        writers = [("hank_primal_jvp", lambda: hb.primal_jvp(c["x"], y0))]
        if schedule == "xcd":
            assert hb.stats()["schedule"] == 1, hb.stats()
            writers.insert(0, ("hank_primal", lambda: hb.primal(c["x"])))
        for name, write in writers:
            hb.primal(c["x"] * 1.01)                         # another record in between: the writer writes
            write()
            if name == "hank_primal_jvp":
                assert hb.info()["last_tangent_family_name"] == cases.FAMILY[schedule], (schedule, hb.info())
            assert hb.stats()["fallbacks"] == 0, (schedule, name, hb.stats())
            _vjp_against_oracle("F", hb, J, yb, f"{schedule} record of {name}, constant beta, M=34")
            _vjp_against_oracle("F", hb, J, np.ascontiguousarray(yb[:, :1, :5]), f"{schedule} record of {name}, constant beta, M=5")
            for N in (4, 33):
                y, db = _seeds(c, N, 10 + N)
                _jvp_against_oracle("F", hb, c, J, J2, y, db, f"{schedule} record of {name}, constant beta, N={N}")
    finally:
        hb.close()
    _report("F")


# ---- G. hank_fake_news_shock against the oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("econ", ["ks30x3", "hank30x3"])
@pytest.mark.parametrize("T", [3, 12])
def test_shock_jacobian_matches_the_oracle(hank, oracle_mod, econ, T):
    from hank_amd.SteadyStateJacobian import shock_jacobian
    c = S.case(econ)
    P, nh = T - 1, c["n_het"]
    x = FR.constant_path(c, P)
    _, Jb = path_refs.jacobians(R.KIND, c["orc"], x, c["V"], c["D"], np.full(P, c["args"][3]), c["gamma"], nh)
    hb = cases.raw_block(hank, c["args"][:6] + (T,) + c["args"][7:], None)
    try:
        hb.set_boundary(c["V"], c["D"])
        hb.set_het_outputs(nh)
        hb.primal(x)
        Jd = shock_jacobian(hb, nh)                                                  # (n_het, P, P)
        for o in range(nh):
            _close("G", Jd[o], Jb[:, o, :], f"{econ} T={T} J_beta of output {o}")
    finally:
        hb.close()
    _report("G")
