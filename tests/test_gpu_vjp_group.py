"""hank_vjp_group on the device: cotangents on the group outputs of hank_set_group_outputs through the transposed sweeps
(csrc/hank_adjoint.h: k_adj_dist_grp). The reference throughout is the dense group Jacobian J (K, P, n_hh, P)
from tests/group_refs.group_reference under unit tangents (at most 32 columns per oracle pass, once per case), transposed:
xbar = sum J[k,t,i,s] g[t,k,m], plus cases.jt(cases.oracle_jacobian(...), agg_bar) when outputs 0 and 1 carry cotangents too — never
another run of the device. Tolerance: cases.close (rel 1e-10 + abs 1e-12 on the reference's largest entry), per input row."""
import numpy as np
import pytest

import cases
import group_refs as gr
import sweep_refs
from cases import block as _block, close as _close
from conftest import ks_paths, ks_setup

pytestmark = pytest.mark.gpu

_J = {}
# every group's block of J exceeds this (measured on the CPU, the smallest block per case: random weights 0.43 at 33x2, 1.05 at
# 257x4, 6.7e-2 at 33x2 with one period; Krusell-Smith 130x3 0.22; one-asset HANK 80x3 0.11)
J_MIN = 1e-2


def group_jacobian(key, orc, xhh, V, D, W, base):
    """J (K, P, n_hh, P): d Y^k_t / d input i at period s from unit tangents through group_refs.group_reference, once per key;
    every group's block must be non-trivial"""
    if key not in _J:
        n_hh, P = xhh.shape
        y = cases.unit_tangents(n_hh, P)
        dagg = np.concatenate([gr.group_reference(orc, xhh, y[:, :, c0:c0 + 32], V, D, W, base)[1] for c0 in range(0, n_hh * P, 32)], axis=2)
        J = np.ascontiguousarray(dagg.reshape(W.shape[1], P, P, n_hh).transpose(0, 1, 3, 2))
        for k in range(J.shape[0]):
            print(f"{key} group {k} (base {int(np.broadcast_to(base, (J.shape[0],))[k])}): max |J| {np.abs(J[k]).max():.3e}")
            assert np.abs(J[k]).max() > J_MIN, (key, k)
        J.setflags(write=False)
        _J[key] = J
    return _J[key]


def _jtg(J, g):
    """J (K, P, n_hh, P), g (P, K, M) -> (n_hh, P, M)"""
    return np.einsum("ktis,tkm->ism", J, g)


def _rows(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for i in range(want.shape[0]):
        _close(got[i], want[i], what=f"{what} input {i}")


_RANDOM = {}


def _random_case(n_a, n_e, T=6):
    """standard-normal weights (G, 32), bases cycling MASS, POLICY, CONS (test_gpu_group_outputs.test_random_weights' case), the group
    Jacobian of all 32 and the oracle's Jacobian of outputs 0 and 1: a call with K groups uses the first K"""
    key = (n_a, n_e, T)
    if key not in _RANDOM:
        m, V, D, xhh, orc = cases.shape(n_a, n_e, T)
        W = np.random.default_rng(n_a).standard_normal((n_a * n_e, 32))
        base = np.arange(32, dtype=np.int32) % 3
        _RANDOM[key] = (W, base, group_jacobian(("random",) + key, orc, xhh, V, D, W, base), cases.oracle_jacobian(orc, V, D, xhh))
    return _RANDOM[key]


def _open(hank, n_a, n_e, T=6, schedule=None):
    m, V, D, xhh, _ = cases.shape(n_a, n_e, T)
    hb = _block(hank, m, schedule)
    hb.set_boundary(V, D)
    hb.primal(xhh)
    return hb


# ---- 1. shapes where the kernel can go wrong ---------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 9, 32])
@pytest.mark.parametrize("n_a,n_e", [(33, 2), (257, 4)])
def test_vjp_group_is_the_group_jacobian_transposed(hank, oracle_mod, n_a, n_e, K):
    """a block edge inside the rows for R = 8 and R = 64 (33 = 4 * 8 + 1, 257 = 4 * 64 + 1); M = 1 (scalar lanes, R = 64), 2 (one
    double2 lane), 3 (odd, NC = 4), 34 (MV = 17: a second, partly empty block column); with and without cotangents on outputs 0, 1"""
    W, base, J, J2 = _random_case(n_a, n_e)
    hb = _open(hank, n_a, n_e)
    try:
        hb.set_group_outputs(W[:, :K], base[:K])
        for M in (1, 2, 3, 34):
            rng = np.random.default_rng(1000 * K + M)
            g, yb = rng.standard_normal((5, K, M)), rng.standard_normal((5, 2, M))
            got = hb.vjp_group(g)
            _rows(got, _jtg(J[:K], g), f"{n_a}x{n_e} K={K} M={M}")
            assert np.array_equal(hb.vjp_group(g), got)                      # asked again: the same bits
            got2 = hb.vjp_group(g, agg_bar=yb, n_het=2)
            _rows(got2, _jtg(J[:K], g) + cases.jt(J2, yb), f"{n_a}x{n_e} K={K} M={M} with agg_bar")
            assert np.array_equal(hb.vjp_group(g, agg_bar=yb, n_het=2), got2)
    finally:
        hb.close()


# ---- 2. one group alone ------------------------------------------------------------------------------------------------------
def test_one_group_alone(hank, oracle_mod):
    """cotangents on a single group of 32: a swapped group or base index shows"""
    W, base, J, _ = _random_case(33, 2)
    hb = _open(hank, 33, 2)
    try:
        hb.set_group_outputs(W, base)
        for k in (0, 1, 2, 31):
            g = np.zeros((5, 32, 2))
            g[:, k, :] = np.random.default_rng(k).standard_normal((5, 2))
            _rows(hb.vjp_group(g), _jtg(J, g), f"group {k} alone")
    finally:
        hb.close()


# ---- 3. every record writer --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", ["launch", "xcd", "wide"])
def test_a_record_of_every_writer_krusell_smith_130x3(hank, oracle_mod, schedule):
    m, ss, orc = ks_setup(130, 3, 40)
    xhh = np.ascontiguousarray(ks_paths(m, ss, "x1", 0.05)[0][2:4])
    W, base = gr.ks_groups()
    J = group_jacobian("ks130", orc, xhh, ss.value, ss.D, W, base)
    rng = np.random.default_rng(5)
    g, y = rng.standard_normal((39, 12, 5)), rng.standard_normal((2, 39, 5))
    hb = _block(hank, m, schedule)
    try:
        hb.set_boundary(ss.value, ss.D)
        hb.set_group_outputs(W, base)
        for entry in ("primal", "primal_jvp"):
            hb.primal(xhh * 1.01)                                            # (a record of another x: every sweep runs)
            if entry == "primal":
                hb.primal(xhh)
            else:
                hb.primal_jvp(xhh, y)
            _rows(hb.vjp_group(g), _jtg(J, g), f"ks130 {schedule} {entry}")
        assert hb.stats()["fallbacks"] == 0
    finally:
        hb.close()


# ---- 4. three inputs ---------------------------------------------------------------------------------------------------------
def test_three_inputs_one_asset_hank(hank, oracle_mod):
    from hank_amd.groups import wealth_groups
    m, ss, xhh, orc = cases.economy("hank", 2.0)
    P = xhh.shape[1]
    Wg = wealth_groups(ss.D, 80, 3, (0.0, 0.7, 0.95, 1.0))
    W, base = np.concatenate([Wg, Wg], axis=1), np.repeat(np.array([gr.CONS, gr.POLICY], dtype=np.int32), 3)
    J = group_jacobian("hank80", orc, xhh, ss.value, ss.D, W, base)
    g = np.random.default_rng(4).standard_normal((P, 6, 4))
    hb = _block(hank, m, None)
    try:
        assert hb.n_hh == 3
        hb.set_boundary(ss.value, ss.D)
        hb.set_group_outputs(W, base)
        hb.primal(xhh)
        got = hb.vjp_group(g)
        assert got.shape == (3, P, 4)
        _rows(got, _jtg(J, g), "hank 80x3")
        gc = g.copy()
        gc[:, 3:, :] = 0.0                                                   # CONS alone: the transfer's row on its own
        want = _jtg(J, gc)
        assert np.abs(want[2]).max() > 1e-2
        _close(hb.vjp_group(gc)[2], want[2], what="hank 80x3, tr row of CONS")
    finally:
        hb.close()


# ---- 5. a horizon of one period ----------------------------------------------------------------------------------------------
def test_horizon_of_one_period(hank, oracle_mod):
    W, base, J, J2 = _random_case(33, 2, 2)
    hb = _open(hank, 33, 2, 2)
    try:
        assert hb.P == 1
        hb.set_group_outputs(W[:, :9], base[:9])
        rng = np.random.default_rng(9)
        g, yb = rng.standard_normal((1, 9, 2)), rng.standard_normal((1, 2, 2))
        _rows(hb.vjp_group(g), _jtg(J[:9], g), "P = 1")
        _rows(hb.vjp_group(g, agg_bar=yb, n_het=2), _jtg(J[:9], g) + cases.jt(J2, yb), "P = 1 with agg_bar")
    finally:
        hb.close()


# ---- 6. changing the groups --------------------------------------------------------------------------------------------------
def test_another_set_of_groups_is_honoured(hank, oracle_mod):
    W, base, J, _ = _random_case(33, 2)
    sel = np.arange(31, 14, -1)                                              # 17 other weights, other bases
    hb = _open(hank, 33, 2)
    try:
        rng = np.random.default_rng(6)
        g9, g17 = rng.standard_normal((5, 9, 2)), rng.standard_normal((5, 17, 2))
        hb.set_group_outputs(W[:, :9], base[:9])
        a = hb.vjp_group(g9)
        _rows(a, _jtg(J[:9], g9), "K = 9")
        hb.set_group_outputs(W[:, sel], base[sel])
        _rows(hb.vjp_group(g17), _jtg(J[sel], g17), "K = 17, other weights")
        hb.set_group_outputs(W[:, :9], base[:9])
        c = hb.vjp_group(g9)
        _rows(c, _jtg(J[:9], g9), "K = 9 again")
        assert np.array_equal(a, c)
    finally:
        hb.close()


# ---- 7. what it leaves alone -------------------------------------------------------------------------------------------------
def test_it_leaves_the_batch_the_memo_and_hank_vjp_alone(hank, oracle_mod):
    W, base, _, _ = _random_case(33, 2)
    m, V, D, xhh, _ = cases.shape(33, 2, 6)
    hb = _block(hank, m, None)
    try:
        rng = np.random.default_rng(7)
        y, yb, g = rng.standard_normal((2, 5, 4)), rng.standard_normal((5, 2, 4)), rng.standard_normal((5, 9, 4))
        hb.set_boundary(V, D)
        hb.set_group_outputs(W[:, :9], base[:9])
        hb.primal_jvp(xhh, y)
        hb.jvp(y)
        a, d = hb.group_outputs(y)
        dpol = hb.dpolicy_seq(4)
        x0, p0 = hb.vjp(yb, 2), hb.policy_cotangent_seq(4)
        st0 = hb.stats()
        hb.vjp_group(g, agg_bar=yb, n_het=2)
        assert not np.array_equal(hb.policy_cotangent_seq(4), p0)            # (the group call's own policy cotangent is served)
        a1, d1 = hb.group_outputs(y)
        assert np.array_equal(a1, a) and np.array_equal(d1, d)
        assert np.array_equal(hb.dpolicy_seq(4), dpol)
        assert np.array_equal(hb.vjp(yb, 2), x0) and np.array_equal(hb.policy_cotangent_seq(4), p0)
        st = hb.stats()
        assert st["primal_sweeps"] == st0["primal_sweeps"] and st["primal_memo_hits"] == st0["primal_memo_hits"]
        hb.primal_jvp(xhh, y)                                                # the memo survived
        assert hb.stats()["primal_memo_hits"] == st0["primal_memo_hits"] + 1
        t = hb.last_vjp_timings()
        assert t["sweep_a"]["launches"] == 5
    finally:
        hb.close()


# ---- 8. the policy cotangent -------------------------------------------------------------------------------------------------
def test_policy_cotangent_pairs_with_the_policy_partials(hank, oracle_mod):
    """MASS and POLICY groups and output 0 reach the outputs through the distribution and the policy partials alone (no direct
    term on the inputs): <pbar, dpol> = <g, dY_group> + <yb0, dY_0>, column by column (tests/test_vjp_het_host.py's pairing)"""
    W, base, _, _ = _random_case(33, 2)
    sel = np.flatnonzero(base != gr.CONS)[:8]
    hb = _open(hank, 33, 2)
    try:
        rng = np.random.default_rng(8)
        y, yb, g = rng.standard_normal((2, 5, 3)), rng.standard_normal((5, 1, 3)), rng.standard_normal((5, 8, 3))
        hb.set_group_outputs(W[:, sel], base[sel])
        dagg = hb.jvp(y)
        dgrp = hb.group_outputs(y)[1]
        dpol = hb.dpolicy_seq(3)
        hb.vjp_group(g, agg_bar=yb, n_het=1)
        pbar = hb.policy_cotangent_seq(3)
        assert pbar.shape == dpol.shape
        for j in range(3):
            lhs = np.sum(pbar[..., j] * dpol[..., j])
            rhs = np.sum(g[:, :, j] * dgrp[:, :, j]) + np.sum(yb[:, 0, j] * dagg[:, j])
            scale = np.sum(np.abs(pbar[..., j] * dpol[..., j]))
            print(f"column {j}: <pbar, dpol> {lhs:.12e}, <g, dY> {rhs:.12e}, scale {scale:.3e}")
            assert abs(rhs) > 1e-3 * scale and abs(lhs - rhs) <= 1e-10 * scale
    finally:
        hb.close()


# ---- 9, 10, 11. the boundary's cotangents ------------------------------------------------------------------------------------
def test_all_ones_weights_give_hank_vjp_boundary(hank, oracle_mod):
    hb = _open(hank, 33, 2)
    try:
        yb = np.random.default_rng(10).standard_normal((5, 2, 3))
        hb.set_group_outputs(np.ones((66, 2)), [gr.POLICY, gr.CONS])
        want = hb.vjp_boundary(yb, 2)
        got = hb.vjp_group(yb, value_end=True, D_init=True)
        for a, b, what in zip(got, want, ("xhh_bar", "value_end_bar", "D_init_bar")):
            assert np.abs(b).max() > 1e-6, what
            _close(a, b, what=f"W = 1: {what}")
        only_d = hb.vjp_group(yb, D_init=True)
        assert only_d[1] is None and np.array_equal(only_d[2], got[2]) and np.array_equal(only_d[0], got[0])
    finally:
        hb.close()


def test_d_init_bar_pairs_with_a_change_of_the_initial_distribution(hank, oracle_mod):
    """the levels are exactly linear in D_0 (the policies do not read it): <D_init_bar, delta> = <g, Y(D_0 + delta) - Y(D_0)>"""
    W, base, _, _ = _random_case(33, 2)
    m, V, D, xhh, _ = cases.shape(33, 2, 6)
    hb = _block(hank, m, None)
    try:
        rng = np.random.default_rng(11)
        g = rng.standard_normal((5, 9))
        delta = D * rng.uniform(-0.5, 0.5, D.shape)
        hb.set_group_outputs(W[:, :9], base[:9])
        hb.set_boundary(V, D + delta)
        hb.primal(xhh)
        Y1 = hb.group_outputs()[0]
        hb.set_boundary(V, D)
        hb.primal(xhh)
        Y0 = hb.group_outputs()[0]
        _, none, db = hb.vjp_group(g, D_init=True)
        assert none is None and db.shape == (33, 2, 1)
        lhs, rhs = np.sum(db[:, :, 0].reshape(-1, order="F") * delta), np.sum(g * (Y1 - Y0))
        scale = np.sum(np.abs(g) * (np.abs(Y1) + np.abs(Y0)))
        print(f"<D_init_bar, delta> {lhs:.12e}, <g, dY> {rhs:.12e}, scale {scale:.3e}")
        assert abs(rhs) > 1e-4 * scale and abs(lhs - rhs) <= 1e-10 * scale
    finally:
        hb.close()


VEND_STEP = 1e-6
VEND_BOUND = 3.8e-8     # ten times the 3.801e-9 measured for hank_vjp_het_boundary (the docstring below)


def test_value_end_bar_against_a_central_difference(hank, oracle_mod):
    """<value_end_bar, dV> against the central difference of sum g Y(V_T +- h dV) along one smooth direction
    (sweep_refs.smooth_value_seeds), h = 1e-6, random weights at 33x2, K = 9. The bound is ten times the relative error the same
    central difference, with the same step, leaves against the existing hank_vjp_het_boundary's value_end_bar on the same case
    (criterion sum yb het_outputs(2)); the factor covers the different criterion.
    Measured on the MI355X: hank_vjp_het_boundary 3.801e-09 (adjoint -1.642492176909, central difference -1.642492183151), so the
    bound is 3.8e-08; hank_vjp_group 4.431e-09 (adjoint -1.596109930413, central difference -1.596109923341)."""
    W, base, _, _ = _random_case(33, 2)
    m, V, D, xhh, _ = cases.shape(33, 2, 6)
    dV = sweep_refs.smooth_value_seeds({"grid": np.asarray(m.heterogeneity["wealth"].grid), "V": V}, 1)[..., 0]
    rng = np.random.default_rng(12)
    g, yb = rng.standard_normal((5, 9)), rng.standard_normal((5, 2, 1))
    hb = _block(hank, m, None)
    try:
        hb.set_group_outputs(W[:, :9], base[:9])
        out = {}
        for sgn in (1.0, -1.0, 0.0):                                         # (the unperturbed boundary last: the adjoints' record)
            hb.set_boundary(V + sgn * VEND_STEP * dV, D)
            hb.primal(xhh)
            out[sgn] = (np.sum(g * hb.group_outputs()[0]), np.sum(yb[:, :, 0] * hb.het_outputs(2)[0]))
        fd_grp, fd_het = ((out[1.0][i] - out[-1.0][i]) / (2 * VEND_STEP) for i in (0, 1))
        vb_het = hb.vjp_het_boundary(yb, 2, D_init=False)[1]
        vb_grp = hb.vjp_group(g, value_end=True)[1]
        ad_het, ad_grp = np.sum(vb_het[:, :, 0] * dV), np.sum(vb_grp[:, :, 0] * dV)
        rel_het, rel_grp = abs(fd_het - ad_het) / abs(ad_het), abs(fd_grp - ad_grp) / abs(ad_grp)
        print(f"hank_vjp_het_boundary: adjoint {ad_het:.12e}, central difference {fd_het:.12e}, relative error {rel_het:.3e}")
        print(f"hank_vjp_group:        adjoint {ad_grp:.12e}, central difference {fd_grp:.12e}, relative error {rel_grp:.3e}")
        assert abs(ad_grp) > 1e-3 * np.sum(np.abs(vb_grp[:, :, 0] * dV))
        assert rel_grp <= VEND_BOUND
    finally:
        hb.close()


# ---- 12. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(hank, oracle_mod):
    from hank_amd.hip import HANK_ERR_BAD_ARG as BAD, HANK_ERR_NOT_READY as NOT_READY
    W, base, J, _ = _random_case(33, 2)
    m, V, D, xhh, _ = cases.shape(33, 2, 6)
    g, yb = np.random.default_rng(13).standard_normal((5, 9, 2)), np.ones((5, 1, 2))
    hb = _block(hank, m, None)
    try:
        def code(fn):
            with pytest.raises(hank.HankHIPError) as e:
                fn()
            return e.value.code
        hb.set_boundary(V, D)
        hb.set_group_outputs(W[:, :9], base[:9])
        assert code(lambda: hb.vjp_group(g)) == NOT_READY                                    # before a primal
        hb.set_group_outputs(None, None)
        hb.primal(xhh)
        assert code(lambda: hb.vjp_group(g)) == NOT_READY                                    # before any groups
        hb.set_group_outputs(W[:, :9], base[:9])
        assert code(lambda: hb.vjp_group(None, agg_bar=yb, n_het=1)) == BAD                  # grp_bar is required
        assert code(lambda: hb.vjp_group(np.zeros((5, 9, 0)))) == BAD                        # M = 0
        assert code(lambda: hb.vjp_group(g, agg_bar=np.ones((5, 3, 2)), n_het=3)) == BAD     # Value: hank_vjp_het's
        assert code(lambda: hb.vjp_group(g, agg_bar=None, n_het=1)) == BAD                   # n_het without agg_bar
        assert code(lambda: hb.vjp_group(g, agg_bar=yb, n_het=0)) == BAD
        _rows(hb.vjp_group(g), _jtg(J[:9], g), "after the refusals")                        # the context still works
        hb.set_boundary(V * 1.0001, D)                                                       # a new boundary (the same one again keeps the record)
        assert code(lambda: hb.vjp_group(g)) == NOT_READY
        hb.set_boundary(V, D)
        hb.primal(xhh)
        _rows(hb.vjp_group(g), _jtg(J[:9], g), "after a new boundary and a primal")
    finally:
        hb.close()
