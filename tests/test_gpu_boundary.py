"""hank_jvp_boundary / hank_vjp_boundary: tangents and cotangents on the boundary of the household block — the terminal marginal
value V_P (`ss_end.value`, BackwardIteration.jl:85) and the initial distribution D_0 (`ss_initial.D`, ForwardIteration.jl:293) — on
the MI355X (csrc/hank_boundary.h). The reference is always the CPU oracle's loop with duals on the boundary
(tests/sweep_refs.py, itself pinned by tests/test_boundary_host.py) or numpy; a device product is compared with another
device product only for bits. (1) the JVP against the oracle loop: dagg, dpolicy_seq, both halves of grid_aggregates,
het_outputs(2); (2) the VJP: the full transposed boundary Jacobian at 40x2, inner products everywhere else, xhh_bar's bits;
(3) bits; (4) the context's state rules and the host layers. Tolerance: the suite's rel 1e-10 + abs 1e-12 (cases.close)."""
import ctypes

import numpy as np
import pytest

import sweep_refs as bc
import cases
from cases import close as _close

pytestmark = pytest.mark.gpu

RAW = ("dense-bottom", "short-top", "both")
SHAPES = ("ks12", "ks13", "hank", "one-column", "40x16") + RAW


def _case(name):
    """-> (HouseholdBlock's arguments, V (n_a, n_e), D (G,), x (n_hh, P), oracle)"""
    if name in RAW:
        ec = cases.raw_economy(name)
        return ec["args"], ec["V"], ec["D"], ec["x"], ec["orc"]
    if name == "one-column":
        return cases.shape_one_column(64, 8)
    if name == "hank":
        m, ss, x, orc = cases.economy("hank", 2.0)
        assert x.shape[0] == 3 and np.all(x[2] != 0.0)
        return cases.model_args(m), np.asarray(ss.value), np.asarray(ss.D), x, orc
    m, V, D, x, orc = cases.shape(*{"ks12": (130, 3, 12), "ks13": (130, 3, 13), "40x16": (40, 16, 6)}[name])
    return cases.model_args(m), V, D, x, orc


def _ctx(hank, name, schedule=None):
    args, V, D, x, orc = _case(name)
    hb = cases.raw_block(hank, args, schedule)
    hb.set_boundary(V, D)
    return hb, V, D, x, orc


def _seeds(name, N, seed=0):
    """N random directions: inputs, terminal value (of the value's own scale, rough: tangents are linear), initial distribution
    (positive entries that grow with the column: it moves total mass and the productivity marginal; the clamped prefix included)"""
    _, V, D, x, _ = _case(name)
    rng = np.random.default_rng(1000 * seed + N)
    n_a, n_e = V.shape
    y = rng.standard_normal(x.shape + (N,)) * 1e-2
    dV = rng.standard_normal((n_a, n_e, N)) * np.abs(V)[:, :, None]
    dD = rng.uniform(0.0, 1.0, (n_a, n_e, N)) * (1.0 + np.arange(n_e))[None, :, None] / (n_a * n_e)
    return y, dV, dD


def _check_jvp(hb, name, y, dV, dD, what):
    """one hank_jvp_boundary and every reader of its batch against the oracle loop"""
    _, V, D, x, orc = _case(name)
    ref = bc.oracle_sweeps(orc, x, V, D, y=y, dV=dV, dD=dD)
    N = ref["dagg"].shape[2]
    dagg = hb.jvp_boundary(y, dV, dD)
    assert dagg.shape == (hb.P, N)
    assert hb.info()["last_tangent_family_name"] == "launch-per-period"
    _close(dagg, ref["dagg"][:, 0], what=what + " dagg")
    _close(hb.dpolicy_seq(N).transpose(2, 0, 1, 3), ref["dpol"], what=what + " dpolicy")
    agg2, dagg2 = hb.grid_aggregates(N)
    _close(agg2, ref["agg2"], what=what + " grid aggregate"); _close(dagg2, ref["dagg2"], what=what + " grid aggregate's partials")
    aggs, daggs = hb.het_outputs(2, np.zeros(x.shape + (N,)) if y is None else y)
    _close(aggs[:, 0], ref["agg"][:, 0], what=what + " agg"); _close(aggs[:, 1], ref["cons"], what=what + " consumption")
    _close(daggs[:, 0, :], ref["dagg"][:, 0], what=what + " het output 0"); _close(daggs[:, 1, :], ref["dcons"], what=what + " het output 1")
    return ref


MODES = {"dV": (False, True, False), "dD": (False, False, True), "dV+dD": (False, True, True), "dx+dV+dD": (True, True, True)}


# ---- 1. the JVP against the oracle loop -------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 5, 32, 33])
@pytest.mark.parametrize("name", ["ks12", "ks13"])
def test_jvp_boundary_matches_the_oracle_loop_krusell_smith_130x3(hank, oracle_mod, name, N):
    """both parities of P; one and two directions per lane, one and two blocks across the directions; every kind of seed"""
    hb, V, D, x, orc = _ctx(hank, name)
    try:
        hb.primal(x)
        y, dV, dD = _seeds(name, N)
        for mode, (wy, wv, wd) in MODES.items():
            ref = _check_jvp(hb, name, y if wy else None, dV if wv else None, dD if wd else None, f"{name} N={N} {mode}")
            assert np.abs(ref["dagg"][:, 0]).max() > 1e-6 and np.abs(ref["dcons"]).max() > 1e-6, mode
    finally:
        hb.close()


@pytest.mark.parametrize("name", ["hank", "one-column", "40x16"] + list(RAW))
def test_jvp_boundary_matches_the_oracle_loop_on_the_other_shapes(hank, oracle_mod, name):
    """three inputs with a transfer (consumption's tr_t sum m_t term); one column; sixteen columns; the raw economies, whose seeds
    on the clamped prefix travel through the virtual rows"""
    hb, V, D, x, orc = _ctx(hank, name)
    try:
        hb.primal(x)
        for N in (4, 5):
            y, dV, dD = _seeds(name, N)
            _check_jvp(hb, name, y, dV, dD, f"{name} N={N} dx+dV+dD")
            _check_jvp(hb, name, None, None, dD, f"{name} N={N} dD")
    finally:
        hb.close()


@pytest.mark.parametrize("schedule", ["launch", "xcd"])
def test_jvp_boundary_serves_a_record_of_either_writer_and_leaves_the_schedule(hank, oracle_mod, schedule):
    hb, V, D, x, orc = _ctx(hank, "ks12", schedule)
    try:
        hb.primal(x)
        want = 0 if schedule == "launch" else 1
        assert hb.stats()["schedule"] == want
        y, dV, dD = _seeds("ks12", 5, seed=1)
        _check_jvp(hb, "ks12", y, dV, dD, f"record by {schedule}")
        st = hb.stats()
        assert st["schedule"] == want and st["fallbacks"] == 0
        t = hb.last_timings()
        assert t["tangent_backward"]["launches"] == hb.P + 4 and t["tangent_forward"]["launches"] == hb.P + 5
        assert t["tangent_backward"]["ms"] > 0 and t["tangent_forward"]["ms"] > 0
        # the schedule's own hank_jvp afterwards: its family, its results
        dagg = hb.jvp(y)
        assert hb.info()["last_tangent_family_name"] == cases.FAMILY[schedule]
        _close(dagg, orc.block(x, y, V, D)[1], what="hank_jvp after hank_jvp_boundary")
    finally:
        hb.close()


# ---- 2. the VJP ---------------------------------------------------------------------------------------------------------------
def test_vjp_boundary_is_the_oracles_full_boundary_jacobian_transposed_40x2(hank, oracle_mod):
    """160 unit seeds (80 on V_P, 80 on D_0) through the oracle loop; every (output, period) cotangent through the device"""
    args, V, D, x, orc = _case40x2()
    n_a, n_e = V.shape
    G, P = n_a * n_e, x.shape[1]
    U = np.eye(G).reshape((n_a, n_e, G), order="F")
    Z = np.zeros_like(U)
    ref = bc.oracle_sweeps(orc, x, V, D, dV=np.concatenate([U, Z], axis=2), dD=np.concatenate([Z, U], axis=2))
    J = np.stack([ref["dagg"][:, 0], ref["dcons"]])                   # (output, t, seed)
    assert np.abs(J[:, :, :G]).max() > 1e-6 and np.abs(J[:, :, G:]).max() > 1e-3
    yb = np.zeros((P, 2, 2 * P))
    for o in range(2):
        for t in range(P):
            yb[t, o, o * P + t] = 1.0
    hb = cases.raw_block(hank, args, None)
    try:
        hb.set_boundary(V, D)
        hb.primal(x)
        xb, Vb, Db = hb.vjp_boundary(yb, 2)
        want = J.reshape(2 * P, 2 * G).T                        # (seed, (output, t))
        _close(Vb.reshape((G, 2 * P), order="F"), want[:G], what="value_end_bar")
        _close(Db.reshape((G, 2 * P), order="F"), want[G:], what="D_init_bar")
        assert np.array_equal(xb, hb.vjp(yb, 2))
        # the policy variable alone
        xb1, Vb1, Db1 = hb.vjp_boundary(yb[:, :1, :P], 1)
        _close(Vb1.reshape((G, P), order="F"), want[:G, :P], what="value_end_bar n_het=1")
        _close(Db1.reshape((G, P), order="F"), want[G:, :P], what="D_init_bar n_het=1")
    finally:
        hb.close()


def _case40x2():
    m, V, D, x, orc = cases.shape(40, 2, 6)
    return cases.model_args(m), V, D, x, orc


_JB = {}


def _boundary_columns(name):
    """J_b b for three boundary directions b through the oracle loop, once per shape: dV only, dD only, both"""
    if name not in _JB:
        _, V, D, x, orc = _case(name)
        _, dV, dD = _seeds(name, 3, seed=2)
        dV[:, :, 1] = 0.0; dD[:, :, 0] = 0.0
        ref = bc.oracle_sweeps(orc, x, V, D, dV=dV, dD=dD)
        _JB[name] = (dV, dD, np.stack([ref["dagg"][:, 0], ref["dcons"]]))
        assert np.all(np.abs(_JB[name][2]).max(axis=1) > 1e-6), name
    return _JB[name]


@pytest.mark.parametrize("name", SHAPES)
def test_vjp_boundary_pairs_with_the_oracles_boundary_columns(hank, oracle_mod, name):
    """<ybar, J_b b>_oracle = <J_b' ybar, b>_device at n_het = 1, 2 and M = 1, 4, 32, 33; xhh_bar is hank_vjp's bit for bit"""
    dV, dD, Jb = _boundary_columns(name)
    hb, V, D, x, orc = _ctx(hank, name)
    try:
        hb.primal(x)
        for M in (1, 4, 32, 33):
            for n_het in (1, 2):
                yb = np.random.default_rng(10 * M + n_het).standard_normal((hb.P, n_het, M))
                xb, Vb, Db = hb.vjp_boundary(yb, n_het)
                lhs = np.einsum("tom,otk->mk", yb, Jb[:n_het])
                rhs = np.einsum("aem,aek->mk", Vb, dV) + np.einsum("aem,aek->mk", Db, dD)
                _close(rhs, lhs, what=f"{name} M={M} n_het={n_het} pairing")
                assert np.array_equal(xb, hb.vjp(yb, n_het)), (name, M, n_het)
    finally:
        hb.close()


# ---- 3. bits ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 5, 32])
def test_zero_or_null_seeds_give_hank_jvps_bits_and_a_repeat_gives_the_same(hank, oracle_mod, N):
    hb, V, D, x, orc = _ctx(hank, "ks13", "launch")
    try:
        hb.primal(x)
        y, dV, dD = _seeds("ks13", N)
        dagg = hb.jvp(y)
        dpol = hb.dpolicy_seq(N)
        for zv, zd in ((None, None), (0 * dV, None), (None, 0 * dD), (0 * dV, 0 * dD)):
            assert np.array_equal(hb.jvp_boundary(y, zv, zd), dagg)
            assert np.array_equal(hb.dpolicy_seq(N), dpol)
        a = hb.jvp_boundary(y, dV, dD)
        pa, ha = hb.dpolicy_seq(N), hb.het_outputs(2, y)[1]
        assert not np.array_equal(a, dagg)
        assert np.array_equal(hb.jvp_boundary(y, dV, dD), a) and np.array_equal(hb.dpolicy_seq(N), pa) and np.array_equal(hb.het_outputs(2, y)[1], ha)
        yb = np.random.default_rng(N).standard_normal((hb.P, 2, N))
        first, second = hb.vjp_boundary(yb, 2), hb.vjp_boundary(yb, 2)
        assert all(np.array_equal(u, v) for u, v in zip(first, second))
    finally:
        hb.close()


# ---- 4. state rules and host layers ---------------------------------------------------------------------------------------------
def test_boundary_entries_need_a_record(hank, oracle_mod):
    hb, V, D, x, orc = _ctx(hank, "ks12")
    try:
        y, dV, dD = _seeds("ks12", 2)
        yb = np.ones((hb.P, 1, 2))
        for call in (lambda: hb.jvp_boundary(y, dV, dD), lambda: hb.vjp_boundary(yb, 1)):
            with pytest.raises(hank.HankHIPError) as ei:
                call()
            assert ei.value.code == hank.hip.HANK_ERR_NOT_READY
        hb.primal(x)
        hb.jvp_boundary(y, dV, dD); hb.vjp_boundary(yb, 1)
        hb.set_boundary(V * 1.01, D)
        for call in (lambda: hb.jvp_boundary(y, dV, dD), lambda: hb.vjp_boundary(yb, 1), lambda: hb.dpolicy_seq(2)):
            with pytest.raises(hank.HankHIPError) as ei:
                call()
            assert ei.value.code == hank.hip.HANK_ERR_NOT_READY
        # bad arguments: no seed at all; Value's cotangent
        out = np.empty((hb.P, 2), order="F")
        hb.primal(x)
        assert hb._lib.hank_jvp_boundary(hb._ctx, None, None, None, 2, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == hank.hip.HANK_ERR_BAD_ARG
        with pytest.raises(ValueError):
            hb.jvp_boundary()
        with pytest.raises(hank.HankHIPError) as ei:
            hb.vjp_boundary(np.ones((hb.P, 3, 2)), 3)
        assert ei.value.code == hank.hip.HANK_ERR_BAD_ARG
    finally:
        hb.close()


def test_value_tangents_are_refused_at_a_boundary_batch_and_served_again_after_hank_jvp(hank, oracle_mod):
    args, V, D, x, orc = _case("ks12")
    hb, *_ = _ctx(hank, "ks12")
    try:
        hb.set_het_outputs(3)
        hb.primal(x)
        y, dV, dD = _seeds("ks12", 3)
        hb.jvp_boundary(y, dV, dD)
        with pytest.raises(hank.HankHIPError, match="boundary seeds") as ei:
            hb.het_outputs(3, y)
        assert ei.value.code == hank.hip.HANK_ERR_NOT_READY
        agg3, _ = hb.het_outputs(3)                              # the values carry no tangent: served
        ref_agg, ref_dagg = orc.het_outputs(x, y, V, D, 3, args[4])
        _close(agg3, ref_agg.T, what="values of three outputs at a boundary batch")
        hb.het_outputs(2, y)
        hb.jvp(y)
        _close(hb.het_outputs(3, y)[1], ref_dagg.transpose(1, 0, 2), what="three outputs' tangents after hank_jvp")
    finally:
        hb.close()


def test_the_tangent_batch_survives_vjp_boundary_and_the_device_pointer_forms_agree(hank, oracle_mod):
    import torch
    hb, V, D, x, orc = _ctx(hank, "ks13")
    try:
        hb.primal(x)
        N = 4
        y, dV, dD = _seeds("ks13", N)
        dagg = hb.jvp_boundary(y, dV, dD)
        dpol, het = hb.dpolicy_seq(N), hb.het_outputs(2, y)[1]
        yb = np.random.default_rng(3).standard_normal((hb.P, 2, N))
        xb, Vb, Db = hb.vjp_boundary(yb, 2)
        assert np.array_equal(hb.dpolicy_seq(N), dpol) and np.array_equal(hb.het_outputs(2, y)[1], het)
        assert hb.policy_cotangent_seq(N).shape == (hb.n_a, hb.n_e, hb.P, N)
        t = hb.last_vjp_timings()
        assert t["sweep_a"]["launches"] == hb.P and t["sweep_b"]["launches"] == hb.P + 4 and t["sweep_b"]["ms"] > 0

        def dev(arr):
            return torch.from_numpy(np.asfortranarray(arr).reshape(-1, order="F").copy()).cuda()
        d_y, d_dV, d_dD, d_yb = dev(y), dev(dV), dev(dD), dev(yb)
        d_out = torch.empty(hb.P * N, dtype=torch.float64, device="cuda")
        d_xb = torch.empty(hb.n_hh * hb.P * N, dtype=torch.float64, device="cuda")
        d_Vb, d_Db = (torch.empty(hb.G * N, dtype=torch.float64, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        hb.jvp_boundary_dev(d_y.data_ptr(), d_dV.data_ptr(), d_dD.data_ptr(), N, d_out.data_ptr())
        hb.sync()
        assert np.array_equal(d_out.cpu().numpy().reshape((hb.P, N), order="F"), dagg)
        hb.jvp_boundary_dev(0, d_dV.data_ptr(), 0, N, d_out.data_ptr())
        hb.sync()
        assert np.array_equal(d_out.cpu().numpy().reshape((hb.P, N), order="F"), hb.jvp_boundary(None, dV, None))
        hb.vjp_boundary_dev(2, d_yb.data_ptr(), N, d_xb.data_ptr(), d_Vb.data_ptr(), d_Db.data_ptr())
        hb.sync()
        assert np.array_equal(d_xb.cpu().numpy().reshape(xb.shape, order="F"), xb)
        assert np.array_equal(d_Vb.cpu().numpy().reshape(Vb.shape, order="F"), Vb) and np.array_equal(d_Db.cpu().numpy().reshape(Db.shape, order="F"), Db)
        d_Vb.zero_()
        torch.cuda.synchronize()
        hb.vjp_boundary_dev(2, d_yb.data_ptr(), N, d_xb.data_ptr(), 0, d_Db.data_ptr())      # a boundary output that is not wanted
        hb.sync()
        assert not d_Vb.cpu().numpy().any() and np.array_equal(d_Db.cpu().numpy().reshape(Db.shape, order="F"), Db)
    finally:
        hb.close()
