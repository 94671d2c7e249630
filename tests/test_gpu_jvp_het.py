"""hank_jvp_het / hank_vjp_het_boundary on the MI355X: every declared output's tangent from one pair of sweeps with seeds on the
inputs, on the terminal marginal value V_P (`ss_end.value`, BackwardIteration.jl:85) and on the initial distribution D_0
(`ss_initial.D`, ForwardIteration.jl:293) — Value and UCE ride in the forward launches (k_tan_fwd_hx) — and
the transpose with the boundary's cotangents. The reference is always the CPU oracle's loop with duals on the boundary
(tests/sweep_refs.py, pinned by tests/test_jvp_het_host.py) or numpy; a device product is compared with another device
product only for bits. (1) against the oracle loop; (2) edges; (3) records; (4) bits; (5) the transposed entry; (6) state rules;
(7) host layers. Tolerance: the suite's rel 1e-10 + abs 1e-12 (cases.close)."""
import ctypes

import numpy as np
import pytest

import cases
import sweep_refs as hbc
from cases import close as _close

pytestmark = pytest.mark.gpu

RAW = ("dense-bottom", "short-top", "both")


def _case(name):
    """-> (HouseholdBlock's arguments, V (n_a, n_e), D (G,), x (n_hh, P), oracle, the family's count of outputs)"""
    if name in RAW:
        ec = cases.raw_economy(name)
        return ec["args"], ec["V"], ec["D"], ec["x"], ec["orc"], 3
    if name == "one-column":
        return cases.shape_one_column(64, 8) + (3,)
    if name in ("hank", "gamma1.5"):
        m, ss, x, orc = cases.economy("hank", 2.0) if name == "hank" else cases.economy("ks", 1.5)
        if name == "hank":
            assert x.shape[0] == 3 and np.all(x[2] != 0.0)
            x = np.ascontiguousarray(x[:, :12])
            args = cases.model_args(m)
            return args[:6] + (13,) + args[7:], np.asarray(ss.value), np.asarray(ss.D), x, orc, 4
        x = np.ascontiguousarray(x[:, :9])
        args = cases.model_args(m)
        return args[:6] + (10,) + args[7:], np.asarray(ss.value), np.asarray(ss.D), x, orc, 3
    m, V, D, x, orc = cases.shape(*{"ks12": (130, 3, 12), "ks13": (130, 3, 13), "40x16": (40, 16, 6), "40x2": (40, 2, 6)}[name])
    return cases.model_args(m), V, D, x, orc, 3


def _ctx(hank, name, schedule=None, declare=True):
    args, V, D, x, orc, n_het = _case(name)
    hb = cases.raw_block(hank, args, schedule)
    hb.set_boundary(V, D)
    if declare:
        hb.set_het_outputs(n_het)
    return hb, V, D, x, orc, n_het


def _seeds(name, N, seed=0):
    """N random directions, as tests/test_gpu_boundary.py draws them: inputs, terminal value (of the value's own scale), initial
    distribution (positive entries that grow with the column: it moves total mass and the productivity marginal)"""
    _, V, D, x, _, _ = _case(name)
    rng = np.random.default_rng(1000 * seed + N)
    n_a, n_e = V.shape
    y = rng.standard_normal(x.shape + (N,)) * 1e-2
    dV = rng.standard_normal((n_a, n_e, N)) * np.abs(V)[:, :, None]
    dD = rng.uniform(0.0, 1.0, (n_a, n_e, N)) * (1.0 + np.arange(n_e))[None, :, None] / (n_a * n_e)
    return y, dV, dD


_REF = {}


def _ref(name, N, mode, seed=0):
    """the oracle loop of one (shape, width, mode), once per session"""
    key = (name, N, mode, seed)
    if key not in _REF:
        args, V, D, x, orc, n_het = _case(name)
        y, dV, dD = _seeds(name, N, seed)
        wy, wv, wd = MODES[mode]
        _REF[key] = hbc.oracle_sweeps(orc, x, V, D, args[4], n_het, y=y if wy else None, dV=dV if wv else None, dD=dD if wd else None)
    return _REF[key]


MODES = {"dx": (True, False, False), "dV": (False, True, False), "dD": (False, False, True), "dx+dV+dD": (True, True, True)}


def _check(hb, name, N, mode, what, seed=0):
    """one hank_jvp_het and every reader of its batch against the oracle loop"""
    n_het = _case(name)[5]
    ref = _ref(name, N, mode, seed)
    y, dV, dD = _seeds(name, N, seed)
    wy, wv, wd = MODES[mode]
    got = hb.jvp_het(y if wy else None, dV if wv else None, dD if wd else None, n_het=n_het)
    assert got.shape == (hb.P, n_het, N)
    assert hb.info()["last_tangent_family_name"] == "launch-per-period"
    for o in range(n_het):
        _close(got[:, o, :], ref["dagg"][:, o, :], what=f"{what} {mode} output {o}")
    _close(hb.dpolicy_seq(N).transpose(2, 0, 1, 3), ref["dpol"], what=f"{what} {mode} dpolicy")
    agg2, dagg2 = hb.grid_aggregates(N)
    _close(agg2, ref["agg2"], what=f"{what} {mode} grid aggregate"); _close(dagg2, ref["dagg2"], what=f"{what} {mode} grid aggregate's partials")
    return ref, got


# ---- 1. against the oracle loop -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 5, 16, 18, 33, 65])
@pytest.mark.parametrize("name", ["ks12", "ks13", "hank"])
def test_jvp_het_matches_the_oracle_loop(hank, oracle_mod, name, N):
    """Krusell-Smith 130x3 with Value at both parities of P, the one-asset HANK 80x3 with Value and UCE and a transfer; one and two
    directions per lane, the gather form (N <= 16) and the source-stationary form with two row groups, one wave per row, two blocks
    across the directions; every kind of seed, and the extra outputs move under each"""
    hb, V, D, x, orc, n_het = _ctx(hank, name)
    try:
        hb.primal(x)
        for mode in MODES:
            ref, _ = _check(hb, name, N, mode, f"{name} N={N}")
            for o in range(2, n_het):
                assert np.abs(ref["dagg"][:, o, :]).max() > 1e-6, (mode, o)
    finally:
        hb.close()


# ---- 2. edges -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one-column", "40x16", "gamma1.5"] + list(RAW))
def test_jvp_het_matches_the_oracle_loop_on_the_edges(hank, oracle_mod, name):
    """one column; sixteen columns; gamma = 1.5 (pow in f and f_c); the raw economies: seeds on the clamped prefix, the virtual rows'
    f of row 0, the clamped sources' f_c term, a mass point that vanishes and returns"""
    hb, V, D, x, orc, n_het = _ctx(hank, name)
    try:
        hb.primal(x)
        for N in (4, 5, 18):
            ref, _ = _check(hb, name, N, "dx+dV+dD", f"{name} N={N}")
            assert np.abs(ref["dagg"][:, 2, :]).max() > 1e-6
            _check(hb, name, N, "dD", f"{name} N={N}")
    finally:
        hb.close()


# ---- 3. records -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", ["launch", "xcd"])
def test_jvp_het_serves_a_record_of_either_writer_and_leaves_the_schedule(hank, oracle_mod, schedule):
    hb, V, D, x, orc, n_het = _ctx(hank, "ks12", schedule)
    try:
        hb.primal(x)
        want = 0 if schedule == "launch" else 1
        assert hb.stats()["schedule"] == want
        _check(hb, "ks12", 5, "dx+dV+dD", f"record by {schedule}", seed=1)
        st = hb.stats()
        assert st["schedule"] == want and st["fallbacks"] == 0
        t = hb.last_timings()
        assert t["tangent_backward"]["launches"] == hb.P + 4 and t["tangent_forward"]["launches"] == hb.P + 6
        assert t["tangent_backward"]["ms"] > 0 and t["tangent_forward"]["ms"] > 0
        _check(hb, "ks12", 5, "dx", f"record by {schedule}", seed=1)
        t = hb.last_timings()
        assert t["tangent_backward"]["launches"] == hb.P + 2 and t["tangent_forward"]["launches"] == hb.P + 4
        y = _seeds("ks12", 5, seed=1)[0]
        hb.jvp_het(y, n_het=2)
        assert hb.last_timings()["tangent_forward"]["launches"] == hb.P + 3
        # the schedule's own hank_jvp afterwards: its family, its results
        dagg = hb.jvp(y)
        assert hb.info()["last_tangent_family_name"] == cases.FAMILY[schedule]
        _close(dagg, orc.block(x, y, V, D)[1], what="hank_jvp after hank_jvp_het")
    finally:
        hb.close()


# ---- 4. bits --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 5, 18, 32])
def test_jvp_het_bits(hank, oracle_mod, N):
    """n_het <= 2 is hank_jvp / hank_jvp_boundary under the launch schedule; at n_het = 3 everything but output 2 is the n_het = 2
    call's (the added sums touch none of those operands); a repeat gives the same bits"""
    hb, V, D, x, orc, n_het = _ctx(hank, "ks13", "launch")
    try:
        hb.primal(x)
        y, dV, dD = _seeds("ks13", N)
        for sv, sd in ((None, None), (dV, dD)):
            d1 = hb.jvp(y) if sv is None else hb.jvp_boundary(y, sv, sd)
            d2 = hb.het_outputs(2, y)[1]
            dpol, (_, dg2) = hb.dpolicy_seq(N), hb.grid_aggregates(N)
            assert np.array_equal(hb.jvp_het(y, sv, sd, n_het=1)[:, 0, :], d1)
            assert np.array_equal(hb.jvp_het(y, sv, sd, n_het=2), d2) and np.array_equal(d2[:, 0, :], d1)
            assert np.array_equal(hb.dpolicy_seq(N), dpol) and np.array_equal(hb.grid_aggregates(N)[1], dg2)
            a = hb.jvp_het(y, sv, sd, n_het=3)
            assert np.array_equal(a[:, :2, :], d2) and np.abs(a[:, 2, :]).max() > 0
            assert np.array_equal(hb.dpolicy_seq(N), dpol) and np.array_equal(hb.grid_aggregates(N)[1], dg2)
            assert np.array_equal(hb.jvp_het(y, sv, sd, n_het=3), a)
    finally:
        hb.close()


@pytest.mark.parametrize("N", [2, 18])
def test_order_of_first_use_does_not_matter(hank, oracle_mod, N):
    """every variant of the launch family's tangent entries at one width, first used in one order on one context and in the reverse
    order on another: the same bits from every call and the same policy partials behind it, and the same count of captured graphs
    — the two pairs (without and with seeds) and the two forward graphs with extra reductions that were asked for. A graph slot
    picked wrongly, or a graph captured before a buffer it names was allocated, shows here. N = 2: two directions per lane, the
    gather form, one row group; N = 18: the source-stationary form, two row groups (the geometries k_tan_fwd_hx exists for)."""
    y, dV, dD = _seeds("hank", N)
    calls = [lambda hb: hb.jvp(y), lambda hb: hb.jvp_boundary(y, dV, dD), lambda hb: hb.jvp_boundary(y), lambda hb: hb.jvp_het(y, n_het=2),
             lambda hb: hb.jvp_het(y, dV, dD, n_het=2), lambda hb: hb.jvp_het(y, n_het=3), lambda hb: hb.jvp_het(y, dV, dD, n_het=4)]

    def run(order):
        hb, V, D, x, orc, n_het = _ctx(hank, "hank", "launch")
        try:
            assert n_het == 4
            hb.primal(x)
            before = hb.stats()["graphs_captured"]
            got = {}
            for k in order:
                got[k] = (calls[k](hb), hb.dpolicy_seq(N))
                assert hb.info()["last_tangent_family_name"] == "launch-per-period"
            return got, hb.stats()["graphs_captured"] - before
        finally:
            hb.close()
    a, captured_a = run(range(len(calls)))
    b, captured_b = run(reversed(range(len(calls))))
    for k in range(len(calls)):
        assert np.array_equal(a[k][0], b[k][0]), f"call {k}"
        assert np.array_equal(a[k][1], b[k][1]), f"dpolicy_seq after call {k}"
    assert np.abs(a[6][0][:, 2:, :]).max() > 0
    assert captured_a == captured_b == 6


def test_the_device_pointer_forms_agree_and_the_tangent_batch_survives_vjp_het_boundary(hank, oracle_mod):
    import torch
    hb, V, D, x, orc, n_het = _ctx(hank, "ks13")
    try:
        hb.primal(x)
        N = 4
        y, dV, dD = _seeds("ks13", N)
        a = hb.jvp_het(y, dV, dD, n_het=3)
        dpol = hb.dpolicy_seq(N)
        yb = np.random.default_rng(3).standard_normal((hb.P, 3, N))
        xb, Vb, Db = hb.vjp_het_boundary(yb, 3)
        assert np.array_equal(hb.dpolicy_seq(N), dpol) and np.array_equal(hb.het_outputs(2, y)[1], a[:, :2, :])
        assert np.array_equal(xb, hb.vjp_het(yb, 3))
        second = hb.vjp_het_boundary(yb, 3)
        assert np.array_equal(second[0], xb) and np.array_equal(second[1], Vb) and np.array_equal(second[2], Db)
        only_D = hb.vjp_het_boundary(yb, 3, value_end=False)
        assert only_D[1] is None and np.array_equal(only_D[2], Db)

        def dev(arr):
            return torch.from_numpy(np.asfortranarray(arr).reshape(-1, order="F").copy()).cuda()
        d_y, d_dV, d_dD, d_yb = dev(y), dev(dV), dev(dD), dev(yb)
        d_out = torch.empty(hb.P * 3 * N, dtype=torch.float64, device="cuda")
        d_xb = torch.empty(hb.n_hh * hb.P * N, dtype=torch.float64, device="cuda")
        d_Vb, d_Db = (torch.empty(hb.G * N, dtype=torch.float64, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        hb.jvp_het_dev(3, d_y.data_ptr(), d_dV.data_ptr(), d_dD.data_ptr(), N, d_out.data_ptr())
        hb.sync()
        assert np.array_equal(d_out.cpu().numpy().reshape((hb.P, 3, N), order="F"), a)
        hb.jvp_het_dev(3, 0, d_dV.data_ptr(), 0, N, d_out.data_ptr())
        hb.sync()
        assert np.array_equal(d_out.cpu().numpy().reshape((hb.P, 3, N), order="F"), hb.jvp_het(None, dV, None, n_het=3))
        hb.vjp_het_boundary_dev(3, d_yb.data_ptr(), N, d_xb.data_ptr(), d_Vb.data_ptr(), d_Db.data_ptr())
        hb.sync()
        assert np.array_equal(d_xb.cpu().numpy().reshape(xb.shape, order="F"), xb)
        assert np.array_equal(d_Vb.cpu().numpy().reshape(Vb.shape, order="F"), Vb) and np.array_equal(d_Db.cpu().numpy().reshape(Db.shape, order="F"), Db)
        d_Vb.zero_()
        torch.cuda.synchronize()
        hb.vjp_het_boundary_dev(3, d_yb.data_ptr(), N, d_xb.data_ptr(), 0, d_Db.data_ptr())      # a boundary output that is not wanted
        hb.sync()
        assert not d_Vb.cpu().numpy().any() and np.array_equal(d_Db.cpu().numpy().reshape(Db.shape, order="F"), Db)
    finally:
        hb.close()


# ---- 5. the transposed entry ------------------------------------------------------------------------------------------------------
def test_vjp_het_boundary_is_the_oracles_full_boundary_jacobian_transposed_40x2(hank, oracle_mod):
    """160 unit seeds (80 on V_P, 80 on D_0) through the oracle loop; every (output, period) cotangent of three outputs"""
    args, V, D, x, orc, n_het = _case("40x2")
    n_a, n_e = V.shape
    G, P = n_a * n_e, x.shape[1]
    U = np.eye(G).reshape((n_a, n_e, G), order="F")
    Z = np.zeros_like(U)
    ref = hbc.oracle_sweeps(orc, x, V, D, args[4], 3, dV=np.concatenate([U, Z], axis=2), dD=np.concatenate([Z, U], axis=2))
    J = ref["dagg"].transpose(1, 0, 2)                          # (output, t, seed)
    assert np.abs(J[2, :, :G]).max() > 1e-6 and np.abs(J[2, :, G:]).max() > 1e-3
    yb = np.zeros((P, 3, 3 * P))
    for o in range(3):
        for t in range(P):
            yb[t, o, o * P + t] = 1.0
    hb, *_ = _ctx(hank, "40x2")
    try:
        hb.primal(x)
        xb, Vb, Db = hb.vjp_het_boundary(yb, 3)
        want = J.reshape(3 * P, 2 * G).T                        # (seed, (output, t))
        _close(Vb.reshape((G, 3 * P), order="F"), want[:G], what="value_end_bar")
        _close(Db.reshape((G, 3 * P), order="F"), want[G:], what="D_init_bar")
        assert np.array_equal(xb, hb.vjp_het(yb, 3))
    finally:
        hb.close()


@pytest.mark.parametrize("name", ["ks13", "hank", "40x16", "one-column", "both"])
def test_vjp_het_boundary_pairs_with_the_oracle_loop(hank, oracle_mod, name):
    """<ybar, J (y, dV, dD)>_oracle = <xbar, y> + <Vbar, dV> + <Dbar, dD> on the device, for three directions and M = 1, 4, 32, 33
    cotangent columns on every output; xhh_bar is hank_vjp_het's bit for bit"""
    ref = _ref(name, 3, "dx+dV+dD", seed=2)
    y, dV, dD = _seeds(name, 3, seed=2)
    hb, V, D, x, orc, n_het = _ctx(hank, name)
    try:
        hb.primal(x)
        for M in (1, 4, 32, 33):
            yb = np.random.default_rng(10 * M + n_het).standard_normal((hb.P, n_het, M))
            xb, Vb, Db = hb.vjp_het_boundary(yb, n_het)
            lhs = np.einsum("tom,tok->mk", yb, ref["dagg"])
            rhs = np.einsum("itm,itk->mk", xb, y) + np.einsum("aem,aek->mk", Vb, dV) + np.einsum("aem,aek->mk", Db, dD)
            _close(rhs, lhs, what=f"{name} M={M} pairing")
            assert np.array_equal(xb, hb.vjp_het(yb, n_het)), (name, M)
    finally:
        hb.close()


# ---- 6. state rules ---------------------------------------------------------------------------------------------------------------
def test_jvp_het_state_rules(hank, oracle_mod):
    args, V, D, x, orc, _ = _case("ks12")
    hb, *_ = _ctx(hank, "ks12", declare=False)
    NOT_READY, BAD_ARG = hank.hip.HANK_ERR_NOT_READY, hank.hip.HANK_ERR_BAD_ARG

    def code(call):
        with pytest.raises(hank.HankHIPError) as ei:
            call()
        return ei.value.code
    try:
        N = 3
        y, dV, dD = _seeds("ks12", N)
        yb = np.ones((hb.P, 2, N))
        # no record
        assert code(lambda: hb.jvp_het(y, dV, dD, n_het=2)) == NOT_READY and code(lambda: hb.vjp_het_boundary(yb, 2)) == NOT_READY
        hb.primal(x)
        # above the family's count; above the declared count
        assert code(lambda: hb.jvp_het(y, n_het=4)) == BAD_ARG and code(lambda: hb.vjp_het_boundary(np.ones((hb.P, 4, N)), 4)) == BAD_ARG
        assert code(lambda: hb.jvp_het(y, n_het=3)) == NOT_READY and code(lambda: hb.vjp_het_boundary(np.ones((hb.P, 3, N)), 3)) == NOT_READY
        hb.set_het_outputs(3)
        # all inputs NULL
        out = np.empty((hb.P, 3, N), order="F")
        assert hb._lib.hank_jvp_het(hb._ctx, 3, None, None, None, N, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == BAD_ARG
        with pytest.raises(ValueError):
            hb.jvp_het(n_het=3)
        # a seeded batch: hank_get_het_outputs keeps refusing n_het > 2, as after hank_jvp_boundary
        seeded = hb.jvp_het(y, dV, dD, n_het=3)
        with pytest.raises(hank.HankHIPError, match="boundary seeds") as ei:
            hb.het_outputs(3, y)
        assert ei.value.code == NOT_READY
        assert np.array_equal(hb.het_outputs(2, y)[1], seeded[:, :2, :])
        # an unseeded one: it serves, and both answers meet the oracle
        mine = hb.jvp_het(y, n_het=3)
        ref_dagg = orc.het_outputs(x, y, V, D, 3, args[4])[1].transpose(1, 0, 2)
        theirs = hb.het_outputs(3, y)[1]
        _close(mine, ref_dagg, what="unseeded hank_jvp_het"); _close(theirs, ref_dagg, what="hank_get_het_outputs at its batch")
        assert np.array_equal(mine[:, :2, :], theirs[:, :2, :])
        # the tangent batch survives hank_vjp_het_boundary
        dpol = hb.dpolicy_seq(N)
        hb.vjp_het_boundary(np.ones((hb.P, 3, N)), 3)
        assert np.array_equal(hb.dpolicy_seq(N), dpol)
        # a new primal or a new boundary leaves nothing current
        hb.primal(x * 1.001)
        assert code(lambda: hb.dpolicy_seq(N)) == NOT_READY
        hb.jvp_het(y, dV, dD, n_het=3)
        hb.set_boundary(V * 1.01, D)
        assert code(lambda: hb.dpolicy_seq(N)) == NOT_READY and code(lambda: hb.jvp_het(y, n_het=3)) == NOT_READY
    finally:
        hb.close()


# ---- 7. host layers ---------------------------------------------------------------------------------------------------------------
def _wages_lin(hank):
    from examples.solve_hank import build
    m, ss = build(80, 3, 13, "one_asset_hank_wages.yaml")
    P = m.compspec.T - 1
    keys = hank.vars_of_type(m, "endogenous")
    x0 = np.tile(np.array([ss.vars[k] for k in keys]), P) * (1 + 1e-4 * np.random.default_rng(0).standard_normal(len(keys) * P))
    lin = hank.LinearizedFunction(x0, {"ei": 0.0025 * 0.6 ** np.arange(P)}, m, ss, ss)
    assert lin._n_out == 4
    return lin, m


def test_linearized_function_het_in_sweep_and_boundary_products_sticky_wage_hank(hank, oracle_mod):
    lin, m = _wages_lin(hank)
    n = lin.x.size
    rng = np.random.default_rng(5)
    y = rng.standard_normal((n, 3)) * 1e-3
    assert hank.LinearizedFunction.het_in_sweep is False
    default = lin.jvp(y)
    lin.het_in_sweep = True
    try:
        _close(lin.jvp(y), default, what="het_in_sweep against the default path")
        _close(lin.jvp(y[:, 0]), default[:, 0], what="het_in_sweep, one direction")
    finally:
        lin.het_in_sweep = False
    # vjp_boundary is the transpose of jvp_boundary
    hb = lin.hb
    K, M = 3, 4
    dV = rng.standard_normal((hb.n_a, hb.n_e, K)) * np.abs(np.asarray(lin.ss_ending.value))[:, :, None]
    dD = rng.uniform(0.0, 1.0, (hb.n_a, hb.n_e, K)) / hb.G
    Jb = lin.jvp_boundary(dV, dD)
    assert Jb.shape == (len(lin.Fx), K) and np.abs(Jb).max() > 1e-6
    _close(lin.jvp_boundary(dV[:, :, 0], dD[:, :, 0]), Jb[:, 0], what="one boundary direction")
    _close(lin.jvp_boundary(dV, None) + lin.jvp_boundary(None, dD), Jb, what="superposition")
    yb = rng.standard_normal((len(lin.Fx), M))
    Vb, Db = lin.vjp_boundary(yb)
    assert Vb.shape == (hb.n_a, hb.n_e, M)
    _close(np.einsum("aem,aek->mk", Vb, dV) + np.einsum("aem,aek->mk", Db, dD), yb.T @ Jb, what="vjp_boundary is jvp_boundary's transpose")


def test_device_group_forms_on_two_contexts_of_one_gpu(hank, oracle_mod):
    from hank_amd.parallel import DeviceGroup
    hb, V, D, x, orc, n_het = _ctx(hank, "ks12")
    grp = DeviceGroup(hb, [0, 0])
    try:
        for b in grp.blocks[1:]:
            b.set_het_outputs(3)
        grp.primal(x)
        y, dV, dD = _seeds("ks12", 5)
        got = grp.jvp_het(y, dV, dD, n_het=3)
        assert got.shape == (hb.P, 3, 5) and np.array_equal(got[:, :, :3], hb.jvp_het(y[:, :, :3], dV[:, :, :3], dD[:, :, :3], n_het=3))
        _close(got, _ref("ks12", 5, "dx+dV+dD")["dagg"], what="DeviceGroup.jvp_het")
        assert grp.jvp_het(None, dV[:, :, :1], None, n_het=3).shape == (hb.P, 3, 1)          # fewer columns than contexts
        yb = np.random.default_rng(1).standard_normal((hb.P, 3, 5))
        xb, Vb, Db = grp.vjp_het_boundary(yb, 3)
        one = hb.vjp_het_boundary(yb[:, :, :3], 3)
        assert xb.shape == (hb.n_hh, hb.P, 5) and all(np.array_equal(u[:, :, :3], v) for u, v in zip((xb, Vb, Db), one))
    finally:
        grp.close()
        hb.close()


def test_abi_lists_the_four_entries(hank):
    import hank_amd
    names = {"hank_jvp_het", "hank_jvp_het_dev", "hank_vjp_het_boundary", "hank_vjp_het_boundary_dev"}
    assert names <= set(hank_amd.hip.ABI_SYMBOLS)
    lib = ctypes.CDLL(str(hank_amd.hip.library_path()))
    for name in names:
        assert getattr(lib, name) is not None
    for attr in ("jvp_het", "jvp_het_dev", "vjp_het_boundary", "vjp_het_boundary_dev"):
        assert hasattr(hank_amd.hip.HouseholdBlock, attr)
