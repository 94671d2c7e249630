"""Group outputs on the device (hank_set_group_outputs, hank_get_group_outputs[_dev], hank_fake_news_group): aggregates of
caller-supplied weight arrays W_k over the grid, Y^k_t = sum W_k f D_t with f = 1, a'_t or c_t, dotted with the same post-transition
D_t as every heterogeneous variable (ForwardIteration.jl:303-307), their tangents and their Toeplitz Jacobian. The reference is
tests/group_refs.py: the oracle's BackwardIteration, its consumption policy and orc_forward_iteration_het on the weighted
sequences. Tolerance: cases.close (rel 1e-10 + abs 1e-12 on the reference's largest entry), applied per output."""
import numpy as np
import pytest

import cases
import group_refs as gr
from cases import block as _block, close as _close, hank_economy, hank_x as _hank_x, raw_block
from conftest import ks_paths, ks_setup

pytestmark = pytest.mark.gpu

GOODS = "one_asset_hank_goods.yaml"


def _per_output(agg, dagg, oagg, odagg, what):
    """agg (P, K), dagg (P, K, N) of the device against oagg (K, P), odagg (K, P, N) of the reference, output by output"""
    assert agg.shape == oagg.T.shape and dagg.shape == (oagg.shape[1], oagg.shape[0], odagg.shape[2]), (what, agg.shape, dagg.shape)
    for k in range(oagg.shape[0]):
        _close(agg[:, k], oagg[k], what=f"{what} output {k} value")
        _close(dagg[:, k, :], odagg[k], what=f"{what} output {k} tangent")


# ---- 1. parity with the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule,family,N", [("launch", "launch-per-period", 5), ("xcd", "xcd-persistent", 5), ("xcd", "xcd-persistent", 40),
                                               ("wide", "on-chip-wide", 5), ("launch", "launch-per-period", 33)])
def test_parity_with_the_oracle_krusell_smith_130x3(hank, schedule, family, N):
    """the twelve outputs (four wealth groups, every base) through both entry paths, whichever kernel family ran the sweep"""
    xhh, y, W, base, oagg, odagg = gr.ks_reference(N)
    gr.nontrivial(oagg, odagg, "ks130")
    m, ss, _ = ks_setup(130, 3, 40)
    hb = _block(hank, m, schedule)
    hb.set_boundary(ss.value, ss.D)
    hb.set_group_outputs(W, base)
    for entry in ("primal_jvp", "primal, jvp"):
        hb.primal(xhh * 1.01)                   # (a record of another x: no memo hit, every sweep runs)
        if entry == "primal_jvp":
            hb.primal_jvp(xhh, y)
        else:
            hb.primal(xhh)
            hb.jvp(y)
        assert hb.info()["last_tangent_family_name"] == family, entry
        agg, dagg = hb.group_outputs(y)
        _per_output(agg, dagg, oagg, odagg, f"{schedule} N={N} {entry}")
        a2, d2 = hb.group_outputs(y)            # asked again: the same bits (fixed summation order, no atomics)
        assert np.array_equal(a2, agg) and np.array_equal(d2, dagg), entry
        a0, none = hb.group_outputs()           # values only
        assert none is None and np.array_equal(a0, agg)
    assert hb.stats()["fallbacks"] == 0
    hb.close()


# ---- 2. random weights --------------------------------------------------------------------------------------------------------
_RANDOM = {}


def _random_case(n_a, n_e):
    """standard-normal weights (G, 32) with the bases cycling MASS, POLICY, CONS, and the reference of all 32 at N = 3, once per
    shape: a call with K groups uses the first K columns, a call with N directions the first N."""
    key = (n_a, n_e)
    if key not in _RANDOM:
        m, V, D, xhh, orc = cases.shape(n_a, n_e, 6)
        rng = np.random.default_rng(n_a)
        W = rng.standard_normal((n_a * n_e, 32))
        base = np.arange(32, dtype=np.int32) % 3
        y = rng.standard_normal((2, 5, 3))
        oagg, odagg = gr.group_reference(orc, xhh, y, V, D, W, base)
        for N in (1, 3):        # no output compares zero with zero (measured: values >= 1.8e-2, tangents >= 1.3)
            gr.nontrivial(oagg, odagg[:, :, :N], f"random weights {n_a}x{n_e} N={N}")
        _RANDOM[key] = (W, base, y, oagg, odagg)
    return _RANDOM[key]


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("K", [1, 9, 17, 32])
@pytest.mark.parametrize("n_a,n_e", [(33, 2), (257, 4)])
def test_random_weights(hank, n_a, n_e, K, N):
    """weights that tell a transposed (a, e) index apart, at every count of accumulators k_grp_mix is compiled for and with a block
    edge inside the rows (33 = 32 + 1, 257 = 4 * 64 + 1)"""
    m, V, D, xhh, _ = cases.shape(n_a, n_e, 6)
    W, base, y, oagg, odagg = _random_case(n_a, n_e)
    hb = _block(hank, m, None)
    hb.set_boundary(V, D)
    hb.set_group_outputs(W[:, :K], base[:K])
    hb.primal_jvp(xhh, y[:, :, :N])
    agg, dagg = hb.group_outputs(y[:, :, :N])
    _per_output(agg, dagg, oagg[:K], odagg[:K, :, :N], f"{n_a}x{n_e} K={K} N={N}")
    hb.close()


# ---- 3. the second family -----------------------------------------------------------------------------------------------------
def test_one_asset_hank_groups_with_a_transfer_tangent(hank):
    """three inputs, a transfer tangent and a borrowing limit off the grid: CONS and POLICY of three wealth groups"""
    from hank_amd.groups import wealth_groups
    m, ss, xhh, orc = cases.economy("hank", 2.0)
    P = xhh.shape[1]
    Wg = wealth_groups(ss.D, 80, 3, (0.0, 0.7, 0.95, 1.0))       # (the bottom half of this economy saves next to nothing: a wider bottom group)
    W, base = np.concatenate([Wg, Wg], axis=1), np.repeat(np.array([gr.CONS, gr.POLICY], dtype=np.int32), 3)
    y = np.random.default_rng(8).standard_normal((3, P, 4))
    oagg, odagg = gr.group_reference(orc, xhh, y, ss.value, ss.D, W, base)
    gr.nontrivial(oagg, odagg, "hank80")        # (measured: values 7.7e-2 .. 1.0, tangents 0.93 .. 24)
    hb = _block(hank, m, None)
    assert hb.n_hh == 3
    hb.set_boundary(ss.value, ss.D)
    hb.set_group_outputs(W, base)
    hb.primal_jvp(xhh, y)
    agg, dagg = hb.group_outputs(y)
    _per_output(agg, dagg, oagg, odagg, "hank 80x3")
    # the transfer's own tangent reaches CONS directly: a direction on tr alone moves it, and by exactly that direct term more
    # than it moves -POLICY
    yt = np.zeros((3, P, 1))
    yt[2, :, 0] = 1.0
    hb.jvp(yt)
    _, dt = hb.group_outputs(yt)
    _, odt = gr.group_reference(orc, xhh, yt, ss.value, ss.D, W, base)
    _per_output(hb.group_outputs()[0], dt, oagg, odt, "hank 80x3 dtr")
    hb.close()


# ---- 4. the edges of the recurrence -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["collapse", "swing"])
def test_clamped_columns_and_the_mass_point(hank, name):
    """whole columns clamped, all mass on row 0: the constrained group (MASS, and POLICY) and a one-hot weight on the last row of the
    last column under every base. The one-hot is NOT a comparison of zero with zero: the r offsets of periods 6 and 7 push mass to the
    top of the grid, so its value reaches 0.30 ("collapse") and 3.8e-3 ("swing") under MASS, and about 1 under CONS. In "collapse" the
    policy is clamped at the top wherever that mass sits, so the one-hot's MASS and POLICY tangents are tiny (measured 9.4e-12: below
    the tolerance's absolute term, they check that nothing spurious appears there); its CONS tangent (0.62) and every one-hot tangent
    of "swing" (0.27, 53, 51) are not."""
    from hank_amd.groups import constrained
    c = cases.raw_economy(name)
    n_a, n_e = c["grid"].size, c["Pi"].shape[0]
    G = n_a * n_e
    hot = np.zeros((G, 1))
    hot[G - 1, 0] = 1.0
    Wc = constrained(n_a, n_e)
    W = np.concatenate([Wc, Wc, hot, hot, hot], axis=1)
    base = np.array([gr.MASS, gr.POLICY, gr.MASS, gr.POLICY, gr.CONS], dtype=np.int32)
    y = np.random.default_rng(12).standard_normal((2, cases.EDGE_P, 3))
    oagg, odagg = gr.group_reference(c["orc"], c["x"], y, c["V"], c["D"], W, base)
    # (measured: the constrained mass reaches 1.0 in "collapse", where whole columns are clamped, and 0.16 in "swing")
    assert oagg[0].max() > (0.99 if name == "collapse" else 0.1), "the case lost its edge"
    for k in range(5):
        print(f"{name} output {k}: max |value| {np.abs(oagg[k]).max():.3e}, max |tangent| {np.abs(odagg[k]).max():.3e}")
    assert np.abs(oagg[2]).max() > 1e-3 and np.abs(oagg[3]).max() > 1e-1 and np.abs(oagg[4]).max() > 1e-1, "the one-hot holds no mass"
    assert np.abs(odagg[0]).max() > 1e-1 and np.abs(odagg[4]).max() > 1e-1
    assert name == "collapse" or all(np.abs(odagg[k]).max() > 1e-1 for k in (2, 3))
    hb = raw_block(hank, c["args"], None)
    hb.set_boundary(c["V"], c["D"])
    hb.set_group_outputs(W, base)
    for entry in ("primal_jvp", "primal, jvp"):
        hb.primal(c["x"] * 1.01)
        if entry == "primal_jvp":
            hb.primal_jvp(c["x"], y)
        else:
            hb.primal(c["x"])
            hb.jvp(y)
        agg, dagg = hb.group_outputs(y)
        _per_output(agg, dagg, oagg, odagg, f"{name} {entry}")
    hb.close()


# ---- 5. identities ------------------------------------------------------------------------------------------------------------
def test_unit_weights_are_the_heterogeneous_outputs(hank):
    xhh, y, _, _, _, _ = gr.ks_reference(5)
    m, ss, _ = ks_setup(130, 3, 40)
    hb = _block(hank, m, None)
    hb.set_boundary(ss.value, ss.D)
    hb.set_group_outputs(np.ones((390, 3)), [gr.MASS, gr.POLICY, gr.CONS])
    hb.primal_jvp(xhh, y)
    a2, d2 = hb.het_outputs(2, y)
    agg, dagg = hb.group_outputs(y)
    for o in range(2):
        _close(agg[:, 1 + o], a2[:, o], 1e-12, what=f"W = 1, output {o} value")
        _close(dagg[:, 1 + o, :], d2[:, o, :], 1e-12, what=f"W = 1, output {o} tangent")
    _close(agg[:, 0], np.ones(39), 1e-12, what="W = 1, MASS")
    print(f"W = 1, MASS tangent: {np.abs(dagg[:, 0, :]).max():.3e}")
    assert np.abs(dagg[:, 0, :]).max() <= 1e-12
    hb.close()


def test_groups_sum_to_the_totals_at_full_size(hank):
    """KS 2000x11, T = 300, N = 32, K = 12 under the default schedule, no oracle: the four wealth groups of each base sum to
    outputs 0 and 1 of hank_get_het_outputs at close(…, 1e-12), values and tangents, and their masses to one with a summed tangent
    of at most 1e-12 — the bounds of the 130x3 identities. Measured: 4.5e-13 and 1.6e-13 on tangents of scale 469 and 12.6, 8.9e-14
    on the summed MASS tangent (the groups' own are of size 11)."""
    from hank_amd.groups import wealth_groups
    m, ss, _ = ks_setup(2000, 11, 300)
    P = m.compspec.T - 1
    x, _ = ks_paths(m, ss, "x1", 0.05)
    y = np.random.default_rng(7).standard_normal((2, P, 32))
    Wg = wealth_groups(ss.D, 2000, 11, gr.EDGES)
    hb = _block(hank, m, None)
    hb.set_boundary(ss.value, ss.D)
    hb.set_group_outputs(np.concatenate([Wg, Wg, Wg], axis=1), np.repeat(np.array([gr.MASS, gr.POLICY, gr.CONS], dtype=np.int32), 4))
    hb.primal_jvp(x[2:4], y)
    assert hb.info()["last_tangent_family_name"] == cases.expected_family(None, "dual", 32)
    a2, d2 = hb.het_outputs(2, y)
    agg, dagg = hb.group_outputs(y)
    assert agg.shape == (P, 12) and dagg.shape == (P, 12, 32)
    for o in range(2):
        sl = slice(4 * (1 + o), 4 * (2 + o))
        assert all(np.abs(dagg[:, k, :]).max() > 1e-3 * np.abs(d2[:, o, :]).max() for k in range(sl.start, sl.stop)), "a group that does not move"
        _close(agg[:, sl].sum(axis=1), a2[:, o], 1e-12, what=f"full size, output {o} value")
        _close(dagg[:, sl, :].sum(axis=1), d2[:, o, :], 1e-12, what=f"full size, output {o} tangent")
    _close(agg[:, :4].sum(axis=1), np.ones(P), 1e-12, what="full size, MASS")
    dm = np.abs(dagg[:, :4, :].sum(axis=1)).max()
    print(f"full size, MASS tangent summed over the groups: {dm:.3e} (the groups' own: {np.abs(dagg[:, :4, :]).max():.3e})")
    assert dm <= 1e-12
    a2b, d2b = hb.group_outputs(y)
    assert np.array_equal(a2b, agg) and np.array_equal(d2b, dagg)
    hb.close()


# ---- 6. protocol --------------------------------------------------------------------------------------------------------------
def _code(hank, call):
    with pytest.raises(hank.HankHIPError) as ei:
        call()
    return ei.value.code


def test_refusals(hank):
    from hank_amd import hip
    xhh, y, W, base, _, _ = gr.ks_reference(5)
    m, ss, _ = ks_setup(130, 3, 40)
    BAD, NOT_READY = hip.HANK_ERR_BAD_ARG, hip.HANK_ERR_NOT_READY
    hb = _block(hank, m, None)
    hb.set_boundary(ss.value, ss.D)
    # hank_set_group_outputs
    assert _code(hank, lambda: hb.set_group_outputs(np.ones((390, 33)), gr.MASS)) == BAD               # K > HANK_GROUP_MAX
    for b in (-1, 3):
        assert _code(hank, lambda: hb.set_group_outputs(np.ones((390, 2)), [gr.MASS, b])) == BAD       # a base outside 0..2
    i32p = hip.C.POINTER(hip.C.c_int32)
    b2 = np.zeros(2, dtype=np.int32)
    assert hb._lib.hank_set_group_outputs(hb._ctx, 2, None, b2.ctypes.data_as(i32p)) == BAD            # null pointers with K > 0
    assert hb._lib.hank_set_group_outputs(hb._ctx, 2, hip._p(np.ones(780)), None) == BAD
    assert hb._lib.hank_set_group_outputs(hb._ctx, -1, None, None) == BAD
    # hank_get_group_outputs, hank_fake_news_group: groups and no primal, then a primal and no groups (cleared; a refused call has
    # set none)
    hb.set_group_outputs(W, base)
    assert _code(hank, hb.group_outputs) == NOT_READY
    assert _code(hank, hb.fake_news_group) == NOT_READY
    hb.set_group_outputs(None, None)
    assert _code(hank, lambda: hb.set_group_outputs(np.ones((390, 33)), gr.MASS)) == BAD
    hb.primal_jvp(xhh, y)
    assert _code(hank, lambda: hb.group_outputs(y)) == NOT_READY
    assert _code(hank, hb.group_outputs) == NOT_READY
    assert _code(hank, hb.fake_news_group) == NOT_READY
    hb.set_group_outputs(W, base)
    # no batch of that width is current
    hb.primal(xhh)
    assert hb.group_outputs()[0].shape == (39, 12)
    assert _code(hank, lambda: hb.group_outputs(y)) == NOT_READY
    hb.jvp(y)
    assert hb.group_outputs(y)[1].shape == (39, 12, 5)
    assert _code(hank, lambda: hb.group_outputs(y[:, :, :4])) == NOT_READY
    assert hb._lib.hank_get_group_outputs(hb._ctx, None, 5, None, hip._p(np.empty(39 * 12 * 5))) == BAD        # tangents without dxhh
    assert hb._lib.hank_get_group_outputs(hb._ctx, None, 0, None, None) == BAD                                 # no output array
    # the current batch carries boundary seeds
    dD = np.random.default_rng(1).standard_normal((130, 3, 5)) * np.asarray(ss.D).reshape((130, 3, 1), order="F")
    hb.jvp_boundary(dxhh=y, dD_init=dD - dD.sum(axis=(0, 1), keepdims=True) / 390)
    assert _code(hank, lambda: hb.group_outputs(y)) == NOT_READY
    assert hb.het_outputs(2, y)[1].shape == (39, 2, 5)                                                  # (outputs 0 and 1 are served)
    assert hb.group_outputs()[0].shape == (39, 12)                                                      # (and the groups' values)
    hb.jvp(y)
    hb.group_outputs(y)
    # hank_fake_news_group refuses what hank_fake_news refuses: a path that varies over time
    assert _code(hank, hb.fake_news) == NOT_READY and _code(hank, hb.fake_news_group) == NOT_READY
    # cleared: not ready again; a clone carries no groups
    hb.set_group_outputs(None, None)
    assert _code(hank, lambda: hb.group_outputs(y)) == NOT_READY
    hb.set_group_outputs(W, base)
    other = hb.clone()
    other.primal(xhh)
    assert other.n_groups == 0 and _code(hank, other.group_outputs) == NOT_READY
    other.close()
    hb.close()


def test_groups_leave_the_record_the_batch_and_the_memo_alone(hank):
    xhh, y, W, base, _, _ = gr.ks_reference(5)
    m, ss, _ = ks_setup(130, 3, 40)
    hb = _block(hank, m, None)
    hb.set_boundary(ss.value, ss.D)
    hb.primal_jvp(xhh, y)
    d0, pol0, dpol0, st0 = hb.jvp(y), hb.policy_seq(), hb.dpolicy_seq(5), hb.stats()
    a2, d2 = hb.het_outputs(2, y)
    for step in ("set", "set again", "clear"):
        if step == "clear":
            hb.set_group_outputs(None, None)
        else:
            hb.set_group_outputs(W, base)
            ag, dg = hb.group_outputs(y)                      # the batch that was current before the groups were set
            if step == "set again":
                assert np.array_equal(ag, ag0) and np.array_equal(dg, dg0)
            ag0, dg0 = ag, dg
        st = hb.stats()
        assert st["primal_memo_hits"] == st0["primal_memo_hits"] and st["primal_sweeps"] == st0["primal_sweeps"], step
        assert np.array_equal(hb.dpolicy_seq(5), dpol0) and np.array_equal(hb.policy_seq(), pol0), step
        b2, e2 = hb.het_outputs(2, y)
        assert np.array_equal(b2, a2) and np.array_equal(e2, d2), step
        assert np.array_equal(hb.jvp(y), d0), step
    hb.primal_jvp(xhh, y)                                     # the memo survived all of it
    assert hb.stats()["primal_memo_hits"] == st0["primal_memo_hits"] + 1
    # a new primal: values at once, tangents NOT_READY until the next jvp
    hb.set_group_outputs(W, base)
    hb.primal(xhh * 1.01)
    a1, _ = hb.group_outputs()
    assert not np.array_equal(a1, ag0)
    assert _code(hank, lambda: hb.group_outputs(y)) == hank.hip.HANK_ERR_NOT_READY
    hb.jvp(y)
    assert np.array_equal(hb.group_outputs(y)[0], a1)
    # another set of groups at the same record: its own values, not the old set's
    hb.set_group_outputs(W[:, ::-1], base[::-1])
    a3, d3 = hb.group_outputs(y)
    assert np.array_equal(a3, a1[:, ::-1]) and np.array_equal(d3, hb.group_outputs(y)[1])
    hb.close()


def test_device_pointer_form_equals_the_host_form(hank):
    import torch
    xhh, y, W, base, _, _ = gr.ks_reference(5)
    m, ss, _ = ks_setup(130, 3, 40)
    P, N, K = 39, 5, 12
    hb = _block(hank, m, None)
    hb.set_boundary(ss.value, ss.D)
    hb.set_group_outputs(W, base)
    hb.primal_jvp(xhh, y)
    aggs, daggs = hb.group_outputs(y)
    dev = torch.device("cuda", 0)
    d_y = torch.from_numpy(np.asfortranarray(y).reshape(-1, order="F").copy()).to(dev)
    d_a = torch.empty(K * P, dtype=torch.float64, device=dev)
    d_d = torch.empty(K * P * N, dtype=torch.float64, device=dev)
    hb.group_outputs_dev(d_y.data_ptr(), N, d_a.data_ptr(), d_d.data_ptr())
    hb.sync()
    assert np.array_equal(d_a.cpu().numpy().reshape(P, K, order="F"), aggs)
    assert np.array_equal(d_d.cpu().numpy().reshape(P, K, N, order="F"), daggs)
    d_a.zero_()
    hb.group_outputs_dev(0, 0, d_a.data_ptr(), 0)             # values only
    hb.sync()
    assert np.array_equal(d_a.cpu().numpy().reshape(P, K, order="F"), aggs)
    hb.close()


# ---- 7. the Toeplitz Jacobian -------------------------------------------------------------------------------------------------
def test_group_jacobian_at_the_steady_state(hank):
    """KS 130x3, T = 40: the twelve outputs and the two W = 1 rows (K = 14: two passes over the expectation workspace) against unit
    tangents pushed through group_outputs and against the oracle's (1e-8 of each output's largest entry, the bar of
    tests/test_gpu_jacobian.py and tests/test_gpu_fake_news_het.py); the W = 1 rows against hank_fake_news_het."""
    from hank_amd.SteadyStateJacobian import group_jacobian, household_jacobian
    m, ss, orc = ks_setup(130, 3, 40)
    P, n_hh = 39, 2
    xhh = np.ascontiguousarray(ks_paths(m, ss, "x0")[0][2:4])
    W12, base12 = gr.ks_groups()
    W = np.concatenate([W12, np.ones((390, 2))], axis=1)
    base = np.concatenate([base12, np.array([gr.POLICY, gr.CONS], dtype=np.int32)])
    hb = _block(hank, m, None)
    hb.set_boundary(ss.value, ss.D)
    hb.set_group_outputs(W, base)
    hb.primal(xhh)
    J = group_jacobian(hb)
    assert J.shape == (14, P, n_hh, P)
    assert np.array_equal(group_jacobian(hb), J)              # the same bits again
    cols = [0, 1, P // 2, P - 2, P - 1]
    y = np.zeros((n_hh, P, n_hh * len(cols)))
    for q, s_ in enumerate(cols):
        for i in range(n_hh):
            y[i, s_, q * n_hh + i] = 1.0
    hb.primal(xhh)
    hb.jvp(y)
    dagg = hb.group_outputs(y)[1]                             # (P, K, N)
    _, odagg = gr.group_reference(orc, xhh, y[:, :, :4 * n_hh], ss.value, ss.D, W, base)      # four shock dates
    for k in range(14):
        scale, oscale = np.abs(dagg[:, k, :]).max(), np.abs(odagg[k]).max()
        assert scale > 1e-6 and oscale > 1e-6, k
        for q, s_ in enumerate(cols):
            for i in range(n_hh):
                err = np.abs(J[k, :, i, s_] - dagg[:, k, q * n_hh + i]).max()
                assert err < 1e-8 * scale, f"output {k}, input {i}, column {s_}: {err:.3e} vs scale {scale:.3e} (unit tangents)"
                if q < 4:
                    err = np.abs(J[k, :, i, s_] - odagg[k][:, q * n_hh + i]).max()
                    assert err < 1e-8 * oscale, f"output {k}, input {i}, column {s_}: {err:.3e} vs scale {oscale:.3e} (oracle)"
    hb.primal(xhh)
    Fh, Dvh = hb.fake_news_het(2)
    F, Dv = hb.fake_news_group()
    for o in range(2):
        _close(F[..., 12 + o], Fh[..., o], 1e-12, what=f"W = 1, F of output {o}")
        _close(Dv[..., 12 + o], Dvh[..., o], 1e-12, what=f"W = 1, Dv of output {o}")
        _close(J[12 + o], household_jacobian(Fh[..., o], Dvh[..., o]).transpose(1, 0, 2), 1e-12, what=f"W = 1, J of output {o}")
    hb.close()


# ---- 8. central differences ---------------------------------------------------------------------------------------------------
def test_central_differences_one_asset_hank(hank):
    """oracle-independent: the device's own values differentiated along one direction (1e-6 relative, per output)"""
    from hank_amd.groups import wealth_groups
    m, ss = hank_economy(130, 3, 60, GOODS)
    P = m.compspec.T - 1
    x = _hank_x(ss, P)
    Wg = wealth_groups(ss.D, 130, 3, (0.0, 0.5, 0.9, 1.0))
    hb = _block(hank, m, None)
    hb.set_boundary(ss.value, ss.D)
    hb.set_group_outputs(np.concatenate([Wg, Wg, Wg], axis=1), np.repeat(np.array([gr.MASS, gr.POLICY, gr.CONS], dtype=np.int32), 3))
    h = 1e-6
    y = np.random.default_rng(5).standard_normal((3, P, 4))
    yd = y[:, :, 0] * np.array([1e-3, 1e-2, 1e-2])[:, None]
    hb.primal_jvp(x, yd[:, :, None])
    dY = hb.group_outputs(yd[:, :, None])[1][:, :, 0]
    hb.primal(x + h * yd)
    yp = hb.group_outputs()[0]
    hb.primal(x - h * yd)
    ym = hb.group_outputs()[0]
    fd = (yp - ym) / (2 * h)
    for k in range(9):
        err, scale = np.max(np.abs(fd[:, k] - dY[:, k])), np.abs(dY[:, k]).max()
        print(f"output {k}: central-difference error {err:.3e} vs scale {scale:.3e}")
        assert scale > 0 and err <= 1e-6 * scale, f"output {k}: central-difference error {err:.3e}"
    hb.close()
