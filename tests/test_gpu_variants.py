"""The sweep variants the other GPU tests never launch, against the CPU oracle (oracle/hank_oracle.c) at rel 1e-10 + abs 1e-12:

1. a parity matrix over the CRRA curvature and the record layout. gamma picks code paths, not only values: pow_crra's branches
   (X half x^(-1/gamma), Y half x^(-gamma): rcp at gamma = 1, rcp(x^2) and rsqrt at gamma = 0.5, pow elsewhere), and the record
   diet (on for gamma in {1, 2}: the tangent sweeps rebuild kc and v; off otherwise, or with HANK_RECORD_DIET=0: they read them,
   and the wide backward sweep is another template). Every schedule (launch, xcd, wide, auto), both entry points;
2. the rest of the pipeline at gamma != 2: the device VFI, the Toeplitz Jacobian, the extra heterogeneous outputs;
3. the shape edges of the persistent and wide families: the 1024-thread persistent family (n_e >= 12), a last 63-row slab full
   or holding one row, the largest grid the XCD schedule takes and the first it refuses, every instantiated n_e of the wide
   family in both geometries and both record layouts, and n_a = WIDE_CS.

The boundary (V_T, D_0) of each curvature is the host steady state of a fresh model (never a model ks_setup cached: its params
are shared by the session). The shape tests take a cheaper boundary, a host VFI iterate and a uniform D_0: parity needs a valid
boundary, not a stationary one."""
import numpy as np
import pytest

from cases import (CASES, FAMILY, against_oracle_and_launches as _against_oracle_and_launches, block as _block, close as _close,
                   economy as _economy, expected_family as _expected_family, raw_block, shape as _shape, sweeps as _sweeps)

pytestmark = pytest.mark.gpu

# the one-asset HANK calibration (the bond supply that clears the asset market) has no steady state at gamma = 0.5 (its Newton
# step is singular); no other gamma takes the rcp(x^2) | rsqrt pair, so Krusell-Smith alone covers it
MATRIX = [(fam, case) for fam in ("ks", "hank") for case in CASES if not (fam == "hank" and case == "gamma0.5")]


NS = (1, 5, 12, 40)          # with 8 groups: D = 1, 1, 2, and two passes (32 at D = 4, then 8)
NWIDE = 96                   # the default schedule sends it to the on-chip wide sweeps


@pytest.mark.parametrize("family,case", MATRIX)
def test_parity_over_curvature_and_record_layout(hank, family, case):
    gamma, diet_env, diet = CASES[case]
    m, ss, xhh, orc = _economy(family, gamma)
    n_hh, P = xhh.shape
    y = np.random.default_rng(17).standard_normal((n_hh, P, NWIDE))
    oagg, odagg, opol, odpol = orc.block(xhh, y[:, :, :max(NS)], ss.value, ss.D)
    res = {}
    for sched in ("launch", "xcd", "wide", None):
        hb = _block(hank, m, sched, HANK_RECORD_DIET=diet_env)
        hb.set_boundary(ss.value, ss.D)
        info = hb.info()
        assert info["record_diet"] == diet, (sched, info)
        assert info["wide_mode"] == {"wide": 2, None: 1}.get(sched, 0), (sched, info)
        Ns = NS + ((NWIDE,) if sched in (None, "launch") else ())
        res[sched] = _sweeps(hb, xhh, y, Ns)
        st = hb.stats()
        assert st["schedule"] == {"launch": 0, "xcd": 1}.get(sched, 2) and st["fallbacks"] == 0, (sched, st)
        hb.close()
        for (entry, N), (fam, agg, dagg, pol, dpol, D) in res[sched].items():
            what = f"{family} {case} {sched} {entry} N={N}"
            assert fam == _expected_family(sched, entry, N), (what, fam)
            k = min(N, max(NS))
            _close(agg, oagg, what=what + " agg"); _close(dagg[:, :k], odagg[:, :k], what=what + " dagg")
            _close(pol, opol, what=what + " policy"); _close(dpol[..., :k], odpol[..., :k], what=what + " dpolicy")
            np.testing.assert_allclose(D.sum(axis=(0, 1)), 1.0, rtol=0, atol=1e-12)
    # the three families against each other; the persistent sweeps and the launches hold the same policy bits whether a kernel
    # reads kc and v from the record or rebuilds them (the wide family rebuilds A and B by a reciprocal: to rounding)
    for sched in ("xcd", "wide", None):
        for (entry, N), (fam, agg, dagg, pol, dpol, D) in res[sched].items():
            _, agg0, dagg0, pol0, dpol0, D0 = res["launch"][entry, N]
            what = f"{family} {case} {sched} vs launch {entry} N={N}"
            _close(agg, agg0, 1e-12, what=what + " agg"); _close(dagg, dagg0, 1e-12, what=what + " dagg")
            _close(dpol, dpol0, 1e-12, what=what + " dpolicy"); _close(D, D0, 1e-12, what=what + " D")
            assert np.array_equal(pol, pol0), what + " policy"
            if fam != FAMILY["wide"]:
                assert np.array_equal(dpol, dpol0), what + " dpolicy bits"
    if diet_env == "0":
        # the same curvature with the diet on: kc and v rebuilt through the cancellation in cm (~1e-13)
        for sched in ("launch", "xcd", "wide", None):
            hb = _block(hank, m, sched)
            hb.set_boundary(ss.value, ss.D)
            assert hb.info()["record_diet"] == 1
            Ns = NS + ((NWIDE,) if sched is None else ())
            on = _sweeps(hb, xhh, y, Ns)
            assert hb.stats()["fallbacks"] == 0
            hb.close()
            for key, (fam, agg, dagg, pol, dpol, D) in on.items():
                what = f"{family} {case} {sched} diet on vs off {key}"
                assert fam == res[sched][key][0], what
                assert np.array_equal(pol, res[sched][key][3]), what + " policy"
                _close(dagg, res[sched][key][2], 1e-12, what=what + " dagg")
                _close(dpol, res[sched][key][4], 1e-12, what=what + " dpolicy")


# ---- 2. the rest of the pipeline at gamma != 2 -------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma", [1.0, 0.5, 3.0])
def test_device_vfi_at_other_curvatures(hank, gamma):
    """hank_vfi (k_xvfi under xcd, k_egm_step under launch) on the other pow_crra branches: the oracle iteration's step count
    within one, value and policy to 1e-10."""
    m, ss, _, orc = _economy("ks", gamma)
    n_a, n_e = ss.value.shape
    r, w, tol = ss.vars["r"], ss.vars["w"], 1e-11
    v_o, p_o, steps_o, _ = orc.vfi((n_a, n_e), r, w, tol)
    for sched in ("launch", "xcd"):
        hb = _block(hank, m, sched)
        v, pol, it, nrm = hb.vfi(np.ones((n_a, n_e)), [r, w], tol)
        assert abs(it - steps_o) <= 1 and nrm < tol, (sched, it, steps_o)
        assert np.max(np.abs(v - v_o)) < 1e-10 * np.abs(v_o).max(), sched
        assert np.max(np.abs(pol - p_o)) < 1e-10 * max(1.0, np.abs(p_o).max()), sched
        assert hb.stats()["fallbacks"] == 0 and hb.stats()["schedule"] == (0 if sched == "launch" else 1)
        hb.close()


@pytest.mark.parametrize("gamma,diet", [(1.0, 1), (1.5, 0)])
def test_toeplitz_jacobian_at_other_curvatures(hank, gamma, diet):
    """hank_fake_news against the unit-tangent J̅ (method="columns": 156 columns, the on-chip wide sweeps) at 1e-8 of the largest
    entry, the bar of tests/test_gpu_jacobian.py."""
    from hank_amd.BackwardIteration import household_block
    m, ss, _, _ = _economy("ks", gamma)
    Jt = hank.getSteadyStateJacobian(ss, m, method="toeplitz").toarray()
    Jc = hank.getSteadyStateJacobian(ss, m, method="columns").toarray()
    hb = household_block(m)
    assert hb.info()["record_diet"] == diet and hb.stats()["fallbacks"] == 0
    assert np.max(np.abs(Jc)) > 0.5
    assert np.max(np.abs(Jt - Jc)) < 1e-8 * np.max(np.abs(Jc))


@pytest.mark.parametrize("family,n_het", [("ks", 3), ("hank", 4)])
def test_nonaffine_outputs_at_gamma_1_5(hank, family, n_het):
    """Value (Krusell-Smith) and UCE (one-asset HANK) at gamma = 1.5 (pow branches, diet off): hank_get_het_outputs after a
    Dual pass, and hank_fake_news_het's columns against the oracle's unit tangents at the steady state (1e-8, the bar of
    tests/test_gpu_fake_news_het.py)."""
    from hank_amd.BackwardIteration import household_inputs
    from hank_amd.GeneralStructures import vars_of_type
    from hank_amd.SteadyStateJacobian import household_jacobian
    gamma = 1.5
    m, ss, xhh, orc = _economy(family, gamma)
    n_hh, P = xhh.shape
    y = np.random.default_rng(23).standard_normal((n_hh, P, 5))
    hb = _block(hank, m, None)
    hb.set_boundary(ss.value, ss.D)
    assert hb.info()["record_diet"] == 0
    hb.set_het_outputs(n_het)
    hb.primal_jvp(xhh, y)
    agg, dagg = hb.het_outputs(n_het, y)
    oagg, odagg = orc.het_outputs(xhh, y, ss.value, ss.D, n_het, gamma)
    for j in range(n_het):
        _close(agg[:, j], oagg[j], what=f"output {j}")
        _close(dagg[:, j, :], odagg[j], what=f"output {j} partials")
    # the Toeplitz form at the stationary primal
    x_ss = np.tile(np.array([ss.vars[k] for k in vars_of_type(m, "endogenous")]), P)
    exog = {k: np.full(P, float(ss.vars[k])) for k in vars_of_type(m, "exogenous")}
    xss = np.asarray(household_inputs(x_ss, exog, m)[0])
    hb.primal(xss)
    F, Dv = hb.fake_news_het(n_het)
    assert hb.stats()["fallbacks"] == 0
    hb.close()
    cols = sorted(set([0, 1, P // 2, P - 2, P - 1]))
    yu = np.zeros((n_hh, P, n_hh * len(cols)))
    for q, s_ in enumerate(cols):
        for k in range(n_hh):
            yu[k, s_, q * n_hh + k] = 1.0
    _, odu = orc.het_outputs(xss, yu, ss.value, ss.D, n_het, gamma)
    for o in range(n_het):
        J = household_jacobian(F[..., o], Dv[..., o])
        scale = np.max(np.abs(odu[o]))
        assert scale > 1e-6, o
        for q, s_ in enumerate(cols):
            for k in range(n_hh):
                err = np.max(np.abs(J[k][:, s_] - odu[o][:, q * n_hh + k]))
                assert err < 1e-8 * scale, f"output {o}, input {k}, column {s_}: {err:.3e} vs scale {scale:.3e}"


# ---- 3. shape edges of the persistent and wide families ----------------------------------------------------------------------
@pytest.mark.parametrize("n_e", [11, 12, 16])
def test_xcd_sweeps_across_the_1024_thread_boundary(hank, n_e):
    """64 (n_e + 1) threads: n_e = 11 is the last 768-thread grid, 12 the first 1024-thread one (dmax = 2). N = 12 is D = 2 in
    one pass, N = 40 one pass at 768 threads and three (16 + 16 + 8) at 1024; with the diet on and off."""
    _against_oracle_and_launches(hank, _shape(40, n_e, 10), [("xcd", {}), ("xcd", {"HANK_RECORD_DIET": 0})], (12, 40))


@pytest.mark.parametrize("n_a", [63, 64, 126, 127])
def test_last_slab_full_or_holding_one_row(hank, n_a):
    """the persistent sweeps work in 63-row slabs, one per CU of an XCD: a last slab exactly full (63, 126) or holding one row
    (64, 127); and the wide family at the same grids (rows in pairs or quads per thread)."""
    _against_oracle_and_launches(hank, _shape(n_a, 3, 12), [("xcd", {}), ("xcd", {"HANK_RECORD_DIET": 0}), ("wide", {}),
                                                                   ("wide", {"HANK_WIDE_R": 4})], (5, 40))


def test_xcd_capacity(hank):
    """the largest grid the XCD schedule takes, one 63-row slab per CU of an XCD, runs forced `xcd`; one more row: a forced `xcd`
    fails at hank_create with its reason, and the default schedule is the launches."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count // 8
    n_a = 63 * cus
    _against_oracle_and_launches(hank, _shape(n_a, 2, 5), [("xcd", {})], (4,))
    args = (np.linspace(0.0, 200.0, n_a + 1), np.array([0.5, 1.5]), np.array([[0.9, 0.1], [0.1, 0.9]]), 0.98, 2.0, 0.0, 5)
    with pytest.raises(hank.HankHIPError, match=f"HANK_SCHEDULE=xcd: n_a={n_a + 1} needs {cus + 1} workgroups per XCD"):
        raw_block(hank, args, "xcd")
    hb = raw_block(hank, args, None)
    assert hb.stats()["schedule"] == 0
    hb.close()


@pytest.mark.parametrize("n_e", [2, 3, 4, 5, 7, 11])
def test_every_instantiated_wide_ne(hank, n_e):
    """k_wide_back / k_wide_fwd of every n_e of HANK_WIDE_NE_LIST, in both geometries (2 rows per thread, 1024-thread workgroups;
    4 rows, 512) and both record layouts (the diet-off backward sweep is another template)."""
    runs = [("wide", {"HANK_WIDE_R": r, "HANK_RECORD_DIET": d}) for r in (2, 4) for d in (None, 0)]
    _against_oracle_and_launches(hank, _shape(40, n_e, 10), runs, (5,))


@pytest.mark.parametrize("n_a", [2047, 2048])
def test_wide_capacity(hank, n_a):
    """WIDE_CS = 2048 rows: at 2047 and 2048 every row slot of a workgroup is live (both geometries, both layouts)."""
    runs = [("wide", {"HANK_WIDE_R": r, "HANK_RECORD_DIET": d}) for r in (2, 4) for d in (None, 0)]
    _against_oracle_and_launches(hank, _shape(n_a, 2, 5), runs, (3,))


def test_wide_refuses_one_row_more_than_it_holds(hank):
    """n_a = 2049: auto reports the wide sweeps unsupported, a forced `wide` fails at hank_create with its reason."""
    args = (np.linspace(0.0, 200.0, 2049), np.array([0.5, 1.5]), np.array([[0.9, 0.1], [0.1, 0.9]]), 0.98, 2.0, 0.0, 5)
    hb = raw_block(hank, args, None)
    assert hb.info()["wide_supported"] == 0 and hb.info()["wide_mode"] == 0
    hb.close()
    with pytest.raises(hank.HankHIPError, match="n_a <= 2048"):
        raw_block(hank, args, "wide")
