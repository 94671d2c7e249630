"""The steady-state Jacobian of EVERY heterogeneous output from its Toeplitz structure (hank_fake_news_het): the policy responses
and the lottery impulses are shared by all outputs (each is dotted with the same post-transition D_t, ForwardIteration.jl:303-307);
only the expectation vectors and the direct term differ per output. Output 0 must equal hank_fake_news bit for bit; the others are
checked against unit-tangent JVPs of the device (hb.jvp + hb.het_outputs), against the CPU oracle's unit-tangent outputs, and
— assembled into J̅ — against method="columns". The reference has no multi-output J̅ (its slicing assumes one heterogeneous
variable, SteadyStateJacobian.jl:295-303), so outputs >= 1 are pinned against these two instead. Tolerance: 1e-8 of the largest
entry, the bar of test_gpu_jacobian.py."""
import numpy as np
import pytest

from cases import hank_economy, model_args, oracle_of
from conftest import ROOT, ks_setup

pytestmark = pytest.mark.gpu

GOODS = "one_asset_hank_goods.yaml"


def _setup(family, n_a, n_e, T):
    """model, steady state, the constant steady-state household inputs (n_hh, P) and the family's output count."""
    from hank_amd.BackwardIteration import household_inputs
    from hank_amd.GeneralStructures import vars_of_type
    m, ss = ks_setup(n_a, n_e, T)[:2] if family == "ks" else hank_economy(n_a, n_e, T, GOODS)
    P = m.compspec.T - 1
    x_ss = np.tile(np.array([ss.vars[k] for k in vars_of_type(m, "endogenous")]), P)
    exog = {k: np.full(P, float(ss.vars[k])) for k in vars_of_type(m, "exogenous")}
    xhh = np.asarray(household_inputs(x_ss, exog, m)[0])
    return m, ss, xhh, len(m.value_fn.outputs)


def _at_the_steady_state(hank, m, ss, xhh):
    hb = hank.HouseholdBlock(*model_args(m))
    hb.set_boundary(ss.value, ss.D)
    hb.primal(xhh)
    return hb


def _unit_tangents(n_hh, P):
    """unit shocks to every household input at columns [0, 1, P//2, P-2, P-1]: y (n_hh, P, n_hh * len(cols)), column q*n_hh + k."""
    cols = sorted(set([0, 1, P // 2, P - 2, P - 1]))
    y = np.zeros((n_hh, P, n_hh * len(cols)))
    for q, s_ in enumerate(cols):
        for k in range(n_hh):
            y[k, s_, q * n_hh + k] = 1.0
    return cols, y


def _check_columns(F, Dv, cols, dagg, what):
    """household_jacobian of every output against dagg (n_het, P, N) at the unit-tangent columns: 1e-8 of the largest entry."""
    from hank_amd.SteadyStateJacobian import household_jacobian
    n_hh, n_het = F.shape[2], F.shape[3]
    for o in range(n_het):
        J = household_jacobian(F[..., o], Dv[..., o])
        scale = np.max(np.abs(dagg[o]))
        assert scale > 1e-6, (what, o)
        for q, s_ in enumerate(cols):
            for k in range(n_hh):
                err = np.max(np.abs(J[k][:, s_] - dagg[o][:, q * n_hh + k]))
                assert err < 1e-8 * scale, f"{what}: output {o}, input {k}, column {s_}: {err:.3e} vs scale {scale:.3e}"


@pytest.mark.parametrize("family,n_a,n_e,T", [("ks", 50, 2, 100), ("hank", 80, 3, 40)])
def test_output_0_is_fake_news_bit_for_bit(hank, family, n_a, n_e, T):
    m, ss, xhh, n_max = _setup(family, n_a, n_e, T)
    P, n_hh = m.compspec.T - 1, xhh.shape[0]
    hb = _at_the_steady_state(hank, m, ss, xhh)
    F0, Dv0 = hb.fake_news()
    last = None
    for n in range(1, n_max + 1):
        F, Dv = hb.fake_news_het(n)
        assert F.shape == (P, P, n_hh, n) and Dv.shape == (P, n_hh, n)
        assert np.array_equal(F[..., 0], F0) and np.array_equal(Dv[..., 0], Dv0), n
        if last is not None:                 # a wider call changes none of the narrower outputs
            assert np.array_equal(F[..., :n - 1], last[0]) and np.array_equal(Dv[..., :n - 1], last[1]), n
        last = (F, Dv)
    # the workspace grown to n_max serves hank_fake_news again with the same bits
    F0b, Dv0b = hb.fake_news()
    assert np.array_equal(F0b, F0) and np.array_equal(Dv0b, Dv0)
    # independent of the hank_set_het_outputs declaration (default 2), which it leaves as it is
    with pytest.raises(hank.HankHIPError):
        hb.het_outputs(3)
    hb.set_het_outputs(n_max)
    F, Dv = hb.fake_news_het(n_max)
    assert np.array_equal(F, last[0]) and np.array_equal(Dv, last[1])
    hb.close()


@pytest.mark.parametrize("family,n_a,n_e,T", [("ks", 130, 3, 20), ("ks", 50, 2, 100), ("hank", 80, 3, 40)])
def test_every_output_against_unit_tangents(hank, family, n_a, n_e, T):
    """household_jacobian of each output against hb.jvp + hb.het_outputs of unit tangents at the same stationary primal."""
    m, ss, xhh, n_max = _setup(family, n_a, n_e, T)
    P, n_hh = m.compspec.T - 1, xhh.shape[0]
    hb = _at_the_steady_state(hank, m, ss, xhh)
    F, Dv = hb.fake_news_het(n_max)
    cols, y = _unit_tangents(n_hh, P)
    hb.set_het_outputs(n_max)
    hb.primal(xhh)
    hb.jvp(y)
    dagg = np.moveaxis(hb.het_outputs(n_max, y)[1], 1, 0)          # (n_het, P, N)
    _check_columns(F, Dv, cols, dagg, f"{family} {n_a}x{n_e} T={T}")
    hb.close()


@pytest.mark.parametrize("family,n_a,n_e,T", [("ks", 130, 3, 20), ("hank", 80, 3, 40)])
def test_every_output_against_the_oracle(hank, family, n_a, n_e, T):
    """the same columns against the CPU oracle's unit-tangent outputs (savings, consumption, Value[, UCE])."""
    m, ss, xhh, n_max = _setup(family, n_a, n_e, T)
    P, n_hh = m.compspec.T - 1, xhh.shape[0]
    hb = _at_the_steady_state(hank, m, ss, xhh)
    F, Dv = hb.fake_news_het(n_max)
    hb.close()
    cols, y = _unit_tangents(n_hh, P)
    _, odagg = oracle_of(m).het_outputs(xhh, y, ss.value, ss.D, n_max, m.params.γ)
    _check_columns(F, Dv, cols, odagg, f"oracle {family} {n_a}x{n_e} T={T}")


def _ks_value_model(hank, tmp_path, n_a, n_e, T):
    """Krusell-Smith with heterogeneous: [KD, Value] (the reference's own ValueFunction return keys)."""
    src = (ROOT / "examples" / "krusell_smith.yaml").read_text()
    line = '    - {name: "KD", description: "capital demand (aggregate household savings)"}\n'
    assert line in src
    spec = tmp_path / "ks_value.yaml"
    spec.write_text(src.replace(line, line + '    - {name: "Value", description: "aggregate value"}\n'))
    m = hank.build_model_from_yaml(str(spec), overrides={"T": T, "dimensions": {"wealth": {"n": n_a}, "productivity": {"n": n_e}}})
    assert hank.vars_of_type(m, "heterogeneous") == ("KD", "Value")
    ss, _ = hank.get_SteadyStates(m, vfi="host")
    return m, ss


@pytest.mark.parametrize("model", ["goods", "wages", "ks_value"])
def test_toeplitz_jacobian_of_multi_output_models_equals_the_columns(hank, model, monkeypatch, tmp_path):
    """the whole J̅ of a model with more than one heterogeneous variable, with the column path made unreachable during the
    toeplitz call."""
    import hank_amd.parallel as par
    if model == "goods":
        m, ss = hank_economy(80, 3, 40, GOODS)
    elif model == "wages":
        m, ss = hank_economy(200, 5, 80, "one_asset_hank_wages.yaml")
    else:
        m, ss = _ks_value_model(hank, tmp_path, 130, 3, 40)
    assert len(hank.vars_of_type(m, "heterogeneous")) > 1

    def no_columns(*a, **k):
        raise AssertionError("the toeplitz J̅ took the unit-tangent column path")

    with monkeypatch.context() as mp:
        mp.setattr(par, "assemble_columns", no_columns)
        Jt = hank.getSteadyStateJacobian(ss, m, method="toeplitz").toarray()
    Jc = hank.getSteadyStateJacobian(ss, m, method="columns").toarray()
    assert Jt.shape == Jc.shape
    scale = np.max(np.abs(Jc))
    assert scale > 0.1
    err = np.max(np.abs(Jt - Jc))
    assert err < 1e-8 * scale, f"{model}: {err:.3e} vs scale {scale:.3e}"


def test_newton_on_the_wage_model_does_not_depend_on_the_jacobian_branch(hank):
    m, ss = hank_economy(200, 5, 80, "one_asset_hank_wages.yaml")
    P = m.compspec.T - 1
    ei = {"ei": 0.0025 * 0.6 ** np.arange(P)}
    x0 = np.tile(np.array([ss.vars[k] for k in hank.vars_of_type(m, "endogenous")]), P)
    xs = [hank.NewtonRaphsonHANK(x0, hank.getSteadyStateJacobian(ss, m, method=meth), ei, m, ss, ss, ε=1e-9)
          for meth in ("toeplitz", "columns")]
    lin = hank.LinearizedFunction(xs[0], ei, m, ss, ss)
    assert np.linalg.norm(lin.Fx) < 1e-8
    assert np.max(np.abs(xs[0] - xs[1])) < 1e-8


@pytest.mark.parametrize("family,n_a,n_e,T", [("ks", 50, 2, 100), ("hank", 80, 3, 40)])
def test_fake_news_het_refuses_what_fake_news_refuses(hank, family, n_a, n_e, T):
    m, ss, xhh, n_max = _setup(family, n_a, n_e, T)
    P = m.compspec.T - 1
    hb = hank.HouseholdBlock(*model_args(m))
    hb.set_boundary(ss.value, ss.D)
    for n in (0, n_max + 1):                 # outside 1..3 (Krusell-Smith) / 1..4 (one-asset HANK)
        with pytest.raises(hank.HankHIPError):
            hb.fake_news_het(n)
    with pytest.raises(hank.HankHIPError):   # no primal
        hb.fake_news_het(1)
    bump = 1.0 + 0.01 * 0.8 ** np.arange(P)
    hb.primal(xhh * bump[None, :])           # a path that varies over time
    for call in (hb.fake_news, lambda: hb.fake_news_het(n_max)):
        with pytest.raises(hank.HankHIPError):
            call()
    hb.primal(xhh)
    for n in (0, n_max + 1):
        with pytest.raises(hank.HankHIPError):
            hb.fake_news_het(n)
    F, Dv = hb.fake_news_het(n_max)
    assert np.all(np.isfinite(F)) and np.all(np.isfinite(Dv))
    hb.close()
