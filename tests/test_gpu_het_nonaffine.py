"""Heterogeneous outputs that are not affine in the policy: Value = (1+r) c^-γ (the reference's own second key, the
value_current of KrusellSmith.jl:80) and UCE = z_e c^-γ (one-asset HANK). The reference dots every key of the value function's
NamedTuple with the same post-transition D_t (BackwardIteration.jl:99-112, ForwardIteration.jl:303-307). The oracle side uses
the reference's semantics with nothing added: Value from orc_value_function (the dual ValueFunction, once per period backward),
UCE from orc_consumption_policy and dual algebra for c^-γ, each aggregated by orc_forward_iteration_het. Tolerance rel 1e-10 +
abs 1e-12 like every sweep test."""
import numpy as np
import pytest

from cases import block as _block, close as _close, hank_economy, hank_x as _hank_x, oracle_of
from conftest import ROOT, ks_paths, ks_setup

pytestmark = pytest.mark.gpu

GOODS = "one_asset_hank_goods.yaml"
_CACHE = {}


@pytest.mark.parametrize("schedule,family,N", [("launch", "launch-per-period", 5), ("xcd", "xcd-persistent", 5), ("xcd", "xcd-persistent", 40),
                                               ("wide", "on-chip-wide", 5), ("launch", "launch-per-period", 33)])
def test_value_krusell_smith_130x3(hank, schedule, family, N):
    m, ss, orc = ks_setup(130, 3, 40)
    P = 39
    x, _ = ks_paths(m, ss, "x1", 0.05)
    y = np.random.default_rng(3).standard_normal((2, P, N))
    k = min(N, 32)
    key = ("ks130", N)
    if key not in _CACHE:
        _CACHE[key] = orc.het_outputs(x[2:4], y[:, :, :k], ss.value, ss.D, 3, m.params.γ)
    oagg, odagg = _CACHE[key]
    hb = _block(hank, m, schedule)
    hb.set_boundary(ss.value, ss.D)
    agg, dagg = hb.primal_jvp(x[2:4], y)
    assert hb.info()["last_tangent_family_name"] == family
    a2, d2 = hb.het_outputs(2, y)
    with pytest.raises(hank.HankHIPError):
        hb.het_outputs(3, y)                                # not declared
    hb.set_het_outputs(3)
    a3, d3 = hb.het_outputs(3, y)
    assert a3.shape == (P, 3) and d3.shape == (P, 3, N)
    assert np.array_equal(a3[:, :2], a2) and np.array_equal(d3[:, :2, :], d2)      # outputs 0, 1 unchanged bit for bit
    for j in range(3):
        _close(a3[:, j], oagg[j])
        _close(d3[:, j, :k], odagg[j])
    # asked again: bit for bit (fixed summation order, no atomics in the extra reductions)
    a3b, d3b = hb.het_outputs(3, y)
    assert np.array_equal(a3b, a3) and np.array_equal(d3b, d3)
    if N > k:               # columns beyond the oracle's: linearity against a batch of the rest alone
        hb.primal_jvp(x[2:4], y[:, :, k:])
        _close(hb.het_outputs(3, y[:, :, k:])[1], d3[:, :, k:], 1e-11)
    # the recorded primal serves the same batch again (hank_primal_jvp's memo: the tangent sweeps alone)
    hb.primal_jvp(x[2:4], y)
    a3b, d3b = hb.het_outputs(3, y)
    _close(a3b, a3, 1e-12); _close(d3b, d3, 1e-11)
    hb.close()


@pytest.mark.parametrize("n_a,n_e,T", [(130, 3, 60), (1000, 7, 500)])
def test_value_and_uce_one_asset_hank(hank, n_a, n_e, T):
    m, ss = hank_economy(n_a, n_e, T, GOODS)
    P = m.compspec.T - 1
    x = _hank_x(ss, P)
    y = np.random.default_rng(5).standard_normal((3, P, 4))
    oagg, odagg = oracle_of(m).het_outputs(x, y, ss.value, ss.D, 4, m.params.γ)
    hb = _block(hank, m, None)
    hb.set_boundary(ss.value, ss.D)
    hb.set_het_outputs(4)
    hb.primal_jvp(x, y)
    a4, d4 = hb.het_outputs(4, y)
    for j in range(4):
        _close(a4[:, j], oagg[j])
        _close(d4[:, j, :], odagg[j])
    # oracle-independent: central differences of the device's own values along one direction
    h = 1e-6
    yd = y[:, :, 0] * np.array([1e-3, 1e-2, 1e-2])[:, None]
    hb.primal_jvp(x, yd[:, :, None])
    dY = hb.het_outputs(4, yd[:, :, None])[1][:, :, 0]
    hb.primal(x + h * yd)
    yp = hb.het_outputs(4)[0]
    hb.primal(x - h * yd)
    ym = hb.het_outputs(4)[0]
    fd = (yp - ym) / (2 * h)
    for j in (2, 3):
        err = np.max(np.abs(fd[:, j] - dY[:, j]))
        assert err <= 1e-6 * np.abs(dY[:, j]).max(), f"output {j}: central-difference error {err:.3e}"
    hb.close()


def test_value_full_size_dual_pass(hank):
    """the benched entry: KS 2000x11, T=300, N=32, the Dual pass of hank_primal_jvp under the default schedule."""
    m, ss, orc = ks_setup(2000, 11, 300)
    P = m.compspec.T - 1
    x, _ = ks_paths(m, ss, "x1", 0.05)
    y = np.random.default_rng(7).standard_normal((2, P, 32))
    hb = _block(hank, m, None)
    hb.set_boundary(ss.value, ss.D)
    hb.primal_jvp(x[2:4], y)
    a2, d2 = hb.het_outputs(2, y)
    hb.set_het_outputs(3)
    hb.primal_jvp(x[2:4], y)
    a3, d3 = hb.het_outputs(3, y)
    assert np.array_equal(a3[:, :2], a2) and np.array_equal(d3[:, :2, :], d2)
    oagg, odagg = orc.het_outputs(x[2:4], y[:, :, :4], ss.value, ss.D, 3, m.params.γ)
    _close(a3[:, 2], oagg[2])
    _close(d3[:, 2, :4], odagg[2])
    hb.close()


def test_device_pointer_form_equals_the_host_form(hank):
    import torch
    m, ss, _ = ks_setup(130, 3, 40)
    P, N = 39, 6
    x, _ = ks_paths(m, ss, "x1", 0.05)
    y = np.random.default_rng(4).standard_normal((2, P, N))
    hb = _block(hank, m, None)
    hb.set_boundary(ss.value, ss.D)
    hb.set_het_outputs(3)
    hb.primal_jvp(x[2:4], y)
    aggs, daggs = hb.het_outputs(3, y)
    dev = torch.device("cuda", 0)
    d_y = torch.from_numpy(np.asfortranarray(y).reshape(-1, order="F").copy()).to(dev)
    d_a = torch.empty(3 * P, dtype=torch.float64, device=dev)
    d_d = torch.empty(3 * P * N, dtype=torch.float64, device=dev)
    hb.het_outputs_dev(3, d_y.data_ptr(), N, d_a.data_ptr(), d_d.data_ptr())
    hb.sync()
    assert np.array_equal(d_a.cpu().numpy().reshape(P, 3, order="F"), aggs)
    assert np.array_equal(d_d.cpu().numpy().reshape(P, 3, N, order="F"), daggs)
    hb.close()


def test_declaration_semantics(hank):
    m, ss, _ = ks_setup(130, 3, 40)
    P, N = 39, 4
    x, _ = ks_paths(m, ss, "x1", 0.05)
    y = np.random.default_rng(9).standard_normal((2, P, N))
    hb = _block(hank, m, None)
    hb.set_boundary(ss.value, ss.D)
    agg, dagg = hb.primal_jvp(x[2:4], y)
    a2, d2 = hb.het_outputs(2, y)
    with pytest.raises(hank.HankHIPError) as ei:
        hb.het_outputs(3, y)
    assert ei.value.code == hank.hip.HANK_ERR_NOT_READY and "hank_set_het_outputs" in str(ei.value)
    with pytest.raises(hank.HankHIPError):
        hb.set_het_outputs(4)                       # Krusell-Smith serves three outputs
    hb.primal_jvp(x[2:4], y)
    hits = hb.stats()["primal_memo_hits"]
    assert hits >= 1
    hb.set_het_outputs(3)                           # a new declaration: the next call records its primal afresh
    hb.primal_jvp(x[2:4], y)
    assert hb.stats()["primal_memo_hits"] == hits
    a3, d3 = hb.het_outputs(3, y)
    assert np.array_equal(a3[:, :2], a2) and np.array_equal(d3[:, :2, :], d2)
    hb.set_het_outputs(2)
    agg2, dagg2 = hb.primal_jvp(x[2:4], y)
    assert np.array_equal(agg2, agg) and np.array_equal(dagg2, dagg)
    assert np.array_equal(hb.het_outputs(2, y)[0], a2) and np.array_equal(hb.het_outputs(2, y)[1], d2)
    with pytest.raises(hank.HankHIPError):
        hb.het_outputs(3, y)
    hb.close()


def test_reference_shaped_api_with_value(hank, tmp_path):
    """heterogeneous: [KD, Value], the reference's own ValueFunction return keys: ForwardIteration(BackwardIteration(...)) on the
    fused path and on the granular generic path both agree with the oracle."""
    src = (ROOT / "examples" / "krusell_smith.yaml").read_text()
    line = '    - {name: "KD", description: "capital demand (aggregate household savings)"}\n'
    assert line in src
    spec = tmp_path / "ks_value.yaml"
    spec.write_text(src.replace(line, line + '    - {name: "Value", description: "aggregate value"}\n'))
    m0, ss, orc = ks_setup(130, 3, 40)
    m = hank.build_model_from_yaml(str(spec), overrides={"T": 40, "dimensions": {"wealth": {"n": 130}, "productivity": {"n": 3}}})
    assert hank.vars_of_type(m, "heterogeneous") == ("KD", "Value")
    P, N = 39, 3
    x, Z = ks_paths(m0, ss, "x1", 0.05)
    y = np.random.default_rng(11).standard_normal((4 * P, N))
    xv = x.reshape(-1, order="F")
    xd = hank.Dual.seed(xv, y)
    from hank_amd.BackwardIteration import household_inputs
    _, dxhh = household_inputs(xd, {"Z": Z}, m)
    dxhh = np.asarray(dxhh)
    oagg, odagg = orc.het_outputs(x[2:4], dxhh, ss.value, ss.D, 3, m.params.γ)
    seqs = hank.BackwardIteration(xd, {"Z": Z}, m, ss)
    fused = hank.ForwardIteration(seqs, m, ss)
    _close(fused["Value"].v, oagg[2]); _close(fused["Value"].p, odagg[2])
    _close(fused["KD"].v, oagg[0]); _close(fused["KD"].p, odagg[0])
    generic = hank.ForwardIteration({k: list(seqs[k]) for k in ("KD", "Value")}, m, ss)
    _close(generic["Value"].v, oagg[2], 1e-9); _close(generic["Value"].p, odagg[2], 1e-9)
    # and the Float64 pass
    fv = hank.ForwardIteration(hank.BackwardIteration(xv, {"Z": Z}, m, ss), m, ss)
    _close(fv["Value"], oagg[2])


def test_fallback_mid_run_still_serves_the_extra_outputs(hank):
    """a context whose persistent sweeps fail (the HANK_XFAULT dev knob pre-sets their status word) continues on the per-period
    launches (hank_check's recovery path); outputs 2 and 3 of the call that fell back equal a launch-family context's."""
    m, ss = hank_economy(130, 3, 60, GOODS)
    P = m.compspec.T - 1
    x = _hank_x(ss, P)
    y = np.random.default_rng(6).standard_normal((3, P, 5))
    ref = _block(hank, m, "launch")
    ref.set_boundary(ss.value, ss.D)
    ref.set_het_outputs(4)
    ref.primal_jvp(x, y)
    a_ref, d_ref = ref.het_outputs(4, y)
    ref.close()
    hb = _block(hank, m, None, HANK_XFAULT="placement")
    hb.set_boundary(ss.value, ss.D)
    hb.set_het_outputs(4)
    hb.primal_jvp(x, y)
    assert hb.stats()["fallbacks"] == 1 and hb.info()["last_tangent_family_name"] == "launch-per-period"
    a4, d4 = hb.het_outputs(4, y)
    _close(a4, a_ref, 1e-13); _close(d4, d_ref, 1e-12)
    hb.close()


@pytest.mark.parametrize("inner", ["fixed_point", "krylov"])
def test_sticky_wage_hank_solves(hank, inner):
    """examples/one_asset_hank_wages.yaml: the wage Phillips curve reads UCE. Newton to 1e-8 with either inner loop and no
    fallback; the converged path's UCE is the oracle's recomputation at the converged x; a contractionary monetary shock lowers
    output and wage inflation on impact (sanity, not parity)."""
    from examples.solve_hank import solve
    from hank_amd.BackwardIteration import household_block, household_inputs
    out, x, m, ss = solve(200, 5, 80, shock=0.0025, spec="one_asset_hank_wages.yaml", inner=inner)
    assert out["residual_norm"] < 1e-8, out
    assert household_block(m).stats()["fallbacks"] == 0
    assert out["impact"]["Y"] < 0 and out["impact"]["piw"] < 0, out["impact"]
    assert abs(ss.vars["Y"] - 1.0) < 1e-8
    P = m.compspec.T - 1
    ei = {"ei": 0.0025 * 0.6 ** np.arange(P)}
    lin = hank.LinearizedFunction(x, ei, m, ss, ss)
    uce = lin.aggs[:, lin._out_idx[lin.het.index("UCE")]]
    xhh, _ = household_inputs(x, ei, m)
    oagg, _ = oracle_of(m).het_outputs(np.asarray(xhh), np.zeros((3, P, 1)), ss.value, ss.D, 4, m.params.γ)
    _close(uce, oagg[3])
