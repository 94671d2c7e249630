"""Host side of the non-affine heterogeneous outputs (Value, UCE): the plugins' derived policies under the dual arithmetic,
the key check of BackwardIteration, the output indexing of LinearizedFunction and the ABI symbol. No GPU."""
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def _model(hank, spec, n_a=12, n_e=3, T=10):
    return hank.build_model_from_yaml(str(ROOT / "examples" / spec), overrides={"T": T, "dimensions": {"wealth": {"n": n_a}, "productivity": {"n": n_e}}})


@pytest.mark.parametrize("spec,inputs,keys", [("krusell_smith.yaml", ("r", "w"), ("C", "Value")),
                                              ("one_asset_hank_goods.yaml", ("r", "om", "Tr"), ("C", "Value", "UCE"))])
def test_derived_policy_dual_matches_central_differences(hank, spec, inputs, keys):
    m = _model(hank, spec)
    vf = m.value_fn
    grid = m.heterogeneity["wealth"].grid
    n_a, n_e = grid.size, m.heterogeneity["productivity"].grid.size
    rng = np.random.default_rng(1)
    base = {"r": 0.01, "w": 1.1, "om": 0.9, "Tr": 0.05}
    xv = {k: base[k] for k in inputs}
    pol = np.clip(grid[:, None] * 0.5 + 0.01 * rng.random((n_a, n_e)), grid[0], None)
    N = len(inputs) + 1
    seeds = np.eye(N)
    xd = {k: hank.Dual(xv[k], seeds[i]) for i, k in enumerate(inputs)}
    dpol = rng.standard_normal((n_a, n_e)) * 1e-2
    pd = hank.Dual(pol, np.concatenate([np.zeros((n_a, n_e, N - 1)), dpol[..., None]], axis=-1))
    h = 1e-6
    for key in keys:
        out = vf.derived_policy(key, pd, xd, m)
        assert np.array_equal(out.v, vf.derived_policy(key, pol, xv, m))
        for i, k in enumerate(inputs):
            up, dn = dict(xv), dict(xv)
            up[k] += h
            dn[k] -= h
            fd = (vf.derived_policy(key, pol, up, m) - vf.derived_policy(key, pol, dn, m)) / (2 * h)
            assert np.allclose(out.p[..., i], fd, rtol=1e-6, atol=1e-7 * np.abs(fd).max()), (key, k)
        fd = (vf.derived_policy(key, pol + h * dpol, xv, m) - vf.derived_policy(key, pol - h * dpol, xv, m)) / (2 * h)
        assert np.allclose(out.p[..., N - 1], fd, rtol=1e-6, atol=1e-7 * np.abs(fd).max()), (key, "policy")
    # the Value of the plugin is the reference's value_current (KrusellSmith.jl:80) of its own EGM step
    r = xv["r"]
    c = vf.derived_policy("C", pol, xv, m)
    assert np.allclose(vf.derived_policy("Value", pol, xv, m), (1 + r) * c ** (-m.params.γ), rtol=1e-15)
    with pytest.raises(KeyError):
        vf.derived_policy("nope", pol, xv, m)


class _StubBlock:
    """stands in for the device context: records the declarations and serves fixed per-output aggregates."""

    def __init__(self, P, G, n_a, n_e, n_hh=2):
        self.P, self.G, self.n_a, self.n_e, self.n_hh = P, G, n_a, n_e, n_hh
        self.declared = []

    def set_boundary(self, v, D):
        pass

    def set_het_outputs(self, n):
        self.declared.append(n)

    def primal(self, xhh):
        return np.full(self.P, 100.0)

    def het_outputs(self, n_het, dxhh=None):
        agg = np.stack([np.full(self.P, 100.0 + j) for j in range(n_het)], axis=1)
        dagg = None if dxhh is None else np.zeros((self.P, n_het, dxhh.shape[2]))
        return agg, dagg


def _with_het(hank, tmp_path, keys):
    src = (ROOT / "examples" / "krusell_smith.yaml").read_text()
    line = '    - {name: "KD", description: "capital demand (aggregate household savings)"}\n'
    assert line in src
    spec = tmp_path / "ks.yaml"
    src = src.replace(line, "".join(f'    - {{name: "{k}", description: "{k}"}}\n' for k in keys))
    if "KD" not in keys:        # the market-clearing equation names a listed variable instead (a toy model: only the indexing matters)
        src = src.replace('"KS = KD"', f'"KS = {keys[-1]}"')
    spec.write_text(src)
    return hank.build_model_from_yaml(str(spec), overrides={"T": 10, "dimensions": {"wealth": {"n": 8}, "productivity": {"n": 2}}})


def test_backward_iteration_accepts_value_and_keeps_the_reference_message(hank, tmp_path):
    P = 9
    x = np.tile(np.array([1.0, 3.0, 0.03, 1.2]), P)
    ss = SimpleNamespace(value=np.ones((8, 2)), D=np.full(16, 1 / 16), vars={})
    m = _with_het(hank, tmp_path, ["KD", "Value"])
    m._hip_block = _StubBlock(P, 16, 8, 2)
    seqs = hank.BackwardIteration(x, {"Z": np.ones(P)}, m, ss)           # no KeyError: Value is a key of the family
    assert set(seqs) == {"KD", "Value"}
    m2 = _with_het(hank, tmp_path, ["KD", "Bogus"])
    m2._hip_block = _StubBlock(P, 16, 8, 2)
    with pytest.raises(KeyError, match=r"value_fn return is missing key :Bogus"):
        hank.BackwardIteration(x, {"Z": np.ones(P)}, m2, ss)


@pytest.mark.parametrize("keys,n_out,col", [(["C"], 2, 1), (["Value"], 3, 2), (["KD", "Value"], 3, 2), (["KD"], 1, 0)])
def test_linearized_function_reads_the_right_output(hank, tmp_path, keys, n_out, col):
    """the column of each heterogeneous variable is its position in value_fn.outputs, also when the policy variable is not
    listed (a model with `heterogeneous: [C]` alone used to take column 0 or index past the outputs)."""
    from hank_amd.NewtonRaphson import LinearizedFunction
    P = 9
    m = _with_het(hank, tmp_path, keys)
    stub = _StubBlock(P, 16, 8, 2)
    m._hip_block = stub
    ss = SimpleNamespace(value=np.ones((8, 2)), D=np.full(16, 1 / 16), vars={k: 1.0 for k in m.variables})
    x = np.tile(np.array([1.0, 3.0, 0.03, 1.2]), P)
    lin = LinearizedFunction(x, {"Z": np.ones(P)}, m, ss, ss)
    assert lin._n_out == n_out
    assert np.array_equal(lin.aggs[:, lin._out_idx[-1]], np.full(P, 100.0 + col))
    assert (n_out > 2) == (n_out in stub.declared)


def test_abi_lists_the_declaration_entry(hank):
    import hank_amd
    assert "hank_set_het_outputs" in hank_amd.hip.ABI_SYMBOLS


def test_host_steady_state_serves_uce(hank):
    """the host steady-state path (vfi="host") fills every listed key the host EGM step does not return — UCE — from the policy,
    as the device path does: the sticky-wage model's steady state reaches Y = 1 at the calibrated disutility of hours."""
    from hank_amd import OneAssetHANK as oa
    m = _model(hank, "one_asset_hank_wages.yaml", n_a=60, n_e=3, T=20)
    m.params.B = oa.calibrate_bond_supply(m)
    m.params.vφ = oa.calibrate_disutility(m)
    ss, _ = hank.get_SteadyStates(m, vfi="host")
    assert abs(ss.vars["Y"] - 1.0) < 1e-8 and abs(ss.vars["piw"]) < 1e-10
    c = m.value_fn.derived_policy("C", ss.policies["A"], ss.vars, m)
    z = m.heterogeneity["productivity"].grid
    uce = float((z[None, :] * c ** (-m.params.γ)).reshape(-1, order="F") @ ss.D)
    assert abs(ss.vars["UCE"] - uce) < 1e-10 * uce
