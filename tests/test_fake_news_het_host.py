"""getSteadyStateJacobian(method="toeplitz") for a model with more than one heterogeneous variable, without a GPU: the household
block is a stub that serves fake-news matrices per output. The toeplitz branch must ask for every output up to the last listed
key at once (hank_fake_news_het), never take the unit-tangent columns, and place each key's own household Jacobian."""
import numpy as np
import pytest

from conftest import ROOT

_SS = {}


class _Block:
    """F (P, P, n_hh, n), Dv (P, n_hh, n): output o from its own seed, the same whichever entry serves it."""

    def __init__(self, n_hh, P, calls):
        self.n_hh, self.P, self.calls = n_hh, P, calls

    def _out(self, o):
        rng = np.random.default_rng(100 + o)
        return rng.standard_normal((self.P, self.P, self.n_hh)), rng.standard_normal((self.P, self.n_hh))

    def fake_news(self):
        self.calls.append(("fake_news", 1))
        return self._out(0)

    def fake_news_het(self, n):
        self.calls.append(("fake_news_het", n))
        outs = [self._out(o) for o in range(n)]
        return np.stack([f for f, _ in outs], axis=-1), np.stack([d for _, d in outs], axis=-1)


def _stub_lin(calls):
    from hank_amd.GeneralStructures import vars_of_type

    class _Lin:
        def __init__(self, x, exog, model, ss_initial, ss_ending):
            self.het = vars_of_type(model, "heterogeneous")
            outs = tuple(model.value_fn.outputs)
            self._out_idx = [outs.index(k) for k in self.het]
            self._n_out = 1 + max(self._out_idx)
            self.hb = _Block(len(model.value_fn.household_inputs), model.compspec.T - 1, calls)

    return _Lin


def _models(hank, tmp_path):
    src = (ROOT / "examples" / "krusell_smith.yaml").read_text()
    line = '    - {name: "KD", description: "capital demand (aggregate household savings)"}\n'
    assert line in src
    ov = {"T": 12, "dimensions": {"wealth": {"n": 30}, "productivity": {"n": 2}}}
    out = {}
    for name, text in (("kd", src), ("kd_value", src.replace(line, line + '    - {name: "Value", description: "aggregate value"}\n'))):
        spec = tmp_path / f"{name}.yaml"
        spec.write_text(text)
        m = hank.build_model_from_yaml(str(spec), overrides=ov)
        if name not in _SS:
            _SS[name] = hank.get_SteadyStates(m, vfi="host")[0]
        out[name] = (m, _SS[name])
    return out


def test_multi_output_model_takes_every_output_from_one_call(hank, tmp_path, monkeypatch):
    import hank_amd.SteadyStateJacobian as ssj
    import hank_amd.parallel as par
    models = _models(hank, tmp_path)
    calls = []
    monkeypatch.setattr(ssj, "LinearizedFunction", _stub_lin(calls))

    def no_columns(*a, **k):
        raise AssertionError("the toeplitz J̅ took the unit-tangent column path")

    monkeypatch.setattr(par, "assemble_columns", no_columns)
    m1, ss1 = models["kd"]
    J1 = ssj.getSteadyStateJacobian(ss1, m1, method="toeplitz").toarray()
    assert calls == [("fake_news", 1)]                 # one heterogeneous key, the policy variable: hank_fake_news as before
    m2, ss2 = models["kd_value"]
    assert hank.vars_of_type(m2, "heterogeneous") == ("KD", "Value")
    J2 = ssj.getSteadyStateJacobian(ss2, m2, method="toeplitz").toarray()
    assert calls[1:] == [("fake_news_het", 3)]         # KD, C, Value: up to the last listed output
    # Value enters no equation: the KD block is output 0's, as in the one-key model
    assert J1.shape == J2.shape
    assert np.max(np.abs(J1)) > 0
    assert np.array_equal(J1, J2)


def test_each_key_gets_its_own_household_jacobian(hank, tmp_path, monkeypatch):
    """the same model with its household outputs relabelled: if the loop over keys reused output 0's Jacobian for every key,
    swapping which output KD reads would not move J̅."""
    import hank_amd.SteadyStateJacobian as ssj
    models = _models(hank, tmp_path)
    m, ss = models["kd_value"]
    calls = []
    monkeypatch.setattr(ssj, "LinearizedFunction", _stub_lin(calls))
    J0 = ssj.getSteadyStateJacobian(ss, m, method="toeplitz").toarray()

    class _Swapped(_Block):          # KD's Jacobian now comes from seed 102, Value's from 100
        def _out(self, o):
            return super()._out({0: 2, 2: 0}.get(o, o))

    Lin = _stub_lin(calls)

    class _LinSwapped(Lin):
        def __init__(self, *a):
            super().__init__(*a)
            self.hb = _Swapped(self.hb.n_hh, self.hb.P, calls)

    monkeypatch.setattr(ssj, "LinearizedFunction", _LinSwapped)
    Js = ssj.getSteadyStateJacobian(ss, m, method="toeplitz").toarray()
    assert np.max(np.abs(Js - J0)) > 1e-3
