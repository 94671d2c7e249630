"""The dense reference of hank_fake_news[_het] (tests/fake_news_refs.py) pinned on the CPU: `household_jacobian` of the dense F and
Dv against the oracle's unit-tangent `het_outputs` on the P-period constant path — the check the older GPU tests make of the device,
made of the reference instead. Every input and output, the columns [0, 1, P//2, P-2, P-1] and, at the smallest P, every column,
under `cases.close` (rel 1e-10 + abs 1e-12 of a slab's largest entry). The largest relative figure per economy is printed: it is
the reference's own error and what tests/test_gpu_fake_news_dense.py's tolerance leaves room for. Measured: ks30x3 3.3e-13,
hank30x3 1.9e-13, ks40x16 9.3e-13 at worst: 100 to 500 times inside the bound, all below a tenth of it."""
import numpy as np
import pytest

import cases
import fake_news_refs as R
import ss_diff_cases as S

PINS = (("ks30x3", 20), ("hank30x3", 33), ("ks40x16", 12))


def _columns(P, every):
    return list(range(P)) if every else sorted({0, 1, P // 2, P - 2, P - 1})


@pytest.mark.parametrize("name,P", PINS)
def test_dense_reference_against_the_oracle_s_unit_tangents(name, P):
    from hank_amd.SteadyStateJacobian import household_jacobian
    c = S.case(name)
    n_hh, n_het = len(c["x"]), c["n_het"]
    cols = _columns(P, every=P == min(p for _, p in PINS))
    y = np.zeros((n_hh, P, n_hh * len(cols)))
    for q, s_ in enumerate(cols):
        for k in range(n_hh):
            y[k, s_, q * n_hh + k] = 1.0
    xhh = R.constant_path(c, P)
    dagg = np.concatenate([c["orc"].het_outputs(xhh, y[:, :, c0:c0 + 32], c["V"], c["D"], n_het, c["gamma"])[1]
                           for c0 in range(0, y.shape[2], 32)], axis=2)           # (n_het, P, n_hh len(cols))
    F, Dv = R.dense_fake_news(c, P, n_het)
    assert F.shape == (P, P, n_hh, n_het) and Dv.shape == (P, n_hh, n_het)
    worst = 0.0
    for o in range(n_het):
        J = household_jacobian(F[..., o], Dv[..., o])                            # (n_hh, P, P)
        for k in range(n_hh):
            got, ref = J[k][:, cols], dagg[o][:, k::n_hh]
            assert np.abs(ref).max() > 1e-6, (name, o, k)
            worst = max(worst, np.max(np.abs(got - ref)) / np.abs(ref).max())
            cases.close(got, ref, what=f"{name} P={P} output {o} input {k}, columns {cols if len(cols) < P else 'all'}")
    print(f"{name} P={P}: the dense reference sits {worst:.2e} of a slab's largest entry from the oracle's unit tangents at worst (close's bound: 1e-10)")
    assert worst <= 1e-11, "the reference alone takes more than a tenth of the bound the GPU module gives the device"


def test_shapes_of_the_gpu_module_are_the_economies():
    """SHAPES names economies ECONOMIES sizes; ks64x4 serves the fake-news module alone"""
    assert {n for n, _ in R.SHAPES} == set(R.ECONOMIES)
    assert "ks64x4" in S._KS_SHAPE and "ks64x4" not in S.NAMES
    assert all(P >= 2 for _, P in R.SHAPES)
