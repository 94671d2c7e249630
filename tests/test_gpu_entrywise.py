"""The step kernels entry by entry, on the MI355X, against tests/ld_refs.py: an extended-precision restatement of the step and the
running error bound of the float64 kernel (each operation 2^-53, the fast reciprocal / root and pow 2 ulps, a sum of n terms
(n - 1) 2^-53 sum|terms|). Where `cases.close` scales by the array's largest entry and sits five decades above the arithmetic,
`cases.within` asks |kernel - reference| <= bound at EVERY entry: a thin row of D, the marginal value of the richest row, a partial
that is small. The inputs are exact (float64 arrays both sides read), their preconditions and the oracle's place inside the same
bound are tests/test_ld_refs_host.py's; figures of the committed run: profiles/entrywise.log.

A. hank_backward_step[_dual]: k_egm_X, k_egm_Y, k_tan_X, k_tan_Y — and with them egm_X / egm_Y / egm_Y_finish / pow_crra / diet_kc /
   diet_v / fast_rcp / fast_rsqrt / fast_sqrt, which every primal kernel shares (the sweeps are pinned to these bits elsewhere);
B. hank_forward_step[_dual]: k_scatter_general, k_mix_general, k_colsum;
C. the sweeps' D_t and agg_t under every schedule: D_0 pushed in long double through the context's OWN exported policy bits (exact
   inputs again), the bound compounding over the periods."""
import numpy as np
import pytest

import cases
from cases import ENTRY_BACKWARD, ENTRY_CASES, ENTRY_FORWARD, raw_block, within

pytestmark = pytest.mark.gpu

BACKWARD = ENTRY_BACKWARD


@pytest.mark.parametrize("family,name,n_a,n_e", BACKWARD)
def test_backward_step_entrywise(hank, family, name, n_a, n_e):
    gamma, diet_env, diet = ENTRY_CASES[name]
    c = cases.entry_backward(family, gamma, n_a, n_e)
    refs = cases.entry_refs(c, diet)
    hb = raw_block(hank, c["args"], None, HANK_RECORD_DIET=diet_env)
    assert hb.info()["record_diet"] == diet and hb.n_hh == len(c["steps"][0][0])
    for k, ((x, dx), R) in enumerate(zip(c["steps"], refs)):
        what = f"gpu {family} {name} {n_a}x{n_e} prices{k}"
        Vo, Po = hb.backward_step(c["V"], x)
        Vd, dVo, Pd, dPo = hb.backward_step_dual(c["V"], c["dV"], x, dx)
        assert np.array_equal(Vo, Vd) and np.array_equal(Po, Pd), what
        amb = R["ambiguous"]
        for q, o in (("V", Vo), ("policy", Po), ("dV", dVo), ("dpolicy", dPo)):
            within(o, R[q].v, R[q].bound(), f"{what} {q}", amb)
        # exact outcomes, asserted on their own: the limit where it binds, the end values outside the knots, zero partials there
        con, lo, hi = R["constrained"] & ~amb, R["below"] & ~amb, R["above"] & ~amb
        assert np.all(Po[con] == c["bc"]) and np.all(dPo[con] == 0.0), what
        assert np.all(Po[lo] == max(c["a"][0], c["bc"])) and np.all(Po[hi] == c["a"][-1]) and np.all(dPo[lo | hi] == 0.0), what
    hb.close()


@pytest.mark.parametrize("name", ENTRY_FORWARD)
def test_forward_step_entrywise(hank, name):
    c, R = cases.entry_forward(name), cases.entry_forward_ref(name)
    hb = hank.HouseholdBlock(*c["args"])
    Do, dDo, agg, dagg = hb.forward_step_dual(c["policy"], c["dpolicy"], c["D"], c["dD"])
    D1, agg1 = hb.forward_step(c["policy"], c["D"])
    hb.close()
    amb, what = R["ambiguous"], f"gpu forward {name}"
    within(Do, R["D"].v, R["D"].bound(), f"{what} D", amb)
    within(dDo, R["dD"].v, R["dD"].bound(), f"{what} dD", amb)
    within(agg, R["agg"].v, R["agg"].bound(), f"{what} agg")
    within(dagg, R["dagg"].v, R["dagg"].bound(), f"{what} dagg")
    within(D1, R["D"].v, R["D"].bound(), f"{what} D (hank_forward_step)", amb)
    within(agg1, R["agg"].v, R["agg"].bound(), f"{what} agg (hank_forward_step)")
    assert np.all(Do[R["mass"] == 0] == 0.0)
    # mass: |sum D_new - 1| within the sum's tracked bound, and the sum against the reference's own (which misses 1 by what the
    # normalised D_prev and Pi's rows miss it: printed)
    total, b = np.longdouble(Do.sum()), float(R["total"].bound())
    print(f"{what}: |sum D_new - 1| {float(abs(total - 1)):.2e}, |sum D_new - reference's| {float(abs(total - R['total'].v)):.2e}, "
          f"bound {b:.2e}; the reference's sum misses 1 by {float(abs(R['total'].v - 1)):.2e}")
    assert abs(total - 1) <= b and abs(total - R["total"].v) <= b


def _sweep_case(econ):
    if econ == "shape-130x3":
        m, V, D, xhh, _ = cases.shape(130, 3, 12)
        return cases.model_args(m), m.heterogeneity["wealth"].grid, np.asarray(m.heterogeneity["productivity"].transition), V, D, xhh
    e = cases.raw_economy(econ)
    return e["args"], e["grid"], e["Pi"], e["V"], e["D"], e["x"]


_PUSH = {}


@pytest.mark.parametrize("econ", ["shape-130x3", "dense-bottom", "deep-prefix", "swing"])
def test_sweeps_distribution_entrywise(hank, econ):
    """dist_seq() and agg_t of hank_primal under the launch, persistent and default schedules: every entry of every period inside the
    compounding bound. swing: more than 64 sources on one target row; deep-prefix: a clamped prefix over several members."""
    args, grid, Pi, V, D0, xhh = _sweep_case(econ)
    P = xhh.shape[1]
    for sched in ("launch", "xcd", None):
        hb = raw_block(hank, args, sched)
        hb.set_boundary(V, D0)
        agg = hb.primal(xhh)
        pol, Dq, st = hb.policy_seq(), hb.dist_seq(), hb.stats()
        hb.close()
        assert st["fallbacks"] == 0 and st["schedule"] == {"launch": 0, "xcd": 1, None: 2}[sched], (econ, sched, st)
        key = (econ, pol.tobytes())                      # the schedules agree on the policy's bits: one reference serves them
        if key not in _PUSH:
            _PUSH[key] = cases.push_distribution(grid, Pi, pol, D0)
        push = _PUSH[key]
        rD, bD = np.stack([R["D"].v for R in push], axis=2), np.stack([R["D"].bound() for R in push], axis=2)
        amb = np.stack([R["ambiguous"] for R in push], axis=2)
        within(Dq, rD, bD, f"gpu sweep {econ} {sched} D_t (t = 1..{P})", amb)
        within(agg, np.stack([R["agg"].v for R in push]), np.stack([R["agg"].bound() for R in push]), f"gpu sweep {econ} {sched} agg_t")
        peak = rD.max(axis=(0, 1))
        print(f"gpu sweep {econ} {sched}: smallest positive D_t entry {float(rD[rD > 0].min()):.1e} under a peak of {float(peak.max()):.1e}; "
              f"bound / mass at most {max(float(np.max(R['D'].bound()[R['mass'] > 0] / R['mass'][R['mass'] > 0])) for R in push):.2e}")
    assert len([k for k in _PUSH if k[0] == econ]) == 1, "the schedules disagree on the policy's bits"
