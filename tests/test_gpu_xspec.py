"""The Dual pass's backward sweep has instances compiled for the model's constants (k_xdual_back<D, 768, NE, CRRA>, hank_xsweep.h;
the rule that chooses: hank_xspec.h, tests/test_xspec_host.py). A compiled-in constant must change no bit: every case runs
hank_primal_jvp under HANK_SCHEDULE=xcd on two contexts, a specialised one (HANK_XSPEC=1: both halves; unset: what the library ships
with, the CRRA half alone; ne, crra: one half) and HANK_XSPEC=0 (the generic instances), and
  * hank_sweep_instance names the expected instance in each (a dispatch that compared generic with generic would pass the rest);
  * aggregates, their partials, policies, their partials and D_t are the same bits in both, and so are the policy partials of a
    hank_jvp at the record the Dual pass wrote (it reads s, kc, ib, A, B, u and v);
  * the specialised context's results pass cases.close against the CPU oracle;
  * no fallback.
The shapes are the smallest at which each instance's code is reached (n_e = 4, 7, 11 at D = 1 and D = 4, a short last member, a
member of one row, an n_e without an instance); other curvatures and a record diet switched off keep NE and drop CRRA; a negative
terminal value raises the same DomainError at the same place from both."""
import numpy as np
import pytest

import cases
from cases import close

pytestmark = pytest.mark.gpu


def _run(hank, args, V, D, xhh, y, xspec, **env):
    N = y.shape[2]
    hb = cases.raw_block(hank, args, "xcd", HANK_XSPEC=xspec, **env)
    try:
        hb.set_boundary(V, D)
        agg, dagg = hb.primal_jvp(xhh, y)
        inst = hb.sweep_instance()
        st = hb.stats()
        assert st["schedule"] == 1 and st["fallbacks"] == 0, (xspec, st)
        assert hb.info()["last_tangent_family_name"] == cases.expected_family("xcd", "dual", N)
        pol, dpol, Dq = hb.policy_seq(), hb.dpolicy_seq(N), hb.dist_seq()
        hb.jvp(y)                                       # reads the record the Dual pass wrote
        dpol_rec = hb.dpolicy_seq(N)
        assert hb.stats()["fallbacks"] == 0
    finally:
        hb.close()
    return inst, {"agg": agg, "dagg": dagg, "policy_seq": pol, "dpolicy_seq": dpol, "dist_seq": Dq, "dpolicy_seq of hank_jvp at the record": dpol_rec}


def _pair(hank, args, V, D, xhh, N, orc, expect, knob="1", **env):
    """both contexts on one input; knob = HANK_XSPEC of the specialised one (None: unset), expect = its (NE, CRRA)."""
    y = np.random.default_rng(7).standard_normal((2, xhh.shape[1], N))
    inst1, r1 = _run(hank, args, V, D, xhh, y, knob, **env)
    inst0, r0 = _run(hank, args, V, D, xhh, y, "0", **env)
    print("instances:", inst1, inst0)
    assert inst1 == {"back": expect, "fwd": (0, 0)}, inst1             # (the forward sweep has no such instance)
    assert inst0 == {"back": (0, 0), "fwd": (0, 0)}, inst0
    for k in r1:
        assert np.array_equal(r1[k], r0[k]), f"{k}: the specialised instance's bits differ from the generic one's ({np.max(np.abs(r1[k] - r0[k])):.3e})"
    oagg, odagg, opol, odpol = orc.block(xhh, y, V, D)
    what = f"{len(args[0])}x{len(args[1])} P={xhh.shape[1]} N={N} gamma={args[4]}"
    close(r1["agg"], oagg, what=what + " agg"); close(r1["dagg"], odagg, what=what + " dagg")
    close(r1["policy_seq"].transpose(2, 0, 1), opol, what=what + " policy"); close(r1["dpolicy_seq"].transpose(2, 0, 1, 3), odpol, what=what + " dpolicy")
    close(r1["dist_seq"].transpose(2, 0, 1), cases.oracle_dist_seq(orc, opol, D), what=what + " D")


@pytest.mark.parametrize("n_a,n_e,T,N,expect", [
    (130, 4, 6, 1, (4, 1)),        # D = 1, one group writes every record array; three members, the last with 4 rows
    (130, 4, 6, 5, (4, 1)),        # D = 1 in five groups, the writer split wraps
    (130, 4, 6, 32, (4, 1)),       # D = 4 in eight groups
    (130, 7, 6, 8, (7, 1)),
    (130, 11, 6, 32, (11, 1)),     # the bench's block of 768 threads, D = 4
    (190, 11, 12, 4, (11, 1)),     # one live group, D = 4; three full members and a member of one row
    (130, 3, 6, 5, (0, 1)),        # no NE instance
])
def test_specialised_instance_returns_the_generic_bits(hank, n_a, n_e, T, N, expect):
    m, V, D, xhh, orc = cases.shape(n_a, n_e, T)
    _pair(hank, cases.model_args(m), V, D, xhh, N, orc, expect)


@pytest.mark.parametrize("knob,n_e,N,expect", [
    (None, 11, 32, (0, 1)),        # what the library ships with, at the bench's block: k_xdual_back<4, 768, 0, 1>
    (None, 11, 16, (0, 1)),        # D = 2
    (None, 4, 5, (0, 1)),          # D = 1, the writer split wraps
    ("crra", 11, 32, (0, 1)),
    ("crra", 7, 16, (0, 1)),       # D = 2
    ("ne", 11, 32, (11, 0)),       # NE alone at gamma = 2: the generic powers on 11 literal columns
    ("ne", 11, 16, (11, 0)),       # D = 2
    ("ne", 4, 1, (4, 0)),
])
def test_each_half_alone_and_the_shipped_default_return_the_generic_bits(hank, knob, n_e, N, expect):
    m, V, D, xhh, orc = cases.shape(130, n_e, 6)
    _pair(hank, cases.model_args(m), V, D, xhh, N, orc, expect, knob=knob)


@pytest.mark.parametrize("gamma", [1.0, 1.5, 3.0])
@pytest.mark.parametrize("n_e,N", [(4, 8), (11, 32)])
def test_other_curvatures_keep_ne_and_the_generic_powers(hank, n_e, N, gamma):
    """cases.shape's constructor arguments and boundary, gamma replaced, the oracle at the same gamma (gamma = 1 keeps the record
    diet, gamma = 1.5 and 3 read kc and v; 11 columns at D = 4 is the instance whose mixing keeps its step-by-step form)."""
    from oracle.oracle import Oracle
    m, V, D, xhh, _ = cases.shape(130, n_e, 6)
    args = list(cases.model_args(m))
    args[4] = gamma
    _pair(hank, tuple(args), V, D, xhh, N, Oracle(*args[:6]), (n_e, 0))


def test_record_diet_off_keeps_the_generic_powers(hank):
    m, V, D, xhh, orc = cases.shape(130, 4, 6)
    _pair(hank, cases.model_args(m), V, D, xhh, 8, orc, (4, 0), HANK_RECORD_DIET=0)


def test_domain_error_is_raised_where_the_generic_instance_raises_it(hank):
    """one negative entry of V_T, small enough that E = Pi V_T turns negative in ONE column of that row only: beta E < 0 under the
    power -1/2 in the last period's X half. Both instances report it through the call's status, at the same place."""
    m, V, D, xhh, _ = cases.shape(130, 4, 6)
    args = cases.model_args(m)
    Pi, P = np.asarray(args[2]), xhh.shape[1]
    a0, e0 = 70, 2
    # E[e] = Pi[e, e0] * (-x) + rest[e] < 0  <=>  x > rest[e] / Pi[e, e0]: x between the two smallest thresholds
    rest = Pi @ V[a0] - Pi[:, e0] * V[a0, e0]
    th = np.sort(rest / Pi[:, e0])
    assert np.all(Pi[:, e0] > 0) and th[0] > 0 and th[1] > th[0] * 1.01
    Vn = V.copy()
    Vn[a0, e0] = -0.5 * (th[0] + th[1])
    E = Pi @ Vn[a0]
    assert (E < 0).sum() == 1 and ((Vn @ Pi.T) < 0).sum() == 1
    e_star = int(np.argmin(E))
    y = np.random.default_rng(7).standard_normal((2, P, 8))
    seen = {}
    for xspec, inst in (("1", (4, 1)), (None, (0, 1)), ("0", (0, 0))):
        hb = cases.raw_block(hank, args, "xcd", HANK_XSPEC=xspec)
        try:
            hb.set_boundary(Vn, D)
            with pytest.raises(hank.DomainError) as ei:
                hb.primal_jvp(xhh, y)
            assert hb.sweep_instance()["back"] == inst
            assert hb.stats()["fallbacks"] == 0
        finally:
            hb.close()
        seen[xspec] = (ei.value.code, str(ei.value))
        print(xspec, seen[xspec])
    assert seen["1"] == seen["0"] and seen[None] == seen["0"]
    assert f"(period {P}, productivity state {e_star + 1}, wealth index {a0 + 1})" in seen["1"][1]
