"""The Dual-pass persistent sweeps (k_xdual_back, k_xfwd<D, true>) address the record, dpol and the state through buffer
descriptors with 32-bit offsets (XRecOff, hank_xsweep.h). Addressing can go wrong where a member is short, where a group
writes several record arrays or none, where a column's offset and a row's offset meet, and in the rows of the mass point — so
every case runs hank_primal_jvp under HANK_SCHEDULE=xcd and under HANK_SCHEDULE=launch on the same inputs:
  * policies and their partials (the dpol export) bit-identical between the two;
  * the record the Dual pass wrote (s, kc, ib, A, B, u, v; lw, ig and D_t through the per-source record built from them) has no
    export of its own: a hank_jvp at that record reads every one of those arrays, and its policy partials must be the launches'
    bits too, its aggregate partials the Dual pass's to summation order;
  * aggregates and their partials, and D_t, to what tests/test_gpu_sweeps.py::test_schedules_agree allows (1e-12, 1e-11);
  * everything against the CPU oracle at 1e-10 (cases.close);
  * the call repeated on the same context (another x in between: no memo hit) returns the same bits."""
import numpy as np
import pytest

import cases
from cases import close

pytestmark = pytest.mark.gpu


def _both(hank, args, V, D, xhh, y, orc):
    N = y.shape[2]
    oagg, odagg, opol, odpol = orc.block(xhh, y, V, D)
    res = {}
    for sched in ("xcd", "launch"):
        hb = cases.raw_block(hank, args, sched)
        hb.set_boundary(V, D)
        agg, dagg = hb.primal_jvp(xhh, y)
        st = hb.stats()
        assert st["schedule"] == (1 if sched == "xcd" else 0) and st["fallbacks"] == 0, (sched, st)
        fam = hb.info()["last_tangent_family_name"]
        assert fam == cases.expected_family(sched, "dual", N), (sched, fam)
        pol, dpol, Dq = hb.policy_seq(), hb.dpolicy_seq(N), hb.dist_seq()
        dagg_rec = hb.jvp(y)                            # reads the record the Dual pass wrote
        dpol_rec = hb.dpolicy_seq(N)
        hb.primal_jvp(xhh * 1.01, y)                    # another x on record: the next call is no memo hit
        agg2, dagg2 = hb.primal_jvp(xhh, y)
        assert np.array_equal(agg2, agg) and np.array_equal(dagg2, dagg), sched + ": a repeated call"
        assert np.array_equal(hb.policy_seq(), pol) and np.array_equal(hb.dpolicy_seq(N), dpol), sched + ": a repeated call"
        assert hb.stats()["fallbacks"] == 0
        hb.close()
        what = f"{len(args[0])}x{len(args[1])} P={xhh.shape[1]} N={N} {sched}"
        close(agg, oagg, what=what + " agg"); close(dagg, odagg, what=what + " dagg")
        close(pol.transpose(2, 0, 1), opol, what=what + " policy"); close(dpol.transpose(2, 0, 1, 3), odpol, what=what + " dpolicy")
        np.testing.assert_allclose(Dq.sum(axis=(0, 1)), 1.0, rtol=0, atol=1e-12)
        close(Dq.transpose(2, 0, 1), cases.oracle_dist_seq(orc, opol, D), what=what + " D")
        close(dagg_rec, dagg, rel=1e-11, what=what + " hank_jvp at the Dual pass's record")
        res[sched] = (agg, dagg, pol, dpol, Dq, dpol_rec)
    x, l = res["xcd"], res["launch"]
    assert np.array_equal(x[2], l[2]), "policy bits"
    assert np.array_equal(x[3], l[3]), "dpol bits"
    assert np.array_equal(x[5], l[5]) and np.array_equal(x[5], x[3]), "dpol bits of hank_jvp at the record the Dual pass wrote"
    close(x[4], l[4], rel=1e-12, what="D vs launch")
    close(x[0], l[0], rel=1e-12, what="agg vs launch")
    close(x[1], l[1], rel=1e-11, what="dagg vs launch")


def _shape_case(hank, n_a, n_e, T, N):
    """cases.shape at horizon T: P = T - 1 periods (the benched T = 300 is 299 periods), y of shape (2, T - 1, N)."""
    m, V, D, xhh, orc = cases.shape(n_a, n_e, T)
    y = np.random.default_rng(7).standard_normal((2, T - 1, N))
    _both(hank, cases.model_args(m), V, D, xhh, y, orc)


@pytest.mark.parametrize("N", [1, 5, 32])
def test_short_last_member(hank, N):
    """130x3, T = 6 (P = T - 1 = 5 periods): three members, the last with 4 rows. N = 1: one group writes every record array; N = 5: D = 1
    in five groups — fewer than eight, the writer split wraps — with three dead groups; N = 32: D = 4 in all eight groups."""
    _shape_case(hank, 130, 3, 6, N)


def test_two_members_one_row_shortest_sweep(hank):
    """64x2, T = 3 (P = 2 periods, the fewest hank_jvp takes): two members, the second with one row. The forward sweep's second
    request for work units, still in its prologue, is the one past the horizon, and its first period prefetches the own row with
    the clamp min(t + 1, P - 1) active; the backward loop runs X | Y X | Y and stops."""
    _shape_case(hank, 64, 2, 3, 4)


def test_three_full_members(hank):
    """189x5, T = 12 (P = 11 periods), N = 8 (D = 1 per group): exactly three full members, no short one."""
    _shape_case(hank, 189, 5, 12, 8)


def test_borrowing_constraint_binds_in_the_lowest_columns(hank):
    """the dense-bottom grid (600x3, P = 9): 32-48 rows of the low-income column clamped at the first grid point, so the members'
    virtual rows carry mass through the forward sweep (cases.raw_economy, measured by tests/test_cases_host.py)."""
    ec = cases.raw_economy("dense-bottom")
    y = np.random.default_rng(7).standard_normal((2, cases.EDGE_P, 32))
    _both(hank, ec["args"], ec["V"], ec["D"], ec["x"], y, ec["orc"])
