"""The forward Dual-pass sweep's mixing loop and state-row index (k_xfwd<4, ...> in hank_xsweep.h) at every shape they take.

xtile_mix takes its first column by itself (the peeled first term), the others in trips of U = 5 columns and what is left one
column at a time; k_xfwd<D, true> sets a unit's state-row index `(j / 63) * 64 + j % 63` with the unit's record (`qrow`, set by
load_rec) and loads the state rows unconditionally. So the cases are

  n_e = 1       the first term only, neither loop entered
  n_e = 2       one single-column trip
  n_e = 5       four single-column trips, no whole one (a build with four columns per trip: exactly one, none left over)
  n_e = 6       exactly one whole trip, none left over
  n_e = 9       one whole trip and three single columns (four columns per trip: two, none left over)
  n_e = 11      two whole trips, none left over: the benched shape

on wealth grids that walk the row index — n_a = 63 (one member), 64 (a second member that holds one row: j = 63 is row 64 of the
column), 130 (three members, the last with four rows) — at the batch widths N = 17 and 32, which both run the D = 4 instances
(four and five tile slots: hank_primal + hank_jvp runs k_xfwd<4, false>, hank_primal_jvp k_xfwd<4, true>); N = 17 leaves the
last group one direction. T = 6, forced HANK_SCHEDULE=xcd, both entry points, against the launches at 1e-12 (policy partials
bit for bit) and against the CPU oracle at rel 1e-10 + abs 1e-12 (cases.against_oracle_and_launches, cases.close).

The lanes of a virtual row and the units of more than 64 sources (the `i0 = 64` trips of load_rec / load_state) need a clamped
prefix and a crowded target row, which these calibrated shapes do not have: this module relies on tests/test_gpu_fwd_edges.py
for them (deep-prefix, swing and collapse at N = 40, whose first pass is D = 4) and is meant to be run together with it."""
import pytest

import cases
from cases import FAMILY, against_oracle_and_launches

pytestmark = pytest.mark.gpu

T = 6
NS = (17, 32)
N_E = (1, 2, 5, 6, 9, 11)
N_A = (63, 64, 130)


def _shape(n_a, n_e):
    return cases.shape_one_column(n_a, T) if n_e == 1 else cases.shape(n_a, n_e, T)


@pytest.mark.parametrize("n_a", N_A)
@pytest.mark.parametrize("n_e", N_E)
def test_mixing_loop_and_row_index(hank, n_e, n_a):
    """both entry points at N = 17 and 32 under the forced persistent schedule: the oracle, the launches, the family that served
    every sweep (asserted per sweep by against_oracle_and_launches), no fallback, schedule 1."""
    seen = against_oracle_and_launches(hank, _shape(n_a, n_e), [("xcd", {})], NS)
    assert len(seen) == 1
    for sched, env, st, info in seen:
        assert st["schedule"] == 1 and st["fallbacks"] == 0, (n_a, n_e, st)
        assert info["last_tangent_family_name"] == FAMILY["xcd"], (n_a, n_e, info)
