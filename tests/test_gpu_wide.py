"""The on-chip wide sweeps (csrc/hank_wide.h: one workgroup per tangent direction, the loop-carried state in registers) through the
C ABI: the partials of BackwardIteration.jl:90-113 / ForwardIteration.jl:297-308 against the CPU oracle (rel 1e-10 + abs 1e-12, the
tolerance of every sweep test) and against the per-period launches, at ragged shapes, both value-function families, odd grids,
batches wider than the chip, and the schedule's own choice."""
import numpy as np
import pytest

from cases import block as _block, close, hank_economy, hank_x, oracle_of, raw_block
from conftest import ks_paths, ks_setup

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n_a,n_e,T,N", [(50, 2, 20, 4), (130, 3, 20, 5), (30, 3, 25, 1), (50, 2, 60, 33), (500, 4, 300, 8)])
def test_wide_sweeps_against_the_oracle_and_the_launches(hank, n_a, n_e, T, N):
    m, ss, orc = ks_setup(n_a, n_e, T)
    P = T - 1
    x, _ = ks_paths(m, ss, "x1", 0.05)
    y = np.random.default_rng(0).standard_normal((2, P, N))
    k = min(N, 32)
    oagg, odagg, _, odpol = orc.block(x[2:4], y[:, :, :k], ss.value, ss.D)
    hb = _block(hank, m, "wide")
    hb.set_boundary(ss.value, ss.D)
    agg, dagg = hb.primal_jvp(x[2:4], y)
    assert hb.info()["last_tangent_family_name"] == "on-chip-wide"
    dpol = hb.dpolicy_seq(N)
    close(agg, oagg); close(dagg[:, :k], odagg)
    close(dpol.transpose(2, 0, 1, 3)[..., :k], odpol)
    assert np.array_equal(hb.jvp(y), dagg)                      # fixed summation order: bit for bit
    hl = _block(hank, m, "launch")
    hl.set_boundary(ss.value, ss.D)
    aggl, daggl = hl.primal_jvp(x[2:4], y)
    close(dagg, daggl, 1e-12); close(dpol, hl.dpolicy_seq(N), 1e-12)
    hb.close(); hl.close()


def test_wide_sweeps_odd_grid_and_a_batch_wider_than_the_chip(hank):
    """n_a odd (a half-filled row pair at the top of the grid) and more directions than CUs (workgroups are independent: the
    hardware runs them in rounds); linearity in the tangent."""
    m, ss, orc = ks_setup(51, 3, 16)
    P, N = 15, 300
    x, _ = ks_paths(m, ss, "x1", 0.05)
    y = np.random.default_rng(3).standard_normal((2, P, N))
    hb = _block(hank, m, "wide")
    hb.set_boundary(ss.value, ss.D)
    agg, dagg = hb.primal_jvp(x[2:4], y)
    oagg, odagg, _, odpol = orc.block(x[2:4], y[:, :, :8], ss.value, ss.D)
    close(agg, oagg); close(dagg[:, :8], odagg)
    close(hb.dpolicy_seq(N).transpose(2, 0, 1, 3)[..., :8], odpol)
    hl = _block(hank, m, "launch")
    hl.set_boundary(ss.value, ss.D)
    close(dagg, hl.primal_jvp(x[2:4], y)[1], 1e-12)
    c = np.random.default_rng(4).standard_normal(N)
    comb = hb.jvp(np.tensordot(y, c, axes=([2], [0]))[:, :, None])[:, 0]
    close(comb, dagg @ c, 1e-9)
    hb.close(); hl.close()


def test_wide_sweeps_one_asset_hank_family(hank):
    """three household inputs (r, w, transfer): the wide sweeps against the launches and the oracle's restatement of the family."""
    m, ss = hank_economy(130, 3, 30)
    P, N = 29, 6
    x = hank_x(ss, P)
    y = np.random.default_rng(5).standard_normal((3, P, N))
    hb = _block(hank, m, "wide")
    hb.set_boundary(ss.value, ss.D)
    agg, dagg = hb.primal_jvp(x, y)
    assert hb.info()["last_tangent_family_name"] == "on-chip-wide"
    hl = _block(hank, m, "launch")
    hl.set_boundary(ss.value, ss.D)
    aggl, daggl = hl.primal_jvp(x, y)
    close(agg, aggl, 1e-12); close(dagg, daggl, 1e-12)
    close(dagg, oracle_of(m).block(x, y, ss.value, ss.D)[1])
    hb.close(); hl.close()


def test_default_schedule_sends_full_rounds_to_the_wide_sweeps(hank):
    """auto: a batch of at least 80 directions goes to the on-chip wide sweeps (a round of them costs what 80 directions cost the
    per-period launches since the L2 warming of round 5: DESIGN.md section 4), a narrower one does not; a forced schedule keeps its
    one implementation."""
    m, ss, _ = ks_setup(50, 2, 20)
    P = 19
    x, _ = ks_paths(m, ss, "x1", 0.05)
    hb = _block(hank, m, None)
    hb.set_boundary(ss.value, ss.D)
    info = hb.info()
    assert info["wide_supported"] == 1 and info["wide_mode"] == 1
    for N, fam in ((256, "on-chip-wide"), (32, "xcd-persistent"), (72, "launch-per-period"), (120, "on-chip-wide"), (300, "on-chip-wide"), (512, "on-chip-wide")):
        y = np.random.default_rng(N).standard_normal((2, P, N))
        agg, dagg = hb.primal_jvp(x[2:4], y)
        assert hb.info()["last_tangent_family_name"] == fam, (N, hb.info())
        if N == 256:
            keep = (y, dagg)
    # the same batch on the launches: equal to rounding
    hl = _block(hank, m, "launch")
    hl.set_boundary(ss.value, ss.D)
    assert hl.info()["wide_mode"] == 0
    close(keep[1], hl.primal_jvp(x[2:4], keep[0])[1], 1e-12)
    hb.close(); hl.close()


def test_wide_sweeps_refuse_what_they_cannot_hold(hank):
    """a horizon whose per-period inputs do not fit LDS, or a productivity grid that is not instantiated: auto keeps the other
    families, a forced `wide` fails at hank_create with the reason. What the default schedule then runs at 129 and 256 directions —
    the per-period launches with 4 backward row groups — is tests/test_gpu_launch_lanes.py's."""
    args = (np.linspace(0.0, 50.0, 40), np.linspace(0.5, 1.5, 6), np.full((6, 6), 1.0 / 6.0), 0.98, 2.0, 0.0, 12)
    hb = raw_block(hank, args, None)
    assert hb.info()["wide_supported"] == 0 and hb.info()["wide_mode"] == 0
    hb.close()
    with pytest.raises(hank.HankHIPError, match="wide"):
        raw_block(hank, args, "wide")
