"""The per-source record {w, ig D_{t-1}} (R.lwg) behind a persistent Dual pass.

The Dual pass's forward half (k_xfwd<D >= 1, true>) does not write that record: nothing of a Dual pass reads it. Whoever reads
it next — a tangent sweep of any family at the recorded primal, hank_fake_news[_het] — has it built first, once, by k_xlwg_build
from what the pass left behind (k_lottery's w and ig, D_t, the mass on the members' virtual rows). The builder repeats the
arithmetic of the Float64 sweep's writer (k_xfwd<0, true>, hank_primal) operand by operand — row 0 of an open column is member
0's own part plus the butterfly sum of the virtual rows — so every comparison below is BIT FOR BIT: a record made by the Dual
pass and the builder against the record hank_primal writes at the same x. (At the parent of this change both records came from
the same writer inside the sweep and the comparisons held bitwise as well; no tolerance is needed or used.)

The Dual pass's own outputs (aggregate path and 32 tangent columns of the benched inputs) against the parent commit's are
compared outside the suite, from `bench.py --dump-outputs` of both builds: the parent's dump is not part of the repository.

HANK_PRIMAL_MEMO=0 at hank_create: every hank_primal_jvp really runs its Dual pass."""
import numpy as np
import pytest

from cases import block
from conftest import ks_paths, ks_setup

pytestmark = pytest.mark.gpu

SMALL = (130, 3, 40)
FULL = (2000, 11, 300)


def assert_row0_path_is_exercised(hb, m):
    """some period has a column with a clamped prefix (its mass goes to the virtual rows) and, one period later, an open column
    (row 0 of its record needs that mass): k_lottery clamps a source whose policy is at or below the first grid point"""
    a0 = m.heterogeneity["wealth"].grid[0]
    clo = (hb.policy_seq() <= a0).sum(axis=0)              # (n_e, P): the policy is monotone in the wealth row
    clamped_before = (clo[:, :-1] > 0).any(axis=0)
    open_now = (clo[:, 1:] == 0).any(axis=0)
    assert (clamped_before & open_now).any(), clo[:, :3]


def dual_pass(hb, x, y32):
    agg, dagg = hb.primal_jvp(x, y32)
    assert hb.info()["last_tangent_family_name"] == "xcd-persistent" and hb.last_timings()["tangent_forward"]["launches"] == 1
    assert hb.last_timings()["dual_backward"]["ms"] <= 0.0          # (not the dual-sweep launches)
    return agg, dagg


@pytest.mark.parametrize("n_a,n_e,T", [SMALL, FULL])
def test_record_built_behind_a_dual_pass_has_the_bits_of_hank_primals(hank, n_a, n_e, T):
    """the same fixed tangent batches through the persistent (N = 32), launch (N = 72) and — at 2000x11 — wide (N = 256) families:
    record by Dual pass + builder against record by hank_primal"""
    m, ss, _ = ks_setup(n_a, n_e, T)
    P = T - 1
    x, _ = ks_paths(m, ss, "x1", 0.01)
    rng = np.random.default_rng(17)
    y32 = rng.standard_normal((2, P, 32))
    batches = {"xcd-persistent": rng.standard_normal((2, P, 32)), "launch-per-period": rng.standard_normal((2, P, 72))}
    if (n_a, n_e, T) == FULL:
        batches["on-chip-wide"] = rng.standard_normal((2, P, 256))
    hb = block(hank, m, None, HANK_PRIMAL_MEMO=0)
    hb.set_boundary(ss.value, ss.D)
    assert hb.info()["lwg_builds"] == 0
    for fam, y in batches.items():
        hb.primal(x[2:4])                                           # the Float64 sweep writes the record itself
        assert_row0_path_is_exercised(hb, m)
        want = hb.jvp(y)
        assert hb.info()["last_tangent_family_name"] == fam, (fam, hb.info())
        builds = hb.info()["lwg_builds"]
        hb.primal_jvp(x[2:4] * 1.03, y32)                           # (another record in between)
        dual_pass(hb, x[2:4], y32)                                  # the Dual pass at x: no per-source record written
        assert hb.info()["lwg_builds"] == builds
        got = hb.jvp(y)                                             # built on demand, then read
        assert hb.info()["last_tangent_family_name"] == fam, (fam, hb.info())
        diff = np.max(np.abs(got - want))
        print(f"{n_a}x{n_e} T={T} {fam}: max |jvp(record by Dual pass + builder) - jvp(record by hank_primal)| = {diff:.3e}")
        assert np.array_equal(got, want), (fam, diff)
        assert hb.info()["lwg_builds"] == builds + 1
    assert hb.stats()["fallbacks"] == 0
    hb.close()


@pytest.mark.parametrize("n_a,n_e,T", [SMALL, FULL])
def test_fake_news_after_a_dual_pass_equals_the_one_after_hank_primal(hank, n_a, n_e, T):
    m, ss, _ = ks_setup(n_a, n_e, T)
    P = T - 1
    x = np.tile(np.array([[ss.vars["r"]], [ss.vars["w"]]]), (1, P))
    y32 = np.random.default_rng(3).standard_normal((2, P, 32))
    hb = block(hank, m, None, HANK_PRIMAL_MEMO=0)
    hb.set_boundary(ss.value, ss.D)
    hb.primal(x)
    assert_row0_path_is_exercised(hb, m)
    F0, Dv0 = hb.fake_news()
    Fh0, Dvh0 = hb.fake_news_het(2)
    assert hb.info()["lwg_builds"] == 0
    dual_pass(hb, x, y32)
    F1, Dv1 = hb.fake_news()
    print(f"{n_a}x{n_e} T={T} fake_news: max |F - F0| = {np.max(np.abs(F1 - F0)):.3e}, max |Dv - Dv0| = {np.max(np.abs(Dv1 - Dv0)):.3e}")
    assert np.array_equal(F1, F0) and np.array_equal(Dv1, Dv0)
    assert hb.info()["lwg_builds"] == 1
    dual_pass(hb, x, y32)
    Fh1, Dvh1 = hb.fake_news_het(2)
    print(f"{n_a}x{n_e} T={T} fake_news_het: max |F - F0| = {np.max(np.abs(Fh1 - Fh0)):.3e}, max |Dv - Dv0| = {np.max(np.abs(Dvh1 - Dvh0)):.3e}")
    assert np.array_equal(Fh1, Fh0) and np.array_equal(Dvh1, Dvh0)
    assert hb.info()["lwg_builds"] == 2
    hb.close()


@pytest.mark.parametrize("n_a,n_e,T", [SMALL, FULL])
def test_every_dual_pass_invalidates_the_record_and_one_build_serves_every_later_reader(hank, n_a, n_e, T):
    m, ss, _ = ks_setup(n_a, n_e, T)
    P = T - 1
    x, _ = ks_paths(m, ss, "x1", 0.01)
    rng = np.random.default_rng(29)
    y32, y = rng.standard_normal((2, P, 32)), rng.standard_normal((2, P, 32))
    hb = block(hank, m, None, HANK_PRIMAL_MEMO=0)
    hb.set_boundary(ss.value, ss.D)
    hb.primal(x[2:4])
    assert_row0_path_is_exercised(hb, m)
    want = hb.jvp(y)
    want72 = hb.jvp(np.concatenate([y, y, y[:, :, :8]], axis=2))    # the launch family at the same record
    assert hb.info()["lwg_builds"] == 0
    dual_pass(hb, x[2:4] * 1.03, y32)
    hb.jvp(y)                                                       # the record of the OTHER x is built ...
    assert hb.info()["lwg_builds"] == 1
    dual_pass(hb, x[2:4] * 0.98, y32)
    dual_pass(hb, x[2:4], y32)                                      # ... two Dual passes in a row: each leaves the record invalid
    assert hb.info()["lwg_builds"] == 1
    got = hb.jvp(y)
    assert hb.info()["lwg_builds"] == 2
    assert np.array_equal(got, want)                                # (a stale record — another x's — is off by percents)
    again = hb.jvp(y)                                               # the same record: no second build
    got72 = hb.jvp(np.concatenate([y, y, y[:, :, :8]], axis=2))
    assert hb.info()["last_tangent_family_name"] == "launch-per-period"
    assert hb.info()["lwg_builds"] == 2
    assert np.array_equal(again, want) and np.array_equal(got72, want72)
    hb.primal(x[2:4])                                               # hank_primal writes the record itself
    assert np.array_equal(hb.jvp(y), want) and hb.info()["lwg_builds"] == 2
    assert hb.stats()["fallbacks"] == 0
    hb.close()
