"""Group outputs, the part that needs no GPU: the CPU reference of tests/group_refs.py (the groups of a partition sum to the
totals, every output of the Krusell-Smith case is non-trivial), the weight arrays of hank_amd.groups, the ABI list and the
host recursion of SteadyStateJacobian.group_jacobian."""
import numpy as np
import pytest

import group_refs as gr
from conftest import ks_setup


def test_reference_groups_sum_to_the_totals_and_none_is_trivial():
    """KS 130x3, T = 40, wealth groups at [0, .2, .5, .9, 1], every base, N = 4: the four groups of a base sum to the base's
    whole-population output (within 5e-14, values and tangents; measured 7e-15 and 4.3e-14), MASS to 1 with a zero tangent, and
    each of the twelve references exceeds 1e-2 in value and 1e-1 in tangent."""
    xhh, y, W, base, agg, dagg = gr.ks_reference(4)
    m, ss, orc = ks_setup(130, 3, 40)
    assert agg.shape == (12, 39) and dagg.shape == (12, 39, 4)
    gr.nontrivial(agg, dagg, "ks130")
    tot, dtot = gr.group_reference(orc, xhh, y, ss.value, ss.D, np.ones((390, 3)), [gr.MASS, gr.POLICY, gr.CONS])
    het, dhet = orc.block_het(xhh, y, ss.value, ss.D)
    for b in range(3):
        s, ds = agg[4 * b:4 * b + 4].sum(axis=0), dagg[4 * b:4 * b + 4].sum(axis=0)
        ev, ed = np.abs(s - tot[b]).max(), np.abs(ds - dtot[b]).max()
        print(f"base {b}: groups vs total {ev:.3e} (values, scale {np.abs(tot[b]).max():.3e}), {ed:.3e} (tangents, scale {np.abs(dtot[b]).max():.3e})")
        assert ev <= 5e-14 and ed <= 5e-14
    assert np.abs(tot[0] - 1.0).max() <= 5e-14 and np.abs(dtot[0]).max() <= 5e-14
    # W = 1: POLICY and CONS are the two-variable household block's outputs, the same arithmetic
    assert np.array_equal(tot[1], het[0]) and np.array_equal(tot[2], het[1])
    assert np.array_equal(dtot[1], dhet[0]) and np.array_equal(dtot[2], dhet[1])


@pytest.mark.parametrize("n_a,n_e,edges", [(130, 3, gr.EDGES), (130, 3, (0.0, 0.5, 0.9, 1.0)), (50, 2, (0.0, 0.5, 1.0))])
def test_wealth_groups_partition_and_masses(n_a, n_e, edges):
    from hank_amd.groups import wealth_groups
    m, ss, _ = ks_setup(n_a, n_e, 40 if n_a == 130 else 100)
    W = wealth_groups(ss.D, n_a, n_e, edges)
    K = len(edges) - 1
    assert W.shape == (n_a * n_e, K) and set(np.unique(W)) <= {0.0, 1.0}
    assert np.array_equal(W.sum(axis=1), np.ones(n_a * n_e))                   # a partition of unity
    Wm = W.reshape(n_a, n_e, K, order="F")
    assert all(np.array_equal(Wm[:, 0], Wm[:, e]) for e in range(n_e))         # rows: the same in every productivity column
    rows = Wm[:, 0, :]
    assert np.all(rows.sum(axis=0) >= 1)                                      # no empty group
    first = np.argmax(rows, axis=0)
    assert np.all(np.diff(first) > 0)                                         # fixed by wealth level, in order
    row_mass = np.asarray(ss.D).reshape((n_a, n_e), order="F").sum(axis=1)
    row_mass = row_mass / row_mass.sum()
    cum = np.cumsum(rows.T @ row_mass)
    for g in range(K - 1):
        nxt = row_mass[first[g + 1]]                                          # the row just above the boundary
        print(f"edge {edges[g + 1]}: mass below {cum[g]:.6f}, the next row holds {nxt:.3e}")
        assert cum[g] <= edges[g + 1] + 1e-15 and edges[g + 1] - cum[g] <= nxt + 1e-15
    assert abs(cum[-1] - 1.0) <= 1e-14
    for bad in ((0.1, 0.5, 1.0), (0.0, 0.5, 0.5, 1.0), (0.0, 0.5)):
        with pytest.raises(ValueError):
            wealth_groups(ss.D, n_a, n_e, bad)


def test_productivity_and_constrained_groups():
    from hank_amd.groups import constrained, productivity_groups
    n_a, n_e = 7, 3
    Wp = productivity_groups(n_a, n_e)
    assert Wp.shape == (21, 3) and np.array_equal(Wp.sum(axis=1), np.ones(21))
    for e in range(n_e):
        assert np.array_equal(np.flatnonzero(Wp[:, e]), np.arange(e * n_a, (e + 1) * n_a))      # pt = e n_a + ia
    Wc = constrained(n_a, n_e)
    assert Wc.shape == (21, 1) and np.array_equal(np.flatnonzero(Wc[:, 0]), np.array([0, 7, 14]))


def test_the_new_symbols_are_in_the_abi(hank):
    from hank_amd import hip
    for name in ("hank_set_group_outputs", "hank_get_group_outputs", "hank_get_group_outputs_dev", "hank_fake_news_group"):
        assert name in hip.ABI_SYMBOLS, name
        assert getattr(hip.load_library(), name) is not None
    assert (hip.HANK_GROUP_MASS, hip.HANK_GROUP_POLICY, hip.HANK_GROUP_CONS, hip.HANK_GROUP_MAX) == (0, 1, 2, 32)
    hb = hip.HouseholdBlock
    assert (hb.GROUP_MASS, hb.GROUP_POLICY, hb.GROUP_CONS) == (0, 1, 2)
    assert (gr.MASS, gr.POLICY, gr.CONS) == (0, 1, 2)


def test_group_jacobian_is_household_jacobian_per_group():
    from hank_amd.SteadyStateJacobian import group_jacobian, household_jacobian
    P, n_hh, K = 7, 3, 5
    rng = np.random.default_rng(0)
    F, Dv = rng.standard_normal((P, P, n_hh, K)), rng.standard_normal((P, n_hh, K))

    class Block:
        def fake_news_group(self):
            return np.asfortranarray(F), np.asfortranarray(Dv)

    J = group_jacobian(Block())
    assert J.shape == (K, P, n_hh, P)
    for k in range(K):
        Jk = household_jacobian(F[..., k], Dv[..., k])                        # (n_hh, P, P)
        assert np.array_equal(J[k], Jk.transpose(1, 0, 2))
        for i in range(n_hh):                                                 # and the recursion itself, entry by entry
            for t in range(P):
                for s in range(P):
                    want = sum(F[t - q, s - q, i, k] for q in range(min(t, s) + 1)) + (Dv[s - t, i, k] if s >= t else 0.0)
                    assert abs(J[k, t, i, s] - want) <= 1e-13, (k, i, t, s)
