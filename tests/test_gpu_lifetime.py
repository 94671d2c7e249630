"""Lifetime of a context's device memory and graphs (csrc/hank_hip.hip): contexts created, used through every
entry that allocates, and destroyed, again and again; workspaces evicted from a cache that holds one; a context after a hank_create
that failed. What is pinned is behaviour — the same bits every time, the readers' answers after an eviction — on Krusell-Smith
65x3, T = 12 (cases.shape: two members per group of the persistent sweeps, the second with two rows; n_e = 3 is instantiated
for the wide sweeps), under every schedule: the default, launch, xcd and wide. A schedule that hank_create refuses fails the test."""
import numpy as np
import pytest

import cases as vc

pytestmark = pytest.mark.gpu

SCHEDULES = (None, "launch", "xcd", "wide")
SHAPE = (65, 3, 12)


def _inputs():
    m, V, D, xhh, orc = vc.shape(*SHAPE)
    n_hh, P = xhh.shape
    rng = np.random.default_rng(65)
    return m, V, D, xhh, orc, rng.standard_normal((n_hh, P, 3)), rng.standard_normal((P, 2, 3))


def _use_everything(hb, V, D, xhh, y, yb):
    """every entry that owns or borrows device memory, once -> its arrays by name"""
    y2 = np.ascontiguousarray(y[:, :, :2])
    out = {}
    hb.set_boundary(V, D)
    out["primal"] = hb.primal(xhh)
    out["jvp2"] = hb.jvp(y2)
    out["jvp3"] = hb.jvp(y)
    out["dual_agg"], out["dual_dagg"] = hb.primal_jvp(xhh * 1.01, y2)           # (another x: no memo hit, the Dual pass runs)
    out["vjp2"] = hb.vjp(yb[:, :, :2], 2)
    out["dpolicy"] = hb.dpolicy_seq(2)
    out["pbar"] = hb.policy_cotangent_seq(2)
    out["het_agg"], out["het_dagg"] = hb.het_outputs(2, y2)
    out["grid_agg"], out["grid_dagg"] = hb.grid_aggregates(2)
    return out


def test_contexts_created_and_destroyed_in_turn_return_the_same_bits(hank):
    """three cycles over the four schedules: create, use everything, close, close again. Cycles 2 and 3 return cycle 1's bits."""
    m, V, D, xhh, _, y, yb = _inputs()
    first = {}
    for cycle in range(3):
        for sched in SCHEDULES:
            hb = vc.block(hank, m, sched)
            got = _use_everything(hb, V, D, xhh, y, yb)
            hb.close()
            hb.close()
            if cycle == 0:
                first[sched] = got
                continue
            assert got.keys() == first[sched].keys()
            for name, a in got.items():
                assert np.array_equal(a, first[sched][name]), (cycle, sched, name)


def _refused_not_ready(hank, call):
    with pytest.raises(hank.HankHIPError) as ei:
        call()
    assert ei.value.code == hank.hip.HANK_ERR_NOT_READY, ei.value


@pytest.mark.parametrize("sched", SCHEDULES)
def test_a_cache_of_one_evicts_on_every_change_of_width(hank, monkeypatch, sched):
    """HANK_TAN_CACHE=1 (read at every cache miss): alternating widths evict the other width's workspace every call — the
    counter says so — and every result equals the first of its width; the evicted batch is no longer anybody's."""
    monkeypatch.setenv("HANK_TAN_CACHE", "1")
    m, V, D, xhh, _, y, yb = _inputs()
    hb = vc.block(hank, m, sched)
    try:
        hb.set_boundary(V, D)
        hb.primal(xhh)

        def alternate(call, columns):
            first = {}
            for _ in range(4):
                for n in (2, 3):
                    before = hb.stats()["tangent_workspaces_allocated"]
                    got = call(np.ascontiguousarray(columns[:, :, :n]))
                    assert hb.stats()["tangent_workspaces_allocated"] == before + 1, (sched, n)
                    assert np.array_equal(got, first.setdefault(n, got)), (sched, n)

        seq_shape = (SHAPE[0], SHAPE[1], SHAPE[2] - 1, 3)
        alternate(hb.jvp, y)
        assert hb.dpolicy_seq(3).shape == seq_shape
        _refused_not_ready(hank, lambda: hb.dpolicy_seq(2))
        alternate(lambda b: hb.vjp(b, 2), yb)
        assert hb.policy_cotangent_seq(3).shape == seq_shape
        _refused_not_ready(hank, lambda: hb.policy_cotangent_seq(2))
        assert hb.stats()["fallbacks"] == 0
    finally:
        hb.close()


def test_a_failed_create_leaves_the_process_usable(hank):
    """hank_create returns its context on failure too (for hank_last_error) and the caller destroys it: a wealth grid that does
    not increase is refused, and a context of the right grid, created next, matches the oracle (rel 1e-10 + abs 1e-12 of the
    output scale, tests/test_gpu_sweeps.py's bound for hank_primal)."""
    m, V, D, xhh, orc, _, _ = _inputs()
    bad = np.array(m.heterogeneity["wealth"].grid, copy=True)
    bad[7] = bad[6]
    with pytest.raises(hank.HankHIPError, match="strictly increasing"):
        hank.HouseholdBlock(bad, *vc.model_args(m)[1:])
    hb = vc.block(hank, m, None)
    try:
        hb.set_boundary(V, D)
        agg = hb.primal(xhh)
    finally:
        hb.close()
    vc.close(agg, orc.block(xhh, None, V, D)[0], what="hank_primal after a failed hank_create")
