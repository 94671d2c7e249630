"""hank_primal_batch: K input paths through one chain of launches (csrc/hank_scen.h).

Scenario k of a batch is the CPU oracle's household block at x_k (`close`) and, in output 0 and the policies, the per-period
launches' hank_primal at x_k bit for bit, whatever K is and wherever the scenario sits; the context's record, batches, memo and
counters stay as they were; every scenario has its own verdict. Shapes (a few periods, every block layout of the 32-row primal
kernels): Krusell-Smith 50x2 (two row blocks, 18 rows in the second), 70x3 (three blocks), one-asset HANK 30x3 (three household
inputs, one partial block) and the sticky-wage HANK 30x3 with all four outputs. The scenarios: the constant path, then geometric
deviations of both signs, three sizes and four decays. The oracle references and the launch context's are computed once per
shape."""
import numpy as np
import pytest
import torch

import cases as vc
from conftest import ks_setup

pytestmark = pytest.mark.gpu

# (sign * size, decay) of scenario k's deviation from the constant path
SCEN = ((0.0, 1.0), (1.0, 0.8), (-1.0, 0.6), (2.0, 0.9), (-0.5, 0.5))
SHAPES = ("ks50", "ks70", "hank30", "wages30")
_CASES, _LAUNCH = {}, {}


def case(name):
    """dict(m, V, D, xs (n_hh, P, 5), n_het, orc, oagg [k] (n_het, P), opol [k] (P, n_a, n_e))"""
    if name in _CASES:
        return _CASES[name]
    if name.startswith("ks"):
        m, V, D, xhh, orc = vc.shape(*{"ks50": (50, 2, 12), "ks70": (70, 3, 12)}[name])
        r, w = xhh[0, 0] - 0.004 * 0.8, xhh[1, 0] / (1.0 + 0.01 * 0.8)          # (cases.shape: the constants of its path)
        base, amp, n_het = np.array([r, w]), np.array([0.004, 0.01 * w]), {"ks50": 3, "ks70": 2}[name]
    else:
        spec = "one_asset_hank_wages.yaml" if name == "wages30" else "one_asset_hank.yaml"
        m, ss = vc.hank_economy(30, 3, 10, spec)
        V, D, orc = np.asarray(ss.value), np.asarray(ss.D), vc.oracle_of(m)
        base = np.array([ss.vars["r"], ss.vars["om"], ss.vars["Tr"]])
        amp, n_het = np.array([0.002, 0.01 * base[1], -0.02 * base[2]]), (4 if name == "wages30" else 3)
    P = m.compspec.T - 1
    t = np.arange(P)
    xs = np.stack([base[:, None] + s * amp[:, None] * d ** t[None, :] for s, d in SCEN], axis=2)
    oagg, opol = [], []
    for k in range(len(SCEN)):
        a0, _, pol, _ = orc.block(xs[:, :, k], None, V, D)
        ah, _ = orc.het_outputs(xs[:, :, k], np.zeros(xs.shape[:2] + (1,)), V, D, max(n_het, 3), m.params.γ)
        vc.close(ah[0], a0, what=f"{name}: the oracle's two routes to output 0, scenario {k}")
        oagg.append(ah[:n_het]); opol.append(pol)
    grid = m.heterogeneity["wealth"].grid
    brackets = [np.searchsorted(grid, p, side="left") for p in opol]
    differing = sum(not np.array_equal(brackets[0], b) for b in brackets[1:])
    assert differing >= 1 and not np.array_equal(brackets[1], brackets[2]), (name, "the scenarios share their lottery brackets")
    _CASES[name] = dict(m=m, V=V, D=D, xs=xs, n_het=n_het, orc=orc, oagg=oagg, opol=opol)
    return _CASES[name]


def launch_refs(hank, name):
    """per scenario, a launch-schedule context's hank_primal / hank_get_het_outputs / hank_get_policy_seq: [(aggs (P, n_het), policy)]"""
    if name not in _LAUNCH:
        c = case(name)
        hl = vc.block(hank, c["m"], "launch")
        hl.set_boundary(c["V"], c["D"])
        hl.set_het_outputs(max(c["n_het"], 2))
        out = []
        for k in range(len(SCEN)):
            agg = hl.primal(c["xs"][:, :, k])
            aggs = hl.het_outputs(c["n_het"])[0]
            assert np.array_equal(aggs[:, 0], agg)
            out.append((aggs, hl.policy_seq()))
        hl.close()
        _LAUNCH[name] = out
    return _LAUNCH[name]


def batch_block(hank, c, sched=None):
    hb = vc.block(hank, c["m"], sched)
    hb.set_boundary(c["V"], c["D"])
    hb.set_het_outputs(max(c["n_het"], 2))
    return hb


@pytest.mark.parametrize("name", SHAPES)
@pytest.mark.parametrize("K", (1, 2, 5))
def test_every_scenario_matches_the_oracle_and_the_launches(hank, name, K):
    """1. aggregates (every output) and policies against Oracle.block / Oracle.het_outputs at x_k under `close`;
    2. output 0 and the policy of scenario k equal a launch-schedule context's hank_primal(x_k) bit for bit (the same bodies in the
    same order), the outputs >= 1 under `close` (their sums are ordered differently from k_hx_record's)."""
    c = case(name)
    ref = launch_refs(hank, name)
    ks = {1: [1], 2: [0, 3], 5: [0, 1, 2, 3, 4]}[K]
    hb = batch_block(hank, c)
    try:
        aggs, status, pols = hb.primal_batch(c["xs"][:, :, ks], n_het=c["n_het"], policy=True)
    finally:
        hb.close()
    assert aggs.shape == (c["xs"].shape[1], c["n_het"], K) and not status.any()
    for i, k in enumerate(ks):
        what = f"{name} K={K} scenario {k}"
        for o in range(c["n_het"]):
            vc.close(aggs[:, o, i], c["oagg"][k][o], what=f"{what} output {o} vs oracle")
        vc.close(pols[:, :, :, i].transpose(2, 0, 1), c["opol"][k], what=f"{what} policy vs oracle")
        laggs, lpol = ref[k]
        assert np.array_equal(aggs[:, 0, i], laggs[:, 0]), what + ": output 0 bits vs the launches"
        assert np.array_equal(pols[:, :, :, i], lpol), what + ": policy bits vs the launches"
        for o in range(1, c["n_het"]):
            vc.close(aggs[:, o, i], laggs[:, o], what=f"{what} output {o} vs the launches")


@pytest.mark.parametrize("name", SHAPES)
def test_a_scenario_does_not_depend_on_K_or_on_its_position(hank, name):
    """3. a permuted batch, a batch of 5 against five batches of 1 and a batch of 2, and the same call twice: the same bits"""
    c = case(name)
    hb = batch_block(hank, c)
    try:
        full = hb.primal_batch(c["xs"], n_het=c["n_het"], policy=True)
        again = hb.primal_batch(c["xs"], n_het=c["n_het"], policy=True)
        assert all(np.array_equal(a, b) for a, b in zip(full, again)), "the same batch twice"
        perm = [3, 0, 4, 2, 1]
        pa, ps, pp = hb.primal_batch(c["xs"][:, :, perm], n_het=c["n_het"], policy=True)
        for i, k in enumerate(perm):
            assert np.array_equal(pa[:, :, i], full[0][:, :, k]) and np.array_equal(pp[..., i], full[2][..., k]), (name, "permuted", k)
        for k in range(5):
            a1, _, p1 = hb.primal_batch(c["xs"][:, :, k], n_het=c["n_het"], policy=True)
            assert np.array_equal(a1[:, :, 0], full[0][:, :, k]) and np.array_equal(p1[..., 0], full[2][..., k]), (name, "K=1", k)
        a2, _, p2 = hb.primal_batch(c["xs"][:, :, [4, 1]], n_het=c["n_het"], policy=True)      # (a narrower batch after a wider one)
        for i, k in enumerate((4, 1)):
            assert np.array_equal(a2[:, :, i], full[0][:, :, k]) and np.array_equal(p2[..., i], full[2][..., k]), (name, "K=2", k)
        bms = hb.last_batch_timings()
        assert bms[0] > 0.0 and bms[1] > 0.0, bms
    finally:
        hb.close()


@pytest.mark.parametrize("name", ("ks50", "wages30"))
def test_the_context_is_left_alone(hank, name):
    """4. between two hank_jvp at one recorded primal, a batch at other paths: the second hank_jvp returns the first one's bits,
    the policy sequence, the counters and the family are unchanged, and hank_primal_jvp at the recorded x still hits the memo"""
    c = case(name)
    xa = c["xs"][:, :, 1]
    y = np.random.default_rng(11).standard_normal(xa.shape + (3,))
    hb = batch_block(hank, c)
    try:
        agg_a = hb.primal(xa)
        d1 = hb.jvp(y)
        pol1, st1, info1 = hb.policy_seq(), hb.stats(), hb.info()
        hb.primal_batch(c["xs"][:, :, [2, 3, 4]], n_het=c["n_het"])
        st2, info2 = hb.stats(), hb.info()
        for key in ("sweep_launches", "primal_memo_hits", "primal_sweeps", "fallbacks", "schedule", "tangent_workspaces_allocated"):
            assert st2[key] == st1[key], (key, st1, st2)
        assert info2 == info1
        assert np.array_equal(hb.policy_seq(), pol1)
        assert np.array_equal(hb.dpolicy_seq(3), hb.dpolicy_seq(3))      # (the batch is still current)
        d2 = hb.jvp(y)
        assert np.array_equal(d2, d1)
        agg_m, d3 = hb.primal_jvp(xa, y)
        assert hb.stats()["primal_memo_hits"] == st1["primal_memo_hits"] + 1 and hb.stats()["primal_sweeps"] == st1["primal_sweeps"]
        assert np.array_equal(agg_m, agg_a) and np.array_equal(d3, d1)
    finally:
        hb.close()


def _bad_path(c):
    """scenario 1 of the verdict test: wages of -50 in every period (negative cash on hand at the low grid points)"""
    x = np.array(c["xs"][:, :, 1], copy=True)
    x[1] = -50.0
    return x


@pytest.mark.parametrize("name", ("ks50", "hank30"))
def test_every_scenario_has_its_own_verdict(hank, name):
    """5. a batch whose scenario 1 raises and whose scenarios 0 and 2 are healthy. The bad path alone: the oracle refuses it and a
    launch-schedule hank_primal returns HANK_ERR_DOMAIN or HANK_ERR_KNOTS (asserted first). The batch: that code as the return
    value and as status[1], HANK_OK for the others, whose outputs equal the clean batch's bit for bit; the context's record and
    batch stay; the _dev form reports at hank_check, once."""
    H = hank.hip
    c = case(name)
    bad = _bad_path(c)
    with pytest.raises(RuntimeError, match="oracle status [34]"):
        c["orc"].block(bad, None, c["V"], c["D"])
    hl = vc.block(hank, c["m"], "launch")
    hl.set_boundary(c["V"], c["D"])
    with pytest.raises((hank.DomainError, hank.KnotsNotSortedError)) as alone:
        hl.primal(bad)
    hl.close()
    code = alone.value.code
    assert code in (H.HANK_ERR_DOMAIN, H.HANK_ERR_KNOTS)
    xs = np.stack([c["xs"][:, :, 1], bad, c["xs"][:, :, 3]], axis=2)
    clean = np.stack([c["xs"][:, :, 1], c["xs"][:, :, 2], c["xs"][:, :, 3]], axis=2)
    y = np.random.default_rng(12).standard_normal(bad.shape + (2,))
    hb = batch_block(hank, c)
    try:
        hb.primal(c["xs"][:, :, 0])
        d1, pol1 = hb.jvp(y), hb.policy_seq()
        ca, cs, cp = hb.primal_batch(clean, n_het=c["n_het"], policy=True)
        assert not cs.any()
        with pytest.raises(hank.HankHIPError, match="scenario 1 of 3") as ei:
            hb.primal_batch(xs, n_het=c["n_het"], policy=True)
        assert ei.value.code == code and "period" in str(ei.value)
        aggs, status, pols = hb.last_batch
        assert status.tolist() == [H.HANK_OK, code, H.HANK_OK]
        a_nc, s_nc = hb.primal_batch(xs, n_het=c["n_het"], check=False)       # (check=False returns what the call has)
        assert s_nc.tolist() == status.tolist() and np.array_equal(a_nc[:, :, [0, 2]], aggs[:, :, [0, 2]])
        for i in (0, 2):
            assert np.array_equal(aggs[:, :, i], ca[:, :, i]) and np.array_equal(pols[..., i], cp[..., i]), (name, i)
        assert np.array_equal(hb.policy_seq(), pol1) and np.array_equal(hb.jvp(y), d1)
        # the device-pointer form: asynchronous, the verdict at hank_check, once; the record and the batch stay
        dev = torch.device("cuda", 0)
        d_x = torch.from_numpy(np.asfortranarray(xs).reshape(-1, order="F").copy()).to(dev)
        d_a = torch.empty(ca.size, dtype=torch.float64, device=dev)
        hb.primal_batch_dev(c["n_het"], d_x.data_ptr(), 3, d_a.data_ptr())
        with pytest.raises(hank.HankHIPError, match="scenario 1 of 3") as ei:
            hb.check()
        assert ei.value.code == code
        hb.check()
        got = d_a.cpu().numpy().reshape(ca.shape, order="F")
        assert np.array_equal(got[:, :, [0, 2]], ca[:, :, [0, 2]])
        assert np.array_equal(hb.dpolicy_seq(2).shape, pol1.shape + (2,)) and np.array_equal(hb.jvp(y), d1)
        hb.primal_batch_dev(c["n_het"], torch.from_numpy(np.asfortranarray(clean).reshape(-1, order="F").copy()).to(dev).data_ptr(), 3, d_a.data_ptr())
        hb.check()
        assert np.array_equal(d_a.cpu().numpy().reshape(ca.shape, order="F"), ca)
    finally:
        hb.close()


def test_bad_arguments_and_lifetime(hank):
    """6. no boundary, K outside 1..64, more outputs than declared; and ten contexts created, batched and destroyed in turn: the
    same bits every time and the device's free memory back where it was (no lifetime test of the suite measures allocations:
    hipMemGetInfo before and after, with the slack of one allocation granule per cycle ruled out by the ten cycles)"""
    H = hank.hip
    c = case("ks50")

    def refused(call, code):
        with pytest.raises(hank.HankHIPError) as ei:
            call()
        assert ei.value.code == code, ei.value

    hb = vc.block(hank, c["m"], None)
    refused(lambda: hb.primal_batch(c["xs"][:, :, :2]), H.HANK_ERR_NOT_READY)
    hb.set_boundary(c["V"], c["D"])
    P = c["xs"].shape[1]
    refused(lambda: hb.primal_batch(np.zeros((2, P, 0))), H.HANK_ERR_BAD_ARG)
    refused(lambda: hb.primal_batch(np.repeat(c["xs"][:, :, :1], 65, axis=2)), H.HANK_ERR_BAD_ARG)
    refused(lambda: hb.primal_batch(c["xs"][:, :, :2], n_het=3), H.HANK_ERR_NOT_READY)
    refused(lambda: hb.primal_batch(c["xs"][:, :, :2], n_het=4), H.HANK_ERR_BAD_ARG)        # (Krusell-Smith serves three outputs)
    x_neg = np.array(c["xs"][:, :, :2], copy=True)
    x_neg[0, 3, 1] = -1.5
    with pytest.raises(hank.DomainError, match="scenario 1, period 4"):
        hb.primal_batch(x_neg)
    first = hb.primal_batch(np.tile(c["xs"], (1, 1, 13))[:, :, :64], n_het=2)             # (K = 64, the widest batch: scenario k % 5 at k)
    assert np.array_equal(first[0][:, :, 5], first[0][:, :, 0]) and not first[1].any()
    hb.close()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for cycle in range(10):
        hb = vc.block(hank, c["m"], None)
        hb.set_boundary(c["V"], c["D"])
        got = hb.primal_batch(c["xs"][:, :, :2 + cycle % 3], n_het=2)                       # (grown from cycle to cycle: 2, 3, 4)
        grown = hb.primal_batch(c["xs"], n_het=2)
        hb.close()
        assert np.array_equal(got[0], first[0][:, :, :2 + cycle % 3]) and np.array_equal(grown[0], first[0][:, :, :5])
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] >= free0 - (2 << 20), (free0, torch.cuda.mem_get_info()[0])


def test_newton_with_the_backtracking_step(hank):
    """7. Krusell-Smith 50x2, T = 60, the shock of test_gpu_jacobian.py's converged-path test: step="backtrack" reaches the path of
    step="full" to 1e-8 (that test's bound between inner loops), every accepted step is a power of one half, ‖F‖ does not increase
    over the outer iterations, and residuals_batch of three columns equals three fullFunction calls under `close`."""
    from hank_amd.NewtonRaphson import make_fullFunction, residuals_batch
    m, ss, _ = ks_setup(50, 2, 60)
    P = 59
    Z = 1.0 + 0.01 * 0.8 ** np.arange(1, P + 1)
    x0 = np.tile(np.array([ss.vars[k] for k in ("Y", "KS", "r", "w")]), P)
    J = hank.getSteadyStateJacobian(ss, m)
    x_full = hank.NewtonRaphsonHANK(x0, J, {"Z": Z}, m, ss, ss, ε=1e-9)
    x_bt = hank.NewtonRaphsonHANK(x0, J, {"Z": Z}, m, ss, ss, ε=1e-9, step="backtrack")
    sizes, norms = hank.NewtonRaphsonHANK.step_sizes, hank.NewtonRaphsonHANK.residual_norms
    print("accepted steps", sizes, "‖F‖", norms)
    assert np.max(np.abs(x_bt - x_full)) < 1e-8
    assert len(sizes) == hank.NewtonRaphsonHANK.iterations >= 1 and all(a in [2.0 ** -j for j in range(6)] for a in sizes)
    # (one ‖F‖ per iterate; the last step, below the tolerance, is taken whole and adds none behind it)
    assert len(norms) in (len(sizes), len(sizes) + 1) and all(b <= a for a, b in zip(norms, norms[1:])), norms
    rng = np.random.default_rng(7)
    xs = np.stack([x_full, x0, x0 * (1.0 + 1e-3 * rng.standard_normal(x0.size))], axis=1)
    F = residuals_batch(xs, {"Z": Z}, m, ss, ss)
    f = make_fullFunction({"Z": Z}, m, ss, ss)
    for k in range(3):
        vc.close(F[:, k], f(xs[:, k]), what=f"residuals_batch column {k}")
