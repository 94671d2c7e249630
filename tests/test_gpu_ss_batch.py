"""hank_ss_batch: the steady state's household side at K price vectors through one chain of launches (csrc/hank_ssbatch.h;
DESIGN.md section 3i).

Scenario k of a batch is the CPU oracle's value iteration at x_k (`close`, steps within one), a fixed point of the host's lottery
matrix of its own policy, and — value, policy, steps, sup-norm and the raw distribution — a launch-schedule context's hank_vfi
and hank_stationary_dist bit for bit, whatever K is and wherever the scenario sits; the scenarios stop at different steps, so the
freezing of a converged scenario is exercised; the context's record, batches, memo and counters stay as they were; every scenario
has its own verdict. Shapes (the block layouts of the 32-row kernels): Krusell-Smith 50x2 (two row blocks, 18 rows in the second)
and 37x3, one-asset HANK 30x3 (three inputs, one partial block), sticky-wage HANK 30x3 with all four outputs. The oracle's and the
launch context's references are computed once per shape."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import cases as vc
from conftest import ks_setup

pytestmark = pytest.mark.gpu

TOL = 1e-11
SHAPES = ("ks50", "ks37", "hank30", "wages30")
# the one-asset HANK scenarios: (r, om, Tr) = steady state + (s_r, s_w om, s_t Tr)
HANK_S = ((0.0, 0.0, 0.0), (0.002, 0.01, -0.02), (-0.002, -0.01, 0.02), (0.004, 0.0, 0.0), (-0.004, 0.02, 0.0))
_CASES, _LAUNCH = {}, {}


def oracle_vfi(orc, shape, x, tol=TOL, cap=20_000):
    """Oracle.vfi with the transfer of the one-asset HANK family: value_function(..., tr=) in a loop of the test's own"""
    if len(x) == 2:
        v, p, steps, _ = orc.vfi(shape, x[0], x[1], tol)
        return v, p, steps
    value = np.ones(shape)
    for k in range(1, cap + 1):
        st, V, KD = orc.value_function(value, x[0], x[1], 1, tr=x[2])
        if st != 0:
            raise RuntimeError(f"oracle status {st}")
        d = float(np.max(np.abs(V[..., 0] - value)))
        value = V[..., 0]
        if d < tol:
            return value, KD[..., 0], k
    raise RuntimeError("oracle VFI did not converge")


def case(name):
    """dict(m, xs (n_hh, 5), n_het, orc, shape, ov [k], op [k], osteps [k])"""
    if name in _CASES:
        return _CASES[name]
    if name.startswith("ks"):
        m, ss, orc = ks_setup(*{"ks50": (50, 2, 100), "ks37": (37, 3, 9)}[name])
        r, w = ss.vars["r"], ss.vars["w"]
        xs = np.array([[r, w], [0.015, 1.0], [0.04, 1.0], [r - 0.004, 1.01 * w], [0.005, 0.9 * w]]).T
        n_het = {"ks50": 3, "ks37": 2}[name]
    else:
        m, ss = vc.hank_economy(30, 3, 10, "one_asset_hank_wages.yaml" if name == "wages30" else "one_asset_hank.yaml")
        orc = vc.oracle_of(m)
        b = np.array([ss.vars["r"], ss.vars["om"], ss.vars["Tr"]])
        xs = np.array([b + np.array([s[0], s[1] * b[1], s[2] * b[2]]) for s in HANK_S]).T
        n_het = 4 if name == "wages30" else 3
    wd, pdm = m.heterogeneity["wealth"], m.heterogeneity["productivity"]
    shape = (wd.n, pdm.n)
    ov, op, osteps = zip(*(oracle_vfi(orc, shape, xs[:, k]) for k in range(5)))
    print(f"{name}: oracle value steps {osteps}")
    # 1. freezing is exercised: the scenarios of a batch stop at least 10 steps apart
    assert all(abs(a - b) >= 10 for i, a in enumerate(osteps) for b in osteps[i + 1:]), (name, osteps)
    _CASES[name] = dict(m=m, ss=ss, xs=np.ascontiguousarray(xs), n_het=n_het, orc=orc, shape=shape, ov=ov, op=op, osteps=osteps)
    return _CASES[name]


def batch_block(hank, c, sched=None):
    hb = vc.block(hank, c["m"], sched)
    hb.set_het_outputs(max(c["n_het"], 2))
    return hb


def raw_stationary(hank, hb, pol, max_iter, tol=1e-15, check_every=25):
    """hank_stationary_dist from the uniform start -> (D_io as the library leaves it, iters)"""
    H = hank.hip
    p = H._f(pol, (hb.n_a, hb.n_e))
    d = np.full(hb.G, 1.0 / hb.G)
    it = C.c_int32()
    hb._chk(hb._lib.hank_stationary_dist(hb._ctx, H._p(p), H._p(d), float(tol), int(max_iter), int(check_every), C.byref(it)))
    return d, it.value


def launch_refs(hank, name):
    """the batch of all five scenarios on a default context, and per scenario a launch-schedule context's hank_vfi from ones and
    hank_stationary_dist (uniform start, max_iter = the batch's count): dict(full, raw, vfi [k] (v, pol, steps, norm), D [k])"""
    if name not in _LAUNCH:
        c = case(name)
        hb = batch_block(hank, c)
        full = hb.ss_batch(c["xs"], TOL, n_het=c["n_het"])
        raw = hb.last_ss_batch
        hb.close()
        hl = vc.block(hank, c["m"], "launch")
        vfi = [hl.vfi(np.ones(c["shape"]), c["xs"][:, k], TOL) for k in range(5)]
        D = [raw_stationary(hank, hl, vfi[k][1], int(full[4][k, 1]))[0] for k in range(5)]
        hl.close()
        _LAUNCH[name] = dict(full=full, raw=raw, vfi=vfi, D=D)
    return _LAUNCH[name]


def same(a, b):
    """two results of ss_batch (or the same columns of two): every output's bits"""
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def cols(res, ks):
    aggs, v, pol, D, iters, status = res
    return aggs[:, ks], v[:, :, ks], pol[:, :, ks], D[:, ks], iters[ks], status[ks]


def host_power_method(L, G, check_every=25, tol=1e-15, cap=500_000):
    """the device's rule on the host: D <- L D from uniform, every `check_every` steps against the iterate of the check before"""
    D = np.full(G, 1.0 / G)
    chk, done = D, 0
    while done < cap:
        for _ in range(check_every):
            D = L @ D
        done += check_every
        if np.max(np.abs(D - chk)) < tol:
            break
        chk = D
    return done


@pytest.mark.parametrize("name", SHAPES)
@pytest.mark.parametrize("K", (1, 2, 5))
def test_every_scenario_matches_the_oracle_and_the_host(hank, name, K):
    """2. value and policy against the oracle's iteration (`close`, steps within one: test_device_vfi_matches_the_oracle_iteration's
    rule); the normalised D a fixed point of the host's transition matrix of the returned policy to 1e-14, its iteration count
    within one check of the host power method's; every aggregate against numpy sums of the returned policy and D"""
    c = case(name)
    m = c["m"]
    ks = {1: [1], 2: [0, 3], 5: [0, 1, 2, 3, 4]}[K]
    hb = batch_block(hank, c)
    try:
        aggs, v, pol, D, iters, status = hb.ss_batch(c["xs"][:, ks], TOL, n_het=c["n_het"])
        sup = hb.last_ss_batch["supnorm"]
    finally:
        hb.close()
    n_a, n_e = c["shape"]
    assert aggs.shape == (c["n_het"], K) and v.shape == pol.shape == (n_a, n_e, K) and D.shape == (n_a * n_e, K) and not status.any()
    wd, pdm = m.heterogeneity["wealth"], m.heterogeneity["productivity"]
    L_exog = sp.kron(sp.csc_matrix(pdm.transition.T), sp.identity(wd.n, format="csc"), format="csc")
    a, z, gam = wd.grid[:, None], pdm.grid[None, :], m.params.γ
    for i, k in enumerate(ks):
        what = f"{name} K={K} scenario {k}"
        vc.close(v[:, :, i], c["ov"][k], what=what + " value vs oracle")
        vc.close(pol[:, :, i], c["op"][k], what=what + " policy vs oracle")
        print(f"{what}: value steps {iters[i, 0]} (oracle {c['osteps'][k]}), distribution iterations {iters[i, 1]}, sup-norm {sup[i]:.3e}")
        assert abs(int(iters[i, 0]) - c["osteps"][k]) <= 1 and sup[i] < TOL, (what, iters[i], c["osteps"][k], sup[i])
        L = (L_exog @ hank.make_endogenous_transition(pol[:, :, i], wd, pdm.n)).tocsr()
        Dk = D[:, i]
        assert abs(Dk.sum() - 1.0) < 1e-13 and Dk.min() >= 0.0, what
        res = np.max(np.abs(L @ Dk - Dk))
        host_iters = host_power_method(L, Dk.size)
        print(f"{what}: max|LD - D| {res:.3e}, host power method {host_iters} iterations")
        assert res < 1e-14, (what, res)
        assert iters[i, 1] % 25 == 0 and abs(int(iters[i, 1]) - host_iters) <= 25, (what, iters[i, 1], host_iters)
        x = c["xs"][:, k]
        r, w, tr = x[0], x[1], (x[2] if len(x) > 2 else 0.0)
        Dm, p = Dk.reshape((n_a, n_e), order="F"), pol[:, :, i]
        cons = (1.0 + r) * a + w * z + tr - p
        f = [p, cons, (1.0 + r) * cons ** -gam, z * cons ** -gam]
        assert aggs[0, i] != 0.0
        for o in range(c["n_het"]):
            vc.close(aggs[o, i], np.sum(f[o] * Dm), what=f"{what} output {o} vs numpy")


@pytest.mark.parametrize("name", SHAPES)
def test_every_scenario_is_the_launches_bit_for_bit(hank, name):
    """3. scenario k's value, policy, steps and sup-norm are hank_vfi's on a launch-schedule context, and its raw D_io column is
    hank_stationary_dist's there with max_iter = the batch's count (so that nothing follows the stop)"""
    ref = launch_refs(hank, name)
    aggs, v, pol, D, iters, status = ref["full"]
    for k in range(5):
        lv, lp, lsteps, lnorm = ref["vfi"][k]
        what = f"{name} scenario {k}"
        assert int(iters[k, 0]) == lsteps and ref["raw"]["supnorm"][k] == lnorm, (what, iters[k], lsteps, ref["raw"]["supnorm"][k], lnorm)
        assert np.array_equal(v[:, :, k], lv), what + ": value bits"
        assert np.array_equal(pol[:, :, k], lp), what + ": policy bits"
        assert np.array_equal(ref["raw"]["D"][:, k], ref["D"][k]), what + ": D_io bits"


@pytest.mark.parametrize("name", SHAPES)
def test_a_scenario_does_not_depend_on_K_or_on_its_position(hank, name):
    """4. the same batch twice, a permuted batch, five batches of 1 and a batch of 2 behind the batch of 5, and K = 64 (scenario
    k % 5 at k): the same bits in every output of a scenario"""
    c = case(name)
    full = launch_refs(hank, name)["full"]
    hb = batch_block(hank, c)
    try:
        assert same(hb.ss_batch(c["xs"], TOL, n_het=c["n_het"]), full), "the same batch twice"
        perm = [3, 0, 4, 2, 1]
        assert same(hb.ss_batch(c["xs"][:, perm], TOL, n_het=c["n_het"]), cols(full, perm)), "permuted"
        for k in range(5):
            assert same(hb.ss_batch(c["xs"][:, k], TOL, n_het=c["n_het"]), cols(full, [k])), ("K=1", k)
        assert same(hb.ss_batch(c["xs"][:, [4, 1]], TOL, n_het=c["n_het"]), cols(full, [4, 1])), "K=2 behind K=5"
        k64 = [k % 5 for k in range(64)]
        assert same(hb.ss_batch(c["xs"][:, k64], TOL, n_het=c["n_het"]), cols(full, k64)), "K=64"
        ms = hb.last_ss_batch_timings()
        assert ms[0] > 0.0 and ms[1] > 0.0, ms
    finally:
        hb.close()


@pytest.mark.parametrize("name", ("ks50", "wages30"))
def test_warm_starts(hank, name):
    """5. from the converged values every scenario stops after 1 step, or 2 (a sup-norm at the edge of tol); a shared value0 and
    K copies of it give the same bits"""
    c = case(name)
    full = launch_refs(hank, name)["full"]
    hb = batch_block(hank, c)
    try:
        warm = hb.ss_batch(c["xs"], TOL, n_het=c["n_het"], value0=full[1], D0=full[3])
        assert not warm[5].any() and np.all((warm[4][:, 0] >= 1) & (warm[4][:, 0] <= 2)), warm[4]
        vc.close(warm[1], full[1], what=f"{name} warm value")
        shared = full[1][:, :, 0]
        a = hb.ss_batch(c["xs"], TOL, n_het=c["n_het"], value0=shared)
        b = hb.ss_batch(c["xs"], TOL, n_het=c["n_het"], value0=np.repeat(shared[:, :, None], 5, axis=2))
        assert same(a, b) and a[4][0, 0] <= 2 and np.all(a[4][1:, 0] > 10), a[4]
    finally:
        hb.close()


@pytest.mark.parametrize("name", ("ks50", "hank30"))
def test_caps(hank, name):
    """6. vfi_max_iter = 100: every scenario reports 100 steps, status OK and the value bits of hank_vfi(max_iter=100) on the
    launches; dist_max_iter = 60 with check_every = 25: every scenario reports 60"""
    c = case(name)
    hb = batch_block(hank, c)
    hl = vc.block(hank, c["m"], "launch")
    try:
        aggs, v, pol, D, iters, status = hb.ss_batch(c["xs"], TOL, n_het=c["n_het"], vfi_max_iter=100, dist_max_iter=60)
        assert not status.any() and iters[:, 0].tolist() == [100] * 5 and iters[:, 1].tolist() == [60] * 5, iters
        for k in range(5):
            lv, lp, lsteps, lnorm = hl.vfi(np.ones(c["shape"]), c["xs"][:, k], TOL, 100)
            assert lsteps == 100 and np.array_equal(v[:, :, k], lv) and np.array_equal(pol[:, :, k], lp), (name, k)
            assert hb.last_ss_batch["supnorm"][k] == lnorm
            assert np.array_equal(hb.last_ss_batch["D"][:, k], raw_stationary(hank, hl, lp, 60)[0]), (name, k)
    finally:
        hb.close()
        hl.close()


def test_values_only(hank):
    """7. dist=False: the value iteration's outputs alone, the same bits; agg_out without D_io is refused"""
    H = hank.hip
    c = case("ks37")
    full = launch_refs(hank, "ks37")["full"]
    hb = batch_block(hank, c)
    try:
        aggs, v, pol, D, iters, status = hb.ss_batch(c["xs"], TOL, dist=False)
        assert aggs is None and D is None and not status.any()
        assert np.array_equal(v, full[1]) and np.array_equal(pol, full[2]) and np.array_equal(iters[:, 0], full[4][:, 0]) and not iters[:, 1].any()
        assert hb.last_ss_batch_timings()[1] == -1.0
        G, ip = hb.G, C.POINTER(C.c_int32)
        x, val, po, ag = H._f(c["xs"][:, :2]), np.ones((G, 2), order="F"), np.empty((G, 2), order="F"), np.empty((1, 2), order="F")
        it, nrm = np.zeros((2, 2), dtype=np.int32), np.zeros(2)
        rc = hb._lib.hank_ss_batch(hb._ctx, 1, H._p(x), 2, TOL, 100, 1e-15, 100, 25, H._p(val), H._p(po), None, H._p(ag), it.ctypes.data_as(ip), H._p(nrm), None)
        assert rc == H.HANK_ERR_BAD_ARG and "D_io" in hb._lib.hank_last_error(hb._ctx).decode()
    finally:
        hb.close()


@pytest.mark.parametrize("name", ("ks50", "wages30"))
def test_the_context_is_left_alone(hank, name):
    """8. between two hank_jvp at one recorded primal, a batch at other prices: the second hank_jvp returns the first one's bits,
    the policy sequence, info() and the memo hit of hank_primal_jvp are unchanged, and so are the counters except vfi_iterations,
    which grows by the sum of the value steps"""
    c = case(name)
    ss = c["ss"]
    hb = batch_block(hank, c)
    try:
        P = hb.P
        t = np.arange(P)
        xa = c["xs"][:, :1] * (1.0 + 0.01 * 0.8 ** t[None, :])
        y = np.random.default_rng(11).standard_normal(xa.shape + (3,))
        hb.set_boundary(np.asarray(ss.value), np.asarray(ss.D))
        agg_a = hb.primal(xa)
        d1 = hb.jvp(y)
        pol1, st1, info1 = hb.policy_seq(), hb.stats(), hb.info()
        res = hb.ss_batch(c["xs"][:, [2, 3, 4]], TOL, n_het=c["n_het"])
        st2, info2 = hb.stats(), hb.info()
        for key in st1:
            if key != "vfi_iterations":
                assert st2[key] == st1[key], (key, st1, st2)
        assert st2["vfi_iterations"] == st1["vfi_iterations"] + int(res[4][:, 0].sum()) and res[4][:, 0].sum() > 0
        assert info2 == info1
        assert np.array_equal(hb.policy_seq(), pol1)
        d2 = hb.jvp(y)
        assert np.array_equal(d2, d1)
        agg_m, d3 = hb.primal_jvp(xa, y)
        assert hb.stats()["primal_memo_hits"] == st1["primal_memo_hits"] + 1 and hb.stats()["primal_sweeps"] == st1["primal_sweeps"]
        assert np.array_equal(agg_m, agg_a) and np.array_equal(d3, d1)
    finally:
        hb.close()


@pytest.mark.parametrize("name", ("ks50", "hank30"))
def test_every_scenario_has_its_own_verdict(hank, name):
    """9. scenario 1 gets a wage of -50. Alone: the oracle refuses it with status 3 and a launch-schedule hank_vfi raises (asserted
    first). The batch: that code as the return value and as status[1], HANK_OK for the others, whose outputs equal the clean
    batch's bit for bit; the message names the scenario; check=False returns the arrays."""
    H = hank.hip
    c = case(name)
    bad = np.array(c["xs"][:, 1], copy=True)
    bad[1] = -50.0
    with pytest.raises(RuntimeError, match="oracle status 3"):
        oracle_vfi(c["orc"], c["shape"], bad)
    hl = vc.block(hank, c["m"], "launch")
    with pytest.raises((hank.DomainError, hank.KnotsNotSortedError)) as alone:
        hl.vfi(np.ones(c["shape"]), bad, TOL)
    hl.close()
    code = alone.value.code
    assert code in (H.HANK_ERR_DOMAIN, H.HANK_ERR_KNOTS)
    xs = np.stack([c["xs"][:, 0], bad, c["xs"][:, 3]], axis=1)
    full = launch_refs(hank, name)["full"]
    hb = batch_block(hank, c)
    try:
        with pytest.raises(hank.HankHIPError, match="scenario 1 of 3") as ei:
            hb.ss_batch(xs, TOL, n_het=c["n_het"])
        assert ei.value.code == code and "step" in str(ei.value)
        raw = hb.last_ss_batch
        assert raw["status"].tolist() == [H.HANK_OK, code, H.HANK_OK]
        got = hb.ss_batch(xs, TOL, n_het=c["n_het"], check=False)
        assert got[5].tolist() == [H.HANK_OK, code, H.HANK_OK]
        assert same(cols(got, [0, 2]), cols(full, [0, 3]))
        assert same(hb.ss_batch(c["xs"], TOL, n_het=c["n_het"]), full), "the context is usable afterwards"
    finally:
        hb.close()


def test_bad_arguments_and_lifetime(hank):
    """10. K outside 1..64, more outputs than declared or than the family has, 1 + r <= 0; and ten contexts created, batched with
    growing K and destroyed in turn: the same bits every time and the device's free memory back where it was (the form of
    test_gpu_primal_batch.py::test_bad_arguments_and_lifetime)"""
    H = hank.hip
    c = case("ks50")
    full = launch_refs(hank, "ks50")["full"]

    def refused(call, code):
        with pytest.raises(hank.HankHIPError) as ei:
            call()
        assert ei.value.code == code, ei.value

    hb = vc.block(hank, c["m"], None)
    refused(lambda: hb.ss_batch(np.zeros((2, 0)), TOL), H.HANK_ERR_BAD_ARG)
    refused(lambda: hb.ss_batch(np.repeat(c["xs"][:, :1], 65, axis=1), TOL), H.HANK_ERR_BAD_ARG)
    refused(lambda: hb.ss_batch(c["xs"][:, :2], TOL, n_het=3), H.HANK_ERR_NOT_READY)
    refused(lambda: hb.ss_batch(c["xs"][:, :2], TOL, n_het=4), H.HANK_ERR_BAD_ARG)        # (Krusell-Smith serves three outputs)
    refused(lambda: hb.ss_batch(c["xs"][:, :2], TOL, vfi_max_iter=0), H.HANK_ERR_BAD_ARG)
    refused(lambda: hb.ss_batch(c["xs"][:, :2], TOL, check_every=0), H.HANK_ERR_BAD_ARG)
    x_neg = np.array(c["xs"][:, :2], copy=True)
    x_neg[0, 1] = -1.5
    with pytest.raises(hank.DomainError, match="scenario 1"):
        hb.ss_batch(x_neg, TOL)
    hb.close()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for cycle in range(10):
        hb = vc.block(hank, c["m"], None)
        K = 2 + cycle % 3
        got = hb.ss_batch(c["xs"][:, :K], TOL, n_het=2)                       # (grown from cycle to cycle: 2, 3, 4)
        grown = hb.ss_batch(c["xs"], TOL, n_het=2)
        hb.close()
        for res, n in ((got, K), (grown, 5)):
            assert np.array_equal(res[0], full[0][:2, :n]) and same(res[1:], cols(full, list(range(n)))[1:]), cycle
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] >= free0 - (2 << 20), (free0, torch.cuda.mem_get_info()[0])


@pytest.mark.parametrize("name", ("ks50", "hank30"))
def test_find_ss_with_batches(hank, name):
    """11. find_ss(batch=True) converges (residual_norm <= eps) to the default loop's free prices (1e-8: the bound
    test_gpu_primal_batch.py uses between step rules; both solves stop at the same eps) in at least one batch, and
    residuals_batch of three price vectors equals three F(p) under `close`"""
    import importlib
    S = importlib.import_module("hank_amd.SteadyState")
    from hank_amd.Aggregation import Residuals
    from conftest import ROOT
    if name == "ks50":
        ov = {"T": 100, "dimensions": {"wealth": {"n": 50}, "productivity": {"n": 2}}}
        m = hank.build_model_from_yaml(str(ROOT / "examples" / "krusell_smith.yaml"), overrides=ov)
    else:
        from hank_amd import OneAssetHANK as oa
        ov = {"T": 10, "dimensions": {"wealth": {"n": 30}, "productivity": {"n": 3}}}
        m = hank.build_model_from_yaml(str(ROOT / "examples" / "one_asset_hank.yaml"), overrides=ov)
        m.params.B = oa.calibrate_bond_supply(m)
    eps = m.compspec.ε
    ss0 = S.find_ss(m, m.ss_initial, "default", vfi="device")
    ss1 = S.find_ss(m, m.ss_initial, "batch", vfi="device", batch=True)
    print(name, "default", ss0.solve_info, "batch", ss1.solve_info)
    assert ss0.solve_info["batches"] == 0 and ss1.solve_info["batches"] >= 1
    assert ss1.solve_info["residual_norm"] <= eps and ss0.solve_info["residual_norm"] <= eps
    asm = S.SSAssembler(m, m.ss_initial, None, "device")
    for k in asm.free_keys:
        assert abs(ss1.vars[k] - ss0.vars[k]) < 1e-8, (k, ss1.vars[k], ss0.vars[k])
    p = np.array([ss0.vars[k] for k in asm.free_keys])
    ps = np.stack([p, p * 1.002, p * 0.999], axis=1)
    Z = S.residuals_batch(asm, ps)
    assert asm._value_warm is None and asm._last_xvals is None
    for k in range(3):
        fresh = S.SSAssembler(m, m.ss_initial, None, "device")
        vc.close(Z[:, k], Residuals(fresh(ps[:, k]), m), what=f"{name} residuals_batch column {k}")
