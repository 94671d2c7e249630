"""hank_vjp: the transposed sweeps of the household block (csrc/hank_adjoint.h) on the MI355X.
x̄ = J(x)ᵀ ȳ is checked (1) against the CPU oracle's Jacobian, transposed, for both value-function families, both outputs,
records written by the launches and by the persistent sweeps, and batch widths 1, 5, 32, 33; (2) Sweep A alone against a numpy
restatement of the reference's ForwardIteration_pullback (ForwardIteration.jl:394-410, with the reverse rule of
transition_step, :164-189) and by the pairing with the policy partials; (3) at the benched size by projection on 32 oracle JVP
columns; (4) the context's state rules; (5) the host layers. Tolerance: the suite's rel 1e-10 + abs 1e-12 on the largest entry
of the compared array unless stated."""
import numpy as np
import pytest

import cases
from cases import block as _block, close as _close, forward_iteration_pullback as _forward_iteration_pullback, jt as _jt, oracle_jacobian
from conftest import ks_paths, ks_setup

pytestmark = pytest.mark.gpu

_JCACHE = {}


def _ks_case():
    if "ks" not in _JCACHE:
        m, ss, orc = ks_setup(130, 3, 40)
        x, _ = ks_paths(m, ss, "x1", 0.05)
        _JCACHE["ks"] = (m, ss, x[2:4], oracle_jacobian(orc, ss.value, ss.D, x[2:4]))
    return _JCACHE["ks"]


def _hank_case():
    if "hank" not in _JCACHE:
        m, ss = cases.hank_economy(80, 3, 40)
        x = cases.hank_x(ss, m.compspec.T - 1)
        orc = cases.oracle_of(m)
        J2 = oracle_jacobian(orc, ss.value, ss.D, x)
        # n_het = 1 from Oracle.household_block (the one-variable block): its own unit-tangent Jacobian
        n_hh, P = x.shape
        dagg = orc.block(x, cases.unit_tangents(n_hh, P), ss.value, ss.D)[1]
        _JCACHE["hank"] = (m, ss, x, J2, np.ascontiguousarray(dagg.reshape(P, P, n_hh).transpose(0, 2, 1)))
    return _JCACHE["hank"]


# ---- 1. against the oracle's Jacobian, transposed -------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 5, 32, 33])
@pytest.mark.parametrize("n_het", [1, 2])
@pytest.mark.parametrize("schedule", ["launch", "xcd"])
def test_vjp_is_the_oracle_jacobian_transposed_krusell_smith_130x3(hank, oracle_mod, schedule, n_het, M):
    m, ss, x, J = _ks_case()
    P = x.shape[1]
    yb = np.random.default_rng(10 * M + n_het).standard_normal((P, n_het, M))
    hb = _block(hank, m, schedule)
    try:
        hb.set_boundary(ss.value, ss.D)
        hb.primal(x)
        assert hb.stats()["schedule"] == (0 if schedule == "launch" else 1)
        got = hb.vjp(yb, n_het)
        assert got.shape == (2, P, M)
        _close(got, _jt(J[:n_het], yb))
    finally:
        hb.close()


@pytest.mark.parametrize("M", [1, 5, 32, 33])
@pytest.mark.parametrize("n_het", [1, 2])
@pytest.mark.parametrize("schedule", ["launch", "xcd"])
def test_vjp_is_the_oracle_jacobian_transposed_one_asset_hank_80x3(hank, oracle_mod, schedule, n_het, M):
    m, ss, x, J2, J1 = _hank_case()
    P = x.shape[1]
    yb = np.random.default_rng(10 * M + n_het).standard_normal((P, n_het, M))
    hb = _block(hank, m, schedule)
    try:
        assert hb.n_hh == 3
        hb.set_boundary(ss.value, ss.D)
        hb.primal(x)
        got = hb.vjp(yb, n_het)
        _close(got, _jt(J1[None], yb) if n_het == 1 else _jt(J2, yb))
    finally:
        hb.close()


# ---- 2. Sweep A alone against the reference's rule ------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", ["launch", "xcd"])
def test_policy_cotangent_is_the_reference_pullback_and_pairs_with_the_policy_partials(hank, oracle_mod, schedule):
    m, ss, x, J = _ks_case()
    P, M = x.shape[1], 6
    rng = np.random.default_rng(5)
    yb = rng.standard_normal((P, 1, M))
    hb = _block(hank, m, schedule)
    try:
        hb.set_boundary(ss.value, ss.D)
        hb.primal(x)
        hb.vjp(yb, 1)
        pbar = hb.policy_cotangent_seq(M)                       # (n_a, n_e, P, M)
        pol, Dseq = hb.policy_seq(), hb.dist_seq()
        D0 = np.asarray(ss.D).reshape(hb.n_a, hb.n_e, order="F")
        for k in (0, M - 1):
            ref = _forward_iteration_pullback(hb.a_grid, hb.Pi, pol, D0, Dseq, yb[:, 0, k])
            _close(pbar[..., k], ref, rel=1e-11, ab=0.0)
        # <pbar, dpol> = <ybar, dagg> for a JVP batch at the same record (the aggregate moves through the policy partials alone)
        y = rng.standard_normal((2, P, M))
        dagg = hb.jvp(y)
        dpol = hb.dpolicy_seq(M)
        lhs, rhs = np.einsum("aetm,aetn->mn", pbar, dpol), np.einsum("tm,tn->mn", yb[:, 0, :], dagg)
        terms = np.einsum("aetm,aetn->mn", np.abs(pbar), np.abs(dpol))
        print(f"pairing: max |lhs - rhs| / sum|terms| = {np.max(np.abs(lhs - rhs) / terms):.3e}")
        assert np.all(np.abs(lhs - rhs) <= 1e-12 * terms)
        assert np.array_equal(hb.policy_cotangent_seq(M), pbar)         # the JVP batch left the cotangent batch alone
    finally:
        hb.close()


# ---- 3. full size, oracle-pinned by projection ----------------------------------------------------------------------------
def test_full_size_2000x11_T300_M32_by_projection_on_oracle_columns(hank, oracle_mod):
    m, ss, xhh, y, Jy2 = cases.fullsize_oracle_columns()              # (computed once; tests/test_gpu_vjp_variants.py reads both aggregates)
    hb = hank.household_block(m)
    hb.set_boundary(ss.value, ss.D)
    P, M = 299, 32
    Jy = Jy2[0]                                                 # (P, 32): (J y_n)_oracle of the policy variable's aggregate
    yb = np.random.default_rng(1).standard_normal((P, 1, M))
    hb.primal(xhh)
    xbar = hb.vjp(yb, 1)                                        # (2, P, M)
    lhs = np.einsum("tm,tn->mn", yb[:, 0, :], Jy)
    rhs = np.einsum("ktm,ktn->mn", xbar, y)
    scale = np.einsum("tm,tn->mn", np.abs(yb[:, 0, :]), np.abs(Jy))
    print(f"projection: max |lhs - rhs| / scale = {np.max(np.abs(lhs - rhs) / scale):.3e}")
    assert np.all(np.abs(lhs - rhs) <= 1e-10 * scale)
    t = hb.last_vjp_timings()
    assert t["sweep_a"]["ms"] > 0 and t["sweep_b"]["ms"] > 0 and t["sweep_a"]["launches"] == P


# ---- 4. state -----------------------------------------------------------------------------------------------------------
def test_state_rules(hank, oracle_mod):
    import torch
    from hank_amd.hip import HANK_ERR_BAD_ARG, HANK_ERR_NOT_READY
    m, ss, x, J = _ks_case()
    P = x.shape[1]
    rng = np.random.default_rng(2)
    yb = rng.standard_normal((P, 2, 32))
    hb = _block(hank, m, "launch")
    try:
        def code(fn):
            with pytest.raises(hank.HankHIPError) as e:
                fn()
            return e.value.code
        hb.set_boundary(ss.value, ss.D)
        assert code(lambda: hb.vjp(yb, 2)) == HANK_ERR_NOT_READY                  # before a primal
        hb.primal(x)
        assert code(lambda: hb.vjp(np.zeros((P, 1, 0)), 1)) == HANK_ERR_BAD_ARG   # M = 0
        assert code(lambda: hb.vjp(yb, 0)) == HANK_ERR_BAD_ARG
        with pytest.raises(hank.HankHIPError, match="not affine") as e3:
            hb.vjp(np.zeros((P, 3, 4)), 3)
        assert e3.value.code == HANK_ERR_BAD_ARG
        assert code(lambda: hb.policy_cotangent_seq(32)) == HANK_ERR_NOT_READY    # no cotangent batch yet
        # the tangent readers are served the same bits before and after
        y = rng.standard_normal((2, P, 4))
        hb.jvp(y)
        dpol0, het0 = hb.dpolicy_seq(4), hb.het_outputs(2, y)
        alloc0 = hb.stats()["tangent_workspaces_allocated"]
        xb = hb.vjp(yb, 2)
        assert np.array_equal(hb.dpolicy_seq(4), dpol0)
        het1 = hb.het_outputs(2, y)
        assert np.array_equal(het1[0], het0[0]) and np.array_equal(het1[1], het0[1])
        _close(xb, _jt(J, yb))
        # the same input, the same bits; zero in, exact zeros out
        pb = hb.policy_cotangent_seq(32)
        assert np.array_equal(hb.vjp(yb, 2), xb) and np.array_equal(hb.policy_cotangent_seq(32), pb)
        z = hb.vjp(np.zeros_like(yb), 2)
        assert not z.any() and not hb.policy_cotangent_seq(32).any()
        # a column alone and inside a batch of 32; width changes allocate nothing new
        alloc1 = hb.stats()["tangent_workspaces_allocated"]
        assert alloc1 == alloc0 + 1
        one = hb.vjp(yb[:, :, 7:8], 2)
        assert np.max(np.abs(one[:, :, 0] - xb[:, :, 7])) <= 1e-13 * np.abs(xb[:, :, 7]).max()
        assert code(lambda: hb.policy_cotangent_seq(32)) == HANK_ERR_NOT_READY    # the current batch is the M = 1 one
        hb.vjp(yb, 2)
        assert hb.stats()["tangent_workspaces_allocated"] == alloc1 + 1
        hb.vjp(yb[:, :, 7:8], 2); hb.vjp(yb, 2)
        assert hb.stats()["tangent_workspaces_allocated"] == alloc1 + 1
        # the device-pointer form: bit for bit
        d_in = torch.from_numpy(np.asfortranarray(yb).reshape(-1, order="F").copy()).cuda()
        d_out = torch.empty(2 * P * 32, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        hb.vjp_dev(2, d_in.data_ptr(), 32, d_out.data_ptr())
        hb.sync()
        assert np.array_equal(d_out.cpu().numpy().reshape((2, P, 32), order="F"), xb)
        # a new primal, a new boundary
        hb.primal(x)
        assert code(lambda: hb.policy_cotangent_seq(32)) == HANK_ERR_NOT_READY
        assert np.array_equal(hb.vjp(yb, 2), xb)
        hb.set_boundary(ss.value * 1.0001, ss.D)
        assert code(lambda: hb.vjp(yb, 2)) == HANK_ERR_NOT_READY
        assert code(lambda: hb.policy_cotangent_seq(32)) == HANK_ERR_NOT_READY
    finally:
        hb.close()


def test_the_wide_familys_record_is_served(hank, oracle_mod):
    m, ss, x, J = _ks_case()
    P = x.shape[1]
    hb = _block(hank, m, None)
    try:
        hb.set_boundary(ss.value, ss.D)
        y = np.random.default_rng(3).standard_normal((2, P, 120))
        hb.primal_jvp(x, y)
        assert hb.info()["last_tangent_family_name"] == "on-chip-wide"
        yb = np.random.default_rng(4).standard_normal((P, 2, 5))
        _close(hb.vjp(yb, 2), _jt(J, yb))
        assert hb.dpolicy_seq(120).shape[-1] == 120                # the wide batch is still current
    finally:
        hb.close()


# ---- 5. host layers -------------------------------------------------------------------------------------------------------
def _pairing(lin, seed):
    n = lin.x.size
    rng = np.random.default_rng(seed)
    y, yb = rng.standard_normal((n, 3)), rng.standard_normal((n, 4))
    lhs, rhs = yb.T @ lin.jvp(y), lin.vjp(yb).T @ y
    print(f"<ybar, J y> vs <J' ybar, y>: {np.max(np.abs(lhs - rhs)) / np.abs(lhs).max():.3e}")
    assert np.max(np.abs(lhs - rhs)) <= 1e-11 * np.abs(lhs).max()


def test_linearized_function_krusell_smith(hank, oracle_mod):
    m, ss, _ = ks_setup(130, 3, 40)
    x, Z = ks_paths(m, ss, "x1", 0.05)
    lin = hank.LinearizedFunction(x.reshape(-1, order="F"), {"Z": Z}, m, ss, ss)
    n = lin.x.size
    assert n == 156
    _pairing(lin, 0)
    Jd, JTd = lin.jvp(np.eye(n)), lin.vjp(np.eye(n))
    _close(JTd, Jd.T)
    op = lin.as_linear_operator()
    _close(op.matmat(np.eye(n)), Jd, rel=1e-13)
    _close(op.rmatmat(np.eye(n)), JTd, rel=1e-13)
    _close(hank.VJP(hank.make_fullFunction({"Z": Z}, m, ss, ss), lin.x, np.eye(n)[:, :3]), JTd[:, :3], rel=1e-13)


def test_linearized_function_goods_market_hank_two_outputs(hank, oracle_mod):
    from examples.solve_hank import build
    m, ss = build(80, 3, 40, "one_asset_hank_goods.yaml")
    P = m.compspec.T - 1
    keys = hank.vars_of_type(m, "endogenous")
    x0 = np.tile(np.array([ss.vars[k] for k in keys]), P) * (1 + 1e-4 * np.random.default_rng(0).standard_normal(len(keys) * P))
    lin = hank.LinearizedFunction(x0, {"ei": 0.0025 * 0.6 ** np.arange(P)}, m, ss, ss)
    assert lin._n_out == 2
    _pairing(lin, 1)


def test_sticky_wage_model_is_refused(hank, oracle_mod):
    from examples.solve_hank import build
    m, ss = build(80, 3, 40, "one_asset_hank_wages.yaml")
    P = m.compspec.T - 1
    keys = hank.vars_of_type(m, "endogenous")
    x0 = np.tile(np.array([ss.vars[k] for k in keys]), P)
    lin = hank.LinearizedFunction(x0, {"ei": np.zeros(P)}, m, ss, ss)
    with pytest.raises(NotImplementedError, match="not affine"):
        lin.vjp(np.ones(x0.size))
