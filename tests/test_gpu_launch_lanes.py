"""The per-period launches (k_tan_back / k_fused_back, k_tan_fwd / k_fused_fwd; csrc/hank_device.h) at 128 lanes of directions and
more, and at the row-group counts only the dev knobs reach. `tan_rg` (csrc/hank_hip.hip) gives the backward kernels 4 row groups per
wave from NV >= 128 on, NV the lanes' worth of directions: N / 2 for an even N (double2 lanes), N for an odd one. The default
schedule sends such batches to the on-chip wide sweeps where those exist, so the other modules reach that geometry only through
hank_primal_jvp at N = 256 and 300 (tests/test_gpu_wide.py's references: k_fused_back<4, double2>); a model whose n_e has no wide
instance, or whose horizon does not fit LDS, keeps the launches at every width.

  forced launches   Krusell-Smith 50x2 and 37x3 (37 rows: no multiple of 4 row groups x rows per wave), T = 6, at N = 129 (odd:
                    double, NV = 129), N = 256 (even: double2, NV = 128) and N = 130 (NV = 65, two row groups: the control) — the
                    Dual pass, hank_primal + hank_jvp, hank_jvp_het and hank_jvp_boundary against the CPU oracle, linearity
  default schedule  a 40x6 raw grid (n_e = 6 has no wide instance: tests/test_gpu_wide.py's refusal case): N = 129 and 256 are
                    served by the launches, both entry points against the oracle
  dev knobs         HANK_RG_B = 1, 4 and HANK_RG_F = 1, 2, 4 with either forward form (HANK_FWD_SS) on 37x3 at N = 5 and 32: the
                    remaining k_tan_* / k_fused_* instances of the shipped code object, against the oracle and the unknobbed launches

The oracle covers the first cases.N_ORACLE columns of a batch and eight more spread over the rest, the last column included; those
eight come from an oracle call of their own on just those tangents. Tolerance: cases.close (rel 1e-10 + abs 1e-12), 1e-12 against
the unknobbed launches, 1e-9 for linearity. tests/test_geom_host.py holds the widths and tan_rg's threshold together. Which
instances ran is recorded by profiles/launch_lanes_kernel_coverage.txt (scripts/dev_kernel_coverage.py), not asserted here."""
import numpy as np
import pytest

import cases
import sweep_refs
from cases import close

pytestmark = pytest.mark.gpu

T = 6
LANES = (129, 256, 130)                  # NV = 129 (double), 128 (double2), 65 (double2: two row groups, the control)
LAUNCH = cases.FAMILY["launch"]
_CACHE = {}


def _shape(name):
    """-> (HouseholdBlock's arguments, V, D, x (2, 5), oracle)"""
    if name not in _CACHE:
        if name == "40x6":
            from oracle.oracle import Oracle
            args = (np.linspace(0.0, 50.0, 40), np.linspace(0.5, 1.5, 6), np.full((6, 6), 1.0 / 6.0), 0.98, 2.0, 0.0, T)
            orc = Oracle(*args[:6])
            V = np.ones((40, 6))
            for _ in range(20):          # a few value iterations from ones: a decreasing, convex-enough V_T
                st, Vn, _ = orc.value_function(V, 0.015, 1.0, 1)
                assert st == 0
                V = Vn[..., 0]
            t = np.arange(1, T)
            x = np.stack([0.015 + 0.004 * 0.8 ** t, 1.0 + 0.01 * 0.8 ** t])
            _CACHE[name] = (args, V, np.full(240, 1.0 / 240), x, orc)
        else:
            m, V, D, x, orc = cases.shape(*{"50x2": (50, 2), "37x3": (37, 3)}[name], T)
            _CACHE[name] = (cases.model_args(m), V, D, x, orc)
    return _CACHE[name]


def _columns(N):
    """the columns the oracle checks: the first N_ORACLE, and eight more spread over the rest with the last one"""
    first = np.arange(min(N, cases.N_ORACLE))
    rest = np.unique(np.linspace(cases.N_ORACLE, N - 1, 8).round().astype(int)) if N > cases.N_ORACLE else np.arange(0)
    assert rest.size in (0, 8) and (rest.size == 0 or rest[-1] == N - 1)
    return first, rest


def _oracle(name, N, seed=17):
    """y (2, P, N) and, per group of `_columns`, (columns, agg, dagg, policy, dpolicy) of Oracle.block on just those tangents"""
    if (name, N) not in _CACHE:
        args, V, D, x, orc = _shape(name)
        y = np.random.default_rng(seed + N).standard_normal(x.shape + (N,))
        _CACHE[name, N] = (y, [(cols,) + orc.block(x, np.ascontiguousarray(y[:, :, cols]), V, D) for cols in _columns(N) if cols.size])
    return _CACHE[name, N]


def _both_entries(hb, name, N, what):
    """the Dual pass and hank_primal + hank_jvp, each from a record of another x, on the launches, against `_oracle`
    -> (y, dagg of hank_jvp, its policy partials)"""
    _, _, _, x, _ = _shape(name)
    y, refs = _oracle(name, N)
    for entry in ("dual", "tan"):
        hb.primal(x * 1.01)
        if entry == "dual":
            agg, dagg = hb.primal_jvp(x, y)
        else:
            agg, dagg = hb.primal(x), hb.jvp(y)
        assert hb.info()["last_tangent_family_name"] == LAUNCH, (what, entry, hb.info())
        assert dagg.shape == (T - 1, N)
        pol, dpol = hb.policy_seq().transpose(2, 0, 1), hb.dpolicy_seq(N).transpose(2, 0, 1, 3)
        for cols, oagg, odagg, opol, odpol in refs:
            w = f"{what} {entry} columns {cols[0]}..{cols[-1]}"
            close(agg, oagg, what=w + " agg"); close(dagg[:, cols], odagg, what=w + " dagg")
            close(pol, opol, what=w + " policy"); close(dpol[..., cols], odpol, what=w + " dpolicy")
    assert hb.stats()["fallbacks"] == 0
    return y, dagg, dpol


# ---- forced launches --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", LANES)
@pytest.mark.parametrize("name", ("50x2", "37x3"))
def test_launches_at_the_row_group_threshold(hank, oracle_mod, name, N):
    """both entry points against the oracle, and hank_jvp's linearity: jvp(y c) = dagg c"""
    args, V, D, x, orc = _shape(name)
    hb = cases.raw_block(hank, args, "launch")
    try:
        hb.set_boundary(V, D)
        y, dagg, _ = _both_entries(hb, name, N, f"{name} launch N={N}")
        c = np.random.default_rng(N).standard_normal(N)
        comb = hb.jvp(np.tensordot(y, c, axes=([2], [0]))[:, :, None])[:, 0]
        close(comb, dagg @ c, 1e-9, what=f"{name} launch N={N} linearity")
        assert hb.stats()["schedule"] == 0 and hb.stats()["fallbacks"] == 0
    finally:
        hb.close()


@pytest.mark.parametrize("N", LANES[:2])
@pytest.mark.parametrize("name", ("50x2", "37x3"))
def test_het_and_boundary_tangents_at_the_row_group_threshold(hank, oracle_mod, name, N):
    """hank_jvp_het (n_het = 3: Value rides in the forward launches) and hank_jvp_boundary with seeds on the inputs, V_T and D_0, every
    column against the oracle's loop with duals on the boundary (tests/sweep_refs.py)"""
    args, V, D, x, orc = _shape(name)
    rng = np.random.default_rng(3 * N)
    n_a, n_e = V.shape
    y = rng.standard_normal(x.shape + (N,)) * 1e-2
    dV = rng.standard_normal((n_a, n_e, N)) * np.abs(V)[:, :, None]
    dD = rng.uniform(0.0, 1.0, (n_a, n_e, N)) * (1.0 + np.arange(n_e))[None, :, None] / (n_a * n_e)
    ref = sweep_refs.oracle_sweeps(orc, x, V, D, args[4], 3, y=y, dV=dV, dD=dD)
    hb = cases.raw_block(hank, args, "launch")
    try:
        hb.set_boundary(V, D)
        hb.set_het_outputs(3)
        hb.primal(x)
        what = f"{name} launch N={N}"
        got = hb.jvp_het(y, dV, dD, n_het=3)
        assert got.shape == (T - 1, 3, N) and hb.info()["last_tangent_family_name"] == LAUNCH
        for o in range(3):
            assert np.abs(ref["dagg"][:, o]).max() > 1e-6
            close(got[:, o, :], ref["dagg"][:, o, :], what=f"{what} jvp_het output {o}")
        close(hb.dpolicy_seq(N).transpose(2, 0, 1, 3), ref["dpol"], what=what + " jvp_het dpolicy")
        close(hb.jvp_boundary(y, dV, dD), ref["dagg"][:, 0], what=what + " jvp_boundary")
        close(hb.dpolicy_seq(N).transpose(2, 0, 1, 3), ref["dpol"], what=what + " jvp_boundary dpolicy")
        agg2, dagg2 = hb.grid_aggregates(N)
        close(agg2, ref["agg2"], what=what + " grid aggregate"); close(dagg2, ref["dagg2"], what=what + " grid aggregate's partials")
        assert hb.stats()["fallbacks"] == 0
    finally:
        hb.close()


# ---- the default schedule where the wide sweeps do not exist ----------------------------------------------------------------------
@pytest.mark.parametrize("N", LANES[:2])
def test_default_schedule_keeps_the_launches_without_a_wide_instance(hank, oracle_mod, N):
    """n_e = 6: wide_supported == 0, so a batch of 129 or 256 directions stays on the launches under the default schedule"""
    args, V, D, x, orc = _shape("40x6")
    hb = cases.raw_block(hank, args, None)
    try:
        info = hb.info()
        assert info["wide_supported"] == 0 and info["wide_mode"] == 0, info
        hb.set_boundary(V, D)
        _both_entries(hb, "40x6", N, f"40x6 default N={N}")
        assert hb.stats()["fallbacks"] == 0
    finally:
        hb.close()


# ---- the dev knobs' geometries ----------------------------------------------------------------------------------------------------
# (an odd width runs the `double` instance of a kernel, an even one the `double2` instance: every knob takes both)
KNOBS = [({"HANK_RG_B": 1}, (5, 32)), ({"HANK_RG_B": 4}, (5, 32)), ({"HANK_RG_F": 1, "HANK_FWD_SS": 1}, (5, 32)),
         ({"HANK_RG_F": 2, "HANK_FWD_SS": 0}, (5, 32)), ({"HANK_RG_F": 4, "HANK_FWD_SS": 0}, (5, 32)), ({"HANK_RG_F": 4, "HANK_FWD_SS": 1}, (5, 32))]
_PLAIN = {}


def _plain(hank, N):
    """the unknobbed launches on 37x3: (dagg of hank_jvp, its policy partials), once per width"""
    if N not in _PLAIN:
        args, V, D, x, orc = _shape("37x3")
        hl = cases.raw_block(hank, args, "launch")
        try:
            hl.set_boundary(V, D)
            _PLAIN[N] = _both_entries(hl, "37x3", N, f"37x3 launch N={N}")[1:]
        finally:
            hl.close()
    return _PLAIN[N]


@pytest.mark.parametrize("knobs,widths", KNOBS, ids=lambda v: "-".join(f"{k[5:]}={q}" for k, q in v.items()) if isinstance(v, dict) else None)
def test_row_group_knobs(hank, oracle_mod, knobs, widths):
    """a fresh context per knob, the knob set around its sweeps as well (tan_rg reads it when a width's workspace is built): both
    entry points against the oracle, hank_jvp and its policy partials against the unknobbed launches at 1e-12"""
    args, V, D, x, orc = _shape("37x3")
    for N in widths:
        dagg0, dpol0 = _plain(hank, N)
        with cases.hank_env(**knobs):
            hb = cases.raw_block(hank, args, "launch", **knobs)
            try:
                hb.set_boundary(V, D)
                what = f"37x3 {knobs} N={N}"
                _, dagg, dpol = _both_entries(hb, "37x3", N, what)
                close(dagg, dagg0, 1e-12, what=what + " dagg vs the unknobbed launches")
                close(dpol, dpol0, 1e-12, what=what + " dpolicy vs the unknobbed launches")
            finally:
                hb.close()
