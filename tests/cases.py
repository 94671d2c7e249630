"""The one case module of the suite: what the GPU modules (tests/test_gpu_*.py) and the CPU tests of their preconditions
(tests/test_vjp_host.py, tests/test_cases_host.py) share. Nothing here needs a GPU except `raw_block` / `block`, which create a
device context.

0. the owners: `close` (the suite's only tolerance function), `raw_block` / `block` (a context under HANK_* variables, every
   variable restored), `model_args` / `oracle_of` (a model's constructor arguments), `hank_economy` / `hank_x` (the one-asset HANK
   economy and its input path). The oracle's references are methods of oracle.oracle.Oracle: block, block_het, het_outputs, vfi;
1. the references of hank_vjp[_het]: the CPU oracle's Jacobian from unit tangents (`oracle_jacobian`, `oracle_jacobian_het` /
   `jacobian_het` for every heterogeneous output, transposed by `jt`) and the numpy
   restatement of the reference's ForwardIteration_pullback for Sweep A alone (`forward_iteration_pullback`);
2. the economies of the variant suite: `economy` (a curvature, its own host steady state), `shape` (a grid shape with a cheap
   valid boundary), `CASES` (curvature x record layout);
3. raw-grid economies (`raw_economy`, `EDGE_GRIDS`) whose oracle policy holds the data-dependent edges the calibrated grids never
   show — a deep clamped prefix, many sources clamped at the top, long runs of rows in one bracket — and `edge_stats`, which
   measures those edges on a policy."""
import os

import numpy as np

from conftest import ROOT, ks_paths, ks_setup


def close(a, b, rel=1e-10, ab=1e-12, what=""):
    """the suite's tolerance: rel 1e-10 + abs 1e-12 on the largest entry of the reference b, no floor on that scale; equal shapes
    (nothing broadcasts); prints the figure before it asserts. A NaN on either side fails it."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err, scale = np.max(np.abs(a - b)), np.abs(b).max()
    print(f"{what}: max err {err:.3e} vs scale {scale:.3e} (bound {ab + rel * scale:.3e})")
    assert err <= ab + rel * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def raw_block(hank, args, schedule, **env):
    """hank.HouseholdBlock(*args) created under HANK_SCHEDULE=schedule (None: the default) and the given HANK_* variables."""
    env = {"HANK_SCHEDULE": schedule, **env}
    old = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        return hank.HouseholdBlock(*args)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def raw_args(grid, z, Pi, m, T):
    """the raw HouseholdBlock constructor's arguments for model m's preferences on (grid, z, Pi)."""
    return (grid, z, Pi, m.params.β, m.params.γ, m.params.borrow_cons, T, m.value_fn.value_fn_id)


def model_args(m):
    """the eight constructor arguments of hank.HouseholdBlock for model m."""
    wd, pd_ = m.heterogeneity["wealth"], m.heterogeneity["productivity"]
    return raw_args(wd.grid, pd_.grid, pd_.transition, m, m.compspec.T)


def oracle_of(m):
    """the CPU oracle of model m's household block."""
    from oracle.oracle import Oracle
    return Oracle(*model_args(m)[:6])


def block(hank, m, schedule, **env):
    """a context of model m created under HANK_SCHEDULE=schedule (None: the default) and the given HANK_* variables."""
    return raw_block(hank, model_args(m), schedule, **env)


_HANK = {}


def hank_economy(n_a, n_e, T, spec="one_asset_hank.yaml"):
    """(model, steady state) of examples.solve_hank.build, cached per size and model file."""
    key = (n_a, n_e, T, spec)
    if key not in _HANK:
        from examples.solve_hank import build
        _HANK[key] = build(n_a, n_e, T, spec)
    return _HANK[key]


def hank_x(ss, P):
    """the household inputs (r, om, Tr) (3, P) of the one-asset HANK tests: geometric deviations from the steady state."""
    t = np.arange(P)
    return np.stack([ss.vars["r"] + 0.002 * 0.8 ** t, ss.vars["om"] * (1 + 0.01 * 0.7 ** t), ss.vars["Tr"] * (1 - 0.02 * 0.9 ** t)])


# ---- 1. references --------------------------------------------------------------------------------------------------------
def unit_tangents(n_hh, P):
    """y (n_hh, P, n_hh P): a unit shock to input k at period s in column k + n_hh s (the layout of dxhh)."""
    y = np.zeros((n_hh, P, n_hh * P))
    for s in range(P):
        for k in range(n_hh):
            y[k, s, k + n_hh * s] = 1.0
    return y


def oracle_jacobian(orc, value, D, x):
    """J (2, P, n_hh, P): d (savings, consumption aggregate)_t / d input k at period s, from unit tangents through the CPU
    oracle's two-variable household block."""
    n_hh, P = x.shape
    _, dagg = orc.block_het(x, unit_tangents(n_hh, P), value, D)
    return np.ascontiguousarray(dagg.reshape(2, P, P, n_hh).transpose(0, 1, 3, 2))


def oracle_jacobian_het(orc, value, D, x, n_het, gamma):
    """J (n_het, P, n_hh, P): d output o at t / d input k at s, from unit tangents through Oracle.het_outputs, 32 columns per pass"""
    n_hh, P = x.shape
    y = unit_tangents(n_hh, P)
    dagg = np.concatenate([orc.het_outputs(x, y[:, :, c0:c0 + 32], value, D, n_het, gamma)[1] for c0 in range(0, n_hh * P, 32)], axis=2)
    return np.ascontiguousarray(dagg.reshape(n_het, P, P, n_hh).transpose(0, 1, 3, 2))


_JHET = {}


def jacobian_het(key, orc, V, D, x, n_het, gamma):
    """`oracle_jacobian_het` of a case, once per session and key; every output's block must be non-trivial"""
    if key not in _JHET:
        _JHET[key] = oracle_jacobian_het(orc, V, D, x, n_het, gamma)
        assert all(np.abs(_JHET[key][o]).max() > 1e-3 for o in range(n_het)), key
    return _JHET[key]


def jt(J, yb):
    """J (n_het, P, n_hh, P), yb (P, n_het, M) -> (n_hh, P, M)"""
    return np.einsum("otks,tom->ksm", J, yb)


def forward_iteration_pullback(grid, Pi, pol, D0, Dseq, yb):
    """ForwardIteration_pullback (ForwardIteration.jl:394-410) with transition_pullback (:164-189) for the policy variable:
    pol, Dseq (n_a, n_e, P), yb (P,) -> Δpolicy (n_a, n_e, P)."""
    n_a, n_e, P = pol.shape
    cols = np.arange(n_e)[None, :]
    dD = np.zeros((n_a, n_e))
    out = np.zeros((n_a, n_e, P))
    for t in range(P - 1, -1, -1):
        Dt, Dprev = Dseq[:, :, t], (Dseq[:, :, t - 1] if t > 0 else D0)
        dD = dD + yb[t] * pol[:, :, t]                          # :399
        out[:, :, t] += yb[t] * Dt                              # :400
        u = dD @ Pi.T                                           # Λ_exog' ΔD (:166): u[r, e] = sum_e2 Pi[e, e2] ΔD[r, e2]
        m0 = np.searchsorted(grid, pol[:, :, t], side="left")   # searchsortedfirst, 0-based (:146)
        interior = (m0 > 0) & (m0 < n_a)
        hi, lo = np.clip(m0, 1, n_a - 1), np.clip(m0, 1, n_a - 1) - 1
        gap = grid[hi] - grid[lo]
        out[:, :, t] += np.where(interior, Dprev * (u[hi, cols] - u[lo, cols]) / gap, 0.0)      # :176-182
        w = (pol[:, :, t] - grid[lo]) / gap
        dD = np.where(m0 == 0, u[0, cols], np.where(m0 >= n_a, u[n_a - 1, cols], (1 - w) * u[lo, cols] + w * u[hi, cols]))   # Λ_endog' u (:169)
    return out


# ---- 2. the variant suite's economies -------------------------------------------------------------------------------------
# case: (gamma, HANK_RECORD_DIET or None, the record diet the context must report)
CASES = {
    "gamma1": (1.0, None, 1),             # pow_crra: rcp | rcp; diet on, its gamma = 1 arm
    "gamma0.5": (0.5, None, 0),           # rcp(x^2) | rsqrt: the fast paths swap halves; diet off
    "gamma1.5": (1.5, None, 0),           # pow | pow
    "gamma3": (3.0, None, 0),
    "gamma2-nodiet": (2.0, "0", 0),       # rsqrt | rcp(x^2), kc and v read from the record
    "gamma1-nodiet": (1.0, "0", 0),
}


_ECON = {}


def economy(family, gamma):
    """(model, steady state, household inputs (n_hh, P), oracle) of Krusell-Smith 130x3 or one-asset HANK 80x3, T = 40, at gamma:
    a fresh model, its gamma set, its steady state solved on the host (cached per family and gamma)."""
    key = (family, gamma)
    if key not in _ECON:
        import hank_amd as h
        spec, n_a = ("krusell_smith.yaml", 130) if family == "ks" else ("one_asset_hank.yaml", 80)
        m = h.build_model_from_yaml(str(ROOT / "examples" / spec), overrides={"T": 40, "dimensions": {"wealth": {"n": n_a}, "productivity": {"n": 3}}})
        m.params.γ = gamma
        if family == "hank":
            from hank_amd import OneAssetHANK as oa
            m.params.B = oa.calibrate_bond_supply(m)
        ss, _ = h.get_SteadyStates(m, vfi="host")
        assert m.params.γ == gamma
        P = m.compspec.T - 1
        xhh = ks_paths(m, ss, "x1", 0.05)[0][2:4] if family == "ks" else hank_x(ss, P)
        _ECON[key] = (m, ss, np.ascontiguousarray(xhh), oracle_of(m))
    return _ECON[key]


_SHAPE = {}


def shape(n_a, n_e, T):
    """Krusell-Smith of the given shape at gamma = 2 with a cheap valid boundary: V_T the 200th host VFI iterate from ones at the
    130x3 steady state's prices, D_0 uniform; the x1 path of those prices (cached per shape)."""
    key = (n_a, n_e, T)
    if key not in _SHAPE:
        import hank_amd as h
        m = h.build_model_from_yaml(str(ROOT / "examples" / "krusell_smith.yaml"),
                                    overrides={"T": T, "dimensions": {"wealth": {"n": n_a}, "productivity": {"n": n_e}}})
        assert m.params.γ == 2.0
        _, ss0, _, _ = economy("ks", 2.0)
        xv = {"r": ss0.vars["r"], "w": ss0.vars["w"]}
        V = np.ones((n_a, n_e))
        for _ in range(200):
            V = m.value_fn.host_steady_state_step(V, xv, m)["Value"]
        D = np.full(n_a * n_e, 1.0 / (n_a * n_e))
        P = T - 1
        t = np.arange(1, P + 1)
        xhh = np.stack([xv["r"] + 0.004 * 0.8 ** t, xv["w"] * (1.0 + 0.01 * 0.8 ** t)])
        _SHAPE[key] = (m, V, D, xhh, oracle_of(m))
    return _SHAPE[key]


def shape_one_column(n_a, T):
    """`shape` at n_e = 1, which no model file describes: the raw constructors' arguments. The wealth grid, prices and preferences
    of shape(n_a, 2, T), z = [1], Pi = [[1]]; V_T the 200th iterate of the oracle's ValueFunction from ones, D_0 uniform.
    -> (HouseholdBlock's arguments, V, D, xhh, oracle)"""
    key = (n_a, 1, T)
    if key not in _SHAPE:
        from oracle.oracle import Oracle
        m, _, _, xhh, _ = shape(n_a, 2, T)
        grid, z, Pi = m.heterogeneity["wealth"].grid, np.array([1.0]), np.array([[1.0]])
        orc = Oracle(grid, z, Pi, m.params.β, m.params.γ, m.params.borrow_cons)
        _, ss0, _, _ = economy("ks", 2.0)
        V = np.ones((n_a, 1))
        for _ in range(200):
            st, Vn, _ = orc.value_function(V, ss0.vars["r"], ss0.vars["w"], 1)
            assert st == 0
            V = Vn[..., 0]
        _SHAPE[key] = (raw_args(grid, z, Pi, m, T), V, np.full(n_a, 1.0 / n_a), xhh, orc)
    return _SHAPE[key]


_FULL = {}


def fullsize_oracle_columns():
    """the benched size (Krusell-Smith 2000x11, T = 300, the x1 path at shock 0.01): J y of BOTH aggregates for 32 random
    directions y (2, 299, 32), through the CPU oracle's two-variable household block — four passes of eight partials, one host
    thread each, computed once per session. -> (m, ss, xhh (2, 299), y, Jy (2, 299, 32))"""
    if not _FULL:
        from concurrent.futures import ThreadPoolExecutor
        m, ss, orc = ks_setup(2000, 11, 300)
        xhh = np.ascontiguousarray(ks_paths(m, ss, "x1", 0.01)[0][2:4])
        P = xhh.shape[1]
        y = np.random.default_rng(0).standard_normal((2, P, 32))

        with ThreadPoolExecutor(max_workers=4) as ex:
            Jy = np.concatenate(list(ex.map(lambda c0: orc.block_het(xhh, y[:, :, c0:c0 + 8], ss.value, ss.D)[1], range(0, 32, 8))), axis=2)
        _FULL["case"] = (m, ss, xhh, y, Jy)
    return _FULL["case"]


# ---- 3. raw-grid economies ------------------------------------------------------------------------------------------------
# Krusell-Smith 130x3's productivity process, prices and preferences on a wealth grid of one's own; what each grid's oracle policy
# shows was measured on the CPU and is asserted by tests/test_vjp_host.py (EDGE_NEEDS: clo >= 8, >= 8 top-clamped, long runs)
EDGE_GRIDS = {
    "dense-bottom": lambda: 200.0 * np.linspace(0.0, 1.0, 600) ** 4,      # clo 32..48 in the low-income column, runs up to 52
    "short-top": lambda: np.linspace(0.0, 2.0, 257),                      # up to 46 sources capped at the top; clo <= 2
    "both": lambda: 1.0 * np.linspace(0.0, 1.0, 192) ** 4,                # clo 39..58, up to 21 capped at the top, runs up to 58
}
EDGE_NEEDS = {"dense-bottom": ("clo", "runs"), "short-top": ("top",), "both": ("clo", "top", "runs")}
EDGE_WIDTHS = (1, 4, 32, 33)          # hank_vjp's batch widths on these economies: R = 64, 32, 8, 8 rows per block
EDGE_P = 9
_RAW = {}


def raw_economy(name):
    """-> dict(args: HouseholdBlock's, grid, Pi, V (n_a, 3), D (n_a * 3,), x (2, 9), orc): EDGE_GRIDS[name] under the
    Krusell-Smith 130x3 calibration; V_T that economy's steady-state value interpolated onto the grid, D_0 uniform, the inputs the
    first 9 periods of its x1 path (shock 0.05)."""
    if name not in _RAW:
        from oracle.oracle import Oracle
        m, ss, _ = ks_setup(130, 3, 40)
        wd, pdm = m.heterogeneity["wealth"], m.heterogeneity["productivity"]
        grid = np.ascontiguousarray(EDGE_GRIDS[name]())
        n_a, n_e = grid.size, pdm.grid.size
        V = np.stack([np.interp(grid, wd.grid, np.asarray(ss.value)[:, e]) for e in range(n_e)], axis=1)
        D = np.full(n_a * n_e, 1.0 / (n_a * n_e))
        x = np.ascontiguousarray(ks_paths(m, ss, "x1", 0.05)[0][2:4, :EDGE_P])
        orc = Oracle(grid, pdm.grid, pdm.transition, m.params.β, m.params.γ, m.params.borrow_cons)
        _RAW[name] = dict(args=raw_args(grid, pdm.grid, pdm.transition, m, EDGE_P + 1), grid=grid, Pi=np.asarray(pdm.transition), V=V, D=D,
                          x=x, orc=orc)
    return _RAW[name]


def edge_stats(grid, pol):
    """the data-dependent edges of a policy sequence pol (P, n_a, n_e) on `grid`: clo (P, n_e), the rows of the clamped prefix
    (pol <= grid[0]: searchsortedfirst gives the first point, all mass on row 0); top (P, n_e), the sources clamped at the top
    (the value function caps the policy at the last grid point, so pol >= grid[-1]: a flat top, one long lottery segment and no
    interpolation weight); runs {length: count}, the runs of unclamped rows of one column that share a bracket
    (searchsorted(grid, pol))."""
    P, n_a, n_e = pol.shape
    m0 = np.searchsorted(grid, pol, side="left")
    low, high = m0 == 0, pol >= grid[-1]
    clo, top = low.sum(axis=1), high.sum(axis=1)
    runs = {}
    for t in range(P):
        for e in range(n_e):
            b = m0[t, :, e][~(low[t, :, e] | high[t, :, e])]
            if b.size:
                edges = np.flatnonzero(np.diff(b)) + 1
                for ln in np.diff(np.concatenate([[0], edges, [b.size]])):
                    runs[int(ln)] = runs.get(int(ln), 0) + 1
    return clo, top, dict(sorted(runs.items()))


def adj_rows_per_block(M):
    """R of hank_vjp's lane geometry at batch width M (build_cotwork, csrc/hank_hip.hip): two columns per lane for an even M, at
    most 16 lanes across the columns, RB = 64 / NC rows per wave instruction, R = max(RB, 8)."""
    MV = M // 2 if M % 2 == 0 else M
    NC = 1
    while NC < MV and NC < 16:
        NC *= 2
    return max(64 // NC, 8)


def check_edges(name, grid, pol):
    """measure and print the edges of EDGE_GRIDS[name] on the policy sequence pol (P, n_a, n_e), and assert the ones EDGE_NEEDS
    promises. -> {"clo_lt_nb": bool, "clo_gt_nb": bool}: on which side of the row-block count the deep prefixes fall."""
    clo, top, runs = edge_stats(grid, pol)
    n_a = grid.size
    print(f"{name} ({n_a} rows): clo {clo.min()}..{clo.max()}, top-clamped {top.min()}..{top.max()}, run lengths {runs}")
    needs, sides = EDGE_NEEDS[name], {"clo_lt_nb": False, "clo_gt_nb": False}
    if "clo" in needs:
        deep = clo[clo >= 8]
        assert deep.size, (name, "no clamped prefix of 8 rows or more")
        for M in EDGE_WIDTHS:
            nb = -(-n_a // adj_rows_per_block(M))
            assert np.any(deep % nb != 0), (name, M, nb, "every deep prefix is a multiple of the row-block count")
            sides["clo_lt_nb"] |= bool(np.any((deep < nb) & (deep % nb != 0)))
            sides["clo_gt_nb"] |= bool(np.any((deep > nb) & (deep % nb != 0)))
    if "top" in needs:
        assert top.max() >= 8, (name, "fewer than 8 sources clamped at the top")
    if "runs" in needs:
        assert any(k >= 5 and k % 2 == 1 for k in runs) and any(k >= 5 and k % 2 == 0 for k in runs), (name, runs)
    return sides
