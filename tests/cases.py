"""The one case module of the suite: what the GPU modules (tests/test_gpu_*.py) and the CPU tests of their preconditions
(tests/test_vjp_host.py, tests/test_cases_host.py) share. Nothing here needs a GPU except `raw_block` / `block`, which create a
device context, and section 4, which runs sweeps on one.

0. the owners: `close` (the suite's tolerance function: a relative figure on the array's largest entry) and `within` (the entry-wise
   one: every entry inside a running error bound of tests/ld_refs.py), `raw_block` / `block` (a context under HANK_* variables, every
   variable restored: `hank_env`), `model_args` / `oracle_of` (a model's constructor arguments), `hank_economy` / `hank_x` (the one-asset HANK
   economy and its input path). The oracle's references are methods of oracle.oracle.Oracle: block, block_het, het_outputs, vfi;
1. the references of hank_vjp[_het]: the CPU oracle's Jacobian from unit tangents (`oracle_jacobian`, `oracle_jacobian_het` /
   `jacobian_het` for every heterogeneous output, transposed by `jt`) and the numpy
   restatement of the reference's ForwardIteration_pullback for Sweep A alone (`forward_iteration_pullback`);
2. the economies of the variant suite: `economy` (a curvature, its own host steady state), `shape` (a grid shape with a cheap
   valid boundary), `CASES` (curvature x record layout);
3. raw-grid economies (`raw_economy`, `EDGE_GRIDS`) whose oracle policy holds the data-dependent edges the calibrated grids never
   show — a deep clamped prefix, many sources clamped at the top, long runs of rows in one bracket — and `edge_stats`, which
   measures those edges on a policy. They serve the forward families too (tests/test_gpu_fwd_edges.py), next to three more
   (`FWD_EDGE_ECONOMIES`: a grid and an offset on the path of r) whose edges only the forward kernels have code for: a prefix over
   several 63-row members and past row 128, every column or a whole column clamped, a clamp that vanishes after a clamped period
   and returns, more than 64 sources on one target row — measured by `forward_edges`, which restates k_xunits_fwd's cut;
4. the forward sweeps' comparison (`sweeps`, `against_oracle_and_launches`, `expected_family`): both entry points at every
   batch width against the oracle and a launch-schedule context, for a model or for raw constructor arguments;
5. the entry-wise tests' exact inputs and their long double references (`entry_backward`, `entry_refs`, `entry_forward`,
   `entry_forward_ref`, `push_distribution`), shared by tests/test_ld_refs_host.py and tests/test_gpu_entrywise.py."""
import contextlib
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


def within(a, ref, bound, what, skip=None):
    """the entry-wise owner: |a - ref| <= bound at EVERY entry (ref and bound of tests/ld_refs.py: an extended-precision value and
    the running error bound of the float64 kernel). `skip` (a's shape, or its leading axes): the entries whose bracket is ambiguous,
    at most 1 % of the array. Prints max |a - ref| / bound, the share skipped and the worst entry before it asserts; a NaN anywhere
    and a shape mismatch fail it. -> the largest ratio."""
    a, ref, bound = np.atleast_1d(a), np.atleast_1d(ref), np.atleast_1d(np.asarray(bound, dtype=np.float64))
    assert a.shape == ref.shape == bound.shape and a.size, (what, a.shape, ref.shape, bound.shape)
    assert not (np.isnan(a).any() or np.isnan(ref).any() or np.isnan(bound).any()), f"{what}: NaN"
    assert np.all(bound >= 0), what
    skip = np.zeros(a.shape, dtype=bool) if skip is None else np.asarray(skip, dtype=bool)
    assert skip.shape == a.shape[:skip.ndim], (what, skip.shape, a.shape)
    skip = np.broadcast_to(skip.reshape(skip.shape + (1,) * (a.ndim - skip.ndim)), a.shape)
    share = float(skip.mean())
    err = np.abs(a - ref).astype(np.float64)                 # (the difference in the reference's precision)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(skip | (err == 0), 0.0, err / bound)      # (an error under a zero bound: inf)
    k = tuple(int(q) for q in np.unravel_index(np.argmax(ratio), a.shape))
    print(f"{what}: max err/bound {ratio.max():.3f} at {k} (a {float(a[k]):.17g}, ref {float(ref[k]):.17g}, bound {float(bound[k]):.3e}), "
          f"skipped {100 * share:.2f} %")
    assert share <= 0.01, f"{what}: {100 * share:.2f} % of the entries have an ambiguous bracket"
    assert np.all((err <= bound) | skip), f"{what}: max err/bound {ratio.max():.3f} at {k}"
    return float(ratio.max())


@contextlib.contextmanager
def hank_env(**env):
    """the given HANK_* variables set (None: unset) for the body, every one restored after it. `raw_block` creates under it; a
    variable the library reads later than hank_create — HANK_RG_B, HANK_RG_F, HANK_FWD_SS, read when a width's workspace is built —
    needs the first sweep of that width inside it as well."""
    old = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def raw_block(hank, args, schedule, **env):
    """hank.HouseholdBlock(*args) created under HANK_SCHEDULE=schedule (None: the default) and the given HANK_* variables."""
    with hank_env(HANK_SCHEDULE=schedule, **env):
        return hank.HouseholdBlock(*args)


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
# the forward families' economies: (grid, an additive offset on the r row of the nine-period x1 path, or None). Measured with the
# oracle's policy (clo per column over the nine periods) and asserted by tests/test_cases_host.py:
#   deep-prefix  column 0: 140 167 182 192 198 203 207 210 177, columns 1, 2: 0 — members 0..3 of the persistent family, wave 1 of
#                the wide family's 2-row geometry; sources clamped at the top of column 2: 10 9 9 8 8 8 7 7 76
#   swing        column 0: 36 128 0 0 0 0 0 39 41, column 1: 0 117 0 .., column 2: 0 62 0 ..: period 1 has every column clamped,
#                periods 2-6 no clamp at all (2 after a clamped period, 3-6 after unclamped ones), the clamp returns in period 7;
#                121-122 sources at the top of every column in period 7
#   collapse     column 0: 155 589 646 0 0 0 0 167 177, column 1: 0 644 700 0 .., column 2: 0 700 700 0 ..: whole columns
#                clamped, all mass on row 0 and the aggregate exactly 0 in periods 1 and 2
_SWING = (0.0, 0.0, -0.6, -0.6, 0.0, 0.0, 1.5, 1.5, 0.0)
FWD_EDGE_ECONOMIES = {
    "deep-prefix": (lambda: 1.0 * np.linspace(0.0, 1.0, 700) ** 4, None),
    "swing": (EDGE_GRIDS["dense-bottom"], _SWING),
    "collapse": (lambda: 1.0 * np.linspace(0.0, 1.0, 700) ** 4, _SWING),
}
FWD_ECONOMIES = tuple(EDGE_GRIDS) + tuple(FWD_EDGE_ECONOMIES)         # what tests/test_gpu_fwd_edges.py runs
_RAW = {}


def raw_economy(name):
    """-> dict(args: HouseholdBlock's, grid, Pi, V (n_a, 3), D (n_a * 3,), x (2, 9), orc): EDGE_GRIDS[name], or the grid and the
    path modifier of FWD_EDGE_ECONOMIES[name], under the Krusell-Smith 130x3 calibration; V_T that economy's steady-state value
    interpolated onto the grid, D_0 uniform, the inputs the first 9 periods of its x1 path (shock 0.05), the modifier added to
    its r row."""
    if name not in _RAW:
        from oracle.oracle import Oracle
        m, ss, _ = ks_setup(130, 3, 40)
        wd, pdm = m.heterogeneity["wealth"], m.heterogeneity["productivity"]
        make_grid, r_offset = FWD_EDGE_ECONOMIES[name] if name in FWD_EDGE_ECONOMIES else (EDGE_GRIDS[name], None)
        grid = np.ascontiguousarray(make_grid())
        n_a, n_e = grid.size, pdm.grid.size
        V = np.stack([np.interp(grid, wd.grid, np.asarray(ss.value)[:, e]) for e in range(n_e)], axis=1)
        D = np.full(n_a * n_e, 1.0 / (n_a * n_e))
        x = np.ascontiguousarray(ks_paths(m, ss, "x1", 0.05)[0][2:4, :EDGE_P])
        if r_offset is not None:
            x[0] += np.asarray(r_offset)
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


XRW, XUCAP = 63, 64          # csrc/hank_xsweep.h: rows per member of the persistent family, work units per member and period


def forward_edges(grid, pol):
    """what the forward kernels care about on a policy sequence pol (P, n_a, n_e), with k_lottery's `start` and k_xunits_fwd's
    greedy cut (csrc/hank_kernels.h, csrc/hank_xsweep.h) restated in numpy. -> dict of
    clo (P, n_e); members (P, n_e) = ceil(clo / 63), the members that hold clamped rows of a column; past128 (P, n_e), the prefix
    passes row 128 (wave 1 of the wide family's 2-row geometry); all_clamped (P,); reopened (P,): no column clamped after a period
    that had one (all virtual mass re-enters through row 0's lottery); quiet (P,): no column clamped after a period without one;
    sources (P, n_e): the most sources on one target row (target r receives the upper parts of [start[r-1], start[r]) and the lower
    parts of [start[r], start[r+1])); units (P, members): work units per member and period, every column's together;
    column_units: the most units of one column of a member; longest: the longest unit in lanes, its virtual lanes included."""
    P, n_a, n_e = pol.shape
    S = -(-n_a // XRW)
    m0 = np.searchsorted(grid, pol, side="left")            # searchsortedfirst: grid[m0 - 1] < pol <= grid[m0]
    clo = (m0 == 0).sum(axis=1)
    lo = np.where(m0 == 0, -1, np.where(m0 >= n_a, n_a - 2, m0 - 1))       # k_lottery's bracket; clamped-low sources sort first
    assert np.all(np.diff(lo, axis=1) >= 0), "the policy is not monotone in wealth"
    start = np.empty((P, n_e, n_a + 1), dtype=np.int64)     # start[r] = max(clo, #sources with lo < r): the first source with lo >= r
    for t in range(P):
        for e in range(n_e):
            start[t, e] = np.searchsorted(lo[t, :, e], np.arange(n_a + 1), side="left")
    assert np.array_equal(start[:, :, 0].T, clo.T)
    sources = np.maximum(start[:, :, 1] - start[:, :, 0], (start[:, :, 2:] - start[:, :, :-2]).max(axis=2))
    anyclo = (clo > 0).any(axis=1)
    prev = np.concatenate([[False], anyclo[:-1]])            # k_xfwd's vnz: some column was clamped in the period before
    units, column_units, longest = np.zeros((P, S), dtype=np.int64), 0, 0
    for t in range(P):
        for m in range(S):
            r0, nrows = m * XRW, min(XRW, n_a - m * XRW)
            for e in range(n_e):
                st = start[t, e]
                n, ta = 0, 0
                while ta < nrows:
                    ja = st[max(r0 + ta - 1, 0)]
                    has0 = ja == 0 and clo[t, e] <= 0 and prev[t]
                    lanes = lambda b: (st[r0 + b] - ja) + (S if has0 and st[r0 + b] > ja else 0)       # noqa: E731
                    tb = ta + 1                             # a unit holds one target row at least, however many lanes that takes
                    while tb < nrows and lanes(tb + 1) <= 64:
                        tb += 1
                    if st[r0 + tb] > ja:
                        n, longest = n + 1, max(longest, int(lanes(tb)))
                    ta = tb
                units[t, m] += n
                column_units = max(column_units, n)
    return dict(clo=clo, members=-(-clo // XRW), past128=clo > 128, all_clamped=(clo > 0).all(axis=1), reopened=~anyclo & prev,
                quiet=~anyclo & ~prev & (np.arange(P) > 0), sources=sources, units=units, column_units=column_units, longest=longest)


def adj_rows_per_block(M):
    """R of hank_vjp's lane geometry at batch width M (adj_geom, csrc/hank_geom.h; tests/test_geom_host.py holds the two together): two columns per lane for an even M, at
    most 16 lanes across the columns, RB = 64 / NC rows per wave instruction, R = max(RB, 8)."""
    MV = M // 2 if M % 2 == 0 else M
    NC = 1
    while NC < MV and NC < 16:
        NC *= 2
    return max(64 // NC, 8)


def shk_mc(M):
    """the cotangent columns across k_shk_bbar's lanes at batch width M (shk_mc, csrc/hank_hip.hip: the next power of two, 64 at
    most); k_inc_ybar takes min(shk_mc(M), INC_MC = 32) of them (tests/test_income_host.py holds the two together)."""
    mc = 1
    while mc < M and mc < 64:
        mc *= 2
    return mc


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


# ---- 4. the forward sweeps against the oracle and the launches ---------------------------------------------------------------
FAMILY = {"launch": "launch-per-period", "xcd": "xcd-persistent", "wide": "on-chip-wide"}
N_ORACLE = 40                # the oracle covers the first 40 columns of a wider batch


def expected_family(sched, entry, N):
    """the kernel family that serves a sweep: the forced schedule's, or the default schedule's choice by entry point and width."""
    if sched is not None:
        return FAMILY[sched]
    if N >= 80:
        return FAMILY["wide"]                   # a full round of the on-chip wide sweeps
    if entry == "dual":
        return FAMILY["xcd" if N <= 32 else "launch"]     # one-pass Dual batches run on the persistent Dual pass
    return FAMILY["xcd"]                        # tangent batches up to xjvp_max = 64


def sweeps(hb, xhh, y, Ns):
    """both entry points at every batch width: the Dual pass (hank_primal_jvp) and the Float64 sweeps followed by the tangent
    sweeps (hank_primal, hank_jvp), each from a record of another x (no memo hit: every sweep runs). A second hank_jvp at the same
    record returns the same bits. -> {(entry, N): (family, agg, dagg, policy (P, n_a, n_e), dpolicy (P, n_a, n_e, N), D)}."""
    out = {}
    for N in Ns:
        yN = np.ascontiguousarray(y[:, :, :N])
        hb.primal(xhh * 1.01)
        agg, dagg = hb.primal_jvp(xhh, yN)
        fam = hb.info()["last_tangent_family_name"]
        out["dual", N] = (fam, agg, dagg, hb.policy_seq().transpose(2, 0, 1), hb.dpolicy_seq(N).transpose(2, 0, 1, 3), hb.dist_seq())
        hb.primal(xhh * 1.01)
        agg = hb.primal(xhh)
        dagg = hb.jvp(yN)
        fam = hb.info()["last_tangent_family_name"]
        out["tan", N] = (fam, agg, dagg, hb.policy_seq().transpose(2, 0, 1), hb.dpolicy_seq(N).transpose(2, 0, 1, 3), hb.dist_seq())
        assert np.array_equal(hb.jvp(yN), dagg), ("a second hank_jvp at the same record", N)
    return out


def oracle_dist_seq(orc, pol, D0):
    """D_t (P, n_a, n_e), post-transition, of the oracle's forward iteration on the policy sequence pol (P, n_a, n_e)."""
    return orc.forward_iteration(np.stack([pol, np.zeros_like(pol)], axis=-1), D0, 1, return_D=True)[1][..., 0]


def against_oracle_and_launches(hank, shape, runs, Ns, seed=29):
    """each (schedule, env) of `runs`, both entry points at every N of Ns (per run: `Ns` may map a schedule to its widths), against
    the oracle — aggregates, policy, partials (the first N_ORACLE columns) and the distribution sequence element-wise — and
    against a launch-schedule context; the family that served each sweep, no fallback, the schedule in use.
    shape: (a model or the raw constructor's arguments, V, D, xhh, oracle). -> [(schedule, env, stats, info)] of the runs."""
    m, V, D, xhh, orc = shape
    args = m if isinstance(m, tuple) else model_args(m)
    n_hh, P = xhh.shape
    widths = (lambda sched: Ns[sched]) if isinstance(Ns, dict) else (lambda sched: Ns)
    Nmax = max(max(widths(sched)) for sched, _ in runs)
    y = np.random.default_rng(seed).standard_normal((n_hh, P, Nmax))
    oagg, odagg, opol, odpol = orc.block(xhh, y[:, :, :min(Nmax, N_ORACLE)], V, D)
    oD = oracle_dist_seq(orc, opol, D)
    refs, seen = {}, []
    for sched, env in runs:
        diet = env.get("HANK_RECORD_DIET")
        if diet not in refs:                # the launches with the same record layout (diet on and off differ by rounding)
            hl = raw_block(hank, args, "launch", HANK_RECORD_DIET=diet)
            hl.set_boundary(V, D)
            refs[diet] = sweeps(hl, xhh, y, sorted({N for s2, e2 in runs if e2.get("HANK_RECORD_DIET") == diet for N in widths(s2)}))
            hl.close()
        ref = refs[diet]
        hb = raw_block(hank, args, sched, **env)
        hb.set_boundary(V, D)
        got = sweeps(hb, xhh, y, widths(sched))
        st, info = hb.stats(), hb.info()
        assert st["fallbacks"] == 0 and info["wide_mode"] == {"wide": 2, None: 1}.get(sched, 0), (sched, env, st, info)
        # (a forced `wide` keeps the persistent sweeps for the primal where the grid fits them, the launches where it does not)
        assert sched == "wide" or st["schedule"] == {"launch": 0, "xcd": 1, None: 2}[sched], (sched, env, st, info)
        seen.append((sched, env, st, info))
        assert info["record_diet"] == (0 if env.get("HANK_RECORD_DIET") == 0 else 1), (sched, env, info)
        hb.close()
        for (entry, N), (fam, agg, dagg, pol, dpol, Dq) in got.items():
            what = f"{len(args[0])}x{len(args[1])} {sched} {env} {entry} N={N}"
            assert fam == expected_family(sched, entry, N), (what, fam)
            k = min(N, N_ORACLE)
            close(agg, oagg, what=what + " agg"); close(dagg[:, :k], odagg[:, :k], what=what + " dagg")
            close(pol, opol, what=what + " policy"); close(dpol[..., :k], odpol[..., :k], what=what + " dpolicy")
            np.testing.assert_allclose(Dq.sum(axis=(0, 1)), 1.0, rtol=0, atol=1e-12)
            close(Dq.transpose(2, 0, 1), oD, what=what + " D")
            _, agg0, dagg0, pol0, dpol0, _ = ref[entry, N]
            close(agg, agg0, 1e-12, what=what + " agg vs launch"); close(dagg, dagg0, 1e-12, what=what + " dagg vs launch")
            assert np.array_equal(pol, pol0), what + " policy vs launch"
            if fam != FAMILY["wide"]:
                assert np.array_equal(dpol, dpol0), what + " dpolicy bits vs launch"
            else:
                close(dpol, dpol0, 1e-12, what=what + " dpolicy vs launch")
    return seen


# ---- 5. the entry-wise tests' inputs (tests/test_ld_refs_host.py, tests/test_gpu_entrywise.py) -------------------------------
# one EGM step and one distribution step at exact inputs, for tests/ld_refs.py's restatement and its running error bound
ENTRY_GRIDS = ((33, 2), (130, 3))            # the primal blocks take 32 rows: 33 is two blocks, the second holding one row
ENTRY_WIDE = (40, 11)                        # once, at gamma = 2
ENTRY_BASE = (0.03, 1.0)
ENTRY_PRICES = ((1.3 * 0.03, 0.97 * 1.0), (-0.5, 0.1), (1.0, 3.0))      # the last two push the grid off both ends of the knots
ENTRY_TR = 0.07                              # the one-asset HANK family's transfer
ENTRY_BC = 0.04                              # ... and its borrowing limit: above the first grid point and on none
ENTRY_N = 3
# the six CASES and the record diet's gamma = 2 arm — what a context takes by default at gamma = 2: diet_kc's k cm^3 and diet_v's
# u sqrt(u), the library's only use of fast_sqrt
ENTRY_CASES = {**CASES, "gamma2": (2.0, None, 1)}
ENTRY_BACKWARD = [(f, name, n_a, n_e) for f in ("ks", "hank") for name in ENTRY_CASES for n_a, n_e in ENTRY_GRIDS] + \
                 [(f, name, *ENTRY_WIDE) for f in ("ks", "hank") for name in ("gamma2", "gamma2-nodiet")]
_ENTRY = {}


def entry_Pi(n_e):
    """a dense row-stochastic transition matrix that is NOT symmetric (a transposed use of Pi must show): 0.8 on the diagonal, the
    rest spread by weights that differ by row and by column"""
    k = np.arange(n_e)
    M = 1.0 + k[None, :] + 0.5 * k[:, None] * (k[None, :] % 2)
    return 0.8 * np.eye(n_e) + 0.2 * M / M.sum(axis=1, keepdims=True)


def entry_backward(family, gamma, n_a, n_e):
    """one EGM step's exact inputs -> dict(args: HouseholdBlock's, a, z, Pi, beta, gamma, bc, V, dV (n_a, n_e, 3), steps: [(x, dx)] at
    ENTRY_PRICES). family "ks": inputs (r, w), the borrowing limit on the first grid point; "hank": (r, w, tr) with the transfer
    ENTRY_TR and the limit ENTRY_BC off the grid, so that the `max` rule binds on interpolated policies too. V_next: three float64
    EGM iterates (ld_refs.egm_step) of a power-law start at ENTRY_BASE — sorted knots, a decreasing value."""
    key = ("back", family, gamma, n_a, n_e)
    if key not in _ENTRY:
        import ld_refs
        a = 50.0 * np.linspace(0.0, 1.0, n_a) ** 2
        z = np.linspace(0.5, 1.5, n_e)
        Pi = entry_Pi(n_e)
        beta, n_hh = 0.95, (2 if family == "ks" else 3)
        bc = a[0] if family == "ks" else ENTRY_BC
        tr = () if family == "ks" else (ENTRY_TR,)
        V = np.outer((2.0 + a) ** -gamma, np.linspace(1.2, 0.8, n_e))
        none = np.zeros((n_a, n_e, 0))
        for _ in range(3):
            V = ld_refs.egm_step(np.float64, a, z, Pi, beta, gamma, bc, V, none, ENTRY_BASE + tr, np.zeros((n_hh, 0)), 0)["V"].v
        assert np.all(np.diff(V, axis=0) < 0)
        rng = np.random.default_rng(n_a * 100 + n_e)
        dV = rng.standard_normal(V.shape + (ENTRY_N,))
        steps = [(np.array(p + tr), rng.standard_normal((n_hh, ENTRY_N))) for p in ENTRY_PRICES]
        _ENTRY[key] = dict(args=(a, z, Pi, beta, gamma, bc, 5, 0 if family == "ks" else 1), a=a, z=z, Pi=Pi, beta=beta, gamma=gamma, bc=bc,
                           V=np.ascontiguousarray(V), dV=dV, steps=steps)
    return _ENTRY[key]


def entry_refs(c, diet):
    """ld_refs.egm_step in long double at every step of the case c (of `entry_backward`), once per case and diet"""
    key = ("ref", id(c), diet)
    if key not in _ENTRY:
        import ld_refs
        _ENTRY[key] = [ld_refs.egm_step(np.longdouble, c["a"], c["z"], c["Pi"], c["beta"], c["gamma"], c["bc"], c["V"], c["dV"], x, dx, diet)
                       for x, dx in c["steps"]]
    return _ENTRY[key]


ENTRY_FORWARD = ("golden", "golden-own", "33x2", "257x4")


def entry_forward(name):
    """one distribution step's exact inputs -> dict(args, a, Pi, policy, dpolicy, D, dD): the committed golden's policy (clamps,
    exact grid hits, non-monotone), or a random non-monotone policy with clamps at both ends and exact grid hits at 33x2 and at
    257x4 (where the 256-thread blocks cross); D_prev log-uniform over 1e-30 .. 1e-2, normalised, dD_prev of its size entry by entry
    ("golden-own": the golden's own D_prev and dD_prev instead)."""
    key = ("fwd", name)
    if key not in _ENTRY:
        rng = np.random.default_rng(len(name))
        if name.startswith("golden"):
            g, k = np.load(ROOT / "tests" / "golden" / "forward_step_edge_30x3_N3.npz"), np.load(ROOT / "tests" / "golden" / "ks_30x3_T25_N3.npz")
            a, z, Pi = k["a_grid"], k["z_grid"], k["Pi"]
            args = (a, z, Pi, float(k["beta"]), float(k["gamma"]), float(k["borrow_cons"]), 5)
            pol, dpol = g["policy"], g["dpolicy"]
        else:
            n_a, n_e = (int(q) for q in name.split("x"))
            a = 50.0 * np.linspace(0.0, 1.0, n_a) ** 2
            z, Pi = np.linspace(0.5, 1.5, n_e), entry_Pi(n_e)
            args = (a, z, Pi, 0.95, 2.0, 0.0, 5)
            pol = rng.uniform(-5.0, 55.0, (n_a, n_e))
            hit = rng.random((n_a, n_e)) < 0.1
            pol[hit] = a[rng.integers(0, n_a, hit.sum())]
            dpol = rng.standard_normal((n_a, n_e, ENTRY_N))
        D = 10.0 ** rng.uniform(-30.0, -2.0, pol.shape)
        D /= D.sum()
        dD = D[..., None] * rng.standard_normal(pol.shape + (dpol.shape[2],))
        if name == "golden-own":
            D, dD = g["D_prev"], g["dD_prev"]
        _ENTRY[key] = dict(args=args, a=np.asarray(a), Pi=np.asarray(Pi), policy=np.ascontiguousarray(pol), dpolicy=np.ascontiguousarray(dpol),
                           D=D, dD=dD)
    return _ENTRY[key]


def entry_forward_ref(name):
    """ld_refs.forward_step in long double on `entry_forward(name)`, once"""
    key = ("fwdref", name)
    if key not in _ENTRY:
        import ld_refs
        c = entry_forward(name)
        _ENTRY[key] = ld_refs.forward_step(np.longdouble, c["a"], c["Pi"], c["policy"], c["dpolicy"], c["D"], c["dD"])
    return _ENTRY[key]


def push_distribution(grid, Pi, pol, D0):
    """D_0 pushed in long double through the policy sequence pol (n_a, n_e, P), the context's own exported bits: exact inputs, a
    bound that compounds from period to period. -> [ld_refs.forward_step's dict per period]"""
    import ld_refs
    n_a, n_e, P = pol.shape
    none = np.zeros((n_a, n_e, 0))
    D, out = np.asarray(D0, dtype=np.float64).reshape((n_a, n_e), order="F"), []
    for t in range(P):
        out.append(ld_refs.forward_step(np.longdouble, grid, Pi, pol[:, :, t], none, D, none))
        D = out[-1]["D"]
    return out
