"""CPU tests of the income path's references and host layers (no GPU):
1. tests/path_refs.oracle_path_sweeps at tests/income_refs.KIND — the oracle's EGM step run once per productivity state with the dual transfer
   (tr_t + y_t[e], dtr_t + dy_t[e]), the columns assembled — against a central difference of ITS OWN level in entries of y_0 and
   y_{P-1} (the step and the agreement of tests/test_shock_host.py: 1e-6, 1e-6 relative);
2. a path of zeros reproduces sweep_refs.oracle_sweeps exactly;
3. the dense pair (Jx, Jy) against the sweeps with random seeds in the inputs and in y together, and its transpose;
4. hank_amd.incidence: the zero-sum property, the z-path's tangent against a difference, the incidence rule's normalisation;
5. SteadyStateJacobian.income_jacobian's recursion on a stand-in block;
6. examples/solve_hank.py's arguments;
7. what tests/test_gpu_income_geometry.py relies on: the raw grids' edges under the income path and exact zeros at clamped points, the
   grid aggregate's pair (J2x, J2y), the reference at n_e = 1 and 16 against a difference of its own level, column masses that follow
   D_0 and not x, and the cotangent widths against k_inc_ybar's launch arithmetic restated in Python."""
import numpy as np
import pytest

import cases
import income_refs as R
import path_checks as C
import path_refs
import shock_refs
import sweep_refs
from cases import close
from test_shock_host import STEP

K = R.KIND


@pytest.mark.parametrize("family,name,n_a,n_e,T", [("ks", "gamma2", 33, 2, 4), ("hank", "gamma1.5", 33, 2, 4), ("ks", "gamma1", 33, 2, 2),
                                                  ("hank", "gamma3", 130, 3, 12)])
def test_the_reference_s_income_tangent_is_the_derivative_of_its_own_level(oracle_mod, family, name, n_a, n_e, T):
    c = R.income_case(family, name, n_a, n_e, T)
    P = T - 1
    entries = sorted({(0, 0), (n_e - 1, P - 1), (n_e - 1, 0)})          # (state, period)
    dy = np.zeros((n_e, P, len(entries)))
    for k, (e, t) in enumerate(entries):
        dy[e, t, k] = 1.0
    args = (c["orc"], c["x"], c["V"], c["D"])
    ref = path_refs.oracle_path_sweeps(K, *args, c["y"], dpath=dy)
    for k, (e, t) in enumerate(entries):
        lv = []
        for sgn in (1.0, -1.0):
            y = c["y"].copy()
            y[e, t] += sgn * STEP
            lv.append(path_refs.oracle_path_sweeps(K, *args, y))
        what = f"{family} {name} {n_a}x{n_e} T={T} y_{t}[{e}]"
        fd_agg = (lv[0]["agg"] - lv[1]["agg"]) / (2 * STEP)
        fd_pol = (lv[0]["pol"] - lv[1]["pol"]) / (2 * STEP)
        assert np.abs(fd_agg).max() > 1e-3, what
        for o in range(2):
            close(ref["dagg"][:, o, k], fd_agg[:, o], rel=1e-6, ab=0.0, what=f"{what} output {o}")
        close(ref["dpol"][..., k], fd_pol, rel=1e-6, ab=0.0, what=f"{what} policy")
        assert not np.any(ref["dpol"][t + 1:, ..., k])                   # y_t moves no policy after t
        assert np.any(ref["dpol"][t, :, e, k])


@pytest.mark.parametrize("family,name,n_a,n_e,T", [("ks", "gamma2", 33, 2, 4), ("hank", "gamma2", 130, 3, 12)])
def test_a_path_of_zeros_is_the_oracle_s_own_loop(oracle_mod, family, name, n_a, n_e, T):
    c = R.income_case(family, name, n_a, n_e, T)
    dx, _ = path_refs.seeds(K, c, 3, 1)
    ref = path_refs.oracle_path_sweeps(K, c["orc"], c["x"], c["V"], c["D"], np.zeros_like(c["y"]), dx=dx)
    own = sweep_refs.oracle_sweeps(c["orc"], c["x"], c["V"], c["D"], c["gamma"], 2, y=dx)
    for k in ("agg", "dagg", "agg2", "dagg2", "pol", "dpol"):
        assert np.array_equal(ref[k], own[k]), (family, name, k, np.abs(ref[k] - own[k]).max())
    moved = path_refs.oracle_path_sweeps(K, c["orc"], c["x"], c["V"], c["D"], c["y"])
    assert np.abs(moved["pol"] - own["pol"]).max() > 1e-3                # (the path moves the policy)
    close(moved["mass"].sum(axis=1), np.ones(T - 1), what="the column masses sum to one")


@pytest.mark.parametrize("family,name,n_a,n_e,T", [("ks", "gamma2", 33, 2, 12), ("hank", "gamma1", 130, 3, 4)])
def test_the_dense_pair_reproduces_the_sweeps_with_both_seeds(oracle_mod, family, name, n_a, n_e, T):
    """(Jx, Jy) against path_refs.oracle_path_sweeps with random dx and dy together: the map is linear, so the two agree to rounding (1e-13
    of the largest entry)"""
    c = R.income_case(family, name, n_a, n_e, T)
    P = T - 1
    r = C.dense_pair_reproduces_sweeps(K, c, f"{family} {name}", 1e-13)
    # the budget, aggregated: dC_t + dA'_t - (1 + r_t) d(sum a D_t) = the direct term, the column mass m_t[e] at s = t and nothing else
    Jy, sy = r.J[1], path_refs.unit_sweeps(*r.args)[1]
    J2y = sy["dagg2"].reshape(P, P, n_e).transpose(0, 2, 1)                        # [t, e, s]
    direct = Jy[:, 0] + Jy[:, 1] - (1.0 + c["x"][0])[:, None, None] * J2y
    want = np.zeros((P, n_e, P))
    want[np.arange(P), :, np.arange(P)] = sy["mass"]
    close(direct, want, rel=1e-12, ab=0.0, what=f"{family} {name} direct term")


# ---- 7. the conditions of tests/test_gpu_income_geometry.py -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.EDGE_ECONOMIES)
def test_the_raw_grids_keep_their_edges_under_an_income_path(oracle_mod, name):
    """section D of the GPU module: under income_path the oracle's policy holds the deep clamped prefix, the capped sources and the
    long runs (measured: clo up to 47 on dense-bottom, 56 on both, 205 on deep-prefix with sources past row 128; swing clamps every
    column in period 1 and none in period 2), and a clamped (t, a, e) does not move with any y_s[e']: its partials are exact zeros"""
    c = R.geometry_case("raw", name)
    n_e, P = c["y"].shape
    assert P == cases.EDGE_P and c["n_het"] == 2 and "path" not in c
    _, sy = path_refs.unit_sweeps(K, c["orc"], c["x"], c["V"], c["D"], c["y"])
    assert np.all(np.isfinite(sy["pol"])) and sy["dpol"].shape == sy["pol"].shape + (n_e * P,)
    shock_refs.check_path_edges(name, c["grid"], sy["pol"])
    clamped = sy["pol"] <= c["grid"][0]
    assert clamped.any(axis=1).any(), name
    assert not np.any(sy["dpol"][clamped]), name
    assert np.any(sy["dpol"][~clamped]), name


GRID_PAIR_ECONOMIES = [("shape", 65, 3, 12), ("shape", 40, 16, 10), ("shape", 40, 1, 10), ("raw", "both")]


@pytest.mark.parametrize("econ", GRID_PAIR_ECONOMIES, ids=lambda e: "-".join(str(q) for q in e))
def test_the_grid_aggregate_s_pair_reproduces_the_sweeps_with_both_seeds(oracle_mod, econ):
    """(J2x, J2y) against path_refs.oracle_path_sweeps' dagg2 with random dx and dy together (1e-13 of the largest entry)"""
    c = R.geometry_case(*econ)
    n_hh, P = c["x"].shape
    n_e = c["y"].shape[0]
    args = (K, c["orc"], c["x"], c["V"], c["D"], c["y"])
    J2x, J2y = J2 = path_refs.grid_jacobians(*args)
    assert J2x.shape == (P, n_hh, P) and J2y.shape == (P, n_e, P)
    rng = np.random.default_rng(P + n_e)
    dx, dy = rng.standard_normal((n_hh, P, 5)), rng.standard_normal((n_e, P, 5))
    ref = path_refs.oracle_path_sweeps(*args, dx=dx, dpath=dy)
    close(path_refs.grid_linear(J2, dx, dy), ref["dagg2"], rel=1e-13, ab=0.0, what=f"{econ} grid aggregate")
    close(path_refs.grid_linear(J2, None, dy), path_refs.oracle_path_sweeps(*args, dpath=dy)["dagg2"], rel=1e-13, ab=0.0, what=f"{econ} grid aggregate, y alone")
    assert np.abs(J2y).max() > 2e-2 and min(np.abs(path_refs.jacobians(*args)[1][:, o]).max() for o in range(2)) > 2e-2


@pytest.mark.parametrize("n_e", [1, 16])
def test_the_reference_at_one_and_at_sixteen_states_is_the_derivative_of_its_own_level(oracle_mod, n_e):
    c = R.geometry_case("shape", 40, n_e, 4)
    P = 3
    assert c["y"].shape == (n_e, P) and c["orc"].n_e == n_e
    entries = sorted({(0, 0), (n_e - 1, P - 1)})                         # (state, period)
    dy = np.zeros((n_e, P, len(entries)))
    for k, (e, t) in enumerate(entries):
        dy[e, t, k] = 1.0
    args = (c["orc"], c["x"], c["V"], c["D"])
    ref = path_refs.oracle_path_sweeps(K, *args, c["y"], dpath=dy)
    for k, (e, t) in enumerate(entries):
        lv = []
        for sgn in (1.0, -1.0):
            y = c["y"].copy()
            y[e, t] += sgn * STEP
            lv.append(path_refs.oracle_path_sweeps(K, *args, y))
        what = f"40x{n_e} T=4 y_{t}[{e}]"
        fd_agg = (lv[0]["agg"] - lv[1]["agg"]) / (2 * STEP)
        fd_pol = (lv[0]["pol"] - lv[1]["pol"]) / (2 * STEP)
        assert np.abs(fd_agg).max() > 1e-3, what
        for o in range(2):
            close(ref["dagg"][:, o, k], fd_agg[:, o], rel=1e-6, ab=0.0, what=f"{what} output {o}")
        close(ref["dpol"][..., k], fd_pol, rel=1e-6, ab=0.0, what=f"{what} policy")
        assert not np.any(ref["dpol"][t + 1:, ..., k]) and np.any(ref["dpol"][t, :, e, k])


def test_the_column_masses_follow_the_initial_distribution_and_not_the_inputs(oracle_mod):
    """m_t[e] = sum_a D_t[e, a] is the productivity chain's alone: it does not move with x (measured: 3.9e-16) and does with a D_0
    whose column masses differ (measured: 0.16). Section F.4 of the GPU module tells a stale m_t[e] from a fresh one by this."""
    c = R.geometry_case("shape", 65, 3, 12)
    args = (c["orc"], c["x"], c["V"])
    mass = path_refs.oracle_path_sweeps(K, *args, c["D"], c["y"])["mass"]
    close(mass.sum(axis=1), np.ones(11), what="the column masses sum to one")
    moved_x = path_refs.oracle_path_sweeps(K, c["orc"], c["x"] * np.array([[1.3], [0.97]]), c["V"], c["D"], c["y"])
    assert np.abs(moved_x["pol"] - path_refs.oracle_path_sweeps(K, *args, c["D"], c["y"])["pol"]).max() > 1e-3
    print(f"column masses under another x: max move {np.abs(moved_x['mass'] - mass).max():.3e}")
    assert np.abs(moved_x["mass"] - mass).max() <= 1e-14
    D2 = R.rescaled_D0(c)
    assert D2.shape == c["D"].shape and abs(D2.sum() - 1.0) <= 1e-15
    mass2 = path_refs.oracle_path_sweeps(K, *args, D2, c["y"])["mass"]
    print(f"column masses under the rescaled D_0: max move {np.abs(mass2 - mass).max():.3e}")
    assert np.abs(mass2 - mass).max() > 0.1


def test_the_cotangent_widths_reach_every_block_shape_of_k_inc_ybar():
    """k_inc_ybar is launched with RO = AdjGeom::R of the batch width and MC = min(shk_mc(M), INC_MC) columns across the lanes: over
    M = 1 .. 256 that is eight (RO, MC) pairs, and R.GEOM_M reaches every one. (8, 8) — M = 5 and 7 alone — is why GEOM_M holds a 5
    that the shock suite's list does not: k_shk_bbar's MC goes on to 64, so its pairs are others. If the rule moves, move GEOM_M."""
    import re
    from pathlib import Path
    csrc = Path(__file__).resolve().parent.parent / "julia-newtonraphsonhank_amd" / "csrc"
    host, inc = (csrc / "hank_hip.hip").read_text(), (csrc / "hank_income.h").read_text()
    assert "static int shk_mc(int M) { int mc = 1; while (mc < M && mc < 64) mc <<= 1; return mc; }" in host, "shk_mc has moved: move cases.shk_mc"
    inc_mc = int(re.search(r"constexpr int INC_BT = 1024, INC_MC = (\d+);", inc).group(1))
    assert inc_mc == 32 and "IMC = std::min(MC, INC_MC)" in host and "inc_ybar_lds(c, w.g.R, IMC)" in host
    assert int(re.search(r"constexpr int INC_NE = (\d+);", inc).group(1)) == 16
    pair = lambda M: (cases.adj_rows_per_block(M), min(cases.shk_mc(M), inc_mc))       # noqa: E731
    every = {pair(M) for M in range(1, 257)}
    assert every == {(64, 1), (64, 2), (16, 4), (32, 4), (8, 8), (16, 8), (8, 16), (8, 32)}, sorted(every)
    assert {pair(M) for M in R.GEOM_M} == every, sorted(every - {pair(M) for M in R.GEOM_M})
    assert {M for M in range(1, 257) if pair(M) == (8, 8)} == {5, 7}
    # the tails section A names: a full and a partial last column block (blockIdx.y > 0), column 70 in blockIdx.y = 2
    assert [(-(-M // 32), M % 32) for M in (65, 66, 97, 130, 256)] == [(3, 1), (3, 2), (4, 1), (5, 2), (8, 0)] and 70 // 32 == 2
    # ... and the row counts: a multiple of every RO but 64's neighbours, one off it on either side, several blocks
    assert all(64 % ro == 0 for ro, _ in every) and [129 % ro for ro in (64, 32, 16, 8)] == [1, 1, 1, 1]
    # the seed's staging limit at the bound on n_e (section B) and at the 11 states of tests/test_gpu_income.py
    lds = lambda n_e, N: 8 * (n_e * n_e + 2 * n_e * N)                                  # noqa: E731
    assert "const size_t b = sizeof(double) * ((size_t)c.n_e * c.n_e + 2 * (size_t)c.n_e * N);" in host and "return b <= 48 * 1024 ? b : 0;" in host
    assert lds(16, 184) <= 48 * 1024 < lds(16, 185) and lds(11, 273) <= 48 * 1024 < lds(11, 274)


def test_redistribution_is_zero_sum_and_a_transfer_reaches_its_states_alone(hank):
    from hank_amd import incidence as I
    rng = np.random.default_rng(3)
    n_e, P = 5, 7
    m = rng.uniform(0.1, 1.0, (n_e, P))
    m /= m.sum(axis=0, keepdims=True)
    y = I.redistribution(m, [0, 1], 0.02, 0.8)
    assert y.shape == (n_e, P)
    assert np.abs((m * y).sum(axis=0)).max() <= 1e-17
    assert np.array_equal(y[0], 0.02 * 0.8 ** np.arange(P)) and np.array_equal(y[0], y[1]) and np.all(y[2:] < 0)
    assert np.array_equal(y[2], y[3]) and np.array_equal(y[3], y[4])
    tr = I.targeted_transfer(n_e, P, [0, 3], 0.01, 0.5)
    assert np.array_equal(tr[0], 0.01 * 0.5 ** np.arange(P)) and np.array_equal(tr[3], tr[0]) and not np.any(tr[[1, 2, 4]])
    for bad in ([], list(range(n_e))):
        with pytest.raises(ValueError):
            I.redistribution(m, bad, 0.02, 0.8)
    with pytest.raises(ValueError):
        I.redistribution(m[:, 0], [0], 0.02, 0.8)


def test_the_z_path_s_tangent_is_the_derivative_of_its_income_and_the_incidence_keeps_the_mean(hank):
    from hank_amd import incidence as I
    rng = np.random.default_rng(5)
    n_e, P, N = 4, 6, 3
    z = np.linspace(0.4, 1.8, n_e)
    pi = rng.uniform(0.1, 1.0, n_e); pi /= pi.sum()
    z = z / (pi @ z)
    Y = 1.0 + 0.03 * np.cos(np.arange(P))
    z_t = I.incidence(z, pi, Y, 0.7)
    assert z_t.shape == (n_e, P)
    close(pi @ z_t, np.ones(P), rel=1e-15, ab=0.0, what="the incidence rule keeps the mean at one")
    assert np.array_equal(I.incidence(z, pi, np.ones(P), 0.7), np.tile(z[:, None], (1, P)) * ((pi @ z) / (pi @ np.tile(z[:, None], (1, P))))[None, :])
    hi = Y > 1.0
    assert np.all(z_t[-1, hi] > z[-1]) and np.all(z_t[0, hi] < z[0])       # zeta > 0: a boom spreads earnings
    w = 1.0 + 0.1 * rng.standard_normal(P)
    y = I.z_path_to_income(z, z_t, w)
    close(y, w[None, :] * (z_t - z[:, None]), rel=1e-16, ab=0.0, what="y = w (z_t - z)")
    dz, dw = rng.standard_normal((n_e, P, N)), rng.standard_normal((P, N))
    dy = I.z_path_to_income_tangent(z, z_t, w, dz, dw)
    h = 1e-6
    for n in range(N):
        fd = (I.z_path_to_income(z, z_t + h * dz[..., n], w + h * dw[:, n]) - I.z_path_to_income(z, z_t - h * dz[..., n], w - h * dw[:, n])) / (2 * h)
        close(dy[..., n], fd, rel=1e-9, ab=0.0, what=f"direction {n}")       # (y is bilinear: the central difference is exact to rounding)
    close(I.z_path_to_income_tangent(z, z_t, w, dz, None) + I.z_path_to_income_tangent(z, z_t, w, None, dw), dy, rel=1e-15, ab=0.0, what="the parts add")


def test_income_jacobian_is_the_toeplitz_recursion_per_output_and_state(hank):
    C.jacobian_is_the_toeplitz_recursion(hank, K, (3,), 2, 1)


def test_the_example_parses_the_redistribution():
    from examples.solve_hank import parse_args
    a = parse_args(["--redistribute", "0.01", "0.8", "2"])
    assert a.redistribute == [0.01, 0.8, 2.0] and not a.gradient and not a.groups
    a = parse_args(["--redistribute", "0.01", "0.8", "2", "--groups", "--gradient", "--n-a", "130", "--n-e", "3", "--T", "40"])
    assert a.redistribute == [0.01, 0.8, 2.0] and a.gradient and a.groups and (a.n_a, a.n_e, a.T) == (130, 3, 40)
    assert parse_args([]).redistribute is None
    with pytest.raises(SystemExit):
        parse_args(["--redistribute", "0.01", "0.8"])
