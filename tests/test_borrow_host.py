"""CPU tests of the borrowing-limit path's references and host layers (no GPU):
1. the economies of tests/borrow_refs.py hold the conditions tests/test_gpu_borrow.py relies on: the path's kinds, a constrained and
   an unconstrained point in every column of every binding period, positive consumption (every oracle status 0, asserted inside the
   sweeps), a monotone policy, and the candidate rule of csrc/hank_borrow.h (brw_constrained) restated on the reference's record;
2. the reference's pins: with damin = 0 it is the constant-limit oracle's loop bit for bit; its amin tangent is the derivative of its
   own level (tests/test_income_host.py's step and agreement: 1e-6, 1e-6 relative) where the constrained set is the same at amin +- h;
   exact zeros for the periods with amin_t <= a[0]; the dense pair against the sweeps with both seeds, and its transpose;
3. include/hank_hip_borrow.h, the binding's table for it and the library's exports agree; the third path kind in hip.py's _PATHS,
   against the header's prototypes through the stand-in library;
4. SteadyStateJacobian.borrow_jacobian's recursion on a stand-in block;
5. the Newton keyword: exclusions, the step rule's refusal, and the order in which a shared context's paths are cleared and set."""
import numpy as np
import pytest

import borrow_refs as R
import cases
import path_checks as C
import path_refs
import shock_refs
from cases import close
from test_shock_host import STEP

K = R.KIND

ECONOMIES = [(f, name, n_a, n_e) for f in ("ks", "hank") for name in cases.ENTRY_CASES for n_a, n_e in cases.ENTRY_GRIDS]


# the economies whose path constrains a point of EVERY column in every binding period at every horizon (borrow_refs.borrow_path chooses
# the limits per economy from the oracle's own windows). At the others the window closes in some period of the longer horizons: the
# most productive state saves more at the bottom of the grid than the least productive one can afford there (gamma = 3, 33x2: 0.46
# against a cash of 0.50), and the 33-row grid has one point, a[3] = 0.439, between 0.2 and 0.78 for the limits that sit on a grid point.
EVERY_COLUMN = {("ks", "gamma1", 130, 3), ("ks", "gamma0.5", 33, 2), ("ks", "gamma0.5", 130, 3), ("ks", "gamma1.5", 130, 3), ("ks", "gamma1-nodiet", 130, 3),
                ("hank", "gamma1", 130, 3), ("hank", "gamma0.5", 33, 2), ("hank", "gamma0.5", 130, 3), ("hank", "gamma1.5", 130, 3),
                ("hank", "gamma2-nodiet", 130, 3), ("hank", "gamma1-nodiet", 130, 3), ("hank", "gamma2", 130, 3)}


@pytest.mark.parametrize("family,name,n_a,n_e", ECONOMIES)
def test_the_economies_hold_their_conditions(oracle_mod, family, name, n_a, n_e):
    """Every binding period has an unconstrained point in every column and a constrained one in the least productive column, at
    every economy and horizon; a constrained point in EVERY column at every economy at T = 2, and at every horizon at exactly the
    economies of EVERY_COLUMN (twelve of the twenty-eight, among them both families, both grids and both record diets)."""
    every_column = True
    for T in R.HORIZONS:
        c = R.borrow_case(family, name, n_a, n_e, T)
        a, amin, kinds = np.asarray(c["args"][0]), c["amin"], c["kinds"]
        for t, k in enumerate(kinds):                                         # the kinds are what they say
            i = int(np.searchsorted(a, amin[t]))
            if k in ("inside", "inside_hi"):
                assert i >= 2 and a[i - 1] < amin[t] < a[i], (T, t, k)
            elif k in ("on", "on_lo"):
                assert i >= 1 and amin[t] == a[i], (T, t, k)
            else:
                assert amin[t] == a[0] if k == "first" else amin[t] < a[0], (T, t, k)
            assert k in ("first", "below") or (a < amin[t]).sum() >= 2            # several grid points below every binding limit
        if T == 12:
            assert {"inside", "on", "first", "below"} <= set(kinds)
            assert np.any(np.diff(amin) > 0) and np.any(np.diff(amin) < 0)        # a tightening and a relaxing step
        s = path_refs.oracle_path_sweeps(K, *R.case_args(c), c["gamma"], 2)                # (every oracle status is 0: asserted inside)
        here = True
        for t, k in enumerate(kinds):
            C = s["C"][t]
            if k in ("first", "below"):
                assert not C.any(), (T, t, k)                                     # convention (i): flat extrapolation binds, not max
            else:
                assert C[:, 0].any() and (~C).any(axis=0).all(), (T, t, k, C.sum(axis=0))
                here &= bool(C.any(axis=0).all())
                assert np.all(s["pol"][t][C] == amin[t])
            # the candidate rule's second half: pol == amin_t outside C happens only at a flat-extrapolation tie (amin_t == a[0])
            tie = (s["pol"][t] == amin[t]) & ~C
            assert not tie.any() or k == "first", (T, t, k)
        assert np.all(np.diff(s["pol"], axis=1) >= 0)                             # monotone in wealth
        assert here or T > 2, (T, "every column is constrained at T = 2")
        every_column &= here
        print(f"{family} {name} {n_a}x{n_e} T={T}: limits {amin.round(4).tolist()}, constrained points per period and column {s['C'].sum(axis=1).tolist()}")
    assert every_column == ((family, name, n_a, n_e) in EVERY_COLUMN), every_column


@pytest.mark.parametrize("family,name,n_a,n_e,T", [("ks", "gamma2", 33, 2, 4), ("hank", "gamma2", 130, 3, 12)])
def test_without_a_seed_in_the_limit_the_reference_is_the_constant_limit_oracle_s_loop(oracle_mod, family, name, n_a, n_e, T):
    c0 = R.borrow_case(family, name, n_a, n_e, T)
    L = R.limits(np.asarray(c0["args"][0]))
    for bc in (c0["bc"], L["inside"]):
        c = R.with_limit(c0, bc)
        P = T - 1
        dx, _ = path_refs.seeds(K, c, 3, 1)
        own = path_refs.oracle_path_sweeps(shock_refs.KIND, c["orc"], c["x"], c["V"], c["D"], np.full(P, c["beta"]), c["gamma"], c["n_het"], dx=dx)
        for damin in (None, np.zeros((P, 3))):
            ref = path_refs.oracle_path_sweeps(K, *R.case_args(c, False), c["gamma"], c["n_het"], dx=dx, dpath=damin)
            for k in ("agg", "dagg", "agg2", "dagg2", "pol", "dpol"):
                assert np.array_equal(ref[k], own[k]), (family, name, bc, k, np.abs(ref[k] - own[k]).max())


@pytest.mark.parametrize("family,name,n_a,n_e,T", [("ks", "gamma2", 33, 2, 6), ("hank", "gamma1.5", 33, 2, 6), ("ks", "gamma1", 33, 2, 2),
                                                  ("hank", "gamma3", 130, 3, 12)])
def test_the_reference_s_limit_tangent_is_the_derivative_of_its_own_level(oracle_mod, family, name, n_a, n_e, T):
    """at the periods whose limit lies strictly inside a bracket: on a grid point the lottery's bracket has a kink in amin (convention
    (ii): the left derivative) and a central difference straddles it"""
    c = R.borrow_case(family, name, n_a, n_e, T)
    P = T - 1
    ts = [t for t, k in enumerate(c["kinds"]) if k in ("inside", "inside_hi")]
    assert ts and ts[0] == 0
    damin = np.zeros((P, len(ts)))
    damin[ts, np.arange(len(ts))] = 1.0
    args = R.case_args(c)
    ref = path_refs.oracle_path_sweeps(K, *args, c["gamma"], c["n_het"], dpath=damin)
    for k, t in enumerate(ts):
        lv = []
        for sgn in (1.0, -1.0):
            am = c["amin"].copy()
            am[t] += sgn * STEP
            lv.append(path_refs.oracle_path_sweeps(K, *args[:4], am, c["gamma"], c["n_het"]))
        what = f"{family} {name} {n_a}x{n_e} T={T} amin_{t}"
        assert np.array_equal(lv[0]["C"], ref["C"]) and np.array_equal(lv[1]["C"], ref["C"]), what      # a condition on the inputs
        fd_agg = (lv[0]["agg"] - lv[1]["agg"]) / (2 * STEP)
        fd_pol = (lv[0]["pol"] - lv[1]["pol"]) / (2 * STEP)
        assert np.abs(fd_pol).max() > 0.5 and (t > 0 or np.abs(fd_agg[:, :2]).max() > 1e-3), what      # (a later, looser limit may find no mass on C_t)
        for o in range(c["n_het"]):
            close(ref["dagg"][:, o, k], fd_agg[:, o], rel=1e-6, ab=0.0, what=f"{what} output {o}")
        close(ref["dpol"][..., k], fd_pol, rel=1e-6, ab=0.0, what=f"{what} policy")
        assert not np.any(ref["dpol"][t + 1:, ..., k])                        # amin_t moves no policy after t
        assert np.array_equal(ref["dpol"][t, ..., k], ref["C"][t].astype(float))      # ... and period t's one for one on C_t, not at all off it


@pytest.mark.parametrize("family,name,n_a,n_e,T", [("ks", "gamma2", 33, 2, 12), ("hank", "gamma1", 130, 3, 5)])
def test_the_dense_pair_reproduces_the_sweeps_with_both_seeds(oracle_mod, family, name, n_a, n_e, T):
    c = R.borrow_case(family, name, n_a, n_e, T)
    r = C.dense_pair_reproduces_sweeps(K, c, f"{family} {name}", 1e-12)
    Ja, sa = r.J[1], path_refs.unit_sweeps(*r.args)[1]
    for s, k in enumerate(c["kinds"]):                                        # convention (i): exact zeros, every output, every period
        if k in ("first", "below"):
            assert not np.any(Ja[:, :, s]) and not np.any(sa["dpol"][..., s]), (s, k)
        else:
            assert np.any(sa["dpol"][s, ..., s]), (s, k)      # (a relaxing step may find no mass on C_s: Ja's column is zero then)
    close(path_refs.linear_policies(*r.args, dx=r.dx, dp=r.dp), r.ref["dpol"], rel=1e-12, ab=0.0, what=f"{family} {name} policy")


# ---- 3. the third kind in the binding's one table ---------------------------------------------------------------------------------------
def _borrow_prototypes(monkeypatch):
    """tests/abi_header.prototypes of include/hank_hip_borrow.h (the parser reads the header its HEADER names)"""
    import abi_header
    monkeypatch.setattr(abi_header, "HEADER", abi_header.HEADER.parent / "hank_hip_borrow.h")
    protos = abi_header.prototypes()
    monkeypatch.undo()
    return protos


def test_the_extension_header_the_binding_and_the_library_agree(hank, monkeypatch):
    """what tests/test_abi.py holds for include/hank_hip.h, for include/hank_hip_borrow.h: names, arity, every parameter's class, the
    return class, the exports; and include/hank_hip.h itself declares none of the limit's entries (its count is pinned there)"""
    import ctypes
    import re
    import abi_header
    from hank_amd import hip
    protos = _borrow_prototypes(monkeypatch)
    assert sorted(protos) == sorted(hip.ABI_BORROW) and len(protos) == 6 and not set(hip.ABI_BORROW) & set(hip.ABI)
    assert not re.search(r"hank_[a-z_]*borrow[a-z_]*\s*\(", abi_header.HEADER.read_text())
    cls = lambda t: "ptr" if t is ctypes.c_void_p or isinstance(t, type(ctypes.POINTER(ctypes.c_double))) else {ctypes.c_int32: "i32", ctypes.c_double: "f64"}[t]      # noqa: E731
    for name, proto in protos.items():
        assert tuple(cls(t) for t in hip.ABI_BORROW[name]) == proto.params and proto.ret == "int", name
    lib = ctypes.CDLL(str(hip.library_path()))
    for name in protos:
        assert getattr(lib, name) is not None, name
    text = (abi_header.HEADER.parent / "hank_hip_borrow.h").read_text()
    assert "KrusellSmith.jl" in text and "BackwardIteration.jl" in text and "SteadyStateJacobian.jl" in text


def test_the_borrow_kind_is_a_row_of_the_paths_table(hank, monkeypatch):
    from abi_header import prototypes
    from hank_amd import hip
    import test_hip_binding_host as B
    from test_hip_binding_host import NULL, In, Lib, Out, verify
    protos = {**prototypes(), **_borrow_prototypes(monkeypatch)}
    monkeypatch.setattr(B, "PROTOS", protos)           # the stand-in library classifies its arguments by the prototypes
    assert set(hip._PATHS) == {"discount", "income", "borrow"}
    assert len({p.attr for p in hip._PATHS.values()}) == 3 and len({p.seed for p in hip._PATHS.values()}) == 3
    k = hip._PATHS["borrow"]
    assert (k.attr, k.seed, k.het) == ("borrow_path", "damin", True)
    for sym in (k.set, k.jvp, k.jvp + "_dev", k.vjp, k.vjp + "_dev", k.fake_news):
        assert sym in hip.ABI_BORROW and sym in protos, sym
    P, NHH, NA, NE = 5, 2, 4, 3
    b = hip.HouseholdBlock.__new__(hip.HouseholdBlock)
    b.P, b.n_hh, b.n_a, b.n_e, b.G, b.n_groups, b._ctx, b._lib = P, NHH, NA, NE, NA * NE, 0, None, Lib()
    b.calls = {"primal": 0, "jvp": 0, "primal_jvp": 0}
    b.discount_path = b.income_path = b.borrow_path = None
    am = 0.1 * np.arange(P)
    b.set_borrow_path(list(am))
    verify(b._lib, "hank_set_borrow_path", In(am))
    assert np.array_equal(b.borrow_path, am) and b.discount_path is None and b.income_path is None
    with pytest.raises(ValueError, match=r"amin_t must be \(5,\), got \(4,\)"):
        b.set_borrow_path(am[:4])
    rng = np.random.default_rng(0)
    dx, da = rng.standard_normal((NHH, P, 3)), rng.standard_normal((P, 3))
    out = b.jvp_borrow(dx, da)
    verify(b._lib, "hank_jvp_borrow", In(dx), In(da), 3, Out(out, (P, 3)))
    out = b.jvp_borrow(None, da[:, 0])
    verify(b._lib, "hank_jvp_borrow", NULL, In(da[:, :1]), 1, Out(out, (P, 1)))
    yb = rng.standard_normal((P, 2, 3))
    xbar, abar = b.vjp_borrow(yb, 2)
    verify(b._lib, "hank_vjp_borrow", 2, In(yb), 3, Out(xbar, (NHH, P, 3)), Out(abar, (P, 3)))
    F, Dv = b.fake_news_borrow(3)
    verify(b._lib, "hank_fake_news_borrow", 3, Out(F, (P, P, 3)), Out(Dv, (P, 3)))
    b.set_borrow_path(None)
    verify(b._lib, "hank_set_borrow_path", NULL)
    assert b.borrow_path is None


def test_the_host_library_names_the_kind_in_its_one_table_and_nowhere_else():
    """PATHS (csrc/hank_hip.hip) owns what differs between the kinds: the third row, its width and neutral value, one case each in the
    primal capture, the tangent capture and Sweep B, the Toeplitz seed — and no other statement asks for the kind"""
    import re
    from pathlib import Path
    csrc = Path(__file__).resolve().parent.parent / "julia-newtonraphsonhank_amd" / "csrc"
    host = (csrc / "hank_hip.hip").read_text()
    assert "enum PathKind { PATH_NONE, PATH_DISCOUNT, PATH_INCOME, PATH_BORROW };" in host and "constexpr int N_PATH_KINDS = 4;" in host
    assert '{"a borrowing-limit path", "hank_set_borrow_path", "hank_jvp_borrow", "hank_vjp_borrow", "hank_fake_news_borrow", "damin", "amin_bar",' in host
    assert "k == PATH_BORROW ? c.bc" in host
    lines = [ln for ln in host.splitlines() if "PATH_BORROW" in ln and not ln.lstrip().startswith("//")]
    assert not any(re.search(r"ctx->path\s*[!=]=\s*PATH_BORROW", ln) for ln in lines)       # set_path and the refusals alone ask which path is set
    assert "hank_borrow.h" in (csrc / "Makefile").read_text()


# ---- 4. the Toeplitz recursion ------------------------------------------------------------------------------------------------------------
def test_borrow_jacobian_is_the_toeplitz_recursion_per_output(hank):
    C.jacobian_is_the_toeplitz_recursion(hank, K, (), 3, 1)


# ---- 5. the Newton keyword ----------------------------------------------------------------------------------------------------------------
def test_the_newton_keyword_excludes_the_other_paths_and_the_backtracking_step(hank):
    from hank_amd import NewtonRaphson as NR
    am = np.zeros(4)
    with pytest.raises(ValueError, match="borrow_path excludes"):
        NR.LinearizedFunction(np.zeros(3), {}, None, None, None, borrow_path=am, discount_path=np.ones(4))
    with pytest.raises(ValueError, match="borrow_path excludes"):
        NR.LinearizedFunction(np.zeros(3), {}, None, None, None, borrow_path=am, income_path=np.zeros((2, 4)))
    with pytest.raises(ValueError, match="defined at one borrowing limit"):
        hank.NewtonRaphsonHANK(np.zeros(3), None, {}, None, None, None, step="backtrack", borrow_path=am)


def test_a_shared_context_s_paths_are_cleared_before_the_limit_s_is_set(hank):
    from hank_amd import NewtonRaphson as NR

    class Block:
        def __init__(self):
            self.discount_path, self.income_path, self.borrow_path, self.log = np.ones(4), None, None, []

        def set_boundary(self, v, d):
            pass

        def primal(self, x):
            self.log.append("primal")
            return np.zeros(4)

    def setter(name):
        def f(self, v):
            assert v is None or all(getattr(self, o) is None for o in ("discount_path", "income_path", "borrow_path") if o != name), (name, self.log)
            setattr(self, name, v)
            self.log.append((name, v is not None))
        return f
    for nm in ("discount_path", "income_path", "borrow_path"):
        setattr(Block, "set_" + nm, setter(nm))

    class SS:
        value, D = None, None
    lin = NR.LinearizedFunction.__new__(NR.LinearizedFunction)
    lin.hb, lin.ss_ending, lin.ss_initial, lin._xhh, lin._n_out = Block(), SS, SS, None, 1
    lin.discount_path, lin.income_path, lin.borrow_path = None, None, np.full(4, 0.1)
    lin._record_primal()
    assert lin.hb.log == [("discount_path", False), ("borrow_path", True), "primal"], lin.hb.log
    assert np.array_equal(lin.hb.borrow_path, lin.borrow_path)
    lin.borrow_path = None
    lin._record_primal()
    assert lin.hb.log[3:] == [("borrow_path", False), "primal"] and lin.hb.borrow_path is None


def test_the_example_parses_the_credit_crunch():
    from examples.solve_hank import parse_args
    a = parse_args(["--credit-crunch", "0.001", "0.8"])
    assert a.credit_crunch == [0.001, 0.8] and not a.gradient and not a.groups
    a = parse_args(["--credit-crunch", "0.001", "0.8", "--groups", "--gradient", "--n-a", "130", "--n-e", "3", "--T", "60"])
    assert a.credit_crunch == [0.001, 0.8] and a.gradient and a.groups and (a.n_a, a.n_e, a.T) == (130, 3, 60)
    assert parse_args([]).credit_crunch is None
    with pytest.raises(SystemExit):
        parse_args(["--credit-crunch", "0.001"])
