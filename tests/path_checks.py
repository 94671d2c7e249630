"""The test bodies that are the same for every household-side path, as plain functions of (hank, kind, case, ...): kind is the
`Kind` row of tests/path_refs.py, which says how the binding names the kind's entries and which key of the case holds its path; what
else differs between the suites travels as arguments. tests/test_gpu_shock.py, test_gpu_income.py and test_gpu_borrow.py call the
device bodies (1-6), tests/test_shock_host.py, test_income_host.py and test_borrow_host.py the host bodies (7, 8).

Tolerances: cases.close (rel 1e-10 + abs 1e-12) against the oracle; bits where the header promises bits; the transposed identity under
the projection bound of tests/test_gpu_vjp_variants.py (1e-10 of the summed magnitudes); the host-side pair at rounding (1e-13)."""
from types import SimpleNamespace

import numpy as np
import pytest

import cases
import path_refs as P
from cases import close, jt

GRID_CASES = [(f, name, n_a, n_e) for f in ("ks", "hank") for name in cases.ENTRY_CASES for n_a, n_e in cases.ENTRY_GRIDS]
grid_cases = pytest.mark.parametrize("family,name,n_a,n_e", GRID_CASES)
NOT_READY, BAD_ARG = 5, 2


# ---- 1. the context and the refusals ------------------------------------------------------------------------------------------------
def ctx(hank, kind, c, schedule="launch", path=True):
    """a context of case c under HANK_SCHEDULE=schedule and the case's record diet, with its boundary, its outputs declared where the
    kind's suite declares them, and (path) the case's path set"""
    hb = cases.raw_block(hank, c["args"], schedule, **c["env"])
    hb.set_boundary(c["V"], c["D"])
    if kind.declares:
        hb.set_het_outputs(c["n_het"])
    assert hb.info()["record_diet"] == c["diet"]
    if path:
        getattr(hb, kind.method("set"))(c[kind.key])
    return hb


def raises(code, fn, *a, **kw):
    from hank_amd.hip import HankHIPError
    with pytest.raises(HankHIPError) as ei:
        fn(*a, **kw)
    assert ei.value.code == code, (ei.value.code, code, str(ei.value))


def ref_args(kind, c, path=True):
    """the leading arguments of path_refs' references for case c: (kind, model, x, V, D, the case's path or None: the neutral one)
    and, where the kind's suite declares the case's outputs, (gamma, n_het)"""
    return (kind, c[kind.model], c["x"], c["V"], c["D"], c[kind.key] if path else None) + ((c["gamma"], c["n_het"]) if kind.declares else ())


# ---- 2. the transposed identity -------------------------------------------------------------------------------------------------------
def transposed_identity(what, kind, yb, Jd, xbar, dx, bar, dp, moves=True):
    """<yb, Jd> = <xbar, dx> + <bar, dp> to 1e-10 of the summed magnitudes: yb (P, n_het, M) the cotangents, Jd (P, >= n_het, N) the
    device's own tangents of the directions dx (n_hh, P, N) and dp (*lead, P, N), xbar (n_hh, P, M) and bar (*lead, P, M) the
    transposed entry's results; moves: the path's cotangent must exceed 1e-6 somewhere"""
    n_het = yb.shape[1]
    lhs = np.einsum("tom,ton->mn", yb, Jd[:, :n_het, :])
    rhs = np.einsum("ktm,ktn->mn", xbar, dx) + np.einsum("tm,tn->mn" if bar.ndim == 2 else "etm,etn->mn", bar, dp)
    scale = np.einsum("tom,ton->mn", np.abs(yb), np.abs(Jd[:, :n_het, :]))
    print(f"{what}: max |lhs - rhs| / scale = {np.max(np.abs(lhs - rhs) / scale):.3e}; |{kind.bar}| {np.abs(bar).max():.3e}")
    if moves:
        assert np.abs(bar).max() > 1e-6, what
    assert np.all(np.abs(lhs - rhs) <= 1e-10 * scale), what


# ---- 3. invalidation ------------------------------------------------------------------------------------------------------------------
def bad_path_and_new_path(hank, kind, c, bad, at, new, vjp, own_entry):
    """a path with a value of `bad` at index `at` is refused and changes nothing — the path in force and the record still serve
    the batch of the kind's own tangent entry (own_entry) or of hank_jvp; the path `new` drops the record: hank_jvp, the kind's
    entry, vjp(hb) and the policies' tangents are refused, and the next primal differs"""
    path, set_path = c[kind.key], kind.method("set")
    hb = ctx(hank, kind, c, None)
    try:
        agg = hb.primal(c["x"])
        dx, dp = P.seeds(kind, c, 3, 1)
        jvp_path = getattr(hb, kind.method("jvp"))
        batch = (lambda: jvp_path(dx, dp)) if own_entry else (lambda: hb.jvp(dx))
        dagg = batch()
        for v in bad:
            b = path.copy()
            b[at] = v
            raises(BAD_ARG, getattr(hb, set_path), b)
            assert np.array_equal(getattr(hb, kind.binding.attr), path)
            assert np.array_equal(batch(), dagg)                                 # the record and the path in force are still valid
        getattr(hb, set_path)(new)
        raises(NOT_READY, hb.jvp, dx)
        raises(NOT_READY, jvp_path, dx, None)
        raises(NOT_READY, vjp, hb)
        raises(NOT_READY, hb.dpolicy_seq, 3)
        assert not np.array_equal(hb.primal(c["x"]), agg)
    finally:
        hb.close()


def memo_and_clone(hank, kind, c, second, ref, hits):
    """hank_primal_jvp under the case's path and then under `second` follows the path (against ref(k, path, dx), the oracle's
    sweeps); hits: the same x under the same path is served by the memo; a clone carries the path in force"""
    hb = ctx(hank, kind, c, None, path=False)
    try:
        dx, _ = P.seeds(kind, c, 3, 2)
        paths = (c[kind.key], second)
        out = []
        for k, p in enumerate(paths):
            getattr(hb, kind.method("set"))(p)
            agg, dagg = hb.primal_jvp(c["x"], dx)
            r = ref(k, p, dx)
            close(agg, r["agg"][:, 0], what=f"path {k}: hank_primal_jvp value")
            close(dagg, r["dagg"][:, 0, :], what=f"path {k}: hank_primal_jvp partials")
            out.append(agg)
        assert not np.array_equal(out[0], out[1])
        if hits:
            n = hb.stats()["primal_memo_hits"]
            agg, _ = hb.primal_jvp(c["x"], dx)                                    # the same x under the same path: the memo serves it
            assert hb.stats()["primal_memo_hits"] == n + 1 and np.array_equal(agg, out[1])
        other = hb.clone()
        try:
            assert np.array_equal(getattr(other, kind.binding.attr), paths[1])
            assert np.array_equal(other.primal(c["x"]), out[1])
        finally:
            other.close()
    finally:
        hb.close()


# ---- 4. bits ----------------------------------------------------------------------------------------------------------------------------
def neutral_path_gives_the_bits_of_no_path(hank, kind, c, what, het=None, default_too=False):
    """under HANK_SCHEDULE=launch: the aggregate, the policies and (het: that many) outputs without a path, then with the kind's
    neutral path, which drops the record and gives the same bits; default_too: a context under the default schedule with the neutral
    path gives them as well"""
    neutral = kind.neutral(c[kind.model], c["x"].shape[1])
    hb = ctx(hank, kind, c, "launch", path=False)
    try:
        agg = hb.primal(c["x"])
        outs = hb.het_outputs(het)[0] if het else None
        pol = hb.policy_seq()
        getattr(hb, kind.method("set"))(neutral)
        raises(NOT_READY, hb.policy_seq)
        assert np.array_equal(hb.primal(c["x"]), agg) and np.array_equal(hb.policy_seq(), pol), what
        if het:
            assert np.array_equal(hb.het_outputs(het)[0], outs), what
    finally:
        hb.close()
    if default_too:
        hb = ctx(hank, kind, c, None, path=False)
        try:
            getattr(hb, kind.method("set"))(neutral)
            assert np.array_equal(hb.primal(c["x"]), agg) and np.array_equal(hb.policy_seq(), pol), what + ("default",)
            assert np.array_equal(hb.het_outputs(het)[0], outs), what + ("default",)
        finally:
            hb.close()


def no_seed_in_the_path_is_hank_jvp_bit_for_bit(hank, kind, c, what, widths, signbits=False, direct=False):
    """the kind's tangent entry with a null or an all-zero seed in the path gives hank_jvp's aggregate and policy tangents bit for
    bit (signbits: the zeros' signs too; direct: and hank_get_het_outputs' tangents with a zero dy), and refuses both seeds null"""
    from hank_amd.hip import _p
    hb = ctx(hank, kind, c, "launch")
    try:
        hb.primal(c["x"])
        out = np.empty((c["x"].shape[1], 3), order="F")
        assert getattr(hb._lib, kind.binding.jvp)(hb._ctx, None, None, 3, _p(out)) == BAD_ARG
        jvp_path = getattr(hb, kind.method("jvp"))
        for N in widths:
            dx, _ = P.seeds(kind, c, N, 5)
            dagg, dpol = hb.jvp(dx), hb.dpolicy_seq(N)
            zero = np.zeros(c[kind.key].shape + (N,))
            if direct:
                het = hb.het_outputs(2, dx)[1]
            for dp in (None, zero):
                assert np.array_equal(jvp_path(dx, dp), dagg), what + (N,)
                got = hb.dpolicy_seq(N)
                assert np.array_equal(got, dpol) and (not signbits or np.array_equal(np.signbit(got), np.signbit(dpol))), what + (N,)
            if direct:
                assert np.array_equal(hb.het_outputs(2, dx, dy=zero)[1], het), what + (N,)
    finally:
        hb.close()


# ---- 5. the host bodies -----------------------------------------------------------------------------------------------------------------
def dense_pair_reproduces_sweeps(kind, c, what, rel):
    """path_refs.jacobians' (Jx, Jp) against path_refs.oracle_path_sweeps with random dx and dpath together: the map is linear, so the
    two agree to rounding (rel of the largest entry); the sweeps ran once; the cotangent formulas are the transposes of the same
    pair (1e-13 of the summed magnitudes). -> what the kind's own checks go on with: args, J, dx, dp, ref, lin"""
    n_hh, Pn = c["x"].shape
    nh, lead = c["n_het"], c[kind.key].shape[:-1]
    args = ref_args(kind, c)
    Jx, Jp = J = P.jacobians(*args)
    assert Jx.shape == (nh, Pn, n_hh, Pn) and Jp.shape == (Pn, nh) + lead + (Pn,)
    assert P.unit_sweeps(*args)[1] is P.unit_sweeps(*args)[1]                    # (the sweeps ran once)
    assert lead or P.jacobians(*args)[1] is Jp
    rng = np.random.default_rng(Pn)
    dx, dp = rng.standard_normal((n_hh, Pn, 5)), rng.standard_normal(lead + (Pn, 5))
    ref = P.oracle_path_sweeps(*args, dx=dx, dpath=dp)
    lin = P.linear(J, dx, dp)
    for o in range(nh):
        close(lin[:, o, :], ref["dagg"][:, o, :], rel=rel, ab=0.0, what=f"{what} output {o}")
    yb = rng.standard_normal((Pn, nh, 4))
    lhs = np.einsum("tom,ton->mn", yb, lin)
    rhs = np.einsum("ksm,ksn->mn", jt(Jx, yb), dx) + np.einsum("esm,esn->mn" if lead else "sm,sn->mn", P.path_bar(Jp, yb), dp)
    scale = np.einsum("tom,ton->mn", np.abs(yb), P.linear((np.abs(Jx), np.abs(Jp)), np.abs(dx), np.abs(dp)))
    assert np.all(np.abs(lhs - rhs) <= 1e-13 * scale), np.max(np.abs(lhs - rhs) / scale)
    return SimpleNamespace(args=args, J=J, dx=dx, dp=dp, ref=ref, lin=lin)


def jacobian_is_the_toeplitz_recursion(hank, kind, lead, nh, fewer):
    """SteadyStateJacobian's `<kind>_jacobian` on a stand-in block that hands out a random F (P, P, *lead, nh) and Dv (P, *lead, nh):
    J (nh, P, *lead, P) is the recursion J[t, s] = F[t, s] + J[t - 1, s - 1], J[0, s] = F[0, s] + Dv[s] per output and leading
    index, household_jacobian's bit for bit; one call of the entry; `fewer` outputs give that many"""
    from hank_amd import SteadyStateJacobian as SSJ
    jacobian = getattr(SSJ, kind.name + "_jacobian")
    rng = np.random.default_rng(4)
    Pn = 6
    F, Dv = rng.standard_normal((Pn, Pn) + lead + (nh,)), rng.standard_normal((Pn,) + lead + (nh,))
    stub = P.StubPathBlock(kind.method("fake_news"), F, Dv)
    J = jacobian(stub, nh)
    assert J.shape == (nh, Pn) + lead + (Pn,) and stub.calls == 1
    for o in range(nh):
        for e in np.ndindex(*lead):
            want = np.empty((Pn, Pn))
            for t in range(Pn):
                for s in range(Pn):
                    want[t, s] = F[(t, s) + e + (o,)] + (want[t - 1, s - 1] if t > 0 and s > 0 else (Dv[(s,) + e + (o,)] if t == 0 else 0.0))
            assert np.allclose(J[(o, slice(None)) + e], want, rtol=0, atol=1e-14)
        if lead:
            assert np.array_equal(J[o], SSJ.household_jacobian(F[..., o], Dv[..., o]).transpose(1, 0, 2))
        else:
            assert np.array_equal(J[o], SSJ.household_jacobian(F[..., o:o + 1], Dv[..., o:o + 1])[0])
    assert jacobian(stub, fewer).shape == (fewer, Pn) + lead + (Pn,)
