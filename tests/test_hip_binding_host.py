"""The argument handling of hip.HouseholdBlock without a device or a built library: a stand-in library records every call on a
context-less block, and each case states the whole argument list the C ABI must see — the symbol, the integers and floats, which
pointers are NULL, the doubles behind every input pointer (the column-major flattening of the expected array), and that every output
pointer is the start of the returned array, whose shape and column-major strides it checks. The stand-in classifies its arguments by
the prototypes of include/hank_hip.h (tests/abi_header.py), so a pointer may arrive as a ctypes pointer, a c_void_p, an int or None.
Dimensions: n_a, n_e, P, n_hh = 4, 3, 5, 2, two groups, batches of 1 and 3 columns."""
import ctypes as C

import numpy as np
import pytest

from abi_header import prototypes

PROTOS = prototypes()
NA, NE, P, NHH, G, K = 4, 3, 5, 2, 12, 2
NULL, PTR = "NULL", "PTR"                                  # a null pointer; any pointer that is not null


class In:
    """an input pointer: the library reads `arr`, flattened column-major"""
    def __init__(self, arr, dtype=np.float64):
        self.arr, self.dtype = np.asarray(arr, dtype=dtype), dtype


class Out:
    """an output pointer: the start of the returned array `arr`, which is column-major (or `order`) of `shape`"""
    def __init__(self, arr, shape, dtype=np.float64, order="F"):
        self.arr, self.shape, self.dtype, self.order = arr, tuple(shape), dtype, order


class Dev:
    """a device pointer handed through as it is"""
    def __init__(self, p):
        self.p = p


class Lib:
    """stands in for libhank_hip: records (symbol, arguments after the context) and answers `rc`; `fill[symbol]` writes outputs"""
    def __init__(self, rc=0, fill=None):
        self.calls, self.rc, self.fill = [], rc, fill or {}

    def hank_last_error(self, ctx):
        return b"refused by the stand-in"

    def __getattr__(self, name):
        if name not in PROTOS:
            raise AttributeError(name)

        def entry(ctx, *args):
            assert len(args) == len(PROTOS[name].params) - 1, (name, len(args))
            self.calls.append((name, args))
            if name in self.fill:
                self.fill[name](*args)
            return self.rc
        return entry


def _addr(a):
    if a is None:
        return 0
    if isinstance(a, int):
        return a
    if isinstance(a, C.c_void_p):
        return a.value or 0
    if isinstance(a, C.Array):
        return C.addressof(a)
    return C.cast(a, C.c_void_p).value or 0


def _fstrides(shape, dtype, order="F"):
    return np.empty(shape, dtype=dtype, order=order).strides


def verify(lib, symbol, *expect):
    """the last call was `symbol` with exactly these arguments after the context"""
    name, args = lib.calls[-1]
    assert name == symbol
    classes = PROTOS[symbol].params[1:]
    assert len(expect) == len(classes), (symbol, len(expect), len(classes))
    for k, (cls, a, e) in enumerate(zip(classes, args, expect)):
        where = f"{symbol} argument {k + 1}"
        if cls == "i32":
            assert type(a) is int and a == e, where                         # (ctypes takes nothing but an int for an int32_t)
        elif cls == "f64":
            assert isinstance(a, (int, float)) and float(a) == float(e), where
        elif e is NULL:
            assert _addr(a) == 0, where
        elif e is PTR:
            assert _addr(a) != 0, where
        elif isinstance(e, Dev):
            assert _addr(a) == e.p, where
        elif isinstance(e, In):
            want = e.arr.ravel(order="F")
            assert _addr(a) != 0, where
            if want.size:
                ct = C.c_double if e.dtype is np.float64 else C.c_int32
                got = np.ctypeslib.as_array(C.cast(a, C.POINTER(ct)), (want.size,))
                assert np.array_equal(got, want), where
        else:
            assert isinstance(e, Out), where
            assert e.arr.shape == e.shape and e.arr.dtype == e.dtype and e.arr.strides == _fstrides(e.shape, e.dtype, e.order), (where, e.arr.shape)
            assert _addr(a) == e.arr.ctypes.data, where


@pytest.fixture
def hb(hank):
    from hank_amd import hip
    b = hip.HouseholdBlock.__new__(hip.HouseholdBlock)               # no context: the argument handling alone
    b.P, b.n_hh, b.n_a, b.n_e, b.G, b.n_groups, b._ctx, b._lib = P, NHH, NA, NE, G, K, None, Lib()
    b.calls = {"primal": 0, "jvp": 0, "primal_jvp": 0}
    return b


def _rand(*shape, seed=0):
    return np.random.default_rng(seed + len(shape)).standard_normal(shape)


def _orders(x):
    """the same array in C order, in Fortran order and as a strided view"""
    big = np.zeros(tuple(2 * s for s in x.shape))
    view = big[tuple(slice(None, None, 2) for _ in x.shape)]
    view[...] = x
    return np.ascontiguousarray(x), np.asfortranarray(x), view


BAD = r"expected array of shape \(%s\), got \(%s\)"


# -- the sweeps on host pointers -----------------------------------------------------------------------------------------------
def test_primal(hb):
    x = _rand(NHH, P)
    for xin in _orders(x):
        agg = hb.primal(xin)
        verify(hb._lib, "hank_primal", In(x), Out(agg, (P,)))
    assert hb.calls["primal"] == 3
    with pytest.raises(ValueError, match=BAD % ("2, 5", "5, 2")):
        hb.primal(x.T)


@pytest.mark.parametrize("N", [1, 3])
def test_jvp_and_primal_jvp(hb, N):
    x, dx = _rand(NHH, P), _rand(NHH, P, N)
    forms = _orders(dx) + ((dx[:, :, 0],) + _orders(dx[:, :, 0]) if N == 1 else ())
    for d in forms:
        out = hb.jvp(d)
        verify(hb._lib, "hank_jvp", In(dx), N, Out(out, (P, N)))
        agg, dagg = hb.primal_jvp(x, d)
        verify(hb._lib, "hank_primal_jvp", In(x), In(dx), N, Out(agg, (P,)), Out(dagg, (P, N)))
    assert hb.calls == {"primal": 0, "jvp": len(forms), "primal_jvp": len(forms)}
    with pytest.raises(ValueError, match=BAD % ("2, 5, %d" % N, "5, 2, %d" % N)):
        hb.jvp(np.swapaxes(dx, 0, 1))
    with pytest.raises(ValueError, match=BAD % ("2, 5, %d" % N, "5, 2, %d" % N)):
        hb.primal_jvp(x, np.swapaxes(dx, 0, 1))
    with pytest.raises(ValueError, match=BAD % ("2, 5", "5, 2")):
        hb.primal_jvp(x.T, dx)
    assert hb.calls["jvp"] == len(forms)                                 # (a refused input is not counted)


@pytest.mark.parametrize("method, symbol, seed_shape, name", [("jvp_shock", "hank_jvp_shock", (P,), "dbeta"),
                                                              ("jvp_income", "hank_jvp_income", (NE, P), "dy")])
def test_jvp_with_a_path_seed(hb, method, symbol, seed_shape, name):
    call = getattr(hb, method)
    for N in (1, 3):
        dx, ds = _rand(NHH, P, N), _rand(*seed_shape, N, seed=1)
        dxs = _orders(dx) + ((dx[..., 0],) if N == 1 else ())
        dss = _orders(ds) + ((ds[..., 0],) if N == 1 else ())
        for d in dxs:
            out = call(d)
            verify(hb._lib, symbol, In(dx), NULL, N, Out(out, (P, N)))
        for s in dss:
            out = call(None, s)
            verify(hb._lib, symbol, NULL, In(ds), N, Out(out, (P, N)))
            out = call(**{name: s})
            verify(hb._lib, symbol, NULL, In(ds), N, Out(out, (P, N)))
        for d in dxs:
            for s in dss:
                out = call(d, s)
                verify(hb._lib, symbol, In(dx), In(ds), N, Out(out, (P, N)))
    n = hb.calls["jvp"]
    with pytest.raises(ValueError, match=f"at least one of dxhh, {name} must be given"):
        call()
    sh = ", ".join(str(s) for s in seed_shape)
    with pytest.raises(ValueError, match=BAD % (sh + ", 3", sh + ", 1")):      # N is the first given seed's
        call(_rand(NHH, P, 3), _rand(*seed_shape))
    with pytest.raises(ValueError, match=BAD % (sh + ", 1", sh + ", 3")):
        call(_rand(NHH, P), _rand(*seed_shape, 3))
    with pytest.raises(ValueError, match=BAD % ("2, 5, 3", "5, 2, 3")):
        call(_rand(P, NHH, 3))
    assert hb.calls["jvp"] == n


def _boundary_forms(s):
    """a boundary seed (n_a, n_e, N) in every form the binding takes"""
    N = s.shape[2]
    return _orders(s) + _orders(s.reshape((G, N), order="F")) + (_orders(s[:, :, 0]) if N == 1 else ())


@pytest.mark.parametrize("het", [False, True])
def test_jvp_boundary_and_jvp_het(hb, het):
    n_het = 3

    def call(dx=None, dv=None, dd=None):
        if het:
            out = hb.jvp_het(dx, dv, dd, n_het=n_het)
            return out, ("hank_jvp_het", n_het), (P, n_het, N)
        out = hb.jvp_boundary(dx, dv, dd)
        return out, ("hank_jvp_boundary",), (P, N)

    for N in (1, 3):
        dx, dv, dd = _rand(NHH, P, N), _rand(NA, NE, N, seed=1), _rand(NA, NE, N, seed=2)
        dxs = _orders(dx) + ((dx[:, :, 0],) if N == 1 else ())
        for d in dxs:
            out, head, shape = call(d)
            verify(hb._lib, *head, In(dx), NULL, NULL, N, Out(out, shape))
        for s in _boundary_forms(dv):
            if N == 3 and s.ndim == 2:
                with pytest.raises(ValueError, match=BAD % ("12, 1", "12, 3")):      # a lone (G, N) seed fixes N = 1: refused for N > 1
                    call(dv=s)
                with pytest.raises(ValueError, match=BAD % ("12, 1", "12, 3")):
                    call(dd=s)
                continue
            out, head, shape = call(dv=s)
            verify(hb._lib, *head, NULL, In(dv), NULL, N, Out(out, shape))
            out, head, shape = call(dd=s)
            verify(hb._lib, *head, NULL, NULL, In(dv), N, Out(out, shape))
        for d in dxs:
            for s, s2 in zip(_boundary_forms(dv), reversed(_boundary_forms(dd))):
                out, head, shape = call(d, s, s2)
                verify(hb._lib, *head, In(dx), In(dv), In(dd), N, Out(out, shape))
        out, head, shape = call(None, dv, dd.reshape((G, N), order="F"))                 # N from a 3-D boundary seed
        verify(hb._lib, *head, NULL, In(dv), In(dd), N, Out(out, shape))
    n = hb.calls["jvp"]
    N = 3
    with pytest.raises(ValueError, match="at least one of dxhh, dvalue_end, dD_init must be given"):
        call()
    with pytest.raises(ValueError, match=BAD % ("12, 3", "12, 1")):
        call(_rand(NHH, P, 3), _rand(NA, NE))
    with pytest.raises(ValueError, match=BAD % ("12, 3", "3, 4, 3")):
        call(_rand(NHH, P, 3), _rand(NE, NA, 3))
    with pytest.raises(ValueError, match=BAD % ("12, 1", "12, 3")):                    # N is the FIRST given argument's, dxhh's here
        call(_rand(NHH, P), _rand(NA, NE, 3))
    assert hb.calls["jvp"] == n
    if het:                                                                             # an n_het the library refuses still gets a buffer
        out = hb.jvp_het(_rand(NHH, P, 3), n_het=0)
        verify(hb._lib, "hank_jvp_het", 0, PTR, NULL, NULL, 3, Out(out, (P, 1, 3)))


# -- the transposed sweeps -----------------------------------------------------------------------------------------------------
def _cot_forms(yb):
    """cotangents (P, n_het, M) in every form `vjp` takes"""
    n_het, M = yb.shape[1:]
    forms = _orders(yb)
    if n_het == 1:
        forms += _orders(yb[:, 0, :]) + ((yb[:, 0, 0],) if M == 1 else ())
    return forms


@pytest.mark.parametrize("M", [1, 3])
def test_vjp_family(hb, M):
    xs, bs = (NHH, P, M), (NA, NE, M)
    for n_het in (1, 2):                                                                # vjp's rule: (P,), (P, M), (P, n_het, M)
        yb = _rand(P, n_het, M)
        for y in _cot_forms(yb):
            out = hb.vjp(y, n_het)
            verify(hb._lib, "hank_vjp", n_het, In(yb), M, Out(out, xs))
            out, vb, db = hb.vjp_boundary(y, n_het)
            verify(hb._lib, "hank_vjp_boundary", n_het, In(yb), M, Out(out, xs), Out(vb, bs), Out(db, bs))
            out, ybar = hb.vjp_income(y, n_het)
            verify(hb._lib, "hank_vjp_income", n_het, In(yb), M, Out(out, xs), Out(ybar, (NE, P, M)))
    assert hb.vjp(_rand(P, 1, M)).shape == xs and hb._lib.calls[-1][1][0] == 1         # n_het defaults to 1
    for n_het in (1, 2, 3, 4):                                                          # vjp_het's rule: (P, n_het, M) only
        yb = _rand(P, n_het, M)
        for y in _orders(yb):
            out = hb.vjp_het(y, n_het)
            verify(hb._lib, "hank_vjp_het", n_het, In(yb), M, Out(out, xs))
            out, bb = hb.vjp_shock(y, n_het)
            verify(hb._lib, "hank_vjp_shock", n_het, In(yb), M, Out(out, xs), Out(bb, (P, M)))
            out, vb, db = hb.vjp_het_boundary(y, n_het)
            verify(hb._lib, "hank_vjp_het_boundary", n_het, In(yb), M, Out(out, xs), Out(vb, bs), Out(db, bs))
            out, vb, db = hb.vjp_het_boundary(y, n_het, value_end=False)
            verify(hb._lib, "hank_vjp_het_boundary", n_het, In(yb), M, Out(out, xs), NULL, Out(db, bs))
            assert vb is None
            out, vb, db = hb.vjp_het_boundary(y, n_het, D_init=False)
            verify(hb._lib, "hank_vjp_het_boundary", n_het, In(yb), M, Out(out, xs), Out(vb, bs), NULL)
            assert db is None
            out, vb, db = hb.vjp_het_boundary(y, n_het, value_end=False, D_init=False)
            verify(hb._lib, "hank_vjp_het_boundary", n_het, In(yb), M, Out(out, xs), NULL, NULL)
            assert vb is None and db is None


def test_vjp_family_refusals_and_what_goes_through_to_the_library(hb):
    for m in (hb.vjp, hb.vjp_boundary, hb.vjp_income):
        with pytest.raises(ValueError, match=r"agg_bar must be \(P, n_het, M\) when n_het > 1"):
            m(_rand(P, 3), 2)
        with pytest.raises(ValueError, match=BAD % ("5, 2, 3", "5, 1, 3")):
            m(_rand(P, 1, 3), 2)
        with pytest.raises(ValueError, match=BAD % ("5, 1, 1", "4, 1, 1")):
            m(_rand(P - 1), 1)
    for m in (hb.vjp_het, hb.vjp_shock, hb.vjp_het_boundary):
        for bad in (_rand(P), _rand(P, 3)):
            with pytest.raises(ValueError, match=r"agg_bar must be \(P, n_het, M\)$"):
                m(bad, 1)
        with pytest.raises(ValueError, match=BAD % ("5, 4, 3", "5, 3, 3")):
            m(_rand(P, 3, 3), 4)
    assert hb._lib.calls == []
    # an n_het the library refuses goes through without a shape check (3 for vjp, 5 for vjp_het), and so does M = 0, on a 1-column buffer
    yb = _rand(P, 2, 3)
    out = hb.vjp(yb, 3)
    verify(hb._lib, "hank_vjp", 3, In(yb), 3, Out(out, (NHH, P, 3)))
    out = hb.vjp_het(yb, 5)
    verify(hb._lib, "hank_vjp_het", 5, In(yb), 3, Out(out, (NHH, P, 3)))
    out = hb.vjp_het(yb, 0)
    verify(hb._lib, "hank_vjp_het", 0, In(yb), 3, Out(out, (NHH, P, 3)))
    out, vb, db = hb.vjp_boundary(np.zeros((P, 1, 0)), 1)
    verify(hb._lib, "hank_vjp_boundary", 1, PTR, 0, Out(out, (NHH, P, 1)), Out(vb, (NA, NE, 1)), Out(db, (NA, NE, 1)))
    out, bb = hb.vjp_shock(np.zeros((P, 2, 0)), 2)
    verify(hb._lib, "hank_vjp_shock", 2, PTR, 0, Out(out, (NHH, P, 1)), Out(bb, (P, 1)))
    out, ybar = hb.vjp_income(np.zeros((P, 0)), 1)
    verify(hb._lib, "hank_vjp_income", 1, PTR, 0, Out(out, (NHH, P, 1)), Out(ybar, (NE, P, 1)))


@pytest.mark.parametrize("M", [1, 3])
def test_vjp_group(hb, M):
    gb, yb = _rand(P, K, M), _rand(P, 2, M, seed=1)
    xs, bs = (NHH, P, M), (NA, NE, M)
    for g in _orders(gb) + ((gb[:, :, 0],) if M == 1 else ()):
        out = hb.vjp_group(g)
        assert isinstance(out, np.ndarray)
        verify(hb._lib, "hank_vjp_group", 0, NULL, In(gb), M, Out(out, xs), NULL, NULL)
        for y in _orders(yb):
            out = hb.vjp_group(g, agg_bar=y, n_het=2)
            verify(hb._lib, "hank_vjp_group", 2, In(yb), In(gb), M, Out(out, xs), NULL, NULL)
        out, vb, db = hb.vjp_group(g, value_end=True)
        verify(hb._lib, "hank_vjp_group", 0, NULL, In(gb), M, Out(out, xs), Out(vb, bs), NULL)
        assert db is None
        out, vb, db = hb.vjp_group(g, yb, 2, D_init=True)
        verify(hb._lib, "hank_vjp_group", 2, In(yb), In(gb), M, Out(out, xs), NULL, Out(db, bs))
        assert vb is None
        out, vb, db = hb.vjp_group(g, value_end=True, D_init=True)
        verify(hb._lib, "hank_vjp_group", 0, NULL, In(gb), M, Out(out, xs), Out(vb, bs), Out(db, bs))
    y1 = _rand(P, 1, M, seed=2)
    for y in _cot_forms(y1):                                                            # agg_bar follows vjp's rule
        out = hb.vjp_group(gb, y, 1)
        verify(hb._lib, "hank_vjp_group", 1, In(y1), In(gb), M, Out(out, xs), NULL, NULL)
    out = hb.vjp_group(None, yb, 2)                                                     # (the library refuses a null grp_bar)
    verify(hb._lib, "hank_vjp_group", 2, In(yb), NULL, M, Out(out, xs), NULL, NULL)


def test_vjp_group_refusals_and_what_goes_through_to_the_library(hb):
    with pytest.raises(ValueError, match=r"grp_bar must be \(P, K\) or \(P, K, M\)"):
        hb.vjp_group(_rand(P))
    with pytest.raises(ValueError, match=BAD % ("5, 2, 3", "5, 3, 3")):
        hb.vjp_group(_rand(P, 3, 3))
    with pytest.raises(ValueError, match="agg_bar has 1 columns, grp_bar 3"):
        hb.vjp_group(_rand(P, K, 3), _rand(P, 2, 1), 2)
    with pytest.raises(ValueError, match=r"agg_bar must be \(P, n_het, M\) when n_het > 1"):
        hb.vjp_group(_rand(P, K, 3), _rand(P, 3), 2)
    assert hb._lib.calls == []
    out = hb.vjp_group(None)                                                            # nothing given: one column, for the library to refuse
    verify(hb._lib, "hank_vjp_group", 0, NULL, NULL, 1, Out(out, (NHH, P, 1)), NULL, NULL)
    hb.n_groups = 0                                                                     # no groups: no shape check either
    g = _rand(P, 7, 3)
    out = hb.vjp_group(g)
    verify(hb._lib, "hank_vjp_group", 0, NULL, In(g), 3, Out(out, (NHH, P, 3)), NULL, NULL)
    out = hb.vjp_group(np.zeros((P, 7, 0)))
    verify(hb._lib, "hank_vjp_group", 0, NULL, PTR, 0, Out(out, (NHH, P, 1)), NULL, NULL)


def test_policy_cotangent_and_tangent_readers(hb):
    for M in (0, 1, 3):
        out = hb.policy_cotangent_seq(M)
        verify(hb._lib, "hank_get_policy_cotangent_seq", M, Out(out, (NA, NE, P, max(M, 1))))
    out = hb.dpolicy_seq(3)
    verify(hb._lib, "hank_get_dpolicy_seq", 3, Out(out, (NA, NE, P, 3)))
    out = hb.policy_seq()
    verify(hb._lib, "hank_get_policy_seq", Out(out, (NA, NE, P)))
    out = hb.dist_seq()
    verify(hb._lib, "hank_get_dist_seq", Out(out, (NA, NE, P)))
    agg2, dagg2 = hb.grid_aggregates()
    verify(hb._lib, "hank_get_grid_aggregates", Out(agg2, (P,)), 0, NULL)
    assert dagg2 is None
    agg2, dagg2 = hb.grid_aggregates(3)
    verify(hb._lib, "hank_get_grid_aggregates", Out(agg2, (P,)), 3, Out(dagg2, (P, 3)))


# -- outputs of the last sweeps ------------------------------------------------------------------------------------------------
def test_het_outputs(hb):
    agg, dagg = hb.het_outputs(3)
    verify(hb._lib, "hank_get_het_outputs", 3, NULL, 0, Out(agg, (P, 3)), NULL)
    assert dagg is None
    for N in (1, 3):
        dx, dy = _rand(NHH, P, N), _rand(NE, P, N, seed=1)
        for d in _orders(dx):
            agg, dagg = hb.het_outputs(2, d)
            verify(hb._lib, "hank_get_het_outputs", 2, In(dx), N, Out(agg, (P, 2)), Out(dagg, (P, 2, N)))
            for y in _orders(dy) + ((dy[:, :, 0],) if N == 1 else ()):
                agg, dagg = hb.het_outputs(2, d, dy=y)
                verify(hb._lib, "hank_get_het_outputs_income", 2, In(dx), In(dy), N, Out(agg, (P, 2)), Out(dagg, (P, 2, N)))
        agg, dagg = hb.het_outputs(1, None, dy)                                          # dxhh None beside a dy: zeros
        verify(hb._lib, "hank_get_het_outputs_income", 1, In(np.zeros((NHH, P, N))), In(dy), N, Out(agg, (P, 1)), Out(dagg, (P, 1, N)))
    n = len(hb._lib.calls)
    with pytest.raises(ValueError, match=r"dxhh must be \(2, 5, N\), got \(2, 5\)"):   # a 2-D dxhh is not promoted here
        hb.het_outputs(2, _rand(NHH, P))
    with pytest.raises(ValueError, match=r"dxhh must be \(2, 5, N\), got \(5, 2, 3\)"):
        hb.het_outputs(2, _rand(P, NHH, 3))
    with pytest.raises(ValueError, match=BAD % ("3, 5, 1", "5, 3, 1")):
        hb.het_outputs(2, None, _rand(P, NE))
    assert len(hb._lib.calls) == n and hb.calls["jvp"] == 0


def test_group_outputs(hb):
    agg, dagg = hb.group_outputs()
    verify(hb._lib, "hank_get_group_outputs", NULL, 0, Out(agg, (P, K)), NULL)
    assert dagg is None
    for N in (1, 3):
        dx = _rand(NHH, P, N)
        for d in _orders(dx):
            agg, dagg = hb.group_outputs(d)
            verify(hb._lib, "hank_get_group_outputs", In(dx), N, Out(agg, (P, K)), Out(dagg, (P, K, N)))
    with pytest.raises(ValueError, match=r"dxhh must be \(2, 5, N\), got \(2, 5\)"):
        hb.group_outputs(_rand(NHH, P))
    hb.n_groups = 0                                                                     # (the library refuses a call without groups)
    agg, dagg = hb.group_outputs(dx)
    verify(hb._lib, "hank_get_group_outputs", In(dx), 3, Out(agg, (P, 1)), Out(dagg, (P, 1, 3)))
    F, Dv = hb.fake_news_group()
    verify(hb._lib, "hank_fake_news_group", Out(F, (P, P, NHH, 1)), Out(Dv, (P, NHH, 1)))


def test_set_group_outputs(hb):
    i32 = np.int32
    W = _rand(G, 3)
    for w in _orders(W) + _orders(W.reshape((NA, NE, 3), order="F")):
        hb.set_group_outputs(w, [0, 1, 2])
        verify(hb._lib, "hank_set_group_outputs", 3, In(W), In([0, 1, 2], i32))
        assert hb.n_groups == 3
    hb.set_group_outputs(W, hb.GROUP_CONS)                                               # one base serves every group
    verify(hb._lib, "hank_set_group_outputs", 3, In(W), In([2, 2, 2], i32))
    hb.set_group_outputs(W[:, 0], 1)                                                     # one weight vector (G,)
    verify(hb._lib, "hank_set_group_outputs", 1, In(W[:, :1]), In([1], i32))
    assert hb.n_groups == 1
    hb.set_group_outputs(None, None)
    verify(hb._lib, "hank_set_group_outputs", 0, NULL, NULL)
    assert hb.n_groups == 0
    n = len(hb._lib.calls)
    for bad in (_rand(G + 1, 3), _rand(NE, NA, 3), _rand(G + 1), _rand(2, 2, 2, 2), _rand(NA, NE)):      # (a lone matrix is not one group)
        with pytest.raises(ValueError, match=r"W must be \(12, K\) or \(4, 3, K\), got "):
            hb.set_group_outputs(bad, 0)
    with pytest.raises(ValueError):
        hb.set_group_outputs(W, [0, 1])                                                  # two bases for three groups
    assert len(hb._lib.calls) == n and hb.n_groups == 0


def test_fake_news(hb):
    F, Dv = hb.fake_news()
    verify(hb._lib, "hank_fake_news", Out(F, (P, P, NHH)), Out(Dv, (P, NHH)))
    F, Dv = hb.fake_news_group()
    verify(hb._lib, "hank_fake_news_group", Out(F, (P, P, NHH, K)), Out(Dv, (P, NHH, K)))
    for n_het in (0, 1, 3):                                                              # (0: a one-output buffer for the library to refuse)
        nb = max(n_het, 1)
        F, Dv = hb.fake_news_het(n_het)
        verify(hb._lib, "hank_fake_news_het", n_het, Out(F, (P, P, NHH, nb)), Out(Dv, (P, NHH, nb)))
        F, Dv = hb.fake_news_shock(n_het)
        verify(hb._lib, "hank_fake_news_shock", n_het, Out(F, (P, P, nb)), Out(Dv, (P, nb)))
        F, Dv = hb.fake_news_income(n_het)
        verify(hb._lib, "hank_fake_news_income", n_het, Out(F, (P, P, NE, nb)), Out(Dv, (P, NE, nb)))


# -- the exogenous paths -------------------------------------------------------------------------------------------------------
def test_set_discount_path_and_set_income_path(hb):
    b = 0.9 + 0.01 * np.arange(P)
    hb.discount_path = hb.income_path = None
    for bin_ in (b, list(b), _orders(b)[2], np.stack([b, b])[0]):
        hb.set_discount_path(bin_)
        verify(hb._lib, "hank_set_discount_path", In(b))
        assert np.array_equal(hb.discount_path, b) and hb.discount_path.shape == (P,) and not np.shares_memory(hb.discount_path, bin_)
    with pytest.raises(ValueError, match=r"beta_t must be \(5,\), got \(4,\)"):
        hb.set_discount_path(b[:4])
    with pytest.raises(ValueError, match=r"beta_t must be \(5,\), got \(5, 1\)"):
        hb.set_discount_path(b[:, None])
    assert np.array_equal(hb.discount_path, b)
    hb.set_discount_path(None)
    verify(hb._lib, "hank_set_discount_path", NULL)
    assert hb.discount_path is None
    y = _rand(NE, P)
    for yin in _orders(y):
        hb.set_income_path(yin)
        verify(hb._lib, "hank_set_income_path", In(y))
        assert np.array_equal(hb.income_path, y) and hb.income_path.flags.f_contiguous and not np.shares_memory(hb.income_path, yin)
    with pytest.raises(ValueError, match=BAD % ("3, 5", "5, 3")):
        hb.set_income_path(y.T)
    assert np.array_equal(hb.income_path, y)
    hb.set_income_path(None)
    verify(hb._lib, "hank_set_income_path", NULL)
    assert hb.income_path is None
    assert [c[0] for c in hb._lib.calls].count("hank_set_discount_path") == 5


def test_set_boundary(hb):
    v, d = _rand(NA, NE), _rand(NA, NE, seed=1)
    for vin, din in zip(_orders(v), (d, d.reshape(-1, order="F"), np.asfortranarray(d))):
        hb.set_boundary(vin, din)
        verify(hb._lib, "hank_set_boundary", In(v), In(d))
        assert np.array_equal(hb._boundary[0], v) and np.array_equal(hb._boundary[1], d)
    with pytest.raises(ValueError, match=BAD % ("4, 3", "3, 4")):
        hb.set_boundary(v.T, d)


# -- through the steady state --------------------------------------------------------------------------------------------------
def _ss_fill(iters, resid):
    def fill(*args):
        it, res = args[-2:]
        it[0], it[1], res[0], res[1] = iters[0], iters[1], resid[0], resid[1]
    return fill


def test_ss_jvp_and_ss_vjp(hb, hank):
    hb._lib.fill = {s: _ss_fill((3, 7), (1e-14, 2e-14)) for s in ("hank_ss_jvp", "hank_ss_vjp", "hank_ss_jvp_dev", "hank_ss_vjp_dev")}
    last = {"iters": (3, 7), "resid": (1e-14, 2e-14)}
    for N in (1, 3):
        dx = _rand(NHH, N)
        bs = (NA, NE, N)
        for d in _orders(dx) + ((dx[:, 0],) if N == 1 else ()):
            hb.last_ss = None
            dagg, dV, dpol, dD, iters = hb.ss_jvp(d, n_het=3, tol=1e-12, max_iter=99)
            verify(hb._lib, "hank_ss_jvp", 3, In(dx), N, 1e-12, 99, Out(dV, bs), Out(dpol, bs), Out(dD, bs), Out(dagg, (3, N)), PTR, PTR)
            assert iters == (3, 7) and hb.last_ss == last
        dagg = hb.ss_jvp(dx, n_het=0)[0]                                                # (an n_het the library refuses still gets a buffer)
        verify(hb._lib, "hank_ss_jvp", 0, In(dx), N, 1e-13, 50_000, PTR, PTR, PTR, Out(dagg, (1, N)), PTR, PTR)
        yb, vb, db = _rand(2, N), _rand(NA, NE, N, seed=1), _rand(NA, NE, N, seed=2)
        ybs = _orders(yb) + ((yb[:, 0],) if N == 1 else ())
        for y in ybs:
            out, iters = hb.ss_vjp(y)
            verify(hb._lib, "hank_ss_vjp", 2, In(yb), NULL, NULL, N, 1e-13, 50_000, Out(out, (NHH, N)), PTR, PTR)
            assert iters == (3, 7) and hb.last_ss == last
        for s in _boundary_forms(vb):                                                   # a lone (G, M) cotangent is taken here
            out, _ = hb.ss_vjp(value_bar=s, tol=1e-9, max_iter=5)
            verify(hb._lib, "hank_ss_vjp", 2, NULL, In(vb), NULL, N, 1e-9, 5, Out(out, (NHH, N)), PTR, PTR)
            out, _ = hb.ss_vjp(D_bar=s, n_het=4)
            verify(hb._lib, "hank_ss_vjp", 4, NULL, NULL, In(vb), N, 1e-13, 50_000, Out(out, (NHH, N)), PTR, PTR)
        for y in ybs:
            for s, s2 in zip(_boundary_forms(vb), reversed(_boundary_forms(db))):
                out, _ = hb.ss_vjp(y, s, s2)
                verify(hb._lib, "hank_ss_vjp", 2, In(yb), In(vb), In(db), N, 1e-13, 50_000, Out(out, (NHH, N)), PTR, PTR)
        y5 = _rand(3, N)
        out, _ = hb.ss_vjp(y5, n_het=5)                                                 # an n_het the library refuses: no shape check
        verify(hb._lib, "hank_ss_vjp", 5, In(y5), NULL, NULL, N, 1e-13, 50_000, Out(out, (NHH, N)), PTR, PTR)
    n = len(hb._lib.calls)
    with pytest.raises(ValueError, match="at least one of agg_bar, value_bar, D_bar must be given"):
        hb.ss_vjp()
    with pytest.raises(ValueError, match=BAD % ("2, 3", "3, 3")):
        hb.ss_vjp(_rand(3, 3))
    with pytest.raises(ValueError, match=BAD % ("12, 3", "12, 1")):
        hb.ss_vjp(_rand(2, 3), _rand(NA, NE))
    with pytest.raises(ValueError, match=BAD % ("12, 3", "12, 1")):                      # M is value_bar's when agg_bar is not given
        hb.ss_vjp(None, _rand(NA, NE, 3), _rand(NA, NE))
    with pytest.raises(ValueError, match=BAD % ("2, 4", "3, 4")):
        hb.ss_jvp(_rand(3, 4))
    assert len(hb._lib.calls) == n
    its = hb.ss_jvp_dev(0x1000, 3, 0x2000, 0x3000, 0x4000, 0x5000, n_het=3, tol=1e-11, max_iter=77)
    verify(hb._lib, "hank_ss_jvp_dev", 3, Dev(0x1000), 3, 1e-11, 77, Dev(0x3000), Dev(0x4000), Dev(0x5000), Dev(0x2000), PTR, PTR)
    assert its == (3, 7) and hb.last_ss == last
    hb.ss_jvp_dev(0x1000, 1, 0x2000)
    verify(hb._lib, "hank_ss_jvp_dev", 2, Dev(0x1000), 1, 1e-13, 50_000, NULL, NULL, NULL, Dev(0x2000), PTR, PTR)
    its = hb.ss_vjp_dev(0x1000, 0x2000, 0x3000, 3, 0x4000, n_het=4, tol=1e-11, max_iter=77)
    verify(hb._lib, "hank_ss_vjp_dev", 4, Dev(0x1000), Dev(0x2000), Dev(0x3000), 3, 1e-11, 77, Dev(0x4000), PTR, PTR)
    assert its == (3, 7)
    hb.ss_vjp_dev(0, 0x2000, 0, 1, 0x4000)
    verify(hb._lib, "hank_ss_vjp_dev", 2, NULL, Dev(0x2000), NULL, 1, 1e-13, 50_000, Dev(0x4000), PTR, PTR)
    # a loop that ran into max_iter above tol: SteadyStateLoopError names the method and the loop, check=False returns
    calls = {"ss_jvp": (lambda **kw: hb.ss_jvp(_rand(NHH, 3), **kw), "value", "distribution"),
             "ss_vjp": (lambda **kw: hb.ss_vjp(_rand(2, 3), **kw), "nu", "lambda"),
             "ss_jvp_dev": (lambda **kw: hb.ss_jvp_dev(0x1000, 3, 0x2000, **kw), "value", "distribution"),
             "ss_vjp_dev": (lambda **kw: hb.ss_vjp_dev(0x1000, 0, 0, 3, 0x4000, **kw), "nu", "lambda")}
    for who, (call, first, second) in calls.items():
        hb._lib.fill = {"hank_" + who: _ss_fill((20, 4), (0.5, 1e-15))}
        with pytest.raises(hank.hip.SteadyStateLoopError, match=f"^{who}: the {first} loop took max_iter = 20 steps"):
            call(max_iter=20)
        assert hb.last_ss == {"iters": (20, 4), "resid": (0.5, 1e-15)}
        got = call(max_iter=20, check=False)
        assert (got if who.endswith("_dev") else got[-1]) == (20, 4)
        hb._lib.fill = {"hank_" + who: _ss_fill((4, 20), (1e-15, np.nan))}
        with pytest.raises(hank.hip.SteadyStateLoopError, match=f"^{who}: the {second} loop took max_iter = 20 steps"):
            call(max_iter=20)
        hb._lib.fill = {"hank_" + who: _ss_fill((20, 20), (1e-15, 1e-13))}              # at max_iter but within tol: fine
        call(max_iter=20)


def test_ss_batch(hb, hank):
    i32 = np.int32
    for Kx in (1, 3):
        x = _rand(NHH, Kx)
        v3 = 1.0 + _rand(NA, NE, Kx, seed=1) ** 2
        d3 = np.random.default_rng(Kx).integers(1, 9, (NA, NE, Kx)).astype(float)      # (small integers: a column's sum is exact in any order)
        shape = (NA, NE, Kx)
        ones, uniform = np.ones((G, Kx)), np.full((G, Kx), 1.0 / G)
        starts = [(None, ones, None, uniform)]
        shared_v, shared_d = np.repeat(v3[:, :, :1], Kx, axis=2), np.repeat(d3[:, :, :1], Kx, axis=2)
        for v0, d0 in zip(_orders(v3[:, :, 0]) + (v3[:, :, 0].reshape(-1, order="F"),), _orders(d3[:, :, 0]) + (d3[:, :, 0].reshape(-1, order="F"),)):
            starts.append((v0, shared_v, d0, shared_d / shared_d.sum(axis=(0, 1), keepdims=True)))
        for v0, d0 in zip(_boundary_forms(v3)[:6], _boundary_forms(d3)[:6]):
            starts.append((v0, v3, d0, d3 / d3.sum(axis=(0, 1), keepdims=True)))
        for xin in _orders(x) + ((x[:, 0],) if Kx == 1 else ()):
            for v0, vwant, d0, dwant in starts:
                keep_v, keep_d = None if v0 is None else v0.copy(), None if d0 is None else d0.copy()
                aggs, v, pol, Dn, iters, status = hb.ss_batch(xin, 1e-9, n_het=2, value0=v0, D0=d0, vfi_max_iter=11, dist_tol=1e-12, dist_max_iter=13, check_every=5)
                L = hb.last_ss_batch
                verify(hb._lib, "hank_ss_batch", 2, In(x), Kx, 1e-9, 11, 1e-12, 13, 5, In(vwant), Out(L["policy"], (G, Kx)), In(dwant),
                       Out(aggs, (2, Kx)), Out(iters, (Kx, 2), i32, "C"), Out(L["supnorm"], (Kx,)), Out(status, (Kx,), i32))
                assert v.shape == shape and v.strides == _fstrides(shape, float) and np.shares_memory(v, L["value"])
                assert pol.shape == shape and pol.strides == _fstrides(shape, float) and np.shares_memory(pol, L["policy"])
                assert L["aggs"] is aggs and L["iters"] is iters and L["status"] is status and L["value"].shape == (G, Kx)
                assert Dn.shape == (G, Kx) and np.allclose(Dn.sum(axis=0), 1.0) and not np.shares_memory(Dn, L["D"])
                assert not np.any(iters) and not np.any(status) and not np.any(L["supnorm"])
                assert (v0 is None or np.array_equal(v0, keep_v)) and (d0 is None or np.array_equal(d0, keep_d))      # the caller's arrays are not written
            aggs, v, pol, Dn, iters, status = hb.ss_batch(xin, 1e-9, dist=False)             # value iteration only
            verify(hb._lib, "hank_ss_batch", 1, In(x), Kx, 1e-9, 10_000, 1e-15, 500_000, 25, In(ones), PTR, NULL, NULL, PTR, PTR, PTR)
            assert aggs is None and Dn is None and hb.last_ss_batch["D"] is None
        aggs = hb.ss_batch(x, 1e-9, n_het=0)[0]                                              # (an n_het the library refuses still gets a buffer)
        assert aggs.shape == (1, Kx)
    n = len(hb._lib.calls)
    with pytest.raises(ValueError, match=BAD % ("2, 0", "2, 3, 1")):                          # a wrong rank is K = 0
        hb.ss_batch(_rand(NHH, 3, 1), 1e-9)
    with pytest.raises(ValueError, match=BAD % ("2, 3", "3, 3")):
        hb.ss_batch(_rand(3, 3), 1e-9)
    with pytest.raises(ValueError, match=BAD % ("12, 3", "12, 2")):
        hb.ss_batch(_rand(NHH, 3), 1e-9, value0=_rand(NA, NE, 2))
    with pytest.raises(ValueError, match=BAD % ("12, 3", "12, 2")):
        hb.ss_batch(_rand(NHH, 3), 1e-9, D0=_rand(G, 2))
    assert len(hb._lib.calls) == n
    x0 = np.zeros((NHH, 0))                                                                   # K = 0 reaches the library on one-column buffers
    aggs, v, pol, Dn, iters, status = hb.ss_batch(x0, 1e-9)
    verify(hb._lib, "hank_ss_batch", 1, PTR, 0, 1e-9, 10_000, 1e-15, 500_000, 25, In(np.ones((G, 1))), PTR, In(np.full((G, 1), 1.0 / G)),
           Out(aggs, (1, 1)), Out(iters, (1, 2), i32, "C"), PTR, Out(status, (1,), i32))
    # the raise rule: a failing scenario raises with check=True; with check=False only a refusal of the call itself (no status set)
    def mark(*args):
        np.ctypeslib.as_array(args[-1], (3,))[1] = 3
    hb._lib = Lib(rc=3, fill={"hank_ss_batch": mark})
    with pytest.raises(hank.HankHIPError, match="refused by the stand-in"):
        hb.ss_batch(_rand(NHH, 3), 1e-9)
    assert list(hb.last_ss_batch["status"]) == [0, 3, 0]
    assert list(hb.ss_batch(_rand(NHH, 3), 1e-9, check=False)[-1]) == [0, 3, 0]
    hb._lib = Lib(rc=2)
    with pytest.raises(hank.HankHIPError, match="refused by the stand-in"):
        hb.ss_batch(_rand(NHH, 3), 1e-9, check=False)


def test_primal_batch(hb, hank):
    i32 = np.int32
    for Kx in (1, 3):
        x = _rand(NHH, P, Kx)
        for xin in _orders(x) + ((x[:, :, 0],) if Kx == 1 else ()):
            aggs, status = hb.primal_batch(xin, n_het=2)
            verify(hb._lib, "hank_primal_batch", 2, In(x), Kx, Out(aggs, (P, 2, Kx)), NULL, Out(status, (Kx,), i32))
            aggs, status, pol = hb.primal_batch(xin, policy=True)
            verify(hb._lib, "hank_primal_batch", 1, In(x), Kx, Out(aggs, (P, 1, Kx)), Out(pol, (NA, NE, P, Kx)), Out(status, (Kx,), i32))
            assert hb.last_batch[0] is aggs and hb.last_batch[1] is status and hb.last_batch[2] is pol
    aggs, status = hb.primal_batch(x, n_het=0)                                                # (an n_het the library refuses still gets a buffer)
    verify(hb._lib, "hank_primal_batch", 0, In(x), 3, Out(aggs, (P, 1, 3)), NULL, PTR)
    aggs, status = hb.primal_batch(np.zeros((NHH, P, 0)))                                     # K = 0 reaches the library on one-column buffers
    verify(hb._lib, "hank_primal_batch", 1, PTR, 0, Out(aggs, (P, 1, 1)), NULL, Out(status, (1,), i32))
    n = len(hb._lib.calls)
    with pytest.raises(ValueError, match=BAD % ("2, 5, 0", "2,")):                             # a wrong rank is K = 0
        hb.primal_batch(_rand(NHH))
    with pytest.raises(ValueError, match=BAD % ("2, 5, 3", "5, 2, 3")):
        hb.primal_batch(_rand(P, NHH, 3))
    assert len(hb._lib.calls) == n and hb.calls == {"primal": 0, "jvp": 0, "primal_jvp": 0}

    def mark(*args):
        np.ctypeslib.as_array(args[-1], (3,))[2] = 4
    hb._lib = Lib(rc=4, fill={"hank_primal_batch": mark})
    with pytest.raises(hank.HankHIPError, match="refused by the stand-in"):
        hb.primal_batch(x)
    assert list(hb.primal_batch(x, check=False)[1]) == [0, 0, 4]
    hb._lib = Lib(rc=2)                                                                       # a refusal of the call itself always raises
    with pytest.raises(hank.HankHIPError, match="refused by the stand-in"):
        hb.primal_batch(x, check=False)
    hb._lib = Lib(rc=4, fill={"hank_primal_batch": lambda *a: a[-1].__setitem__(0, 4)})       # ... and so does K = 0, whatever the status says
    with pytest.raises(hank.HankHIPError):
        hb.primal_batch(np.zeros((NHH, P, 0)), check=False)


# -- device pointers: 0 (or None) is NULL, anything else goes through ----------------------------------------------------------
A, B_, C_, D_, E_, F_ = (Dev(0x1000 * k) for k in range(1, 7))
DEV_CASES = [
    ("primal_dev", (A.p, B_.p), "hank_primal_dev", (A, B_)),
    ("primal_dev", (A.p,), "hank_primal_dev", (A, NULL)),
    ("jvp_dev", (A.p, 3, B_.p), "hank_jvp_dev", (A, 3, B_)),
    ("jvp_dev", (A.p, 1), "hank_jvp_dev", (A, 1, NULL)),
    ("primal_jvp_dev", (A.p, B_.p, 3, C_.p, D_.p), "hank_primal_jvp_dev", (A, B_, 3, C_, D_)),
    ("primal_jvp_dev", (A.p, B_.p, 32), "hank_primal_jvp_dev", (A, B_, 32, NULL, NULL)),
    ("primal_batch_dev", (2, A.p, 3, B_.p, C_.p), "hank_primal_batch_dev", (2, A, 3, B_, C_)),
    ("primal_batch_dev", (1, A.p, 3, B_.p), "hank_primal_batch_dev", (1, A, 3, B_, NULL)),
    ("vjp_dev", (2, A.p, 3, B_.p), "hank_vjp_dev", (2, A, 3, B_)),
    ("vjp_het_dev", (4, A.p, 3, B_.p), "hank_vjp_het_dev", (4, A, 3, B_)),
    ("jvp_boundary_dev", (A.p, B_.p, C_.p, 3, D_.p), "hank_jvp_boundary_dev", (A, B_, C_, 3, D_)),
    ("jvp_boundary_dev", (0, B_.p, 0, 3), "hank_jvp_boundary_dev", (NULL, B_, NULL, 3, NULL)),
    ("jvp_boundary_dev", (A.p, 0, C_.p, 1, 0), "hank_jvp_boundary_dev", (A, NULL, C_, 1, NULL)),
    ("vjp_boundary_dev", (2, A.p, 3, B_.p, C_.p, D_.p), "hank_vjp_boundary_dev", (2, A, 3, B_, C_, D_)),
    ("vjp_boundary_dev", (1, A.p, 3, B_.p), "hank_vjp_boundary_dev", (1, A, 3, B_, NULL, NULL)),
    ("vjp_boundary_dev", (1, A.p, 3, B_.p, 0, D_.p), "hank_vjp_boundary_dev", (1, A, 3, B_, NULL, D_)),
    ("jvp_het_dev", (3, A.p, B_.p, C_.p, 3, D_.p), "hank_jvp_het_dev", (3, A, B_, C_, 3, D_)),
    ("jvp_het_dev", (3, 0, 0, C_.p, 3), "hank_jvp_het_dev", (3, NULL, NULL, C_, 3, NULL)),
    ("vjp_het_boundary_dev", (4, A.p, 3, B_.p, C_.p, D_.p), "hank_vjp_het_boundary_dev", (4, A, 3, B_, C_, D_)),
    ("vjp_het_boundary_dev", (4, A.p, 3, B_.p), "hank_vjp_het_boundary_dev", (4, A, 3, B_, NULL, NULL)),
    ("vjp_het_boundary_dev", (4, A.p, 3, B_.p, C_.p, 0), "hank_vjp_het_boundary_dev", (4, A, 3, B_, C_, NULL)),
    ("het_outputs_dev", (2, A.p, 3, B_.p, C_.p), "hank_get_het_outputs_dev", (2, A, 3, B_, C_)),
    ("het_outputs_dev", (2, 0, 0, B_.p, 0), "hank_get_het_outputs_dev", (2, NULL, 0, B_, NULL)),
    ("het_outputs_dev", (2, A.p, 3, B_.p, C_.p, 0), "hank_get_het_outputs_dev", (2, A, 3, B_, C_)),
    ("het_outputs_dev", (2, A.p, 3, B_.p, C_.p, D_.p), "hank_get_het_outputs_income_dev", (2, A, D_, 3, B_, C_)),
    ("het_outputs_dev", (2, 0, 3, 0, C_.p, D_.p), "hank_get_het_outputs_income_dev", (2, NULL, D_, 3, NULL, C_)),
    ("group_outputs_dev", (A.p, 3, B_.p, C_.p), "hank_get_group_outputs_dev", (A, 3, B_, C_)),
    ("group_outputs_dev", (0, 0, B_.p, 0), "hank_get_group_outputs_dev", (NULL, 0, B_, NULL)),
    ("vjp_group_dev", (2, A.p, B_.p, 3, C_.p, D_.p, E_.p), "hank_vjp_group_dev", (2, A, B_, 3, C_, D_, E_)),
    ("vjp_group_dev", (0, 0, B_.p, 3, C_.p), "hank_vjp_group_dev", (0, NULL, B_, 3, C_, NULL, NULL)),
    ("vjp_group_dev", (0, 0, 0, 3, C_.p, 0, E_.p), "hank_vjp_group_dev", (0, NULL, NULL, 3, C_, NULL, E_)),
    ("jvp_shock_dev", (A.p, B_.p, 3, C_.p), "hank_jvp_shock_dev", (A, B_, 3, C_)),
    ("jvp_shock_dev", (0, B_.p, 3), "hank_jvp_shock_dev", (NULL, B_, 3, NULL)),
    ("jvp_shock_dev", (A.p, 0, 3, 0), "hank_jvp_shock_dev", (A, NULL, 3, NULL)),
    ("vjp_shock_dev", (3, A.p, 3, B_.p, C_.p), "hank_vjp_shock_dev", (3, A, 3, B_, C_)),
    ("jvp_income_dev", (A.p, B_.p, 3, C_.p), "hank_jvp_income_dev", (A, B_, 3, C_)),
    ("jvp_income_dev", (0, B_.p, 3), "hank_jvp_income_dev", (NULL, B_, 3, NULL)),
    ("jvp_income_dev", (A.p, 0, 3, 0), "hank_jvp_income_dev", (A, NULL, 3, NULL)),
    ("vjp_income_dev", (2, A.p, 3, B_.p, C_.p), "hank_vjp_income_dev", (2, A, 3, B_, C_)),
    ("set_stream", (A.p,), "hank_set_stream", (A,)),
    ("set_stream", (None,), "hank_set_stream", (NULL,)),
    ("set_stream", (0,), "hank_set_stream", (NULL,)),
]


@pytest.mark.parametrize("method, args, symbol, expect", DEV_CASES, ids=[f"{c[0]}-{k}" for k, c in enumerate(DEV_CASES)])
def test_device_pointer_forms(hb, method, args, symbol, expect):
    assert getattr(hb, method)(*args) is None
    assert len(hb._lib.calls) == 1
    verify(hb._lib, symbol, *expect)
    assert hb.calls == {"primal": 0, "jvp": 0, "primal_jvp": 0}


# -- getters and the status ----------------------------------------------------------------------------------------------------
def _fill_seq(*starts):
    """writes start, start + 1, ... through each array argument"""
    def fill(*arrays):
        for a, s in zip(arrays, starts):
            for i in range(len(a)):
                a[i] = s + i
    return fill


def test_timing_and_counter_getters(hb):
    pairs = ("hank_last_batch_timings", "hank_last_ss_batch_timings", "hank_last_ss_timings")
    hb._lib.fill = {s: _fill_seq(1.5 + k) for k, s in enumerate(pairs)}
    hb._lib.fill.update({"hank_last_timings": _fill_seq(0.5, 10), "hank_last_vjp_timings": _fill_seq(0.25, 20), "hank_stats": _fill_seq(100),
                         "hank_info": _fill_seq(1), "hank_sweep_instance": _fill_seq(-1)})
    for k, s in enumerate(pairs):
        got = getattr(hb, s[len("hank_"):])()
        assert got == (1.5 + k, 2.5 + k) and type(got) is tuple and type(got[0]) is float and hb._lib.calls[-1][0] == s
    names = ("primal_backward", "primal_forward", "tangent_backward", "tangent_forward", "dual_backward", "dual_forward")
    assert hb.last_timings() == {n: {"ms": 0.5 + i, "launches": 10 + i} for i, n in enumerate(names)}
    assert hb.last_vjp_timings() == {"sweep_a": {"ms": 0.25, "launches": 20}, "sweep_b": {"ms": 1.25, "launches": 21}}
    names = ("sweep_launches", "tangent_workspaces_allocated", "graphs_captured", "schedule", "fallbacks", "vfi_iterations", "primal_memo_hits", "primal_sweeps")
    st = hb.stats()
    assert st == {n: 100 + i for i, n in enumerate(names)} and list(st) == list(names) and all(type(v) is int for v in st.values())
    names = ("last_tangent_family", "wide_mode", "wide_min", "wide_supported", "xjvp_max", "record_diet", "record_bytes", "lwg_builds")
    want = {n: 1 + i for i, n in enumerate(names)}
    want["last_tangent_family_name"] = "xcd-persistent"
    assert hb.info() == want
    assert hb.sweep_instance() == {"back": (-1, 0), "fwd": (1, 2)}
    for name, args in hb._lib.calls:
        assert all(_addr(a) != 0 for a in args), name


def test_a_status_becomes_the_exception_of_its_class(hb, hank):
    hip = hank.hip
    for rc, cls in ((hip.HANK_ERR_KNOTS, hip.KnotsNotSortedError), (hip.HANK_ERR_DOMAIN, hip.DomainError), (hip.HANK_ERR_NO_DEVICE, hip.NoDeviceError),
                    (hip.HANK_ERR_BAD_ARG, hip.HankHIPError), (hip.HANK_ERR_NOT_READY, hip.HankHIPError), (77, hip.HankHIPError)):
        hb._lib = Lib(rc=rc)
        for call in (hb.sync, hb.check, lambda: hb.primal(_rand(NHH, P)), lambda: hb.jvp_dev(0x1000, 1), hb.stats, lambda: hb.set_het_outputs(3)):
            with pytest.raises(hip.HankHIPError, match=rf"^\[hank_hip status {rc}\] refused by the stand-in$") as e:
                call()
            assert type(e.value) is cls and e.value.code == rc
    hb._lib = Lib()
    hb.sync(), hb.check(), hb.set_het_outputs(3)
    assert [c[0] for c in hb._lib.calls] == ["hank_sync", "hank_check", "hank_set_het_outputs"] and hb._lib.calls[-1][1] == (3,)
    seen = []
    hb._chk = seen.append                                                                     # a stand-in verdict sees every status
    hb._lib = Lib(rc=5)
    hb.jvp(_rand(NHH, P, 3)), hb.vjp(_rand(P)), hb.het_outputs(2), hb.last_ss_timings(), hb.fake_news_income(1), hb.set_income_path(None)
    assert seen == [5] * 6
