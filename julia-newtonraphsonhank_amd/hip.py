"""ctypes binding of the C ABI in include/hank_hip.h (libhank_hip.so, hand-written HIP for gfx950).

There is no CPU fallback on this path: if the shared library is missing or no MI355X is usable the
constructors raise — the product never silently computes the household block anywhere else.

Every fact of the boundary has one owner here. `ABI` is the C ABI, one row per symbol (tests/test_abi.py holds it against the header
by arity and parameter class); `load_library` applies it in one loop. The module functions under "argument shapes" own one shape
each: a path or a batch of paths (`_batch`), a group of optional seeds (`_seeds`), output buffers and their clamp (`_out`, `_n1`),
device pointers (`_dev`), a status (`_raise_status`); `HouseholdBlock` adds the ones that need its dimensions. `_PATHS` says what
differs between the two exogenous paths. A new entry point is one row of `ABI` and one thin method.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from pathlib import Path

import numpy as np

import os

# HANK_HIP_LIB: a dev knob (instrumented builds of the same library, e.g. `make stamp`)
_LIB_PATH = Path(os.environ.get("HANK_HIP_LIB") or Path(__file__).resolve().parent / "libhank_hip.so")
_lib = None

HANK_OK = 0
HANK_ERR_NO_DEVICE, HANK_ERR_BAD_ARG, HANK_ERR_KNOTS, HANK_ERR_DOMAIN = 1, 2, 3, 4
HANK_ERR_NOT_READY, HANK_ERR_NONMONOTONE, HANK_ERR_NOMEM, HANK_ERR_SWEEP, HANK_ERR_LAUNCH = 5, 6, 7, 8, 9
HANK_VF_KRUSELL_SMITH = 0
HANK_GROUP_MASS, HANK_GROUP_POLICY, HANK_GROUP_CONS = 0, 1, 2      # the base of a group output (hank_set_group_outputs)
HANK_GROUP_MAX = 32


class HankHIPError(RuntimeError):
    """Base class: a non-zero status from libhank_hip (message = hank_last_error)."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"[hank_hip status {code}] {msg}")
        self.code = code


class KnotsNotSortedError(HankHIPError):
    """Interpolations.jl's 'knot-vectors must be unique and sorted' (KrusellSmith.jl:69-72)."""


class DomainError(HankHIPError):
    """Julia's DomainError: negative base under a non-integer power (KrusellSmith.jl:59, :80)."""


class NoDeviceError(HankHIPError):
    """No usable gfx950 device / HIP runtime failure."""


class SteadyStateLoopError(RuntimeError):
    """A fixed-point loop of hank_ss_jvp / hank_ss_vjp ran into max_iter (the library reports that as HANK_OK, like hank_vfi)."""


_ERR_CLASSES = {HANK_ERR_KNOTS: KnotsNotSortedError, HANK_ERR_DOMAIN: DomainError,
                HANK_ERR_NO_DEVICE: NoDeviceError}


class hank_model(C.Structure):
    _fields_ = [("n_a", C.c_int32), ("n_e", C.c_int32), ("T", C.c_int32), ("value_fn_id", C.c_int32),
                ("a_grid", C.POINTER(C.c_double)), ("z_grid", C.POINTER(C.c_double)),
                ("Pi", C.POINTER(C.c_double)),
                ("beta", C.c_double), ("gamma", C.c_double), ("borrow_cons", C.c_double)]


# -- the C ABI -------------------------------------------------------------------------------------------------------------------
# One row per symbol of include/hank_hip.h: its parameters in order, one letter each. Every function returns a status (c_int)
# except those in ABI_RESTYPE.
_ARG = {"v": C.c_void_p,                    # a context, a stream, a device pointer, host memory that is not doubles
        "d": C.POINTER(C.c_double),         # doubles on the host (double x[n] included)
        "i": C.c_int32, "f": C.c_double,
        "I": C.POINTER(C.c_int32), "L": C.POINTER(C.c_int64),
        "m": C.POINTER(hank_model), "V": C.POINTER(C.c_void_p)}
ABI = {name: tuple(_ARG[a] for a in row.split()) for name, row in {
    # lifetime, stream, verdict
    "hank_create": "m V", "hank_create_on": "m i V", "hank_destroy": "v", "hank_gather_columns": "V i V I v", "hank_last_error": "v",
    "hank_n_hh": "v", "hank_device_available": "", "hank_set_stream": "v v", "hank_sync": "v", "hank_check": "v",
    # boundary and the fused sweeps
    "hank_set_boundary": "v d d", "hank_primal": "v d d", "hank_primal_dev": "v v v", "hank_jvp": "v d i d", "hank_jvp_dev": "v v i v",
    "hank_primal_jvp": "v d d i d d", "hank_primal_jvp_dev": "v v v i v v",
    # what the last sweeps left
    "hank_get_policy_seq": "v d", "hank_get_dpolicy_seq": "v i d", "hank_get_dist_seq": "v d",
    "hank_get_lottery_record": "v v d d v d", "hank_get_forward_units": "v v v",
    "hank_set_het_outputs": "v i", "hank_get_het_outputs": "v i d i d d", "hank_get_het_outputs_dev": "v i v i v v",
    "hank_get_het_outputs_income": "v i d d i d d", "hank_get_het_outputs_income_dev": "v i v v i v v",
    "hank_get_grid_aggregates": "v d i d", "hank_get_grid_aggregates_dev": "v v i v",
    "hank_last_timings": "v d I", "hank_stats": "v L", "hank_info": "v L", "hank_sweep_instance": "v I",
    # granular steps, steady state, Toeplitz forms
    "hank_backward_step": "v d d d d", "hank_backward_step_dual": "v d d d d i d d d d",
    "hank_forward_step": "v d d d d", "hank_forward_step_dual": "v d d d d i d d d d",
    "hank_vfi": "v d f i d d I d", "hank_stationary_dist": "v d d f i i I",
    "hank_fake_news": "v d d", "hank_fake_news_het": "v i d d", "hank_fake_news_group": "v d d",
    # the transposed block
    "hank_vjp": "v i d i d", "hank_vjp_dev": "v i v i v", "hank_vjp_het": "v i d i d", "hank_vjp_het_dev": "v i v i v",
    "hank_get_policy_cotangent_seq": "v i d", "hank_last_vjp_timings": "v d I",
    # the boundary, every output in one pair of sweeps
    "hank_jvp_boundary": "v d d d i d", "hank_jvp_boundary_dev": "v v v v i v",
    "hank_vjp_boundary": "v i d i d d d", "hank_vjp_boundary_dev": "v i v i v v v",
    "hank_jvp_het": "v i d d d i d", "hank_jvp_het_dev": "v i v v v i v",
    "hank_vjp_het_boundary": "v i d i d d d", "hank_vjp_het_boundary_dev": "v i v i v v v",
    # through the steady state
    "hank_ss_jvp": "v i d i f i d d d d I d", "hank_ss_jvp_dev": "v i v i f i v v v v I d",
    "hank_ss_vjp": "v i d d d i f i d I d", "hank_ss_vjp_dev": "v i v v v i f i v I d", "hank_last_ss_timings": "v d",
    # scenarios
    "hank_primal_batch": "v i d i d d I", "hank_primal_batch_dev": "v i v i v v", "hank_last_batch_timings": "v d",
    "hank_ss_batch": "v i d i f i f i i d d d d I d I", "hank_last_ss_batch_timings": "v d",
    # group outputs
    "hank_set_group_outputs": "v i d I", "hank_get_group_outputs": "v d i d d", "hank_get_group_outputs_dev": "v v i v v",
    "hank_vjp_group": "v i d d i d d d", "hank_vjp_group_dev": "v i v v i v v v",
    # the exogenous paths (_PATHS)
    "hank_set_discount_path": "v d", "hank_jvp_shock": "v d d i d", "hank_jvp_shock_dev": "v v v i v",
    "hank_vjp_shock": "v i d i d d", "hank_vjp_shock_dev": "v i v i v v", "hank_fake_news_shock": "v i d d",
    "hank_set_income_path": "v d", "hank_jvp_income": "v d d i d", "hank_jvp_income_dev": "v v v i v",
    "hank_vjp_income": "v i d i d d", "hank_vjp_income_dev": "v i v i v v", "hank_fake_news_income": "v i d d",
}.items()}
ABI_RESTYPE = {"hank_last_error": C.c_char_p}
ABI_OPTIONAL = frozenset({"hank_get_lottery_record", "hank_get_forward_units"})      # (an older library named by HANK_HIP_LIB for an A-B has none)
# the symbols include/hank_hip.h declares (tests check that every one is exported)
ABI_SYMBOLS = tuple(ABI)
# The rows of the extension headers, in the same letters and bound by the same loop (load_library): one table per header, so that
# ABI stays the image of include/hank_hip.h. include/hank_hip_borrow.h: the borrowing-limit path (_PATHS["borrow"]).
ABI_BORROW = {name: tuple(_ARG[a] for a in row.split()) for name, row in {
    "hank_set_borrow_path": "v d", "hank_jvp_borrow": "v d d i d", "hank_jvp_borrow_dev": "v v v i v",
    "hank_vjp_borrow": "v i d i d d", "hank_vjp_borrow_dev": "v i v i v v", "hank_fake_news_borrow": "v i d d",
}.items()}


def library_path() -> Path:
    return _LIB_PATH


def load_library() -> C.CDLL:
    """dlopen libhank_hip.so (built by __graft_entry__.build() / csrc/Makefile). Fails loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if not _LIB_PATH.exists():
        raise RuntimeError(
            f"{_LIB_PATH} is missing: the HIP extension has not been built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback.")
    lib = C.CDLL(str(_LIB_PATH))
    for name, argtypes in {**ABI, **ABI_BORROW}.items():
        if name in ABI_OPTIONAL and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = list(argtypes), ABI_RESTYPE.get(name, C.c_int)
    _lib = lib
    return lib


def device_available() -> bool:
    """True when libhank_hip.so is built and the current HIP device is an MI355X (gfx950)."""
    try:
        return bool(load_library().hank_device_available())
    except (RuntimeError, OSError):
        return False


# -- argument shapes: one owner each -----------------------------------------------------------------------------------------------
def _raise_status(lib, ctx, rc: int, msg=None):
    """a status that is not HANK_OK becomes the exception of its class, with `msg` or the context's hank_last_error"""
    if rc != HANK_OK:
        raise _ERR_CLASSES.get(rc, HankHIPError)(rc, lib.hank_last_error(ctx).decode() if msg is None else msg)


def _f(x, shape=None) -> np.ndarray:
    """contiguous column-major float64 copy (Julia's memory layout), optionally shape-checked."""
    arr = np.asfortranarray(np.asarray(x, dtype=np.float64))
    if shape is not None and tuple(arr.shape) != tuple(shape):
        raise ValueError(f"expected array of shape {tuple(shape)}, got {tuple(arr.shape)}")
    return arr


def _p(arr: np.ndarray):
    return arr.ctypes.data_as(C.POINTER(C.c_double))


def _opt(arr):
    """an optional array's pointer: None (a null pointer) stays None"""
    return None if arr is None else _p(arr)


def _ip(arr: np.ndarray):
    return arr.ctypes.data_as(C.POINTER(C.c_int32))


def _dev(ptr):
    """a device pointer (or a stream handle) as the library takes it: 0 or None is NULL"""
    return C.c_void_p(ptr or None)


def _n1(n) -> int:
    """a count of columns or outputs as a buffer's extent: at least 1, so that a count of 0 reaches the library's own refusal"""
    return max(int(n), 1)


def _out(*dims) -> np.ndarray:
    """a column-major output buffer"""
    return np.empty(dims, order="F")


def _cols(x, rank: int) -> np.ndarray:
    """x as float64 with its trailing batch axis: an array of `rank` axes is one column"""
    a = np.asarray(x, dtype=np.float64)
    return a[..., None] if a.ndim == rank else a


def _batch(x, dims, N=None, strict=False):
    """a path or a batch of paths: x of shape `dims` or (*dims, N) -> ((*dims, N) column-major, N). A given N is checked, not
    taken from x; strict: any other rank is a batch of no columns (primal_batch, ss_batch)."""
    a = _cols(x, len(dims))
    if N is None:
        N = 0 if strict and a.ndim != len(dims) + 1 else a.shape[len(dims)]
    return _f(a, (*dims, N)), N


def _seeds(named, N=None, last_first=False):
    """a group of optional seeds, `named` = ((name, seed, dims), ...): at least one is given; N is the caller's or the first given
    seed's; every given seed -> (*dims, N) column-major (`_batch`), or what `dims(seed, N)` makes of it where dims is a function;
    None stays None. last_first: the seeds are checked from the last to the first. -> (N, [seeds])"""
    given = [(seed, dims) for _, seed, dims in named if seed is not None]
    if not given:
        raise ValueError(f"at least one of {', '.join(name for name, _, _ in named)} must be given")
    if N is None:
        seed, dims = given[0]
        N = _cols(seed, len(dims)).shape[len(dims)]
    out = [None] * len(named)
    for i in reversed(range(len(named))) if last_first else range(len(named)):
        _, seed, dims = named[i]
        if seed is not None:
            out[i] = dims(seed, N) if callable(dims) else _batch(seed, dims, N)[0]
    return N, out


def _grid_batch(x, n_a: int, n_e: int) -> np.ndarray:
    """a batch on the grid, (n_a, n_e) or (n_a, n_e, N) -> (G, N) with pt = e n_a + a; any other shape ((G, N) among them) as it is"""
    s = np.asarray(x, dtype=np.float64)
    if s.shape == (n_a, n_e):
        s = _cols(s, 2)
    if s.ndim == 3 and s.shape[:2] == (n_a, n_e):
        s = s.reshape((n_a * n_e, s.shape[2]), order="F")
    return s


# What differs between the exogenous paths: the attribute that holds the path in force, the name of its seed, the axes in
# front of the period axis (the path is (*axes, P), a seed (*axes, P, N), the Toeplitz form (P, P, *axes, n_het)), the C symbols
# (the device-pointer forms add _dev), and whether its transposed entry takes cotangents by `vjp_het`'s rule or by `vjp`'s.
_Path = namedtuple("_Path", "attr seed axes set jvp vjp fake_news het")
_PATHS = {
    "discount": _Path("discount_path", "dbeta", lambda hb: (), "hank_set_discount_path", "hank_jvp_shock", "hank_vjp_shock", "hank_fake_news_shock", True),
    "income": _Path("income_path", "dy", lambda hb: (hb.n_e,), "hank_set_income_path", "hank_jvp_income", "hank_vjp_income", "hank_fake_news_income", False),
    "borrow": _Path("borrow_path", "damin", lambda hb: (), "hank_set_borrow_path", "hank_jvp_borrow", "hank_vjp_borrow", "hank_fake_news_borrow", True),
}


def gather_columns(blocks, d_block_ptrs, N_k, d_out_ptr: int):
    """hank_gather_columns: the (P, N_k) column blocks the contexts `blocks` hold in their own GPUs' memory (device pointers
    `d_block_ptrs`, as written by jvp_dev / primal_jvp_dev) assembled as one (P, sum N_k) matrix at `d_out_ptr` on blocks[0]'s device
    — over xGMI where the devices differ. Asynchronous: blocks[0].sync() before reading."""
    lib = load_library()
    n = len(blocks)
    ctxs = (C.c_void_p * n)(*[b._ctx for b in blocks])
    ptrs = (C.c_void_p * n)(*[C.c_void_p(int(p)) for p in d_block_ptrs])
    nk = (C.c_int32 * n)(*[int(v) for v in N_k])
    _raise_status(lib, blocks[0]._ctx, lib.hank_gather_columns(ctxs, n, ptrs, nk, C.c_void_p(int(d_out_ptr))))


class HouseholdBlock:
    """One hank_ctx: the device-resident household block of a SequenceModel.

    Mirrors what `BackwardIteration` / `ForwardIteration` read from `model` (grids, Π, β, γ,
    borrow_cons, T; GeneralStructures.jl:216-226) and from `ss_end` / `ss_initial`.
    All matrices are (n_a, n_e); numpy arrays of that shape are accepted in any memory order.
    """
    GROUP_MASS, GROUP_POLICY, GROUP_CONS = HANK_GROUP_MASS, HANK_GROUP_POLICY, HANK_GROUP_CONS

    def __init__(self, a_grid, z_grid, Pi, beta, gamma, borrow_cons, T, value_fn_id=HANK_VF_KRUSELL_SMITH, device=None):
        """device: HIP device ordinal of the context (hank_create_on); None = the calling thread's current device."""
        self._lib = load_library()
        self.device = device
        self._ctx = C.c_void_p()
        self.a_grid = np.ascontiguousarray(a_grid, dtype=np.float64)
        self.z_grid = np.ascontiguousarray(z_grid, dtype=np.float64)
        self.n_a, self.n_e = self.a_grid.size, self.z_grid.size
        self.Pi = _f(Pi, (self.n_e, self.n_e))
        self.T, self.P, self.G = int(T), int(T) - 1, self.n_a * self.n_e
        self._params = (float(beta), float(gamma), float(borrow_cons), value_fn_id)
        self._boundary = None
        self.discount_path = None      # the beta_t path in force (set_discount_path), or None: the model's constant beta
        self.income_path = None        # the y_t[e] path in force (set_income_path), or None
        self.borrow_path = None        # the amin_t path in force (set_borrow_path), or None: the model's constant borrow_cons
        m = hank_model(self.n_a, self.n_e, self.T, value_fn_id, _p(self.a_grid), _p(self.z_grid),
                       _p(self.Pi), float(beta), float(gamma), float(borrow_cons))
        if device is None:
            rc = self._lib.hank_create(C.byref(m), C.byref(self._ctx))
        else:
            rc = self._lib.hank_create_on(C.byref(m), int(device), C.byref(self._ctx))
        if rc != HANK_OK:
            msg = self._lib.hank_last_error(self._ctx).decode() if self._ctx else "hank_create failed"
            if not msg and rc == HANK_ERR_NO_DEVICE:
                msg = "no HIP device available"
            if self._ctx:
                self._lib.hank_destroy(self._ctx)
                self._ctx = C.c_void_p()
            _raise_status(self._lib, None, rc, msg or "no HIP device available (gfx950 required)")
        self.n_hh = self._lib.hank_n_hh(self._ctx)
        # sweeps issued through this context, by entry point (tests assert "ONE sweep per fullFunction")
        self.calls = {"primal": 0, "jvp": 0, "primal_jvp": 0}
        self.n_groups = 0      # group outputs set on this context (set_group_outputs)

    # -- plumbing ---------------------------------------------------------------------------
    def _chk(self, rc: int):
        _raise_status(self._lib, self._ctx, rc)

    def _call(self, symbol: str, *args):
        """one entry of the library on this context; its status through `_chk`"""
        self._chk(getattr(self._lib, symbol)(self._ctx, *args))

    def _read(self, symbol: str, *bufs):
        """a getter that fills small ctypes arrays -> their contents, a list each"""
        self._call(symbol, *bufs)
        return [list(b) for b in bufs]

    def _ms_pair(self, symbol: str):
        """the two times (ms, HIP events on the stream) a timing getter reports"""
        ms, = self._read(symbol, (C.c_double * 2)())
        return (ms[0], ms[1])

    def _ms_launches(self, symbol: str, names):
        ms, ln = self._read(symbol, (C.c_double * len(names))(), (C.c_int32 * len(names))())
        return {k: {"ms": ms[i], "launches": ln[i]} for i, k in enumerate(names)}

    def _counters(self, symbol: str, names):
        out, = self._read(symbol, (C.c_int64 * 8)())
        return {k: int(out[i]) for i, k in enumerate(names)}

    def _cot_outputs(self, M, value_end=False, D_init=False):
        """the outputs of a transposed sweep of M columns: (xhh_bar (n_hh, P, M), value_end_bar, D_init_bar (n_a, n_e, M)), a boundary
        cotangent that is not wanted None"""
        M = _n1(M)
        return (_out(self.n_hh, self.P, M), _out(self.n_a, self.n_e, M) if value_end else None,
                _out(self.n_a, self.n_e, M) if D_init else None)

    def _sweep_input(self, dxhh):
        """`dxhh` (n_hh, P, N), the input of the last tangent sweep, passed again to a reader of that batch -> (column-major, N)"""
        dxhh = np.asfortranarray(dxhh, dtype=np.float64)
        if dxhh.ndim != 3 or dxhh.shape[:2] != (self.n_hh, self.P):      # (a 2-D dxhh is not promoted here, as it never was)
            raise ValueError(f"dxhh must be ({self.n_hh}, {self.P}, N), got {dxhh.shape}")
        return dxhh, dxhh.shape[2]

    def clone(self, device=None) -> "HouseholdBlock":
        """A second, independent context of the same model and boundary (its own device memory, graphs and
        stream): independent tangent batches — Jacobian column chunks — can be in flight on both. `device`: put the
        clone on another GPU of the node (default: this context's). The clone carries no group outputs: call
        `set_group_outputs` on it."""
        beta, gamma, bc, vf = self._params
        other = HouseholdBlock(self.a_grid, self.z_grid, self.Pi, beta, gamma, bc, self.T, vf, device=self.device if device is None else device)
        if self._boundary is not None:
            other.set_boundary(*self._boundary)
        for kind, path in _PATHS.items():
            if getattr(self, path.attr) is not None:
                other._set_path(kind, getattr(self, path.attr))
        return other

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.hank_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream_handle: int | None):
        self._call("hank_set_stream", _dev(hip_stream_handle))

    def sync(self):
        self._call("hank_sync")

    def check(self):
        self._call("hank_check")

    # -- boundary + fused sweeps ------------------------------------------------------------
    def set_boundary(self, ss_end_value, ss_init_D):
        v = _f(ss_end_value, (self.n_a, self.n_e))
        d = _f(np.asarray(ss_init_D, dtype=np.float64).reshape((self.n_a, self.n_e), order="F"))
        self._call("hank_set_boundary", _p(v), _p(d))
        self._boundary = (v, d)

    def primal(self, xhh) -> np.ndarray:
        x = _f(xhh, (self.n_hh, self.P))
        agg = np.empty(self.P)
        self.calls["primal"] += 1
        self._call("hank_primal", _p(x), _p(agg))
        return agg

    def jvp(self, dxhh) -> np.ndarray:
        dx, N = _batch(dxhh, (self.n_hh, self.P))
        out = _out(self.P, N)
        self.calls["jvp"] += 1
        self._call("hank_jvp", _p(dx), N, _p(out))
        return out

    def primal_jvp(self, xhh, dxhh):
        """value and N partials in one dual-sweep pass (what JVP(fullFunction, x, y) does in the reference)."""
        x = _f(xhh, (self.n_hh, self.P))
        dx, N = _batch(dxhh, (self.n_hh, self.P))
        agg = np.empty(self.P)
        dagg = _out(self.P, N)
        self.calls["primal_jvp"] += 1
        self._call("hank_primal_jvp", _p(x), _p(dx), N, _p(agg), _p(dagg))
        return agg, dagg

    def primal_jvp_dev(self, d_xhh_ptr: int, d_dxhh_ptr: int, N: int, d_agg_ptr: int = 0, d_dagg_ptr: int = 0):
        self._call("hank_primal_jvp_dev", _dev(d_xhh_ptr), _dev(d_dxhh_ptr), int(N), _dev(d_agg_ptr), _dev(d_dagg_ptr))

    def primal_dev(self, d_xhh_ptr: int, d_agg_ptr: int = 0):
        self._call("hank_primal_dev", _dev(d_xhh_ptr), _dev(d_agg_ptr))

    def jvp_dev(self, d_dxhh_ptr: int, N: int, d_dagg_ptr: int = 0):
        self._call("hank_jvp_dev", _dev(d_dxhh_ptr), int(N), _dev(d_dagg_ptr))

    # -- the exogenous paths: one body each, the kinds in _PATHS -------------------------------
    def _set_path(self, kind, path):
        k = _PATHS[kind]
        if path is not None:
            path = _f(path, (*k.axes(self), self.P))
        self._call(k.set, _opt(path))
        setattr(self, k.attr, None if path is None else path.copy(order="F"))

    def _path_dirs(self, kind, dxhh, seed):
        """the directions of a path's tangent entry: dxhh (n_hh, P[, N]) or None, seed (*axes, P[, N]) or None -> (N, dx, seed) column-major"""
        k = _PATHS[kind]
        N, (dx, seed) = _seeds((("dxhh", dxhh, (self.n_hh, self.P)), (k.seed, seed, (*k.axes(self), self.P))),
                               last_first=True)      # (a bad path seed has always been reported before a bad dxhh)
        return N, dx, seed

    def _jvp_path(self, kind, dxhh, seed):
        N, dx, seed = self._path_dirs(kind, dxhh, seed)
        out = _out(self.P, N)
        self.calls["jvp"] += 1
        self._call(_PATHS[kind].jvp, _opt(dx), _opt(seed), N, _p(out))
        return out

    def _jvp_path_dev(self, kind, d_dxhh_ptr, d_seed_ptr, N, d_dagg_ptr):
        self._call(_PATHS[kind].jvp + "_dev", _dev(d_dxhh_ptr), _dev(d_seed_ptr), int(N), _dev(d_dagg_ptr))

    def _vjp_path(self, kind, agg_bar, n_het):
        k = _PATHS[kind]
        M, yb = self._cotangents(agg_bar, n_het, het=k.het)
        out = self._cot_outputs(M)[0]
        bar = _out(*k.axes(self), self.P, _n1(M))
        self._call(k.vjp, int(n_het), _p(yb), M, _p(out), _p(bar))
        return out, bar

    def _vjp_path_dev(self, kind, n_het, d_agg_bar_ptr, M, d_xhh_bar_ptr, d_bar_ptr):
        self._call(_PATHS[kind].vjp + "_dev", int(n_het), _dev(d_agg_bar_ptr), int(M), _dev(d_xhh_bar_ptr), _dev(d_bar_ptr))

    def _fake_news_path(self, kind, n_het):
        k = _PATHS[kind]
        F = _out(self.P, self.P, *k.axes(self), _n1(n_het))
        Dv = _out(self.P, *k.axes(self), _n1(n_het))
        self._call(k.fake_news, int(n_het), _p(F), _p(Dv))
        return F, Dv

    def set_discount_path(self, beta_t):
        """a path beta_t (P,) of the discount factor (hank_set_discount_path): beta_t is the factor in period t's Euler equation,
        u'(c_t) = beta_t E_t[V_{t+1}], so beta_{P-1} multiplies the expectation of the terminal value. None returns to the
        model's constant. Like a new boundary it drops the record: the next tangent sweep needs a primal first. While a path is
        set every sweep runs on the per-period launches; the scenario, steady-state and `fake_news*` entries are refused."""
        if beta_t is not None:
            beta_t = np.ascontiguousarray(beta_t, dtype=np.float64)
            if beta_t.shape != (self.P,):
                raise ValueError(f"beta_t must be ({self.P},), got {beta_t.shape}")
        self._set_path("discount", beta_t)

    def jvp_shock(self, dxhh=None, dbeta=None) -> np.ndarray:
        """the tangent sweeps with seeds in the discount-factor path as well (hank_jvp_shock): dxhh (n_hh, P, N) as in `jvp`,
        dbeta (P,) or (P, N); None means zeros, at least one must be given. -> dagg (P, N). Works with or without a path set;
        always the launch family. The batch is current afterwards as `jvp`'s is: `dpolicy_seq`, `grid_aggregates`,
        `het_outputs(n_het, dxhh)` and `group_outputs(dxhh)` serve it — beta has no direct term in any output, so pass the same
        dxhh (zeros for None)."""
        return self._jvp_path("discount", dxhh, dbeta)

    def jvp_shock_dev(self, d_dxhh_ptr: int, d_dbeta_ptr: int, N: int, d_dagg_ptr: int = 0):
        """device-pointer form (asynchronous on the context's stream); a pointer of 0 is a zero seed."""
        self._jvp_path_dev("discount", d_dxhh_ptr, d_dbeta_ptr, N, d_dagg_ptr)

    def vjp_shock(self, agg_bar, n_het: int):
        """`vjp_het` with the cotangent of the discount-factor path (hank_vjp_shock): agg_bar (P, n_het, M) -> (xhh_bar
        (n_hh, P, M), beta_bar (P, M)); the exact transpose of `jvp_shock` followed by `het_outputs(n_het)`. xhh_bar equals
        `vjp_het`'s bit for bit; beta_bar is a fixed-order reduction (the same inputs give the same bits)."""
        return self._vjp_path("discount", agg_bar, n_het)

    def vjp_shock_dev(self, n_het: int, d_agg_bar_ptr: int, M: int, d_xhh_bar_ptr: int, d_beta_bar_ptr: int):
        """device-pointer form (asynchronous on the context's stream)."""
        self._vjp_path_dev("discount", n_het, d_agg_bar_ptr, M, d_xhh_bar_ptr, d_beta_bar_ptr)

    def fake_news_shock(self, n_het: int):
        """the Toeplitz form of every output's Jacobian with respect to the discount-factor path at the steady state
        (hank_fake_news_shock): -> (F (P, P, n_het), Dv (P, n_het)), the definitions of `fake_news_het` with the input fixed to
        beta. `SteadyStateJacobian.shock_jacobian` does the recursion. Same precondition as `fake_news`; no path may be set."""
        return self._fake_news_path("discount", n_het)

    def set_income_path(self, y):
        """a path y (n_e, P) of additive income by productivity state (hank_set_income_path): the budget of period t is
        c + a' = (1 + r_t) a + w_t z_e + tr_t + y_t[e]. None clears it. Like a new boundary it drops the record: the next tangent
        sweep needs a primal first. While a path is set every sweep runs on the per-period launches and the entries that rebuild
        consumption from the inputs or are defined at one income process are refused; it excludes a discount-factor path."""
        self._set_path("income", y)

    def jvp_income(self, dxhh=None, dy=None) -> np.ndarray:
        """the tangent sweeps with seeds in the income path as well (hank_jvp_income): dxhh (n_hh, P, N) as in `jvp`, dy (n_e, P)
        or (n_e, P, N); None means zeros, at least one must be given. -> dagg (P, N). Works with or without a path set; always the
        launch family. The batch is current afterwards as `jvp`'s is: `dpolicy_seq`, `grid_aggregates`, `group_outputs` (mass and
        policy bases) and `het_outputs(n_het, dxhh)` serve it — y has a direct term in consumption, which `het_outputs` adds from
        the dy the batch carries (or from a `dy=` of the caller's); Value, UCE and consumption groups have no tangent at such a batch."""
        return self._jvp_path("income", dxhh, dy)

    def jvp_income_dev(self, d_dxhh_ptr: int, d_dy_ptr: int, N: int, d_dagg_ptr: int = 0):
        """device-pointer form (asynchronous on the context's stream); a pointer of 0 is a zero seed."""
        self._jvp_path_dev("income", d_dxhh_ptr, d_dy_ptr, N, d_dagg_ptr)

    def vjp_income(self, agg_bar, n_het: int = 1):
        """`vjp` with the cotangent of the income path (hank_vjp_income): agg_bar as in `vjp` -> (xhh_bar (n_hh, P, M), y_bar
        (n_e, P, M)); the exact transpose of `jvp_income` followed by `het_outputs(n_het, dxhh, dy=dy)`. xhh_bar equals `vjp`'s bit
        for bit; y_bar is a fixed-order reduction (the same inputs give the same bits)."""
        return self._vjp_path("income", agg_bar, n_het)

    def vjp_income_dev(self, n_het: int, d_agg_bar_ptr: int, M: int, d_xhh_bar_ptr: int, d_y_bar_ptr: int):
        """device-pointer form (asynchronous on the context's stream)."""
        self._vjp_path_dev("income", n_het, d_agg_bar_ptr, M, d_xhh_bar_ptr, d_y_bar_ptr)

    def fake_news_income(self, n_het: int):
        """the Toeplitz form of the Jacobian of outputs 0 .. n_het-1 (n_het <= 2) with respect to the income path at the steady
        state (hank_fake_news_income): -> (F (P, P, n_e, n_het), Dv (P, n_e, n_het)), the definitions of `fake_news_het` with the
        input fixed to y[e]. `SteadyStateJacobian.income_jacobian` does the recursion. Same precondition as `fake_news`; no path
        may be set."""
        return self._fake_news_path("income", n_het)

    def set_borrow_path(self, amin_t):
        """a path amin_t (P,) of the borrowing limit (hank_set_borrow_path): amin_t is the limit in period t's choice,
        a'_t = max(g_t, amin_t). None returns to the model's constant. Like a new boundary it drops the record. While a path is set
        every sweep runs on the per-period launches; the scenario, steady-state and `fake_news*` entries are refused; it excludes
        the other two paths. MIND THE KINK: with amin_t <= a_grid[0] the limit never binds through max — the grid's flat
        extrapolation binds instead — and every partial in amin_t is an exact zero: a grid that is to show a response carries
        points below the limit. With amin_t on a grid point a_grid[k], k > 0, the derivative is the left one."""
        if amin_t is not None:
            amin_t = np.ascontiguousarray(amin_t, dtype=np.float64)
            if amin_t.shape != (self.P,):
                raise ValueError(f"amin_t must be ({self.P},), got {amin_t.shape}")
        self._set_path("borrow", amin_t)

    def jvp_borrow(self, dxhh=None, damin=None) -> np.ndarray:
        """the tangent sweeps with seeds in the borrowing-limit path as well (hank_jvp_borrow): dxhh (n_hh, P, N) as in `jvp`,
        damin (P,) or (P, N); None means zeros, at least one must be given. -> dagg (P, N). Works with or without a path set;
        always the launch family. The batch is current afterwards as `jvp`'s is: `dpolicy_seq`, `grid_aggregates`,
        `het_outputs(n_het, dxhh)` and `group_outputs(dxhh)` serve it — the limit has no direct term in any output, so pass the
        same dxhh (zeros for None)."""
        return self._jvp_path("borrow", dxhh, damin)

    def jvp_borrow_dev(self, d_dxhh_ptr: int, d_damin_ptr: int, N: int, d_dagg_ptr: int = 0):
        """device-pointer form (asynchronous on the context's stream); a pointer of 0 is a zero seed."""
        self._jvp_path_dev("borrow", d_dxhh_ptr, d_damin_ptr, N, d_dagg_ptr)

    def vjp_borrow(self, agg_bar, n_het: int):
        """`vjp_het` with the cotangent of the borrowing-limit path (hank_vjp_borrow): agg_bar (P, n_het, M) -> (xhh_bar
        (n_hh, P, M), amin_bar (P, M)); the exact transpose of `jvp_borrow` followed by `het_outputs(n_het)`. xhh_bar equals
        `vjp_het`'s bit for bit; amin_bar is a fixed-order reduction (the same inputs give the same bits)."""
        return self._vjp_path("borrow", agg_bar, n_het)

    def vjp_borrow_dev(self, n_het: int, d_agg_bar_ptr: int, M: int, d_xhh_bar_ptr: int, d_amin_bar_ptr: int):
        """device-pointer form (asynchronous on the context's stream)."""
        self._vjp_path_dev("borrow", n_het, d_agg_bar_ptr, M, d_xhh_bar_ptr, d_amin_bar_ptr)

    def fake_news_borrow(self, n_het: int):
        """the Toeplitz form of every output's Jacobian with respect to the borrowing-limit path at the steady state
        (hank_fake_news_borrow): -> (F (P, P, n_het), Dv (P, n_het)), the definitions of `fake_news_het` with the input fixed to
        the limit. `SteadyStateJacobian.borrow_jacobian` does the recursion. Same precondition as `fake_news`; no path may be
        set. A steady state whose limit is a_grid[0] gives zeros (the kink convention of `set_borrow_path`)."""
        return self._fake_news_path("borrow", n_het)

    # -- K input paths through one chain of launches ------------------------------------------
    def primal_batch(self, xhh, n_het: int = 1, policy: bool = False, check: bool = True):
        """the household block at K input paths at once (hank_primal_batch): xhh (n_hh, P, K) — or (n_hh, P) for one path —
        -> (aggs (P, n_het, K), status (K,) int32[, policies (n_a, n_e, P, K) with policy=True]). Scenario k is `primal` at
        xhh[:, :, k] on the per-period launches, bit for bit in output 0 and in the policies; n_het up to the count declared
        with `set_het_outputs`. The context's recorded primal, its batches and its memo stay as they were. status[k] is scenario
        k's status code; the healthy scenarios' outputs are valid whatever the others did. check=True raises the first failing
        scenario's exception (the arrays of the call are then at `last_batch`)."""
        x, K = _batch(xhh, (self.n_hh, self.P), strict=True)
        aggs = _out(self.P, _n1(n_het), _n1(K))
        status = np.zeros(_n1(K), dtype=np.int32)
        pol = _out(self.n_a, self.n_e, self.P, _n1(K)) if policy else None
        rc = self._lib.hank_primal_batch(self._ctx, int(n_het), _p(x), K, _p(aggs), _opt(pol), _ip(status))
        self.last_batch = (aggs, status, pol)
        if rc != HANK_OK and (check or not (1 <= K <= 64) or not np.any(status)):      # (a refusal of the call itself always raises)
            self._chk(rc)
        return (aggs, status, pol) if policy else (aggs, status)

    def primal_batch_dev(self, n_het: int, d_xhh_ptr: int, K: int, d_agg_ptr: int, d_policy_ptr: int = 0):
        """device-pointer form (asynchronous on the context's stream; the verdict arrives at `check`)."""
        self._call("hank_primal_batch_dev", int(n_het), _dev(d_xhh_ptr), int(K), _dev(d_agg_ptr), _dev(d_policy_ptr))

    def last_batch_timings(self):
        """time (ms, HIP events on the stream) of the last batch's backward and forward chains (hank_last_batch_timings)"""
        return self._ms_pair("hank_last_batch_timings")

    # -- the steady state's household side at K price vectors ---------------------------------
    def _per_scenario(self, arr, K, fill):
        """a start of `ss_batch`: None (`fill` everywhere), (n_a, n_e) or (G,) shared, (n_a, n_e, K) or (G, K) -> (G, K) column-major"""
        if arr is None:
            return np.full((self.G, K), fill, order="F")
        s = np.asarray(arr, dtype=np.float64)
        if s.shape in ((self.n_a, self.n_e), (self.G,)):
            return np.asfortranarray(np.repeat(s.reshape((self.G, 1), order="F"), K, axis=1))
        return _f(np.array(_grid_batch(s, self.n_a, self.n_e), copy=True), (self.G, K))

    def ss_batch(self, xhh, vfi_tol: float, n_het: int = 1, value0=None, D0=None, vfi_max_iter: int = 10_000, dist_tol: float = 1e-15,
                 dist_max_iter: int = 500_000, check_every: int = 25, dist: bool = True, check: bool = True):
        """the steady state's household side at K constant price vectors at once (hank_ss_batch): xhh (n_hh, K) — or (n_hh,) for
        one scenario — -> (aggs (n_het, K), value (n_a, n_e, K), policy (n_a, n_e, K), D (G, K) with every column summing to one,
        iters (K, 2) = value steps and distribution iterations, status (K,) int32). Scenario k is `vfi` at xhh[:, k] on the per-step
        launches followed by `stationary_dist` on its policy, bit for bit. value0: None (ones), (n_a, n_e) shared or (n_a, n_e, K);
        D0 likewise (normalised to sum to one; None = uniform). dist=False: value iteration only (aggs and D are None). The
        context's record, batches and memo stay as they were. check=True raises the first failing scenario's exception; the raw
        arrays of the call (D as the library left it, the sup-norms) are at `last_ss_batch` either way."""
        x, K = _batch(xhh, (self.n_hh,), strict=True)
        Kb = _n1(K)
        v = self._per_scenario(value0, Kb, 1.0)
        pol = _out(self.G, Kb)
        d = aggs = None
        if dist:
            d = self._per_scenario(D0, Kb, 1.0 / self.G)
            if D0 is not None:
                d /= d.sum(axis=0, keepdims=True)
            aggs = _out(_n1(n_het), Kb)
        iters = np.zeros((Kb, 2), dtype=np.int32)
        nrm = np.zeros(Kb)
        status = np.zeros(Kb, dtype=np.int32)
        rc = self._lib.hank_ss_batch(self._ctx, int(n_het), _p(x), K, float(vfi_tol), int(vfi_max_iter), float(dist_tol), int(dist_max_iter),
                                     int(check_every), _p(v), _p(pol), _opt(d), _opt(aggs), _ip(iters), _p(nrm), _ip(status))
        self.last_ss_batch = {"aggs": aggs, "value": v, "policy": pol, "D": d, "iters": iters, "supnorm": nrm, "status": status}
        if rc != HANK_OK and (check or not np.any(status)):      # (a refusal of the call itself always raises)
            self._chk(rc)
        Dn = None
        if dist:
            with np.errstate(invalid="ignore", divide="ignore"):
                Dn = d / d.sum(axis=0, keepdims=True)
        shape = (self.n_a, self.n_e, Kb)
        return aggs, v.reshape(shape, order="F"), pol.reshape(shape, order="F"), Dn, iters, status

    def last_ss_batch_timings(self):
        """time (ms, HIP events on the stream) of the last `ss_batch`'s value loops and distribution loops (hank_last_ss_batch_timings)"""
        return self._ms_pair("hank_last_ss_batch_timings")

    # -- the transposed block ---------------------------------------------------------------
    def _cotangents(self, agg_bar, n_het, het):
        """the cotangents of `vjp` (het False: (P,), (P, M) for n_het = 1, or (P, n_het, M)) or of `vjp_het` (het True:
        (P, n_het, M) only) -> (M, yb (P, n_het, M) column-major)"""
        yb = np.asarray(agg_bar, dtype=np.float64)
        if het and yb.ndim != 3:
            raise ValueError("agg_bar must be (P, n_het, M)")
        yb = _cols(yb, 1)
        if yb.ndim == 2:
            if int(n_het) != 1:
                raise ValueError("agg_bar must be (P, n_het, M) when n_het > 1")
            yb = yb[:, None, :]
        M = yb.shape[2]
        served = 1 <= int(n_het) <= (4 if het else 2)
        return M, _f(yb, (self.P, int(n_het), M) if served else None)      # (the library refuses any other n_het)

    def vjp(self, agg_bar, n_het: int = 1) -> np.ndarray:
        """J(x)' agg_bar at the recorded primal (hank_vjp; the reverse rules of ForwardIteration.jl:339-420 and of the
        backward loop). agg_bar: (P,) or (P, M) for n_het = 1, (P, n_het, M) in general — cotangents of the aggregates of
        the policy variable and (n_het = 2) of consumption. -> xhh_bar (n_hh, P, M)."""
        M, yb = self._cotangents(agg_bar, n_het, het=False)
        out = self._cot_outputs(M)[0]
        self._call("hank_vjp", int(n_het), _p(yb), M, _p(out))
        return out

    def vjp_dev(self, n_het: int, d_agg_bar_ptr: int, M: int, d_xhh_bar_ptr: int):
        """device-pointer form (asynchronous on the context's stream)."""
        self._call("hank_vjp_dev", int(n_het), _dev(d_agg_bar_ptr), int(M), _dev(d_xhh_bar_ptr))

    def vjp_het(self, agg_bar, n_het: int) -> np.ndarray:
        """`vjp` with cotangents on every heterogeneous output (hank_vjp_het): agg_bar (P, n_het, M), n_het up to the count
        declared with `set_het_outputs` — outputs 2, 3 are Value and UCE, which are not affine in the policy.
        -> xhh_bar (n_hh, P, M). n_het <= 2 runs `vjp`'s path: the same bits."""
        M, yb = self._cotangents(agg_bar, n_het, het=True)
        out = self._cot_outputs(M)[0]
        self._call("hank_vjp_het", int(n_het), _p(yb), M, _p(out))
        return out

    def vjp_het_dev(self, n_het: int, d_agg_bar_ptr: int, M: int, d_xhh_bar_ptr: int):
        """device-pointer form (asynchronous on the context's stream)."""
        self._call("hank_vjp_het_dev", int(n_het), _dev(d_agg_bar_ptr), int(M), _dev(d_xhh_bar_ptr))

    # -- tangents and cotangents on the boundary ---------------------------------------------
    def _boundary_seed(self, seed, N):
        """a boundary seed (n_a, n_e), (n_a, n_e, N) or (G, N) -> (G, N) column-major, pt = e n_a + a; None stays None"""
        return None if seed is None else _f(_grid_batch(seed, self.n_a, self.n_e), (self.G, N))

    def _directions(self, dxhh, dvalue_end, dD_init):
        """the inputs of `jvp_boundary` / `jvp_het` -> (N, dx (n_hh, P, N), dv (G, N), dd (G, N)), column-major; None stays None"""
        first = next((np.asarray(v) for v in (dxhh, dvalue_end, dD_init) if v is not None), None)
        N = None if first is None else first.shape[-1] if first.ndim == 3 else 1      # (so a lone (G, N) seed with N > 1 is refused, as it always was)
        N, (dx, dv, dd) = _seeds((("dxhh", dxhh, (self.n_hh, self.P)), ("dvalue_end", dvalue_end, self._boundary_seed),
                                  ("dD_init", dD_init, self._boundary_seed)), N)
        return N, dx, dv, dd

    def jvp_boundary(self, dxhh=None, dvalue_end=None, dD_init=None) -> np.ndarray:
        """the tangent sweeps with seeds on the boundary as well (hank_jvp_boundary): dxhh (n_hh, P, N) as in `jvp`, dvalue_end
        and dD_init (n_a, n_e, N) — tangents of `ss_end.value` (BackwardIteration.jl:85) and `ss_initial.D`
        (ForwardIteration.jl:293); None means zeros, at least one must be given. -> dagg (P, N). Always the launch family. The
        batch is current afterwards: `dpolicy_seq`, `grid_aggregates`, `het_outputs(2, dxhh)` serve it (pass zeros for a dxhh of
        None)."""
        N, dx, dv, dd = self._directions(dxhh, dvalue_end, dD_init)
        out = _out(self.P, N)
        self.calls["jvp"] += 1
        self._call("hank_jvp_boundary", _opt(dx), _opt(dv), _opt(dd), N, _p(out))
        return out

    def jvp_boundary_dev(self, d_dxhh_ptr: int, d_dvalue_end_ptr: int, d_dD_init_ptr: int, N: int, d_dagg_ptr: int = 0):
        """device-pointer form (asynchronous on the context's stream); a pointer of 0 is a zero seed."""
        self._call("hank_jvp_boundary_dev", _dev(d_dxhh_ptr), _dev(d_dvalue_end_ptr), _dev(d_dD_init_ptr), int(N), _dev(d_dagg_ptr))

    def vjp_boundary(self, agg_bar, n_het: int = 1):
        """`vjp` with the boundary's cotangents (hank_vjp_boundary): -> (xhh_bar (n_hh, P, M), value_end_bar (n_a, n_e, M),
        D_init_bar (n_a, n_e, M)) — the cotangents of the household inputs, of `ss_end.value` and of `ss_initial.D`; the exact
        transpose of `jvp_boundary` followed by `het_outputs(n_het)`. agg_bar as in `vjp`; xhh_bar equals `vjp`'s bit for bit."""
        M, yb = self._cotangents(agg_bar, n_het, het=False)
        out, vb, db = self._cot_outputs(M, True, True)
        self._call("hank_vjp_boundary", int(n_het), _p(yb), M, _p(out), _p(vb), _p(db))
        return out, vb, db

    def vjp_boundary_dev(self, n_het: int, d_agg_bar_ptr: int, M: int, d_xhh_bar_ptr: int, d_value_end_bar_ptr: int = 0, d_D_init_bar_ptr: int = 0):
        """device-pointer form (asynchronous on the context's stream); a boundary pointer of 0 is not wanted."""
        self._call("hank_vjp_boundary_dev", int(n_het), _dev(d_agg_bar_ptr), int(M), _dev(d_xhh_bar_ptr), _dev(d_value_end_bar_ptr), _dev(d_D_init_bar_ptr))

    # -- every output's tangent in one pair of sweeps; its transpose on the boundary ----------
    def jvp_het(self, dxhh=None, dvalue_end=None, dD_init=None, n_het: int = 2) -> np.ndarray:
        """every declared output's tangent from one pair of sweeps (hank_jvp_het): inputs as in `jvp_boundary` (None means zeros,
        at least one must be given), n_het up to the count declared with `set_het_outputs`. -> dagg (P, n_het, N), the shape of
        `het_outputs`' dagg. Value and UCE ride in the forward sweep, so boundary seeds reach them too. Always the launch
        family; n_het <= 2 gives the bits of `jvp` / `jvp_boundary` under the launch schedule."""
        N, dx, dv, dd = self._directions(dxhh, dvalue_end, dD_init)
        out = _out(self.P, _n1(n_het), N)
        self.calls["jvp"] += 1
        self._call("hank_jvp_het", int(n_het), _opt(dx), _opt(dv), _opt(dd), N, _p(out))
        return out

    def jvp_het_dev(self, n_het: int, d_dxhh_ptr: int, d_dvalue_end_ptr: int, d_dD_init_ptr: int, N: int, d_dagg_ptr: int = 0):
        """device-pointer form (asynchronous on the context's stream); a pointer of 0 is a zero seed."""
        self._call("hank_jvp_het_dev", int(n_het), _dev(d_dxhh_ptr), _dev(d_dvalue_end_ptr), _dev(d_dD_init_ptr), int(N), _dev(d_dagg_ptr))

    def vjp_het_boundary(self, agg_bar, n_het: int, value_end: bool = True, D_init: bool = True):
        """`vjp_het` with the boundary's cotangents (hank_vjp_het_boundary): agg_bar (P, n_het, M) -> (xhh_bar (n_hh, P, M),
        value_end_bar (n_a, n_e, M), D_init_bar (n_a, n_e, M)); the exact transpose of `jvp_het`. A boundary cotangent that is
        not wanted (value_end / D_init False) is not computed and comes back as None. xhh_bar equals `vjp_het`'s bit for bit."""
        M, yb = self._cotangents(agg_bar, n_het, het=True)
        out, vb, db = self._cot_outputs(M, value_end, D_init)
        self._call("hank_vjp_het_boundary", int(n_het), _p(yb), M, _p(out), _opt(vb), _opt(db))
        return out, vb, db

    def vjp_het_boundary_dev(self, n_het: int, d_agg_bar_ptr: int, M: int, d_xhh_bar_ptr: int, d_value_end_bar_ptr: int = 0, d_D_init_bar_ptr: int = 0):
        """device-pointer form (asynchronous on the context's stream); a boundary pointer of 0 is not wanted."""
        self._call("hank_vjp_het_boundary_dev", int(n_het), _dev(d_agg_bar_ptr), int(M), _dev(d_xhh_bar_ptr), _dev(d_value_end_bar_ptr), _dev(d_D_init_bar_ptr))

    # -- derivatives through the steady state -------------------------------------------------
    def _ss_done(self, who, names, it, res, tol, max_iter, check):
        self.last_ss = {"iters": (int(it[0]), int(it[1])), "resid": (float(res[0]), float(res[1]))}
        if check:
            for k in range(2):
                if it[k] >= max_iter and not res[k] <= tol:
                    raise SteadyStateLoopError(f"{who}: the {names[k]} loop took max_iter = {max_iter} steps and its last increment ratio "
                                               f"{res[k]:.3g} is above tol = {tol:.3g}")

    def _ss_loops(self, who, names, tol, max_iter, check, symbol, *args):
        """a steady-state entry, whose last two arguments are its loops' (iters, resid) pair: `last_ss`, the verdict of `_ss_done` -> iters"""
        it, res = (C.c_int32 * 2)(), (C.c_double * 2)()
        self._call(symbol, *args, it, res)
        self._ss_done(who, names, it, res, tol, max_iter, check)
        return (int(it[0]), int(it[1]))

    def ss_jvp(self, dxhh, n_het: int = 2, tol: float = 1e-13, max_iter: int = 50_000, check: bool = True):
        """derivatives of the steady state's household objects in the household prices (hank_ss_jvp; what
        ForwardDiff.jacobian carries through the VFI and invariant_dist at SteadyState.jl:195). Needs `primal` at the constant
        steady-state path with the steady state as both boundaries (the precondition of `fake_news`). dxhh (n_hh,) or (n_hh, N).
        -> (dagg (n_het, N), dV (n_a, n_e, N), dpol (n_a, n_e, N), dD (n_a, n_e, N), iters (value loop, distribution loop)).
        Raises SteadyStateLoopError when a loop ran into max_iter (check=False: returns what it has; `last_ss` holds the
        increment ratios)."""
        dx, N = _batch(dxhh, (self.n_hh,))
        dagg = _out(_n1(n_het), N)
        dV, dpol, dD = (_out(self.n_a, self.n_e, N) for _ in range(3))
        iters = self._ss_loops("ss_jvp", ("value", "distribution"), tol, max_iter, check,
                               "hank_ss_jvp", int(n_het), _p(dx), N, float(tol), int(max_iter), _p(dV), _p(dpol), _p(dD), _p(dagg))
        return dagg, dV, dpol, dD, iters

    def ss_vjp(self, agg_bar=None, value_bar=None, D_bar=None, n_het: int = 2, tol: float = 1e-13, max_iter: int = 50_000, check: bool = True):
        """the transpose of `ss_jvp` (hank_ss_vjp): cotangents agg_bar (n_het,) or (n_het, M) of the steady state's aggregates,
        value_bar and D_bar (n_a, n_e[, M]) or (G, M) of V_ss and D_ss — e.g. `vjp_het_boundary`'s value_end_bar — any of them
        None (not given), at least one given. -> (xhh_bar (n_hh, M), iters (nu loop, lambda loop))."""
        M = None
        if agg_bar is not None:
            M = _cols(agg_bar, 1).shape[1]
        elif value_bar is not None or D_bar is not None:
            b = np.asarray(value_bar if value_bar is not None else D_bar)
            M = 1 if b.shape == (self.n_a, self.n_e) else b.shape[-1]
        served = 1 <= int(n_het) <= 4      # (the library refuses any other n_het)
        M, (yb, vb, db) = _seeds((("agg_bar", agg_bar, lambda y, M: _f(_cols(y, 1), (int(n_het), M) if served else None)),
                                  ("value_bar", value_bar, self._boundary_seed), ("D_bar", D_bar, self._boundary_seed)), M)
        out = _out(self.n_hh, M)
        iters = self._ss_loops("ss_vjp", ("nu", "lambda"), tol, max_iter, check,
                               "hank_ss_vjp", int(n_het), _opt(yb), _opt(vb), _opt(db), M, float(tol), int(max_iter), _p(out))
        return out, iters

    def ss_jvp_dev(self, d_dxhh_ptr: int, N: int, d_dagg_ptr: int, d_dvalue_ptr: int = 0, d_dpolicy_ptr: int = 0, d_dD_ptr: int = 0,
                   n_het: int = 2, tol: float = 1e-13, max_iter: int = 50_000, check: bool = True):
        """device-pointer form of `ss_jvp` (hank_ss_jvp_dev): d_dxhh (n_hh, N) in; d_dagg (n_het, N) and the exports (G, N) out,
        all column-major, written straight to the caller's buffers; an export pointer of 0 is not wanted. The loops read their
        stop word on the host, so the call returns with the stream drained. -> iters; `last_ss` as after `ss_jvp`."""
        return self._ss_loops("ss_jvp_dev", ("value", "distribution"), tol, max_iter, check,
                              "hank_ss_jvp_dev", int(n_het), _dev(d_dxhh_ptr), int(N), float(tol), int(max_iter), _dev(d_dvalue_ptr), _dev(d_dpolicy_ptr),
                              _dev(d_dD_ptr), _dev(d_dagg_ptr))

    def ss_vjp_dev(self, d_agg_bar_ptr: int, d_value_bar_ptr: int, d_D_bar_ptr: int, M: int, d_xhh_bar_ptr: int,
                   n_het: int = 2, tol: float = 1e-13, max_iter: int = 50_000, check: bool = True):
        """device-pointer form of `ss_vjp` (hank_ss_vjp_dev): d_agg_bar (n_het, M), d_value_bar and d_D_bar (G, M) in, a pointer
        of 0 is a cotangent not given (at least one must be); d_xhh_bar (n_hh, M) out. -> iters; `last_ss` as after `ss_vjp`."""
        return self._ss_loops("ss_vjp_dev", ("nu", "lambda"), tol, max_iter, check,
                              "hank_ss_vjp_dev", int(n_het), _dev(d_agg_bar_ptr), _dev(d_value_bar_ptr), _dev(d_D_bar_ptr), int(M), float(tol), int(max_iter),
                              _dev(d_xhh_bar_ptr))

    def policy_cotangent_seq(self, M: int) -> np.ndarray:
        """(n_a, n_e, P, M): cotangent of the policy sequence of the last vjp / vjp_het (hank_get_policy_cotangent_seq)."""
        out = _out(self.n_a, self.n_e, self.P, _n1(M))
        self._call("hank_get_policy_cotangent_seq", int(M), _p(out))
        return out

    # -- timings and counters -----------------------------------------------------------------
    def last_vjp_timings(self):
        return self._ms_launches("hank_last_vjp_timings", ("sweep_a", "sweep_b"))

    def last_ss_timings(self):
        """time (ms, HIP events on the stream) of the two loops of the last ss_jvp / ss_vjp, in the order of their `iters` (hank_last_ss_timings)"""
        return self._ms_pair("hank_last_ss_timings")

    def last_timings(self):
        return self._ms_launches("hank_last_timings", ("primal_backward", "primal_forward", "tangent_backward", "tangent_forward", "dual_backward", "dual_forward"))

    def stats(self):
        """counters of the context (include/hank_hip.h: hank_stats)."""
        return self._counters("hank_stats", ("sweep_launches", "tangent_workspaces_allocated", "graphs_captured", "schedule", "fallbacks", "vfi_iterations",
                                             "primal_memo_hits", "primal_sweeps"))

    def info(self):
        """which kernel family served the last tangent sweep and how the context chooses (include/hank_hip.h: hank_info)."""
        d = self._counters("hank_info", ("last_tangent_family", "wide_mode", "wide_min", "wide_supported", "xjvp_max", "record_diet", "record_bytes", "lwg_builds"))
        d["last_tangent_family_name"] = ("launch-per-period", "xcd-persistent", "on-chip-wide")[d["last_tangent_family"]]
        return d

    def sweep_instance(self):
        """which instances of the Dual pass's persistent sweeps were enqueued last (include/hank_hip.h: hank_sweep_instance):
        {"back": (NE, CRRA), "fwd": (NE, CRRA)}; -1 before the first Dual pass."""
        out, = self._read("hank_sweep_instance", (C.c_int32 * 4)())
        return {"back": (int(out[0]), int(out[1])), "fwd": (int(out[2]), int(out[3]))}

    # -- what the last sweeps left ------------------------------------------------------------
    def policy_seq(self) -> np.ndarray:
        """(n_a, n_e, P): policy matrix of every period (BackwardIteration's return value)."""
        out = _out(self.n_a, self.n_e, self.P)
        self._call("hank_get_policy_seq", _p(out))
        return out

    def lottery_record(self):
        """the Young lottery of the last primal as the record holds it (hank_get_lottery_record): lo, lw, ig of shape (n_a, n_e, P),
        the packed records lq (structured: w, lo, flags) of the same shape and the grid's inverse gaps iga (n_a,)."""
        shp = (self.n_a, self.n_e, self.P)
        lo, lw, ig = np.empty(shp, np.int32, order="F"), _out(*shp), _out(*shp)
        lq = np.empty(shp, np.dtype([("w", "<f8"), ("lo", "<i4"), ("flags", "<i4")]), order="F")
        iga = np.empty(self.n_a)
        self._call("hank_get_lottery_record", lo.ctypes.data_as(C.c_void_p), _p(lw), _p(ig), lq.ctypes.data_as(C.c_void_p), _p(iga))
        return {"lo": lo, "lw": lw, "ig": ig, "lq": lq, "iga": iga}

    def forward_units(self):
        """the persistent forward sweeps' work units of the recorded lottery (hank_get_forward_units): src (P, S) and units
        (P, S, 64, 2) as the library lays them out, S = ceil(n_a / 63) members; src >> 18 is a member's unit count."""
        S = (self.n_a + 62) // 63
        src, units = np.empty((self.P, S), np.int32), np.empty((self.P, S, 64, 2), np.int32)
        self._call("hank_get_forward_units", src.ctypes.data_as(C.c_void_p), units.ctypes.data_as(C.c_void_p))
        return src, units

    def dist_seq(self) -> np.ndarray:
        out = _out(self.n_a, self.n_e, self.P)
        self._call("hank_get_dist_seq", _p(out))
        return out

    def dpolicy_seq(self, N: int) -> np.ndarray:
        """(n_a, n_e, P, N): partials of the policy sequence of the last jvp."""
        out = _out(self.n_a, self.n_e, self.P, N)
        self._call("hank_get_dpolicy_seq", int(N), _p(out))
        return out

    def het_outputs(self, n_het: int = 2, dxhh=None, dy=None):
        """every heterogeneous variable's aggregate of the last sweeps (hank_get_het_outputs; ForwardIteration.jl:303-307):
        output 0 the policy variable (KD / A), output 1 consumption, output 2 Value, output 3 UCE (one-asset HANK), up to the
        count declared with `set_het_outputs`. -> agg (P, n_het), and dagg (P, n_het, N) when `dxhh`
        (n_hh, P, N) — the input of the last tangent sweep — is given (else None). dy (n_e, P, N): income directions
        (hank_get_het_outputs_income, n_het <= 2) for consumption's direct term, in place of the ones a batch of `jvp_income`
        carries and adds by itself; dxhh may then be None (zeros)."""
        agg = _out(self.P, n_het)
        if dy is not None:
            N, dx, d = self._path_dirs("income", dxhh, dy)
            if dx is None:
                dx = np.zeros((self.n_hh, self.P, N), order="F")
            dagg = _out(self.P, n_het, N)
            self._call("hank_get_het_outputs_income", int(n_het), _p(dx), _p(d), N, _p(agg), _p(dagg))
            return agg, dagg
        if dxhh is None:
            self._call("hank_get_het_outputs", int(n_het), None, 0, _p(agg), None)
            return agg, None
        dxhh, N = self._sweep_input(dxhh)
        dagg = _out(self.P, n_het, N)
        self._call("hank_get_het_outputs", int(n_het), _p(dxhh), N, _p(agg), _p(dagg))
        return agg, dagg

    def set_het_outputs(self, n_het: int):
        """declare how many heterogeneous outputs het_outputs will be asked for (hank_set_het_outputs; default 2)."""
        self._call("hank_set_het_outputs", int(n_het))
        self._n_het_declared = int(n_het)

    def het_outputs_dev(self, n_het: int, d_dxhh: int, N: int, d_agg: int, d_dagg: int, d_dy: int = 0):
        """device-pointer form (asynchronous on the context's stream); d_dy: the income directions (hank_get_het_outputs_income_dev)."""
        if d_dy:
            self._call("hank_get_het_outputs_income_dev", int(n_het), _dev(d_dxhh), _dev(d_dy), int(N), _dev(d_agg), _dev(d_dagg))
            return
        self._call("hank_get_het_outputs_dev", int(n_het), _dev(d_dxhh), int(N), _dev(d_agg), _dev(d_dagg))

    def grid_aggregates(self, N: int = 0):
        """the grid-weighted aggregate sum_pt a(pt) D_t(pt) of the last primal sweep, and (N > 0) its partials (P, N) of the
        last tangent sweep (hank_get_grid_aggregates)."""
        agg2 = np.empty(self.P)
        dagg2 = _out(self.P, N) if N > 0 else None
        self._call("hank_get_grid_aggregates", _p(agg2), int(N), _opt(dagg2))
        return agg2, dagg2

    def fake_news(self):
        """the household block's Jacobian at the steady state from its Toeplitz structure (hank_fake_news):
        -> F (P, P, n_hh), Dv (P, n_hh); `SteadyStateJacobian.household_jacobian` turns them into d agg_t / d xhh_{k,s}."""
        F = _out(self.P, self.P, self.n_hh)
        Dv = _out(self.P, self.n_hh)
        self._call("hank_fake_news", _p(F), _p(Dv))
        return F, Dv

    def fake_news_het(self, n_het: int):
        """the same Toeplitz form for heterogeneous outputs 0 .. n_het-1 of `het_outputs` (hank_fake_news_het):
        -> F (P, P, n_hh, n_het), Dv (P, n_hh, n_het); output 0 equals `fake_news()` bit for bit, and
        `household_jacobian(F[..., o], Dv[..., o])` is d agg^o_t / d xhh_{k,s}."""
        nb = _n1(n_het)                  # (the library refuses an n_het outside 1..3 / 1..4)
        F = _out(self.P, self.P, self.n_hh, nb)
        Dv = _out(self.P, self.n_hh, nb)
        self._call("hank_fake_news_het", int(n_het), _p(F), _p(Dv))
        return F, Dv

    # -- group outputs: aggregates by household group -------------------------------------------
    def set_group_outputs(self, W, base):
        """the groups `group_outputs` and `fake_news_group` serve (hank_set_group_outputs): W (G, K) — or (n_a, n_e, K) — holds
        one weight vector per group, indexed like D (pt = e n_a + ia), any real values; base[k] is GROUP_MASS, GROUP_POLICY or
        GROUP_CONS (one value serves every group). K = 0 (W=None) clears them. The record, the current tangent batch, the primal memo
        and the `set_het_outputs` count stay as they are. `clone()` does not carry the groups."""
        if W is None:
            self._call("hank_set_group_outputs", 0, None, None)
            self.n_groups = 0
            return
        W = np.asarray(W, dtype=np.float64)
        if W.ndim == 3:      # (a lone (n_a, n_e) matrix is not one group here, as it never was)
            W = _grid_batch(W, self.n_a, self.n_e)
        W = _cols(W, 1)
        if W.ndim != 2 or W.shape[0] != self.G:
            raise ValueError(f"W must be ({self.G}, K) or ({self.n_a}, {self.n_e}, K), got {W.shape}")
        W = np.asfortranarray(W)
        K = W.shape[1]
        b = np.ascontiguousarray(np.broadcast_to(np.asarray(base, dtype=np.int32), (K,)))
        self._call("hank_set_group_outputs", K, _p(W), _ip(b))
        self.n_groups = K

    def group_outputs(self, dxhh=None):
        """the group outputs of the last sweeps (hank_get_group_outputs; ForwardIteration.jl:303-307): Y^k_t = sum W_k f D_t.
        -> agg (P, K), and dagg (P, K, N) when `dxhh` (n_hh, P, N) — the input of the last tangent sweep — is given (else
        None). The rules of `het_outputs`; a batch with boundary seeds is refused."""
        K = _n1(self.n_groups)      # (the library refuses a call without groups)
        agg = _out(self.P, K)
        if dxhh is None:
            self._call("hank_get_group_outputs", None, 0, _p(agg), None)
            return agg, None
        dxhh, N = self._sweep_input(dxhh)
        dagg = _out(self.P, K, N)
        self._call("hank_get_group_outputs", _p(dxhh), N, _p(agg), _p(dagg))
        return agg, dagg

    def group_outputs_dev(self, d_dxhh: int, N: int, d_agg: int, d_dagg: int):
        """device-pointer form (asynchronous on the context's stream)."""
        self._call("hank_get_group_outputs_dev", _dev(d_dxhh), int(N), _dev(d_agg), _dev(d_dagg))

    def vjp_group(self, grp_bar, agg_bar=None, n_het: int = 0, value_end: bool = False, D_init: bool = False):
        """the transpose of `group_outputs`' tangent map (hank_vjp_group; the reverse rules of ForwardIteration.jl:339-420 with the
        weighted dot of :303-307): grp_bar (P, K, M) — or (P, K) for M = 1 — holds cotangents on the K group outputs, the shape of
        `group_outputs`' dagg. agg_bar (P, n_het, M), n_het 1 or 2, adds cotangents on outputs 0 and 1 (`vjp`'s) in the same product;
        without it n_het is 0. -> xhh_bar (n_hh, P, M); with value_end or D_init the triple (xhh_bar, value_end_bar, D_init_bar) of
        `vjp_het_boundary`, an unwanted one None. `policy_cotangent_seq(M)` serves its policy cotangent afterwards."""
        gb, M = None, None
        if grp_bar is not None:
            gb = _cols(grp_bar, 2)
            if gb.ndim != 3:
                raise ValueError("grp_bar must be (P, K) or (P, K, M)")
            M = gb.shape[2]
            gb = _f(gb, (self.P, self.n_groups, M) if self.n_groups > 0 else None)      # (the library refuses a call without groups)
        yb = None
        if agg_bar is not None:
            Ma, yb = self._cotangents(agg_bar, n_het, het=False)
            if M is not None and Ma != M:
                raise ValueError(f"agg_bar has {Ma} columns, grp_bar {M}")
            M = Ma
        M = 1 if M is None else M
        out, vb, db = self._cot_outputs(M, value_end, D_init)
        self._call("hank_vjp_group", int(n_het), _opt(yb), _opt(gb), M, _p(out), _opt(vb), _opt(db))
        return (out, vb, db) if (value_end or D_init) else out

    def vjp_group_dev(self, n_het: int, d_agg_bar_ptr: int, d_grp_bar_ptr: int, M: int, d_xhh_bar_ptr: int, d_value_end_bar_ptr: int = 0,
                      d_D_init_bar_ptr: int = 0):
        """device-pointer form (asynchronous on the context's stream); an agg_bar pointer of 0 goes with n_het = 0, a boundary pointer
        of 0 is not wanted."""
        self._call("hank_vjp_group_dev", int(n_het), _dev(d_agg_bar_ptr), _dev(d_grp_bar_ptr), int(M), _dev(d_xhh_bar_ptr), _dev(d_value_end_bar_ptr),
                   _dev(d_D_init_bar_ptr))

    def fake_news_group(self):
        """the Toeplitz form of `fake_news_het` for the group outputs (hank_fake_news_group): -> F (P, P, n_hh, K),
        Dv (P, n_hh, K); `household_jacobian(F[..., k], Dv[..., k])` is d Y^k_t / d xhh_{i,s}."""
        K = _n1(self.n_groups)
        F = _out(self.P, self.P, self.n_hh, K)
        Dv = _out(self.P, self.n_hh, K)
        self._call("hank_fake_news_group", _p(F), _p(Dv))
        return F, Dv

    def vfi(self, value0, xhh_t, tol: float, max_iter: int = 10_000):
        """device-resident inner fixed point of the steady state (hank_vfi; SteadyState.jl:132-141):
        -> (value, policy, steps, last sup-norm)."""
        v = _f(np.array(value0, dtype=np.float64, copy=True), (self.n_a, self.n_e))
        x = _f(xhh_t, (self.n_hh,))
        pol = _out(self.n_a, self.n_e)
        it, nrm = C.c_int32(), C.c_double()
        self._call("hank_vfi", _p(x), float(tol), int(max_iter), _p(v), _p(pol), C.byref(it), C.byref(nrm))
        return v, pol, it.value, nrm.value

    def stationary_dist(self, policy, D0=None, tol: float = 1e-15, max_iter: int = 500_000, check_every: int = 25):
        """stationary distribution of the steady state by the power method on the device (hank_stationary_dist):
        -> (D as a length-G vector summing to one, steps)."""
        p = _f(policy, (self.n_a, self.n_e))
        d = np.full(self.G, 1.0 / self.G) if D0 is None else np.asarray(D0, dtype=np.float64).reshape(-1, order="F") / np.sum(D0)
        d = _f(d.reshape((self.n_a, self.n_e), order="F"))
        it = C.c_int32()
        self._call("hank_stationary_dist", _p(p), _p(d), float(tol), int(max_iter), int(check_every), C.byref(it))
        out = d.reshape(-1, order="F")
        return out / out.sum(), it.value

    # -- granular steps ---------------------------------------------------------------------
    def backward_step(self, value_next, xhh_t):
        v = _f(value_next, (self.n_a, self.n_e))
        x = _f(xhh_t, (self.n_hh,))
        vo, po = _out(self.n_a, self.n_e), _out(self.n_a, self.n_e)
        self._call("hank_backward_step", _p(v), _p(x), _p(vo), _p(po))
        return vo, po

    def backward_step_dual(self, value_next, dvalue_next, xhh_t, dxhh_t):
        dv = np.asarray(dvalue_next, dtype=np.float64)
        N = dv.shape[-1]
        v = _f(value_next, (self.n_a, self.n_e))
        dv = _f(dv, (self.n_a, self.n_e, N))
        x = _f(xhh_t, (self.n_hh,))
        dx = _f(dxhh_t, (self.n_hh, N))
        vo, po = _out(self.n_a, self.n_e), _out(self.n_a, self.n_e)
        dvo, dpo = _out(self.n_a, self.n_e, N), _out(self.n_a, self.n_e, N)
        self._call("hank_backward_step_dual", _p(v), _p(dv), _p(x), _p(dx), N, _p(vo), _p(dvo), _p(po), _p(dpo))
        return vo, dvo, po, dpo

    def forward_step(self, policy, D_prev):
        p = _f(policy, (self.n_a, self.n_e))
        d = _f(np.asarray(D_prev, dtype=np.float64).reshape((self.n_a, self.n_e), order="F"))
        do = _out(self.n_a, self.n_e)
        agg = C.c_double()
        self._call("hank_forward_step", _p(p), _p(d), _p(do), C.byref(agg))
        return do, agg.value

    def forward_step_dual(self, policy, dpolicy, D_prev, dD_prev):
        dp_ = np.asarray(dpolicy, dtype=np.float64)
        N = dp_.shape[-1]
        p = _f(policy, (self.n_a, self.n_e))
        dp_ = _f(dp_, (self.n_a, self.n_e, N))
        d = _f(np.asarray(D_prev, dtype=np.float64).reshape((self.n_a, self.n_e), order="F"))
        dd = _f(np.asarray(dD_prev, dtype=np.float64).reshape((self.n_a, self.n_e, N), order="F"))
        do, ddo = _out(self.n_a, self.n_e), _out(self.n_a, self.n_e, N)
        agg = C.c_double()
        dagg = np.empty(N)
        self._call("hank_forward_step_dual", _p(p), _p(dp_), _p(d), _p(dd), N, _p(do), _p(ddo), C.byref(agg), _p(dagg))
        return do, ddo, agg.value, dagg
