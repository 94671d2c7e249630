"""ctypes binding of the C ABI in include/hank_hip.h (libhank_hip.so, hand-written HIP for gfx950).

There is no CPU fallback on this path: if the shared library is missing or no MI355X is usable the
constructors raise — the product never silently computes the household block anywhere else.
"""
from __future__ import annotations

import ctypes as C
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

# the symbols include/hank_hip.h declares (tests check that every one is exported)
ABI_SYMBOLS = (
    "hank_create", "hank_create_on", "hank_gather_columns", "hank_destroy", "hank_last_error", "hank_n_hh", "hank_set_stream", "hank_sync",
    "hank_set_boundary", "hank_primal", "hank_jvp", "hank_primal_dev", "hank_jvp_dev", "hank_check",
    "hank_primal_jvp", "hank_primal_jvp_dev",
    "hank_get_policy_seq", "hank_get_dpolicy_seq", "hank_get_dist_seq", "hank_get_het_outputs", "hank_get_het_outputs_dev", "hank_set_het_outputs",
    "hank_get_grid_aggregates", "hank_get_grid_aggregates_dev", "hank_backward_step",
    "hank_backward_step_dual", "hank_forward_step", "hank_forward_step_dual", "hank_last_timings", "hank_stats", "hank_info", "hank_sweep_instance", "hank_vfi", "hank_stationary_dist", "hank_fake_news", "hank_fake_news_het", "hank_device_available",
    "hank_vjp", "hank_vjp_dev", "hank_get_policy_cotangent_seq", "hank_last_vjp_timings", "hank_vjp_het", "hank_vjp_het_dev",
    "hank_jvp_boundary", "hank_jvp_boundary_dev", "hank_vjp_boundary", "hank_vjp_boundary_dev",
    "hank_jvp_het", "hank_jvp_het_dev", "hank_vjp_het_boundary", "hank_vjp_het_boundary_dev",
    "hank_ss_jvp", "hank_ss_jvp_dev", "hank_ss_vjp", "hank_ss_vjp_dev", "hank_last_ss_timings",
    "hank_primal_batch", "hank_primal_batch_dev", "hank_last_batch_timings",
    "hank_ss_batch", "hank_last_ss_batch_timings",
    "hank_get_lottery_record", "hank_get_forward_units",
    "hank_set_group_outputs", "hank_get_group_outputs", "hank_get_group_outputs_dev", "hank_fake_news_group",
    "hank_vjp_group", "hank_vjp_group_dev",
    "hank_set_discount_path", "hank_jvp_shock", "hank_jvp_shock_dev", "hank_vjp_shock", "hank_vjp_shock_dev", "hank_fake_news_shock",
    "hank_set_income_path", "hank_jvp_income", "hank_jvp_income_dev", "hank_vjp_income", "hank_vjp_income_dev", "hank_fake_news_income",
    "hank_get_het_outputs_income", "hank_get_het_outputs_income_dev",
)


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
    dp, vp, i32 = C.POINTER(C.c_double), C.c_void_p, C.c_int32
    lib.hank_create.argtypes = [C.POINTER(hank_model), C.POINTER(vp)]
    lib.hank_create_on.argtypes = [C.POINTER(hank_model), i32, C.POINTER(vp)]
    lib.hank_destroy.argtypes = [vp]
    lib.hank_gather_columns.argtypes = [C.POINTER(vp), i32, C.POINTER(vp), C.POINTER(i32), vp]
    lib.hank_last_error.argtypes = [vp]
    lib.hank_last_error.restype = C.c_char_p
    lib.hank_n_hh.argtypes = [vp]
    lib.hank_set_stream.argtypes = [vp, vp]
    lib.hank_sync.argtypes = [vp]
    lib.hank_set_boundary.argtypes = [vp, dp, dp]
    lib.hank_primal.argtypes = [vp, dp, dp]
    lib.hank_jvp.argtypes = [vp, dp, i32, dp]
    lib.hank_primal_dev.argtypes = [vp, vp, vp]
    lib.hank_jvp_dev.argtypes = [vp, vp, i32, vp]
    lib.hank_check.argtypes = [vp]
    lib.hank_primal_jvp.argtypes = [vp, dp, dp, i32, dp, dp]
    lib.hank_primal_jvp_dev.argtypes = [vp, vp, vp, i32, vp, vp]
    lib.hank_get_policy_seq.argtypes = [vp, dp]
    lib.hank_get_dpolicy_seq.argtypes = [vp, i32, dp]
    lib.hank_get_dist_seq.argtypes = [vp, dp]
    if hasattr(lib, "hank_get_lottery_record"):      # (an older library named by HANK_HIP_LIB for an A-B has none)
        lib.hank_get_lottery_record.argtypes = [vp, vp, dp, dp, vp, dp]
    if hasattr(lib, "hank_get_forward_units"):       # (likewise)
        lib.hank_get_forward_units.argtypes = [vp, vp, vp]
    lib.hank_get_het_outputs.argtypes = [vp, i32, dp, i32, dp, dp]
    lib.hank_get_het_outputs_dev.argtypes = [vp, i32, vp, i32, vp, vp]
    lib.hank_set_het_outputs.argtypes = [vp, i32]
    lib.hank_get_grid_aggregates.argtypes = [vp, dp, i32, dp]
    lib.hank_get_grid_aggregates_dev.argtypes = [vp, vp, i32, vp]
    lib.hank_backward_step.argtypes = [vp, dp, dp, dp, dp]
    lib.hank_backward_step_dual.argtypes = [vp, dp, dp, dp, dp, i32, dp, dp, dp, dp]
    lib.hank_forward_step.argtypes = [vp, dp, dp, dp, dp]
    lib.hank_forward_step_dual.argtypes = [vp, dp, dp, dp, dp, i32, dp, dp, dp, dp]
    lib.hank_last_timings.argtypes = [vp, dp, C.POINTER(i32)]
    lib.hank_stats.argtypes = [vp, C.POINTER(C.c_int64)]
    lib.hank_info.argtypes = [vp, C.POINTER(C.c_int64)]
    lib.hank_sweep_instance.argtypes = [vp, C.POINTER(i32)]
    lib.hank_vfi.argtypes = [vp, dp, C.c_double, i32, dp, dp, C.POINTER(i32), dp]
    lib.hank_stationary_dist.argtypes = [vp, dp, dp, C.c_double, i32, i32, C.POINTER(i32)]
    lib.hank_fake_news.argtypes = [vp, dp, dp]
    lib.hank_fake_news_het.argtypes = [vp, i32, dp, dp]
    lib.hank_device_available.argtypes = []
    lib.hank_vjp.argtypes = [vp, i32, dp, i32, dp]
    lib.hank_vjp_dev.argtypes = [vp, i32, vp, i32, vp]
    lib.hank_vjp_het.argtypes = [vp, i32, dp, i32, dp]
    lib.hank_vjp_het_dev.argtypes = [vp, i32, vp, i32, vp]
    lib.hank_get_policy_cotangent_seq.argtypes = [vp, i32, dp]
    lib.hank_last_vjp_timings.argtypes = [vp, dp, C.POINTER(i32)]
    lib.hank_jvp_boundary.argtypes = [vp, dp, dp, dp, i32, dp]
    lib.hank_jvp_boundary_dev.argtypes = [vp, vp, vp, vp, i32, vp]
    lib.hank_vjp_boundary.argtypes = [vp, i32, dp, i32, dp, dp, dp]
    lib.hank_vjp_boundary_dev.argtypes = [vp, i32, vp, i32, vp, vp, vp]
    lib.hank_jvp_het.argtypes = [vp, i32, dp, dp, dp, i32, dp]
    lib.hank_jvp_het_dev.argtypes = [vp, i32, vp, vp, vp, i32, vp]
    lib.hank_vjp_het_boundary.argtypes = [vp, i32, dp, i32, dp, dp, dp]
    lib.hank_vjp_het_boundary_dev.argtypes = [vp, i32, vp, i32, vp, vp, vp]
    lib.hank_ss_jvp.argtypes = [vp, i32, dp, i32, C.c_double, i32, dp, dp, dp, dp, C.POINTER(i32), dp]
    lib.hank_ss_jvp_dev.argtypes = [vp, i32, vp, i32, C.c_double, i32, vp, vp, vp, vp, C.POINTER(i32), dp]
    lib.hank_ss_vjp.argtypes = [vp, i32, dp, dp, dp, i32, C.c_double, i32, dp, C.POINTER(i32), dp]
    lib.hank_ss_vjp_dev.argtypes = [vp, i32, vp, vp, vp, i32, C.c_double, i32, vp, C.POINTER(i32), dp]
    lib.hank_last_ss_timings.argtypes = [vp, dp]
    lib.hank_primal_batch.argtypes = [vp, i32, dp, i32, dp, dp, C.POINTER(i32)]
    lib.hank_primal_batch_dev.argtypes = [vp, i32, vp, i32, vp, vp]
    lib.hank_last_batch_timings.argtypes = [vp, dp]
    lib.hank_ss_batch.argtypes = [vp, i32, dp, i32, C.c_double, i32, C.c_double, i32, i32, dp, dp, dp, dp, C.POINTER(i32), dp, C.POINTER(i32)]
    lib.hank_last_ss_batch_timings.argtypes = [vp, dp]
    lib.hank_set_group_outputs.argtypes = [vp, i32, dp, C.POINTER(i32)]
    lib.hank_get_group_outputs.argtypes = [vp, dp, i32, dp, dp]
    lib.hank_get_group_outputs_dev.argtypes = [vp, vp, i32, vp, vp]
    lib.hank_fake_news_group.argtypes = [vp, dp, dp]
    lib.hank_vjp_group.argtypes = [vp, i32, dp, dp, i32, dp, dp, dp]
    lib.hank_vjp_group_dev.argtypes = [vp, i32, vp, vp, i32, vp, vp, vp]
    lib.hank_set_discount_path.argtypes = [vp, dp]
    lib.hank_jvp_shock.argtypes = [vp, dp, dp, i32, dp]
    lib.hank_jvp_shock_dev.argtypes = [vp, vp, vp, i32, vp]
    lib.hank_vjp_shock.argtypes = [vp, i32, dp, i32, dp, dp]
    lib.hank_vjp_shock_dev.argtypes = [vp, i32, vp, i32, vp, vp]
    lib.hank_fake_news_shock.argtypes = [vp, i32, dp, dp]
    lib.hank_set_income_path.argtypes = [vp, dp]
    lib.hank_jvp_income.argtypes = [vp, dp, dp, i32, dp]
    lib.hank_jvp_income_dev.argtypes = [vp, vp, vp, i32, vp]
    lib.hank_vjp_income.argtypes = [vp, i32, dp, i32, dp, dp]
    lib.hank_vjp_income_dev.argtypes = [vp, i32, vp, i32, vp, vp]
    lib.hank_fake_news_income.argtypes = [vp, i32, dp, dp]
    lib.hank_get_het_outputs_income.argtypes = [vp, i32, dp, dp, i32, dp, dp]
    lib.hank_get_het_outputs_income_dev.argtypes = [vp, i32, vp, vp, i32, vp, vp]
    for name in ABI_SYMBOLS:
        if name in ("hank_get_lottery_record", "hank_get_forward_units") and not hasattr(lib, name):
            continue
        if name != "hank_last_error":
            getattr(lib, name).restype = C.c_int
    _lib = lib
    return lib


def device_available() -> bool:
    """True when libhank_hip.so is built and the current HIP device is an MI355X (gfx950)."""
    try:
        return bool(load_library().hank_device_available())
    except (RuntimeError, OSError):
        return False


def gather_columns(blocks, d_block_ptrs, N_k, d_out_ptr: int):
    """hank_gather_columns: the (P, N_k) column blocks the contexts `blocks` hold in their own GPUs' memory (device pointers
    `d_block_ptrs`, as written by jvp_dev / primal_jvp_dev) assembled as one (P, sum N_k) matrix at `d_out_ptr` on blocks[0]'s device
    — over xGMI where the devices differ. Asynchronous: blocks[0].sync() before reading."""
    lib = load_library()
    n = len(blocks)
    ctxs = (C.c_void_p * n)(*[b._ctx for b in blocks])
    ptrs = (C.c_void_p * n)(*[C.c_void_p(int(p)) for p in d_block_ptrs])
    nk = (C.c_int32 * n)(*[int(v) for v in N_k])
    rc = lib.hank_gather_columns(ctxs, n, ptrs, nk, C.c_void_p(int(d_out_ptr)))
    if rc != HANK_OK:
        raise _ERR_CLASSES.get(rc, HankHIPError)(rc, lib.hank_last_error(blocks[0]._ctx).decode())


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
            raise _ERR_CLASSES.get(rc, HankHIPError)(rc, msg or "no HIP device available (gfx950 required)")
        self.n_hh = self._lib.hank_n_hh(self._ctx)
        # sweeps issued through this context, by entry point (tests assert "ONE sweep per fullFunction")
        self.calls = {"primal": 0, "jvp": 0, "primal_jvp": 0}
        self.n_groups = 0      # group outputs set on this context (set_group_outputs)

    # -- plumbing ---------------------------------------------------------------------------
    def _chk(self, rc: int):
        if rc != HANK_OK:
            raise _ERR_CLASSES.get(rc, HankHIPError)(rc, self._lib.hank_last_error(self._ctx).decode())

    def clone(self, device=None) -> "HouseholdBlock":
        """A second, independent context of the same model and boundary (its own device memory, graphs and
        stream): independent tangent batches — Jacobian column chunks — can be in flight on both. `device`: put the
        clone on another GPU of the node (default: this context's). The clone carries no group outputs: call
        `set_group_outputs` on it."""
        beta, gamma, bc, vf = self._params
        other = HouseholdBlock(self.a_grid, self.z_grid, self.Pi, beta, gamma, bc, self.T, vf, device=self.device if device is None else device)
        if self._boundary is not None:
            other.set_boundary(*self._boundary)
        if self.discount_path is not None:
            other.set_discount_path(self.discount_path)
        if self.income_path is not None:
            other.set_income_path(self.income_path)
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
        self._chk(self._lib.hank_set_stream(self._ctx, C.c_void_p(hip_stream_handle or 0)))

    def sync(self):
        self._chk(self._lib.hank_sync(self._ctx))

    def check(self):
        self._chk(self._lib.hank_check(self._ctx))

    # -- boundary + fused sweeps ------------------------------------------------------------
    def set_boundary(self, ss_end_value, ss_init_D):
        v = _f(ss_end_value, (self.n_a, self.n_e))
        d = _f(np.asarray(ss_init_D, dtype=np.float64).reshape((self.n_a, self.n_e), order="F"))
        self._chk(self._lib.hank_set_boundary(self._ctx, _p(v), _p(d)))
        self._boundary = (v, d)

    # -- the discount-factor path -------------------------------------------------------------
    def set_discount_path(self, beta_t):
        """a path beta_t (P,) of the discount factor (hank_set_discount_path): beta_t is the factor in period t's Euler equation,
        u'(c_t) = beta_t E_t[V_{t+1}], so beta_{P-1} multiplies the expectation of the terminal value. None returns to the
        model's constant. Like a new boundary it drops the record: the next tangent sweep needs a primal first. While a path is
        set every sweep runs on the per-period launches; the scenario, steady-state and `fake_news*` entries are refused."""
        if beta_t is None:
            self._chk(self._lib.hank_set_discount_path(self._ctx, None))
            self.discount_path = None
            return
        b = np.ascontiguousarray(beta_t, dtype=np.float64)
        if b.shape != (self.P,):
            raise ValueError(f"beta_t must be ({self.P},), got {b.shape}")
        self._chk(self._lib.hank_set_discount_path(self._ctx, _p(b)))
        self.discount_path = b.copy()

    def jvp_shock(self, dxhh=None, dbeta=None) -> np.ndarray:
        """the tangent sweeps with seeds in the discount-factor path as well (hank_jvp_shock): dxhh (n_hh, P, N) as in `jvp`,
        dbeta (P,) or (P, N); None means zeros, at least one must be given. -> dagg (P, N). Works with or without a path set;
        always the launch family. The batch is current afterwards as `jvp`'s is: `dpolicy_seq`, `grid_aggregates`,
        `het_outputs(n_het, dxhh)` and `group_outputs(dxhh)` serve it — beta has no direct term in any output, so pass the same
        dxhh (zeros for None)."""
        if dxhh is None and dbeta is None:
            raise ValueError("at least one of dxhh, dbeta must be given")
        dx = db = None
        if dxhh is not None:
            dx = np.asarray(dxhh, dtype=np.float64)
            dx = dx[:, :, None] if dx.ndim == 2 else dx
            N = dx.shape[2]
        if dbeta is not None:
            db = np.asarray(dbeta, dtype=np.float64)
            db = db[:, None] if db.ndim == 1 else db
            N = db.shape[1] if dx is None else N
            db = _f(db, (self.P, N))
        if dx is not None:
            dx = _f(dx, (self.n_hh, self.P, N))
        out = np.empty((self.P, N), order="F")
        self.calls["jvp"] += 1
        self._chk(self._lib.hank_jvp_shock(self._ctx, _opt(dx), _opt(db), N, _p(out)))
        return out

    def jvp_shock_dev(self, d_dxhh_ptr: int, d_dbeta_ptr: int, N: int, d_dagg_ptr: int = 0):
        """device-pointer form (asynchronous on the context's stream); a pointer of 0 is a zero seed."""
        self._chk(self._lib.hank_jvp_shock_dev(self._ctx, C.c_void_p(d_dxhh_ptr or None), C.c_void_p(d_dbeta_ptr or None), int(N), C.c_void_p(d_dagg_ptr or None)))

    def vjp_shock(self, agg_bar, n_het: int):
        """`vjp_het` with the cotangent of the discount-factor path (hank_vjp_shock): agg_bar (P, n_het, M) -> (xhh_bar
        (n_hh, P, M), beta_bar (P, M)); the exact transpose of `jvp_shock` followed by `het_outputs(n_het)`. xhh_bar equals
        `vjp_het`'s bit for bit; beta_bar is a fixed-order reduction (the same inputs give the same bits)."""
        M, yb = self._cotangents(agg_bar, n_het, het=True)
        out = np.empty((self.n_hh, self.P, max(M, 1)), order="F")
        bb = np.empty((self.P, max(M, 1)), order="F")
        self._chk(self._lib.hank_vjp_shock(self._ctx, int(n_het), _p(yb), M, _p(out), _p(bb)))
        return out, bb

    def vjp_shock_dev(self, n_het: int, d_agg_bar_ptr: int, M: int, d_xhh_bar_ptr: int, d_beta_bar_ptr: int):
        """device-pointer form (asynchronous on the context's stream)."""
        self._chk(self._lib.hank_vjp_shock_dev(self._ctx, int(n_het), C.c_void_p(d_agg_bar_ptr), int(M), C.c_void_p(d_xhh_bar_ptr), C.c_void_p(d_beta_bar_ptr)))

    def fake_news_shock(self, n_het: int):
        """the Toeplitz form of every output's Jacobian with respect to the discount-factor path at the steady state
        (hank_fake_news_shock): -> (F (P, P, n_het), Dv (P, n_het)), the definitions of `fake_news_het` with the input fixed to
        beta. `SteadyStateJacobian.shock_jacobian` does the recursion. Same precondition as `fake_news`; no path may be set."""
        nh = max(int(n_het), 1)
        F = np.empty((self.P, self.P, nh), order="F")
        Dv = np.empty((self.P, nh), order="F")
        self._chk(self._lib.hank_fake_news_shock(self._ctx, int(n_het), _p(F), _p(Dv)))
        return F, Dv

    # -- the income path by productivity state ------------------------------------------------
    def set_income_path(self, y):
        """a path y (n_e, P) of additive income by productivity state (hank_set_income_path): the budget of period t is
        c + a' = (1 + r_t) a + w_t z_e + tr_t + y_t[e]. None clears it. Like a new boundary it drops the record: the next tangent
        sweep needs a primal first. While a path is set every sweep runs on the per-period launches and the entries that rebuild
        consumption from the inputs or are defined at one income process are refused; it excludes a discount-factor path."""
        if y is None:
            self._chk(self._lib.hank_set_income_path(self._ctx, None))
            self.income_path = None
            return
        yy = _f(y, (self.n_e, self.P))
        self._chk(self._lib.hank_set_income_path(self._ctx, _p(yy)))
        self.income_path = yy.copy(order="F")

    def _income_dirs(self, dxhh, dy):
        """the directions of `jvp_income`: dxhh (n_hh, P[, N]) or None, dy (n_e, P[, N]) or None -> (N, dx, dy) column-major"""
        if dxhh is None and dy is None:
            raise ValueError("at least one of dxhh, dy must be given")
        dx = d = None
        if dxhh is not None:
            dx = np.asarray(dxhh, dtype=np.float64)
            dx = dx[:, :, None] if dx.ndim == 2 else dx
            N = dx.shape[2]
        if dy is not None:
            d = np.asarray(dy, dtype=np.float64)
            d = d[:, :, None] if d.ndim == 2 else d
            N = d.shape[2] if dx is None else N
            d = _f(d, (self.n_e, self.P, N))
        if dx is not None:
            dx = _f(dx, (self.n_hh, self.P, N))
        return N, dx, d

    def jvp_income(self, dxhh=None, dy=None) -> np.ndarray:
        """the tangent sweeps with seeds in the income path as well (hank_jvp_income): dxhh (n_hh, P, N) as in `jvp`, dy (n_e, P)
        or (n_e, P, N); None means zeros, at least one must be given. -> dagg (P, N). Works with or without a path set; always the
        launch family. The batch is current afterwards as `jvp`'s is: `dpolicy_seq`, `grid_aggregates`, `group_outputs` (mass and
        policy bases) and `het_outputs(n_het, dxhh)` serve it — y has a direct term in consumption, which `het_outputs` adds from
        the dy the batch carries (or from a `dy=` of the caller's); Value, UCE and consumption groups have no tangent at such a batch."""
        N, dx, d = self._income_dirs(dxhh, dy)
        out = np.empty((self.P, N), order="F")
        self.calls["jvp"] += 1
        self._chk(self._lib.hank_jvp_income(self._ctx, _opt(dx), _opt(d), N, _p(out)))
        return out

    def jvp_income_dev(self, d_dxhh_ptr: int, d_dy_ptr: int, N: int, d_dagg_ptr: int = 0):
        """device-pointer form (asynchronous on the context's stream); a pointer of 0 is a zero seed."""
        self._chk(self._lib.hank_jvp_income_dev(self._ctx, C.c_void_p(d_dxhh_ptr or None), C.c_void_p(d_dy_ptr or None), int(N), C.c_void_p(d_dagg_ptr or None)))

    def vjp_income(self, agg_bar, n_het: int = 1):
        """`vjp` with the cotangent of the income path (hank_vjp_income): agg_bar as in `vjp` -> (xhh_bar (n_hh, P, M), y_bar
        (n_e, P, M)); the exact transpose of `jvp_income` followed by `het_outputs(n_het, dxhh, dy=dy)`. xhh_bar equals `vjp`'s bit
        for bit; y_bar is a fixed-order reduction (the same inputs give the same bits)."""
        M, yb = self._cotangents(agg_bar, n_het, het=False)
        out = np.empty((self.n_hh, self.P, max(M, 1)), order="F")
        ybar = np.empty((self.n_e, self.P, max(M, 1)), order="F")
        self._chk(self._lib.hank_vjp_income(self._ctx, int(n_het), _p(yb), M, _p(out), _p(ybar)))
        return out, ybar

    def vjp_income_dev(self, n_het: int, d_agg_bar_ptr: int, M: int, d_xhh_bar_ptr: int, d_y_bar_ptr: int):
        """device-pointer form (asynchronous on the context's stream)."""
        self._chk(self._lib.hank_vjp_income_dev(self._ctx, int(n_het), C.c_void_p(d_agg_bar_ptr), int(M), C.c_void_p(d_xhh_bar_ptr), C.c_void_p(d_y_bar_ptr)))

    def fake_news_income(self, n_het: int):
        """the Toeplitz form of the Jacobian of outputs 0 .. n_het-1 (n_het <= 2) with respect to the income path at the steady
        state (hank_fake_news_income): -> (F (P, P, n_e, n_het), Dv (P, n_e, n_het)), the definitions of `fake_news_het` with the
        input fixed to y[e]. `SteadyStateJacobian.income_jacobian` does the recursion. Same precondition as `fake_news`; no path
        may be set."""
        nh = max(int(n_het), 1)
        F = np.empty((self.P, self.P, self.n_e, nh), order="F")
        Dv = np.empty((self.P, self.n_e, nh), order="F")
        self._chk(self._lib.hank_fake_news_income(self._ctx, int(n_het), _p(F), _p(Dv)))
        return F, Dv

    def primal(self, xhh) -> np.ndarray:
        x = _f(xhh, (self.n_hh, self.P))
        agg = np.empty(self.P)
        self.calls["primal"] += 1
        self._chk(self._lib.hank_primal(self._ctx, _p(x), _p(agg)))
        return agg

    def jvp(self, dxhh) -> np.ndarray:
        dx = np.asarray(dxhh, dtype=np.float64)
        if dx.ndim == 2:
            dx = dx[:, :, None]
        N = dx.shape[2]
        dx = _f(dx, (self.n_hh, self.P, N))
        out = np.empty((self.P, N), order="F")
        self.calls["jvp"] += 1
        self._chk(self._lib.hank_jvp(self._ctx, _p(dx), N, _p(out)))
        return out

    def primal_jvp(self, xhh, dxhh):
        """value and N partials in one dual-sweep pass (what JVP(fullFunction, x, y) does in the reference)."""
        x = _f(xhh, (self.n_hh, self.P))
        dx = np.asarray(dxhh, dtype=np.float64)
        if dx.ndim == 2:
            dx = dx[:, :, None]
        N = dx.shape[2]
        dx = _f(dx, (self.n_hh, self.P, N))
        agg = np.empty(self.P)
        dagg = np.empty((self.P, N), order="F")
        self.calls["primal_jvp"] += 1
        self._chk(self._lib.hank_primal_jvp(self._ctx, _p(x), _p(dx), N, _p(agg), _p(dagg)))
        return agg, dagg

    # -- K input paths through one chain of launches ------------------------------------------
    def primal_batch(self, xhh, n_het: int = 1, policy: bool = False, check: bool = True):
        """the household block at K input paths at once (hank_primal_batch): xhh (n_hh, P, K) — or (n_hh, P) for one path —
        -> (aggs (P, n_het, K), status (K,) int32[, policies (n_a, n_e, P, K) with policy=True]). Scenario k is `primal` at
        xhh[:, :, k] on the per-period launches, bit for bit in output 0 and in the policies; n_het up to the count declared
        with `set_het_outputs`. The context's recorded primal, its batches and its memo stay as they were. status[k] is scenario
        k's status code; the healthy scenarios' outputs are valid whatever the others did. check=True raises the first failing
        scenario's exception (the arrays of the call are then at `last_batch`)."""
        x = np.asarray(xhh, dtype=np.float64)
        if x.ndim == 2:
            x = x[:, :, None]
        K = x.shape[2] if x.ndim == 3 else 0
        x = _f(x, (self.n_hh, self.P, K))
        nh = max(int(n_het), 1)
        aggs = np.empty((self.P, nh, max(K, 1)), order="F")
        status = np.zeros(max(K, 1), dtype=np.int32)
        pol = np.empty((self.n_a, self.n_e, self.P, max(K, 1)), order="F") if policy else None
        rc = self._lib.hank_primal_batch(self._ctx, int(n_het), _p(x), K, _p(aggs), _opt(pol), status.ctypes.data_as(C.POINTER(C.c_int32)))
        self.last_batch = (aggs, status, pol)
        if rc != HANK_OK and (check or not (1 <= K <= 64) or not np.any(status)):      # (a refusal of the call itself always raises)
            self._chk(rc)
        return (aggs, status, pol) if policy else (aggs, status)

    def primal_batch_dev(self, n_het: int, d_xhh_ptr: int, K: int, d_agg_ptr: int, d_policy_ptr: int = 0):
        """device-pointer form (asynchronous on the context's stream; the verdict arrives at `check`)."""
        self._chk(self._lib.hank_primal_batch_dev(self._ctx, int(n_het), C.c_void_p(d_xhh_ptr), int(K), C.c_void_p(d_agg_ptr), C.c_void_p(d_policy_ptr or None)))

    def last_batch_timings(self):
        """time (ms, HIP events on the stream) of the last batch's backward and forward chains (hank_last_batch_timings)"""
        ms = (C.c_double * 2)()
        self._chk(self._lib.hank_last_batch_timings(self._ctx, ms))
        return (ms[0], ms[1])

    # -- the steady state's household side at K price vectors ---------------------------------
    def _per_scenario(self, arr, K, fill):
        """a start of `ss_batch`: None (`fill` everywhere), (n_a, n_e) or (G,) shared, (n_a, n_e, K) or (G, K) -> (G, K) column-major"""
        if arr is None:
            return np.full((self.G, K), fill, order="F")
        s = np.asarray(arr, dtype=np.float64)
        if s.shape in ((self.n_a, self.n_e), (self.G,)):
            return np.asfortranarray(np.repeat(s.reshape((self.G, 1), order="F"), K, axis=1))
        if s.ndim == 3 and s.shape[:2] == (self.n_a, self.n_e):
            s = s.reshape((self.G, s.shape[2]), order="F")
        return _f(np.array(s, copy=True), (self.G, K))

    def ss_batch(self, xhh, vfi_tol: float, n_het: int = 1, value0=None, D0=None, vfi_max_iter: int = 10_000, dist_tol: float = 1e-15,
                 dist_max_iter: int = 500_000, check_every: int = 25, dist: bool = True, check: bool = True):
        """the steady state's household side at K constant price vectors at once (hank_ss_batch): xhh (n_hh, K) — or (n_hh,) for
        one scenario — -> (aggs (n_het, K), value (n_a, n_e, K), policy (n_a, n_e, K), D (G, K) with every column summing to one,
        iters (K, 2) = value steps and distribution iterations, status (K,) int32). Scenario k is `vfi` at xhh[:, k] on the per-step
        launches followed by `stationary_dist` on its policy, bit for bit. value0: None (ones), (n_a, n_e) shared or (n_a, n_e, K);
        D0 likewise (normalised to sum to one; None = uniform). dist=False: value iteration only (aggs and D are None). The
        context's record, batches and memo stay as they were. check=True raises the first failing scenario's exception; the raw
        arrays of the call (D as the library left it, the sup-norms) are at `last_ss_batch` either way."""
        x = np.asarray(xhh, dtype=np.float64)
        if x.ndim == 1:
            x = x[:, None]
        K = x.shape[1] if x.ndim == 2 else 0
        x = _f(x, (self.n_hh, K))
        Kb, nh = max(K, 1), max(int(n_het), 1)
        v = self._per_scenario(value0, Kb, 1.0)
        pol = np.empty((self.G, Kb), order="F")
        d = aggs = None
        if dist:
            d = self._per_scenario(D0, Kb, 1.0 / self.G)
            if D0 is not None:
                d /= d.sum(axis=0, keepdims=True)
            aggs = np.empty((nh, Kb), order="F")
        iters = np.zeros((Kb, 2), dtype=np.int32)
        nrm = np.zeros(Kb)
        status = np.zeros(Kb, dtype=np.int32)
        ip = C.POINTER(C.c_int32)
        rc = self._lib.hank_ss_batch(self._ctx, int(n_het), _p(x), K, float(vfi_tol), int(vfi_max_iter), float(dist_tol), int(dist_max_iter),
                                     int(check_every), _p(v), _p(pol), _opt(d), _opt(aggs), iters.ctypes.data_as(ip), _p(nrm), status.ctypes.data_as(ip))
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
        ms = (C.c_double * 2)()
        self._chk(self._lib.hank_last_ss_batch_timings(self._ctx, ms))
        return (ms[0], ms[1])

    def primal_jvp_dev(self, d_xhh_ptr: int, d_dxhh_ptr: int, N: int, d_agg_ptr: int = 0, d_dagg_ptr: int = 0):
        self._chk(self._lib.hank_primal_jvp_dev(self._ctx, C.c_void_p(d_xhh_ptr), C.c_void_p(d_dxhh_ptr), int(N),
                                                C.c_void_p(d_agg_ptr), C.c_void_p(d_dagg_ptr)))

    def primal_dev(self, d_xhh_ptr: int, d_agg_ptr: int = 0):
        self._chk(self._lib.hank_primal_dev(self._ctx, C.c_void_p(d_xhh_ptr), C.c_void_p(d_agg_ptr)))

    def jvp_dev(self, d_dxhh_ptr: int, N: int, d_dagg_ptr: int = 0):
        self._chk(self._lib.hank_jvp_dev(self._ctx, C.c_void_p(d_dxhh_ptr), int(N), C.c_void_p(d_dagg_ptr)))

    # -- the transposed block ---------------------------------------------------------------
    def _cotangents(self, agg_bar, n_het, het):
        """the cotangents of `vjp` (het False: (P,), (P, M) for n_het = 1, or (P, n_het, M)) or of `vjp_het` (het True:
        (P, n_het, M) only) -> (M, yb (P, n_het, M) column-major)"""
        yb = np.asarray(agg_bar, dtype=np.float64)
        if het and yb.ndim != 3:
            raise ValueError("agg_bar must be (P, n_het, M)")
        if yb.ndim == 1:
            yb = yb[:, None]
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
        out = np.empty((self.n_hh, self.P, max(M, 1)), order="F")
        self._chk(self._lib.hank_vjp(self._ctx, int(n_het), _p(yb), M, _p(out)))
        return out

    def vjp_dev(self, n_het: int, d_agg_bar_ptr: int, M: int, d_xhh_bar_ptr: int):
        """device-pointer form (asynchronous on the context's stream)."""
        self._chk(self._lib.hank_vjp_dev(self._ctx, int(n_het), C.c_void_p(d_agg_bar_ptr), int(M), C.c_void_p(d_xhh_bar_ptr)))

    def vjp_het(self, agg_bar, n_het: int) -> np.ndarray:
        """`vjp` with cotangents on every heterogeneous output (hank_vjp_het): agg_bar (P, n_het, M), n_het up to the count
        declared with `set_het_outputs` — outputs 2, 3 are Value and UCE, which are not affine in the policy.
        -> xhh_bar (n_hh, P, M). n_het <= 2 runs `vjp`'s path: the same bits."""
        M, yb = self._cotangents(agg_bar, n_het, het=True)
        out = np.empty((self.n_hh, self.P, max(M, 1)), order="F")
        self._chk(self._lib.hank_vjp_het(self._ctx, int(n_het), _p(yb), M, _p(out)))
        return out

    def vjp_het_dev(self, n_het: int, d_agg_bar_ptr: int, M: int, d_xhh_bar_ptr: int):
        """device-pointer form (asynchronous on the context's stream)."""
        self._chk(self._lib.hank_vjp_het_dev(self._ctx, int(n_het), C.c_void_p(d_agg_bar_ptr), int(M), C.c_void_p(d_xhh_bar_ptr)))

    # -- tangents and cotangents on the boundary ---------------------------------------------
    def _boundary_seed(self, seed, N):
        """a boundary seed (n_a, n_e), (n_a, n_e, N) or (G, N) -> (G, N) column-major, pt = e n_a + a; None stays None"""
        if seed is None:
            return None
        s = np.asarray(seed, dtype=np.float64)
        if s.shape == (self.n_a, self.n_e):
            s = s[:, :, None]
        if s.ndim == 3 and s.shape[:2] == (self.n_a, self.n_e):
            s = s.reshape((self.G, s.shape[2]), order="F")
        return _f(s, (self.G, N))

    def _directions(self, dxhh, dvalue_end, dD_init):
        """the inputs of `jvp_boundary` / `jvp_het` -> (N, dx (n_hh, P, N), dv (G, N), dd (G, N)), column-major; None stays None"""
        given = [np.asarray(v) for v in (dxhh, dvalue_end, dD_init) if v is not None]
        if not given:
            raise ValueError("at least one of dxhh, dvalue_end, dD_init must be given")
        N = given[0].shape[-1] if given[0].ndim == 3 else 1
        dx = None
        if dxhh is not None:
            dx = np.asarray(dxhh, dtype=np.float64)
            dx = _f(dx[:, :, None] if dx.ndim == 2 else dx, (self.n_hh, self.P, N))
        return N, dx, self._boundary_seed(dvalue_end, N), self._boundary_seed(dD_init, N)

    def jvp_boundary(self, dxhh=None, dvalue_end=None, dD_init=None) -> np.ndarray:
        """the tangent sweeps with seeds on the boundary as well (hank_jvp_boundary): dxhh (n_hh, P, N) as in `jvp`, dvalue_end
        and dD_init (n_a, n_e, N) — tangents of `ss_end.value` (BackwardIteration.jl:85) and `ss_initial.D`
        (ForwardIteration.jl:293); None means zeros, at least one must be given. -> dagg (P, N). Always the launch family. The
        batch is current afterwards: `dpolicy_seq`, `grid_aggregates`, `het_outputs(2, dxhh)` serve it (pass zeros for a dxhh of
        None)."""
        N, dx, dv, dd = self._directions(dxhh, dvalue_end, dD_init)
        out = np.empty((self.P, N), order="F")
        self.calls["jvp"] += 1
        self._chk(self._lib.hank_jvp_boundary(self._ctx, _opt(dx), _opt(dv), _opt(dd), N, _p(out)))
        return out

    def jvp_boundary_dev(self, d_dxhh_ptr: int, d_dvalue_end_ptr: int, d_dD_init_ptr: int, N: int, d_dagg_ptr: int = 0):
        """device-pointer form (asynchronous on the context's stream); a pointer of 0 is a zero seed."""
        self._chk(self._lib.hank_jvp_boundary_dev(self._ctx, C.c_void_p(d_dxhh_ptr or None), C.c_void_p(d_dvalue_end_ptr or None),
                                                  C.c_void_p(d_dD_init_ptr or None), int(N), C.c_void_p(d_dagg_ptr or None)))

    def vjp_boundary(self, agg_bar, n_het: int = 1):
        """`vjp` with the boundary's cotangents (hank_vjp_boundary): -> (xhh_bar (n_hh, P, M), value_end_bar (n_a, n_e, M),
        D_init_bar (n_a, n_e, M)) — the cotangents of the household inputs, of `ss_end.value` and of `ss_initial.D`; the exact
        transpose of `jvp_boundary` followed by `het_outputs(n_het)`. agg_bar as in `vjp`; xhh_bar equals `vjp`'s bit for bit."""
        M, yb = self._cotangents(agg_bar, n_het, het=False)
        out = np.empty((self.n_hh, self.P, max(M, 1)), order="F")
        vb = np.empty((self.n_a, self.n_e, max(M, 1)), order="F")
        db = np.empty((self.n_a, self.n_e, max(M, 1)), order="F")
        self._chk(self._lib.hank_vjp_boundary(self._ctx, int(n_het), _p(yb), M, _p(out), _p(vb), _p(db)))
        return out, vb, db

    def vjp_boundary_dev(self, n_het: int, d_agg_bar_ptr: int, M: int, d_xhh_bar_ptr: int, d_value_end_bar_ptr: int = 0, d_D_init_bar_ptr: int = 0):
        """device-pointer form (asynchronous on the context's stream); a boundary pointer of 0 is not wanted."""
        self._chk(self._lib.hank_vjp_boundary_dev(self._ctx, int(n_het), C.c_void_p(d_agg_bar_ptr), int(M), C.c_void_p(d_xhh_bar_ptr),
                                                  C.c_void_p(d_value_end_bar_ptr or None), C.c_void_p(d_D_init_bar_ptr or None)))

    # -- every output's tangent in one pair of sweeps; its transpose on the boundary ----------
    def jvp_het(self, dxhh=None, dvalue_end=None, dD_init=None, n_het: int = 2) -> np.ndarray:
        """every declared output's tangent from one pair of sweeps (hank_jvp_het): inputs as in `jvp_boundary` (None means zeros,
        at least one must be given), n_het up to the count declared with `set_het_outputs`. -> dagg (P, n_het, N), the shape of
        `het_outputs`' dagg. Value and UCE ride in the forward sweep, so boundary seeds reach them too. Always the launch
        family; n_het <= 2 gives the bits of `jvp` / `jvp_boundary` under the launch schedule."""
        N, dx, dv, dd = self._directions(dxhh, dvalue_end, dD_init)
        out = np.empty((self.P, max(int(n_het), 1), N), order="F")
        self.calls["jvp"] += 1
        self._chk(self._lib.hank_jvp_het(self._ctx, int(n_het), _opt(dx), _opt(dv), _opt(dd), N, _p(out)))
        return out

    def jvp_het_dev(self, n_het: int, d_dxhh_ptr: int, d_dvalue_end_ptr: int, d_dD_init_ptr: int, N: int, d_dagg_ptr: int = 0):
        """device-pointer form (asynchronous on the context's stream); a pointer of 0 is a zero seed."""
        self._chk(self._lib.hank_jvp_het_dev(self._ctx, int(n_het), C.c_void_p(d_dxhh_ptr or None), C.c_void_p(d_dvalue_end_ptr or None),
                                             C.c_void_p(d_dD_init_ptr or None), int(N), C.c_void_p(d_dagg_ptr or None)))

    def vjp_het_boundary(self, agg_bar, n_het: int, value_end: bool = True, D_init: bool = True):
        """`vjp_het` with the boundary's cotangents (hank_vjp_het_boundary): agg_bar (P, n_het, M) -> (xhh_bar (n_hh, P, M),
        value_end_bar (n_a, n_e, M), D_init_bar (n_a, n_e, M)); the exact transpose of `jvp_het`. A boundary cotangent that is
        not wanted (value_end / D_init False) is not computed and comes back as None. xhh_bar equals `vjp_het`'s bit for bit."""
        M, yb = self._cotangents(agg_bar, n_het, het=True)
        out = np.empty((self.n_hh, self.P, max(M, 1)), order="F")
        vb = np.empty((self.n_a, self.n_e, max(M, 1)), order="F") if value_end else None
        db = np.empty((self.n_a, self.n_e, max(M, 1)), order="F") if D_init else None
        self._chk(self._lib.hank_vjp_het_boundary(self._ctx, int(n_het), _p(yb), M, _p(out), _opt(vb), _opt(db)))
        return out, vb, db

    def vjp_het_boundary_dev(self, n_het: int, d_agg_bar_ptr: int, M: int, d_xhh_bar_ptr: int, d_value_end_bar_ptr: int = 0, d_D_init_bar_ptr: int = 0):
        """device-pointer form (asynchronous on the context's stream); a boundary pointer of 0 is not wanted."""
        self._chk(self._lib.hank_vjp_het_boundary_dev(self._ctx, int(n_het), C.c_void_p(d_agg_bar_ptr), int(M), C.c_void_p(d_xhh_bar_ptr),
                                                      C.c_void_p(d_value_end_bar_ptr or None), C.c_void_p(d_D_init_bar_ptr or None)))

    # -- derivatives through the steady state -------------------------------------------------
    def _ss_done(self, who, names, it, res, tol, max_iter, check):
        self.last_ss = {"iters": (int(it[0]), int(it[1])), "resid": (float(res[0]), float(res[1]))}
        if check:
            for k in range(2):
                if it[k] >= max_iter and not res[k] <= tol:
                    raise SteadyStateLoopError(f"{who}: the {names[k]} loop took max_iter = {max_iter} steps and its last increment ratio "
                                               f"{res[k]:.3g} is above tol = {tol:.3g}")

    def ss_jvp(self, dxhh, n_het: int = 2, tol: float = 1e-13, max_iter: int = 50_000, check: bool = True):
        """derivatives of the steady state's household objects in the household prices (hank_ss_jvp; what
        ForwardDiff.jacobian carries through the VFI and invariant_dist at SteadyState.jl:195). Needs `primal` at the constant
        steady-state path with the steady state as both boundaries (the precondition of `fake_news`). dxhh (n_hh,) or (n_hh, N).
        -> (dagg (n_het, N), dV (n_a, n_e, N), dpol (n_a, n_e, N), dD (n_a, n_e, N), iters (value loop, distribution loop)).
        Raises SteadyStateLoopError when a loop ran into max_iter (check=False: returns what it has; `last_ss` holds the
        increment ratios)."""
        dx = np.asarray(dxhh, dtype=np.float64)
        if dx.ndim == 1:
            dx = dx[:, None]
        N = dx.shape[1]
        dx = _f(dx, (self.n_hh, N))
        dagg = np.empty((max(int(n_het), 1), N), order="F")
        dV, dpol, dD = (np.empty((self.n_a, self.n_e, N), order="F") for _ in range(3))
        it, res = (C.c_int32 * 2)(), (C.c_double * 2)()
        self._chk(self._lib.hank_ss_jvp(self._ctx, int(n_het), _p(dx), N, float(tol), int(max_iter), _p(dV), _p(dpol), _p(dD), _p(dagg), it, res))
        self._ss_done("ss_jvp", ("value", "distribution"), it, res, tol, max_iter, check)
        return dagg, dV, dpol, dD, (int(it[0]), int(it[1]))

    def ss_vjp(self, agg_bar=None, value_bar=None, D_bar=None, n_het: int = 2, tol: float = 1e-13, max_iter: int = 50_000, check: bool = True):
        """the transpose of `ss_jvp` (hank_ss_vjp): cotangents agg_bar (n_het,) or (n_het, M) of the steady state's aggregates,
        value_bar and D_bar (n_a, n_e[, M]) or (G, M) of V_ss and D_ss — e.g. `vjp_het_boundary`'s value_end_bar — any of them
        None (not given), at least one given. -> (xhh_bar (n_hh, M), iters (nu loop, lambda loop))."""
        if agg_bar is None and value_bar is None and D_bar is None:
            raise ValueError("at least one of agg_bar, value_bar, D_bar must be given")
        yb = None
        M = None
        if agg_bar is not None:
            yb = np.asarray(agg_bar, dtype=np.float64)
            yb = yb[:, None] if yb.ndim == 1 else yb
            M = yb.shape[1]
        else:
            b = np.asarray(value_bar if value_bar is not None else D_bar)
            M = 1 if b.shape == (self.n_a, self.n_e) else b.shape[-1]
        if yb is not None:
            yb = _f(yb, (int(n_het), M) if 1 <= int(n_het) <= 4 else None)
        vb, db = self._boundary_seed(value_bar, M), self._boundary_seed(D_bar, M)
        out = np.empty((self.n_hh, M), order="F")
        it, res = (C.c_int32 * 2)(), (C.c_double * 2)()
        self._chk(self._lib.hank_ss_vjp(self._ctx, int(n_het), _opt(yb), _opt(vb), _opt(db), M, float(tol), int(max_iter), _p(out), it, res))
        self._ss_done("ss_vjp", ("nu", "lambda"), it, res, tol, max_iter, check)
        return out, (int(it[0]), int(it[1]))

    def ss_jvp_dev(self, d_dxhh_ptr: int, N: int, d_dagg_ptr: int, d_dvalue_ptr: int = 0, d_dpolicy_ptr: int = 0, d_dD_ptr: int = 0,
                   n_het: int = 2, tol: float = 1e-13, max_iter: int = 50_000, check: bool = True):
        """device-pointer form of `ss_jvp` (hank_ss_jvp_dev): d_dxhh (n_hh, N) in; d_dagg (n_het, N) and the exports (G, N) out,
        all column-major, written straight to the caller's buffers; an export pointer of 0 is not wanted. The loops read their
        stop word on the host, so the call returns with the stream drained. -> iters; `last_ss` as after `ss_jvp`."""
        it, res = (C.c_int32 * 2)(), (C.c_double * 2)()
        self._chk(self._lib.hank_ss_jvp_dev(self._ctx, int(n_het), C.c_void_p(d_dxhh_ptr), int(N), float(tol), int(max_iter), C.c_void_p(d_dvalue_ptr or None),
                                            C.c_void_p(d_dpolicy_ptr or None), C.c_void_p(d_dD_ptr or None), C.c_void_p(d_dagg_ptr), it, res))
        self._ss_done("ss_jvp_dev", ("value", "distribution"), it, res, tol, max_iter, check)
        return (int(it[0]), int(it[1]))

    def ss_vjp_dev(self, d_agg_bar_ptr: int, d_value_bar_ptr: int, d_D_bar_ptr: int, M: int, d_xhh_bar_ptr: int,
                   n_het: int = 2, tol: float = 1e-13, max_iter: int = 50_000, check: bool = True):
        """device-pointer form of `ss_vjp` (hank_ss_vjp_dev): d_agg_bar (n_het, M), d_value_bar and d_D_bar (G, M) in, a pointer
        of 0 is a cotangent not given (at least one must be); d_xhh_bar (n_hh, M) out. -> iters; `last_ss` as after `ss_vjp`."""
        it, res = (C.c_int32 * 2)(), (C.c_double * 2)()
        self._chk(self._lib.hank_ss_vjp_dev(self._ctx, int(n_het), C.c_void_p(d_agg_bar_ptr or None), C.c_void_p(d_value_bar_ptr or None),
                                            C.c_void_p(d_D_bar_ptr or None), int(M), float(tol), int(max_iter), C.c_void_p(d_xhh_bar_ptr), it, res))
        self._ss_done("ss_vjp_dev", ("nu", "lambda"), it, res, tol, max_iter, check)
        return (int(it[0]), int(it[1]))

    def policy_cotangent_seq(self, M: int) -> np.ndarray:
        """(n_a, n_e, P, M): cotangent of the policy sequence of the last vjp / vjp_het (hank_get_policy_cotangent_seq)."""
        out = np.empty((self.n_a, self.n_e, self.P, max(int(M), 1)), order="F")
        self._chk(self._lib.hank_get_policy_cotangent_seq(self._ctx, int(M), _p(out)))
        return out

    def last_vjp_timings(self):
        ms = (C.c_double * 2)()
        ln = (C.c_int32 * 2)()
        self._chk(self._lib.hank_last_vjp_timings(self._ctx, ms, ln))
        return {k: {"ms": ms[i], "launches": ln[i]} for i, k in enumerate(("sweep_a", "sweep_b"))}

    def last_ss_timings(self):
        """time (ms, HIP events on the stream) of the two loops of the last ss_jvp / ss_vjp, in the order of their `iters` (hank_last_ss_timings)"""
        ms = (C.c_double * 2)()
        self._chk(self._lib.hank_last_ss_timings(self._ctx, ms))
        return (ms[0], ms[1])

    def last_timings(self):
        ms = (C.c_double * 6)()
        ln = (C.c_int32 * 6)()
        self._chk(self._lib.hank_last_timings(self._ctx, ms, ln))
        names = ("primal_backward", "primal_forward", "tangent_backward", "tangent_forward", "dual_backward", "dual_forward")
        return {k: {"ms": ms[i], "launches": ln[i]} for i, k in enumerate(names)}

    def stats(self):
        """counters of the context (include/hank_hip.h: hank_stats)."""
        out = (C.c_int64 * 8)()
        self._chk(self._lib.hank_stats(self._ctx, out))
        names = ("sweep_launches", "tangent_workspaces_allocated", "graphs_captured", "schedule", "fallbacks", "vfi_iterations",
                 "primal_memo_hits", "primal_sweeps")
        return {k: int(out[i]) for i, k in enumerate(names)}

    def info(self):
        """which kernel family served the last tangent sweep and how the context chooses (include/hank_hip.h: hank_info)."""
        out = (C.c_int64 * 8)()
        self._chk(self._lib.hank_info(self._ctx, out))
        names = ("last_tangent_family", "wide_mode", "wide_min", "wide_supported", "xjvp_max", "record_diet", "record_bytes", "lwg_builds")
        d = {k: int(out[i]) for i, k in enumerate(names)}
        d["last_tangent_family_name"] = ("launch-per-period", "xcd-persistent", "on-chip-wide")[d["last_tangent_family"]]
        return d

    def sweep_instance(self):
        """which instances of the Dual pass's persistent sweeps were enqueued last (include/hank_hip.h: hank_sweep_instance):
        {"back": (NE, CRRA), "fwd": (NE, CRRA)}; -1 before the first Dual pass."""
        out = (C.c_int32 * 4)()
        self._chk(self._lib.hank_sweep_instance(self._ctx, out))
        return {"back": (int(out[0]), int(out[1])), "fwd": (int(out[2]), int(out[3]))}

    def policy_seq(self) -> np.ndarray:
        """(n_a, n_e, P): policy matrix of every period (BackwardIteration's return value)."""
        out = np.empty((self.n_a, self.n_e, self.P), order="F")
        self._chk(self._lib.hank_get_policy_seq(self._ctx, _p(out)))
        return out

    def lottery_record(self):
        """the Young lottery of the last primal as the record holds it (hank_get_lottery_record): lo, lw, ig of shape (n_a, n_e, P),
        the packed records lq (structured: w, lo, flags) of the same shape and the grid's inverse gaps iga (n_a,)."""
        shp = (self.n_a, self.n_e, self.P)
        lo, lw, ig = np.empty(shp, np.int32, order="F"), np.empty(shp, order="F"), np.empty(shp, order="F")
        lq = np.empty(shp, np.dtype([("w", "<f8"), ("lo", "<i4"), ("flags", "<i4")]), order="F")
        iga = np.empty(self.n_a)
        self._chk(self._lib.hank_get_lottery_record(self._ctx, lo.ctypes.data_as(C.c_void_p), _p(lw), _p(ig), lq.ctypes.data_as(C.c_void_p), _p(iga)))
        return {"lo": lo, "lw": lw, "ig": ig, "lq": lq, "iga": iga}

    def forward_units(self):
        """the persistent forward sweeps' work units of the recorded lottery (hank_get_forward_units): src (P, S) and units
        (P, S, 64, 2) as the library lays them out, S = ceil(n_a / 63) members; src >> 18 is a member's unit count."""
        S = (self.n_a + 62) // 63
        src, units = np.empty((self.P, S), np.int32), np.empty((self.P, S, 64, 2), np.int32)
        self._chk(self._lib.hank_get_forward_units(self._ctx, src.ctypes.data_as(C.c_void_p), units.ctypes.data_as(C.c_void_p)))
        return src, units

    def dist_seq(self) -> np.ndarray:
        out = np.empty((self.n_a, self.n_e, self.P), order="F")
        self._chk(self._lib.hank_get_dist_seq(self._ctx, _p(out)))
        return out

    def dpolicy_seq(self, N: int) -> np.ndarray:
        """(n_a, n_e, P, N): partials of the policy sequence of the last jvp."""
        out = np.empty((self.n_a, self.n_e, self.P, N), order="F")
        self._chk(self._lib.hank_get_dpolicy_seq(self._ctx, int(N), _p(out)))
        return out

    def het_outputs(self, n_het: int = 2, dxhh=None, dy=None):
        """every heterogeneous variable's aggregate of the last sweeps (hank_get_het_outputs; ForwardIteration.jl:303-307):
        output 0 the policy variable (KD / A), output 1 consumption, output 2 Value, output 3 UCE (one-asset HANK), up to the
        count declared with `set_het_outputs`. -> agg (P, n_het), and dagg (P, n_het, N) when `dxhh`
        (n_hh, P, N) — the input of the last tangent sweep — is given (else None). dy (n_e, P, N): income directions
        (hank_get_het_outputs_income, n_het <= 2) for consumption's direct term, in place of the ones a batch of `jvp_income`
        carries and adds by itself; dxhh may then be None (zeros)."""
        agg = np.empty((self.P, n_het), order="F")
        if dy is not None:
            N, dx, d = self._income_dirs(dxhh, dy)
            if dx is None:
                dx = np.zeros((self.n_hh, self.P, N), order="F")
            dagg = np.empty((self.P, n_het, N), order="F")
            self._chk(self._lib.hank_get_het_outputs_income(self._ctx, int(n_het), _p(dx), _p(d), N, _p(agg), _p(dagg)))
            return agg, dagg
        if dxhh is None:
            self._chk(self._lib.hank_get_het_outputs(self._ctx, int(n_het), None, 0, _p(agg), None))
            return agg, None
        dxhh = np.asfortranarray(dxhh, dtype=np.float64)
        if dxhh.ndim != 3 or dxhh.shape[:2] != (self.n_hh, self.P):
            raise ValueError(f"dxhh must be ({self.n_hh}, {self.P}, N), got {dxhh.shape}")
        N = dxhh.shape[2]
        dagg = np.empty((self.P, n_het, N), order="F")
        self._chk(self._lib.hank_get_het_outputs(self._ctx, int(n_het), _p(dxhh), N, _p(agg), _p(dagg)))
        return agg, dagg

    def set_het_outputs(self, n_het: int):
        """declare how many heterogeneous outputs het_outputs will be asked for (hank_set_het_outputs; default 2)."""
        self._chk(self._lib.hank_set_het_outputs(self._ctx, int(n_het)))
        self._n_het_declared = int(n_het)

    def het_outputs_dev(self, n_het: int, d_dxhh: int, N: int, d_agg: int, d_dagg: int, d_dy: int = 0):
        """device-pointer form (asynchronous on the context's stream); d_dy: the income directions (hank_get_het_outputs_income_dev)."""
        if d_dy:
            self._chk(self._lib.hank_get_het_outputs_income_dev(self._ctx, int(n_het), d_dxhh or None, d_dy, int(N), d_agg or None, d_dagg or None))
            return
        self._chk(self._lib.hank_get_het_outputs_dev(self._ctx, int(n_het), d_dxhh or None, int(N), d_agg or None, d_dagg or None))

    def grid_aggregates(self, N: int = 0):
        """the grid-weighted aggregate sum_pt a(pt) D_t(pt) of the last primal sweep, and (N > 0) its partials (P, N) of the
        last tangent sweep (hank_get_grid_aggregates)."""
        agg2 = np.empty(self.P)
        dagg2 = np.empty((self.P, N), order="F") if N > 0 else None
        self._chk(self._lib.hank_get_grid_aggregates(self._ctx, _p(agg2), int(N), _p(dagg2) if N > 0 else None))
        return agg2, dagg2

    def fake_news(self):
        """the household block's Jacobian at the steady state from its Toeplitz structure (hank_fake_news):
        -> F (P, P, n_hh), Dv (P, n_hh); `SteadyStateJacobian.household_jacobian` turns them into d agg_t / d xhh_{k,s}."""
        F = np.empty((self.P, self.P, self.n_hh), order="F")
        Dv = np.empty((self.P, self.n_hh), order="F")
        self._chk(self._lib.hank_fake_news(self._ctx, _p(F), _p(Dv)))
        return F, Dv

    def fake_news_het(self, n_het: int):
        """the same Toeplitz form for heterogeneous outputs 0 .. n_het-1 of `het_outputs` (hank_fake_news_het):
        -> F (P, P, n_hh, n_het), Dv (P, n_hh, n_het); output 0 equals `fake_news()` bit for bit, and
        `household_jacobian(F[..., o], Dv[..., o])` is d agg^o_t / d xhh_{k,s}."""
        nb = max(int(n_het), 1)                  # (the library refuses an n_het outside 1..3 / 1..4)
        F = np.empty((self.P, self.P, self.n_hh, nb), order="F")
        Dv = np.empty((self.P, self.n_hh, nb), order="F")
        self._chk(self._lib.hank_fake_news_het(self._ctx, int(n_het), _p(F), _p(Dv)))
        return F, Dv

    # -- group outputs: aggregates by household group -------------------------------------------
    def set_group_outputs(self, W, base):
        """the groups `group_outputs` and `fake_news_group` serve (hank_set_group_outputs): W (G, K) — or (n_a, n_e, K) — holds
        one weight vector per group, indexed like D (pt = e n_a + ia), any real values; base[k] is GROUP_MASS, GROUP_POLICY or
        GROUP_CONS (one value serves every group). K = 0 (W=None) clears them. The record, the current tangent batch, the primal memo
        and the `set_het_outputs` count stay as they are. `clone()` does not carry the groups."""
        if W is None:
            self._chk(self._lib.hank_set_group_outputs(self._ctx, 0, None, None))
            self.n_groups = 0
            return
        W = np.asarray(W, dtype=np.float64)
        if W.ndim == 3 and W.shape[:2] == (self.n_a, self.n_e):
            W = W.reshape(self.G, W.shape[2], order="F")
        if W.ndim == 1:
            W = W[:, None]
        if W.ndim != 2 or W.shape[0] != self.G:
            raise ValueError(f"W must be ({self.G}, K) or ({self.n_a}, {self.n_e}, K), got {W.shape}")
        W = np.asfortranarray(W)
        K = W.shape[1]
        b = np.ascontiguousarray(np.broadcast_to(np.asarray(base, dtype=np.int32), (K,)))
        self._chk(self._lib.hank_set_group_outputs(self._ctx, K, _p(W), b.ctypes.data_as(C.POINTER(C.c_int32))))
        self.n_groups = K

    def group_outputs(self, dxhh=None):
        """the group outputs of the last sweeps (hank_get_group_outputs; ForwardIteration.jl:303-307): Y^k_t = sum W_k f D_t.
        -> agg (P, K), and dagg (P, K, N) when `dxhh` (n_hh, P, N) — the input of the last tangent sweep — is given (else
        None). The rules of `het_outputs`; a batch with boundary seeds is refused."""
        K = max(self.n_groups, 1)      # (the library refuses a call without groups)
        agg = np.empty((self.P, K), order="F")
        if dxhh is None:
            self._chk(self._lib.hank_get_group_outputs(self._ctx, None, 0, _p(agg), None))
            return agg, None
        dxhh = np.asfortranarray(dxhh, dtype=np.float64)
        if dxhh.ndim != 3 or dxhh.shape[:2] != (self.n_hh, self.P):
            raise ValueError(f"dxhh must be ({self.n_hh}, {self.P}, N), got {dxhh.shape}")
        N = dxhh.shape[2]
        dagg = np.empty((self.P, K, N), order="F")
        self._chk(self._lib.hank_get_group_outputs(self._ctx, _p(dxhh), N, _p(agg), _p(dagg)))
        return agg, dagg

    def group_outputs_dev(self, d_dxhh: int, N: int, d_agg: int, d_dagg: int):
        """device-pointer form (asynchronous on the context's stream)."""
        self._chk(self._lib.hank_get_group_outputs_dev(self._ctx, d_dxhh or None, int(N), d_agg or None, d_dagg or None))

    def vjp_group(self, grp_bar, agg_bar=None, n_het: int = 0, value_end: bool = False, D_init: bool = False):
        """the transpose of `group_outputs`' tangent map (hank_vjp_group; the reverse rules of ForwardIteration.jl:339-420 with the
        weighted dot of :303-307): grp_bar (P, K, M) — or (P, K) for M = 1 — holds cotangents on the K group outputs, the shape of
        `group_outputs`' dagg. agg_bar (P, n_het, M), n_het 1 or 2, adds cotangents on outputs 0 and 1 (`vjp`'s) in the same product;
        without it n_het is 0. -> xhh_bar (n_hh, P, M); with value_end or D_init the triple (xhh_bar, value_end_bar, D_init_bar) of
        `vjp_het_boundary`, an unwanted one None. `policy_cotangent_seq(M)` serves its policy cotangent afterwards."""
        gb, M = None, None
        if grp_bar is not None:
            gb = np.asarray(grp_bar, dtype=np.float64)
            if gb.ndim == 2:
                gb = gb[:, :, None]
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
        out = np.empty((self.n_hh, self.P, max(M, 1)), order="F")
        vb = np.empty((self.n_a, self.n_e, max(M, 1)), order="F") if value_end else None
        db = np.empty((self.n_a, self.n_e, max(M, 1)), order="F") if D_init else None
        self._chk(self._lib.hank_vjp_group(self._ctx, int(n_het), _opt(yb), _opt(gb), M, _p(out), _opt(vb), _opt(db)))
        return (out, vb, db) if (value_end or D_init) else out

    def vjp_group_dev(self, n_het: int, d_agg_bar_ptr: int, d_grp_bar_ptr: int, M: int, d_xhh_bar_ptr: int, d_value_end_bar_ptr: int = 0,
                      d_D_init_bar_ptr: int = 0):
        """device-pointer form (asynchronous on the context's stream); an agg_bar pointer of 0 goes with n_het = 0, a boundary pointer
        of 0 is not wanted."""
        self._chk(self._lib.hank_vjp_group_dev(self._ctx, int(n_het), C.c_void_p(d_agg_bar_ptr or None), C.c_void_p(d_grp_bar_ptr or None), int(M),
                                               C.c_void_p(d_xhh_bar_ptr), C.c_void_p(d_value_end_bar_ptr or None), C.c_void_p(d_D_init_bar_ptr or None)))

    def fake_news_group(self):
        """the Toeplitz form of `fake_news_het` for the group outputs (hank_fake_news_group): -> F (P, P, n_hh, K),
        Dv (P, n_hh, K); `household_jacobian(F[..., k], Dv[..., k])` is d Y^k_t / d xhh_{i,s}."""
        K = max(self.n_groups, 1)
        F = np.empty((self.P, self.P, self.n_hh, K), order="F")
        Dv = np.empty((self.P, self.n_hh, K), order="F")
        self._chk(self._lib.hank_fake_news_group(self._ctx, _p(F), _p(Dv)))
        return F, Dv

    def vfi(self, value0, xhh_t, tol: float, max_iter: int = 10_000):
        """device-resident inner fixed point of the steady state (hank_vfi; SteadyState.jl:132-141):
        -> (value, policy, steps, last sup-norm)."""
        v = _f(np.array(value0, dtype=np.float64, copy=True), (self.n_a, self.n_e))
        x = _f(xhh_t, (self.n_hh,))
        pol = np.empty((self.n_a, self.n_e), order="F")
        it, nrm = C.c_int32(), C.c_double()
        self._chk(self._lib.hank_vfi(self._ctx, _p(x), float(tol), int(max_iter), _p(v), _p(pol), C.byref(it), C.byref(nrm)))
        return v, pol, it.value, nrm.value

    def stationary_dist(self, policy, D0=None, tol: float = 1e-15, max_iter: int = 500_000, check_every: int = 25):
        """stationary distribution of the steady state by the power method on the device (hank_stationary_dist):
        -> (D as a length-G vector summing to one, steps)."""
        p = _f(policy, (self.n_a, self.n_e))
        d = np.full(self.G, 1.0 / self.G) if D0 is None else np.asarray(D0, dtype=np.float64).reshape(-1, order="F") / np.sum(D0)
        d = _f(d.reshape((self.n_a, self.n_e), order="F"))
        it = C.c_int32()
        self._chk(self._lib.hank_stationary_dist(self._ctx, _p(p), _p(d), float(tol), int(max_iter), int(check_every), C.byref(it)))
        out = d.reshape(-1, order="F")
        return out / out.sum(), it.value

    # -- granular steps ---------------------------------------------------------------------
    def backward_step(self, value_next, xhh_t):
        v = _f(value_next, (self.n_a, self.n_e))
        x = _f(xhh_t, (self.n_hh,))
        vo = np.empty((self.n_a, self.n_e), order="F")
        po = np.empty((self.n_a, self.n_e), order="F")
        self._chk(self._lib.hank_backward_step(self._ctx, _p(v), _p(x), _p(vo), _p(po)))
        return vo, po

    def backward_step_dual(self, value_next, dvalue_next, xhh_t, dxhh_t):
        dv = np.asarray(dvalue_next, dtype=np.float64)
        N = dv.shape[-1]
        v = _f(value_next, (self.n_a, self.n_e))
        dv = _f(dv, (self.n_a, self.n_e, N))
        x = _f(xhh_t, (self.n_hh,))
        dx = _f(dxhh_t, (self.n_hh, N))
        vo = np.empty((self.n_a, self.n_e), order="F")
        po = np.empty((self.n_a, self.n_e), order="F")
        dvo = np.empty((self.n_a, self.n_e, N), order="F")
        dpo = np.empty((self.n_a, self.n_e, N), order="F")
        self._chk(self._lib.hank_backward_step_dual(self._ctx, _p(v), _p(dv), _p(x), _p(dx), N,
                                                    _p(vo), _p(dvo), _p(po), _p(dpo)))
        return vo, dvo, po, dpo

    def forward_step(self, policy, D_prev):
        p = _f(policy, (self.n_a, self.n_e))
        d = _f(np.asarray(D_prev, dtype=np.float64).reshape((self.n_a, self.n_e), order="F"))
        do = np.empty((self.n_a, self.n_e), order="F")
        agg = C.c_double()
        self._chk(self._lib.hank_forward_step(self._ctx, _p(p), _p(d), _p(do), C.byref(agg)))
        return do, agg.value

    def forward_step_dual(self, policy, dpolicy, D_prev, dD_prev):
        dp_ = np.asarray(dpolicy, dtype=np.float64)
        N = dp_.shape[-1]
        p = _f(policy, (self.n_a, self.n_e))
        dp_ = _f(dp_, (self.n_a, self.n_e, N))
        d = _f(np.asarray(D_prev, dtype=np.float64).reshape((self.n_a, self.n_e), order="F"))
        dd = _f(np.asarray(dD_prev, dtype=np.float64).reshape((self.n_a, self.n_e, N), order="F"))
        do = np.empty((self.n_a, self.n_e), order="F")
        ddo = np.empty((self.n_a, self.n_e, N), order="F")
        agg = C.c_double()
        dagg = np.empty(N)
        self._chk(self._lib.hank_forward_step_dual(self._ctx, _p(p), _p(dp_), _p(d), _p(dd), N,
                                                   _p(do), _p(ddo), C.byref(agg), _p(dagg)))
        return do, ddo, agg.value, dagg
