"""ctypes harness of the CPU oracle (oracle/hank_oracle.c) — TEST INFRASTRUCTURE ONLY.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg import this module; the
product package never does (tests/test_layout.py enforces it).

Duals are numpy arrays with a trailing axis of length 1+N: [..., 0] = value, [..., 1:] = partials
(the AoS layout of ForwardDiff's Dual{T,Float64,N}).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np

_DIR = Path(__file__).resolve().parent
_LIB = _DIR / "libhank_oracle.so"
_REF = _DIR / "_ref" / "libref_cppdual.so"
SUPPORTED_N = (1, 2, 3, 4, 8, 16, 32)

ORC_OK, ORC_ERR_KNOTS, ORC_ERR_DOMAIN = 0, 3, 4


class orc_model(C.Structure):
    _fields_ = [("n_a", C.c_int32), ("n_e", C.c_int32), ("a", C.POINTER(C.c_double)),
                ("z", C.POINTER(C.c_double)), ("Pi", C.POINTER(C.c_double)),
                ("beta", C.c_double), ("gamma", C.c_double), ("borrow_cons", C.c_double)]


def _reference_present() -> bool:
    """the reference's C++ sources are readable here (a user who may not enter their parent directory has none)."""
    ref = Path("/root/reference/ForwardDiff.jl/benchmarks/cpp")
    try:
        return ref.is_dir() and os.access(ref, os.R_OK | os.X_OK)
    except OSError:
        return False


def build(force: bool = False) -> None:
    """compile the oracle (and oracle/_ref when /root/reference is present) with make."""
    if force or not _LIB.exists() or _LIB.stat().st_mtime < (_DIR / "hank_oracle.c").stat().st_mtime:
        subprocess.run(["make", "-C", str(_DIR), "libhank_oracle.so"], check=True, capture_output=True)
    if _reference_present() and (force or not _REF.exists()):
        subprocess.run(["make", "-C", str(_DIR), "ref"], check=True, capture_output=True)


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not _LIB.exists():
            build()
        _lib = C.CDLL(str(_LIB))
    return _lib


def ref_lib() -> C.CDLL | None:
    """the reference's own C++ dual classes (oracle/_ref), or None when it was never built."""
    return C.CDLL(str(_REF)) if _REF.exists() else None


def _dp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _fn(name: str, N: int):
    if N not in SUPPORTED_N:
        raise ValueError(f"oracle compiled for N in {SUPPORTED_N}, got {N}")
    f = getattr(lib(), f"{name}_n{N}")
    return f


def pad_N(N: int) -> int:
    """smallest compiled partial count >= N (extra partials are carried as zeros)."""
    for n in SUPPORTED_N:
        if n >= N:
            return n
    raise ValueError(f"N={N} exceeds the oracle's largest compiled chunk {SUPPORTED_N[-1]}")


def _ok(st: int) -> None:
    if st != ORC_OK:
        raise RuntimeError(f"oracle status {st}")


def _cat(parts, axis):
    """the passes' partials side by side (a single pass as it is: no copy of a full-size policy sequence)."""
    return parts[0] if len(parts) == 1 else np.concatenate(parts, axis=axis)


class Oracle:
    """CPU restatement of the household block + KS residuals for one model."""

    def __init__(self, a_grid, z_grid, Pi, beta, gamma, borrow_cons):
        self.a = np.ascontiguousarray(a_grid, dtype=np.float64)
        self.z = np.ascontiguousarray(z_grid, dtype=np.float64)
        self.Pi = np.asfortranarray(np.asarray(Pi, dtype=np.float64))
        self.n_a, self.n_e = self.a.size, self.z.size
        self.G = self.n_a * self.n_e
        self.m = orc_model(self.n_a, self.n_e, _dp(self.a), _dp(self.z), _dp(self.Pi),
                           float(beta), float(gamma), float(borrow_cons))

    # duals: (n_a, n_e, 1+N) logically; memory = [e][a][1+N] (column-major matrix of AoS duals)
    def _mat_to_mem(self, M: np.ndarray, N: int) -> np.ndarray:
        M = np.asarray(M, dtype=np.float64)
        if M.ndim == 2:
            M = np.concatenate([M[..., None], np.zeros(M.shape + (N,))], axis=-1)
        assert M.shape == (self.n_a, self.n_e, 1 + N), M.shape
        return np.ascontiguousarray(M.transpose(1, 0, 2))

    def _mem_to_mat(self, mem: np.ndarray, N: int) -> np.ndarray:
        return mem.reshape(self.n_e, self.n_a, 1 + N).transpose(1, 0, 2).copy()

    @staticmethod
    def _scalar(x, N: int) -> np.ndarray:
        x = np.atleast_1d(np.asarray(x, dtype=np.float64))
        out = np.zeros(1 + N)
        out[: x.size] = x
        return out

    def value_function(self, value_next, r, w, N: int, tr=None):
        """ValueFunction (KrusellSmith.jl:43-83). Returns (status, Value, KD) as (n_a,n_e,1+N).
        `tr` (a dual, like r and w): the lump-sum transfer of the one-asset HANK family (not in the reference)."""
        vin = self._mat_to_mem(value_next, N)
        V = np.empty_like(vin)
        KD = np.empty_like(vin)
        if tr is None:
            f = _fn("orc_value_function", N)
            f.restype = C.c_int
            st = f(C.byref(self.m), _dp(vin), _dp(self._scalar(r, N)), _dp(self._scalar(w, N)), _dp(V), _dp(KD))
        else:
            f = _fn("orc_value_function_tr", N)
            f.restype = C.c_int
            st = f(C.byref(self.m), _dp(vin), _dp(self._scalar(r, N)), _dp(self._scalar(w, N)), _dp(self._scalar(tr, N)), _dp(V), _dp(KD))
        return st, self._mem_to_mat(V, N), self._mem_to_mat(KD, N)

    def backward_iteration(self, xr, xw, ss_end_value, N: int, xt=None):
        """BackwardIteration (BackwardIteration.jl:46-116). xr/xw: (P,1+N). -> (status, (P,n_a,n_e,1+N)).
        `xt` (P,1+N): the transfer path of the one-asset HANK family."""
        xr = np.ascontiguousarray(xr, dtype=np.float64)
        xw = np.ascontiguousarray(xw, dtype=np.float64)
        P = xr.shape[0]
        assert xr.shape == (P, 1 + N) and xw.shape == (P, 1 + N)
        vT = np.ascontiguousarray(np.asarray(ss_end_value, dtype=np.float64).T)  # [e][a]
        pol = np.empty((P, self.n_e, self.n_a, 1 + N))
        if xt is None:
            f = _fn("orc_backward_iteration", N)
            f.restype = C.c_int
            st = f(C.byref(self.m), P, _dp(xr), _dp(xw), _dp(vT), _dp(pol))
        else:
            xt = np.ascontiguousarray(xt, dtype=np.float64)
            assert xt.shape == (P, 1 + N)
            f = _fn("orc_backward_iteration_tr", N)
            f.restype = C.c_int
            st = f(C.byref(self.m), P, _dp(xr), _dp(xw), _dp(xt), _dp(vT), _dp(pol))
        return st, pol.transpose(0, 2, 1, 3).copy()

    def _consumption(self, xr, xw, xt, ps, N: int) -> np.ndarray:
        """the c_grid of KrusellSmith.jl:79 as a policy, for the policy sequence ps in memory order [t][e][a][1+N]."""
        cons = np.empty_like(ps)
        xr, xw = np.ascontiguousarray(xr, dtype=np.float64), np.ascontiguousarray(xw, dtype=np.float64)
        xt = None if xt is None else np.ascontiguousarray(xt, dtype=np.float64)
        _fn("orc_consumption_policy", N)(C.byref(self.m), ps.shape[0], _dp(xr), _dp(xw), None if xt is None else _dp(xt), _dp(ps), _dp(cons))
        return cons

    def _aggregate(self, seqs, ss_init_D, N: int) -> np.ndarray:
        """each sequence of seqs ([t][e][a][1+N]) dotted with the same D_t (ForwardIteration.jl:303-307) -> (len(seqs), P, 1+N)."""
        seqs = np.ascontiguousarray(np.stack(seqs))
        D0 = np.ascontiguousarray(np.asarray(ss_init_D, dtype=np.float64).reshape((self.n_a, self.n_e), order="F").T)
        agg = np.empty(seqs.shape[:2] + (1 + N,))
        _fn("orc_forward_iteration_het", N)(C.byref(self.m), seqs.shape[1], seqs.shape[0], _dp(seqs), _dp(D0), _dp(agg))
        return agg

    def transition_step(self, policy, D_prev, N: int):
        """transition_step (ForwardIteration.jl:95-99). policy/D_prev: (n_a,n_e[,1+N])."""
        p = self._mat_to_mem(policy, N)
        d = self._mat_to_mem(np.asarray(D_prev).reshape((self.n_a, self.n_e) + np.asarray(D_prev).shape[2:], order="F")
                             if np.asarray(D_prev).ndim == 1 else D_prev, N)
        out = np.empty_like(p)
        _fn("orc_transition_step", N)(C.byref(self.m), _dp(p), _dp(d), _dp(out))
        return self._mem_to_mat(out, N)

    def forward_iteration(self, policy_seq, ss_init_D, N: int, return_D: bool = False):
        """ForwardIteration (ForwardIteration.jl:253-311). policy_seq: (P,n_a,n_e,1+N) -> agg (P,1+N)."""
        ps = np.ascontiguousarray(np.asarray(policy_seq, dtype=np.float64).transpose(0, 2, 1, 3))
        P = ps.shape[0]
        D0 = np.ascontiguousarray(np.asarray(ss_init_D, dtype=np.float64).reshape((self.n_a, self.n_e), order="F").T)
        agg = np.empty((P, 1 + N))
        Dseq = np.empty((P, self.n_e, self.n_a, 1 + N)) if return_D else None
        _fn("orc_forward_iteration", N)(C.byref(self.m), P, _dp(ps), _dp(D0), _dp(agg),
                                        _dp(Dseq) if return_D else None)
        if return_D:
            return agg, Dseq.transpose(0, 2, 1, 3).copy()
        return agg

    def household_block(self, xr, xw, ss_end_value, ss_init_D, N: int, xt=None):
        """ForwardIteration(BackwardIteration(...)) -> (status, agg (P,1+N), policy_seq)."""
        st, pol = self.backward_iteration(xr, xw, ss_end_value, N, xt)
        agg = self.forward_iteration(pol, ss_init_D, N)
        return st, agg, pol

    def household_block_het(self, xr, xw, ss_end_value, ss_init_D, N: int, xt=None):
        """the household block of a value function with TWO heterogeneous variables, savings and consumption (the c_grid of
        KrusellSmith.jl:79 returned as a policy): BackwardIteration keeps one policy sequence per variable
        (BackwardIteration.jl:99-112), ForwardIteration aggregates each with the same D_t (ForwardIteration.jl:303-307).
        -> (status, agg (2, P, 1+N), policy_seq, cons_seq)."""
        st, pol = self.backward_iteration(xr, xw, ss_end_value, N, xt)
        ps = np.ascontiguousarray(pol.transpose(0, 2, 1, 3))
        cons = self._consumption(xr, xw, xt, ps, N)
        return st, self._aggregate([ps, cons], ss_init_D, N), pol, cons.transpose(0, 2, 1, 3).copy()

    # ---- the references of the GPU suite: seeded, checked, partials split from the value ----
    @staticmethod
    def _seeded(xhh, y):
        """xhh (n_hh, P) with the partials y (n_hh, P, N), or None for the value alone -> per pass (n, Nc, xd): n partials in a
        dual xd (n_hh, P, 1 + Nc) of the compiled width Nc = pad_N(n); at most SUPPORTED_N[-1] partials per pass."""
        xhh = np.asarray(xhh, dtype=np.float64)
        N = 0 if y is None else y.shape[2]
        for c0 in range(0, max(N, 1), SUPPORTED_N[-1]):
            n = min(N, c0 + SUPPORTED_N[-1]) - c0
            xd = np.zeros(xhh.shape + (1 + pad_N(n),))
            xd[..., 0] = xhh
            if n:
                xd[..., 1:1 + n] = y[:, :, c0:c0 + n]
            yield n, xd.shape[2] - 1, xd

    def block(self, xhh, y, value, D):
        """household_block at xhh (n_hh, P) with the partials y (n_hh, P, N), or y=None for the value alone; row 2 of xhh / y is
        the transfer path when n_hh > 2. -> agg (P,), dagg (P, N), policy (P, n_a, n_e), dpolicy (P, n_a, n_e, N)."""
        dagg, dpol = [], []
        for n, Nc, xd in self._seeded(xhh, y):
            st, oa, op = self.household_block(xd[0], xd[1], value, D, Nc, xd[2] if len(xd) > 2 else None)
            _ok(st)
            agg, pol = oa[:, 0], op[..., 0]
            dagg.append(oa[:, 1:1 + n]); dpol.append(op[..., 1:1 + n])
        return agg, _cat(dagg, 1), pol, _cat(dpol, -1)

    def block_het(self, xhh, y, value, D):
        """`block` through household_block_het -> agg (2, P), dagg (2, P, N) of (savings, consumption)."""
        dagg = []
        for n, Nc, xd in self._seeded(xhh, y):
            st, oa, _, _ = self.household_block_het(xd[0], xd[1], value, D, Nc, xd[2] if len(xd) > 2 else None)
            _ok(st)
            agg = oa[..., 0]
            dagg.append(oa[..., 1:1 + n])
        return agg, _cat(dagg, 2)

    def het_outputs(self, xhh, y, value, D, n_het, gamma):
        """agg (n_het, P), dagg (n_het, P, N) of (savings, consumption, Value[, UCE]) under the dual arithmetic, one pass. The
        reference dots every key of the value function's NamedTuple with the same post-transition D_t (BackwardIteration.jl:99-112,
        ForwardIteration.jl:303-307): Value is the reference's ValueFunction itself, once per period backward
        (BackwardIteration.jl:90-113); UCE = z_e c^-γ of the one-asset HANK family, c^-γ and its partials by the chain rule."""
        (n, Nc, xd), = self._seeded(xhh, y)
        P, xt = xd.shape[1], xd[2] if len(xd) > 2 else None
        st, pol = self.backward_iteration(xd[0], xd[1], value, Nc, xt)
        _ok(st)
        V = np.empty((P, self.n_a, self.n_e, 1 + Nc))
        Vn = np.asarray(value, dtype=np.float64)
        for t in range(P - 1, -1, -1):
            st, Vt, KD = self.value_function(Vn, xd[0, t], xd[1, t], Nc, None if xt is None else xt[t])
            _ok(st)
            err = np.max(np.abs(KD - pol[t]))
            assert err <= 1e-12 + 1e-12 * np.abs(pol[t]).max(), f"period {t}: the policies of value_function and backward_iteration differ by {err:.3e}"
            V[t], Vn = Vt, Vt
        ps = np.ascontiguousarray(pol.transpose(0, 2, 1, 3))                       # [t][e][a][1+N]
        cons = self._consumption(xd[0], xd[1], xt, ps, Nc)
        seqs = [ps, cons, np.ascontiguousarray(V.transpose(0, 2, 1, 3))]
        if n_het > 3:
            c0 = cons[..., 0]
            u = np.empty_like(cons)
            u[..., 0] = c0 ** (-gamma)
            u[..., 1:] = (-gamma * c0 ** (-gamma - 1.0))[..., None] * cons[..., 1:]
            seqs.append(self.z[None, :, None, None] * u)
        agg = self._aggregate(seqs[:n_het], D, Nc)
        return agg[..., 0], agg[..., 1:1 + n]

    def vfi(self, shape, r, w, tol, cap=20_000):
        """the reference's inner fixed point (SteadyState.jl:132-141) on ValueFunction: value <- value_fn(value).Value from ones
        until max|new - old| < tol -> (value, policy, steps, per-step sup-norms)."""
        value, norms = np.ones(shape), []
        for k in range(1, cap + 1):
            st, V, KD = self.value_function(value, r, w, 1)
            _ok(st)
            norms.append(float(np.max(np.abs(V[..., 0] - value))))
            value = V[..., 0]
            if norms[-1] < tol:
                return value, KD[..., 0], k, norms
        raise RuntimeError(f"oracle VFI did not converge in {cap} steps")

    def ks_full_function(self, x, Z, alpha, delta, KS_ss_start, ss_end_value, ss_init_D, N: int):
        """fullFunction of y_Iteration for KrusellSmith.yaml (NewtonRaphson.jl:77-83).
        x: (4, P, 1+N) duals of (Y, KS, r, w). Returns (status, F (4,P,1+N), agg (P,1+N))."""
        x = np.asarray(x, dtype=np.float64)
        P = x.shape[1]
        assert x.shape == (4, P, 1 + N)
        xm = np.ascontiguousarray(x.transpose(1, 0, 2))  # [t][k][1+N] == column-major (4,P) of duals
        Z = np.ascontiguousarray(Z, dtype=np.float64)
        vT = np.ascontiguousarray(np.asarray(ss_end_value, dtype=np.float64).T)
        D0 = np.ascontiguousarray(np.asarray(ss_init_D, dtype=np.float64).reshape((self.n_a, self.n_e), order="F").T)
        out = np.empty((P, 4, 1 + N))
        agg = np.empty((P, 1 + N))
        f = _fn("orc_ks_full_function", N)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double),
                      C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                      C.POINTER(C.c_double)]
        st = f(C.cast(C.byref(self.m), C.c_void_p), P, float(alpha), float(delta), _dp(xm), _dp(Z),
               float(KS_ss_start), _dp(vT), _dp(D0), _dp(out), _dp(agg))
        return st, out.transpose(1, 0, 2).copy(), agg

    def ks_jvp(self, x, y, Z, alpha, delta, KS_ss_start, ss_end_value, ss_init_D):
        """JVP(fullFunction, x, y) for a batch of tangents y (4,P,N): seeds x + t*y exactly like
        GeneralStructures.jl:546-547 (one partial per direction). Returns (F (4P,), J·y (4P,N))."""
        y = np.asarray(y, dtype=np.float64)
        if y.ndim == 2:
            y = y[:, :, None]
        Nreq = y.shape[2]
        N = pad_N(Nreq)
        P = y.shape[1]
        xd = np.zeros((4, P, 1 + N))
        xd[..., 0] = np.asarray(x, dtype=np.float64).reshape(4, P, order="F") if np.asarray(x).ndim == 1 else x
        xd[..., 1:1 + Nreq] = y
        st, F, _ = self.ks_full_function(xd, Z, alpha, delta, KS_ss_start, ss_end_value, ss_init_D, N)
        _ok(st)
        Fv = F[..., 0].reshape(-1, order="F")
        J = F[..., 1:1 + Nreq].reshape(4 * P, Nreq, order="F")
        return Fv, J


def dual_binop(op: int, x, y, N: int) -> np.ndarray:
    out = np.empty(1 + N)
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    _fn("orc_dual_binop", N)(int(op), _dp(x), _dp(y), _dp(out))
    return out
