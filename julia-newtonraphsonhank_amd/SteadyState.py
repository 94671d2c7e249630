"""Steady-state solver — host-side Python mirror of SteadyState.jl (north star: stays on the host).

It manufactures the boundary inputs of the GPU hot path: `ss.value` (terminal marginal value),
`ss.D` (initial distribution) and `ss.vars`. Algorithm as in the reference: Newton on the free
endogenous prices (find_ss, SteadyState.jl:184-233) around an inner VFI on the value function
(get_xVals, :111-154) and the stationary distribution by sparse linear solve
(invariant_dist, ForwardIteration.jl:436-442). The price Jacobian is taken by forward differences
instead of ForwardDiff.jacobian — only the fixed point matters.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Tuple

import numpy as np
import scipy.sparse as sp

from .Aggregation import Residuals
from .ForwardIteration import make_endogenous_transition
from .GeneralStructures import SequenceModel, invariant_dist, var_names, vars_of_type
from ._threads import host_algebra


@dataclass
class SteadyState:
    """SteadyState.jl:21-27."""
    vars: Dict[str, float]
    policies: Dict[str, np.ndarray]
    Λ: sp.csc_matrix
    D: np.ndarray
    value: np.ndarray


class SSAssembler:
    """variable roles + padded-matrix assembly for the steady-state Newton solve (SteadyState.jl:55-93)."""

    def __init__(self, model: SequenceModel, ss_spec, vfi_tol: float | None = None, vfi: str = "auto"):
        """`vfi`: where the inner value-function fixed point runs — "device" (hank_vfi: the EGM step kernels of the hot
        path iterated on the GPU), "host" (numpy), or "auto" = the device when an MI355X is present. Everything else of
        the steady state (price Newton, lottery matrix, invariant_dist) is host work either way (north star)."""
        self.model, self.ss_spec = model, ss_spec
        if vfi not in ("auto", "device", "host"):
            raise ValueError(f"vfi must be 'auto', 'device' or 'host' (got {vfi!r})")
        from .hip import device_available
        self.vfi_on_device = vfi == "device" or (vfi == "auto" and device_available())
        if vfi == "auto" and self.vfi_on_device:
            # a model the device block cannot take (more than one exogenous dimension, a grid it refuses) keeps the host
            # loop, which handles it through the kron of the transitions. Errors of the device sweeps themselves
            # (KnotsNotSorted / DomainError at a price iterate) surface from F(p) as they do on the host.
            from .BackwardIteration import household_block
            from .hip import HANK_ERR_BAD_ARG, HANK_ERR_NO_DEVICE, HankHIPError
            try:
                household_block(model)
            except ValueError:
                self.vfi_on_device = False
            except HankHIPError as e:
                # only "this model / this machine cannot": a device fault (out of memory, a refused launch, a failed sweep)
                # must not turn into a silent hundredfold slowdown on the host loop
                if e.code not in (HANK_ERR_BAD_ARG, HANK_ERR_NO_DEVICE):
                    raise
                self.vfi_on_device = False
        self.vfi_steps = 0
        self.all_keys = var_names(model)
        self.free_keys = tuple(k for k in vars_of_type(model, "endogenous") if k not in ss_spec.fixed)
        self.n_free = len(self.free_keys)
        endog = [d for d in model.heterogeneity.values() if d.dim_type == "endogenous"]
        exog = [d for d in model.heterogeneity.values() if d.dim_type == "exogenous"]
        if len(endog) != 1:
            raise ValueError("SSAssembler: exactly one endogenous heterogeneity dimension is currently supported")
        self.endog_dim = endog[0]
        self.n_exog = int(np.prod([d.n for d in exog])) if exog else 1
        Λ_exog = sp.identity(self.endog_dim.n, format="csc")
        for d in exog:
            Λ_exog = sp.kron(sp.csc_matrix(d.transition.T), Λ_exog, format="csc")
        self.Λ_exog = Λ_exog
        # the reference stops the VFI at compspec.ε; a tighter default makes ss.value a clean fixed point
        self.vfi_tol = vfi_tol if vfi_tol is not None else min(model.compspec.ε, 1e-11)
        self._value_warm = None
        self._last_xvals, self._last_p = None, None

    def get_xVals(self, p_vec) -> Tuple[np.ndarray, np.ndarray, dict]:
        """full length-n_v aggregate vector for price iterate p_vec + converged marginal value
        (SteadyState.jl:111-154). VFI starts from ones (:132) or from the last converged value."""
        model = self.model
        xv = {k: 0.0 for k in self.all_keys}
        for i, k in enumerate(self.free_keys):
            xv[k] = float(p_vec[i])
        for k, v in self.ss_spec.fixed.items():
            xv[k] = float(v)
        vf = model.value_fn
        value = self._value_warm if self._value_warm is not None else np.ones((self.endog_dim.n, self.n_exog))
        if self.vfi_on_device:
            from .BackwardIteration import household_block
            from .hip import DomainError, KnotsNotSortedError
            hb = household_block(model)
            try:
                v, pol, steps, _ = hb.vfi(value, [xv[k] for k in vf.household_inputs], self.vfi_tol, 10_000)
            except (KnotsNotSortedError, DomainError) as e:      # what the host step raises / turns non-finite: find_ss halves the step
                raise ValueError(str(e)) from e
            self.vfi_steps += steps
            res = {"Value": v, self.endog_dim.policy_var: pol}
            for k in vars_of_type(model, "heterogeneous"):
                if k not in res:
                    res[k] = vf.derived_policy(k, pol, xv, model)
        else:
            res = vf.host_steady_state_step(value, xv, model)
            for _ in range(10_000):
                value_new = res["Value"]
                tol = np.max(np.abs(value_new - value))
                value = value_new
                self.vfi_steps += 1
                if tol < self.vfi_tol:
                    break
                res = vf.host_steady_state_step(value, xv, model)
            pol = res[self.endog_dim.policy_var]
            for k in vars_of_type(model, "heterogeneous"):
                if k not in res:          # (keys the host step does not return, UCE: from the policy, as on the device branch)
                    res[k] = vf.derived_policy(k, pol, xv, model)
        if self.vfi_on_device and self.endog_dim.n * self.n_exog > 4000:
            # chains this large take the power method on the host too (invariant_dist): the same iteration, run with the
            # forward step kernel of the hot path, warm-started from the last iterate
            D, _ = hb.stationary_dist(res[self.endog_dim.policy_var], getattr(self, "_D_warm", None))
        else:
            Λ_endog = make_endogenous_transition(res[self.endog_dim.policy_var], self.endog_dim, self.n_exog)
            D = invariant_dist((self.Λ_exog @ Λ_endog).T, D0=getattr(self, "_D_warm", None))
        self._D_warm = D
        for k in vars_of_type(model, "heterogeneous"):
            xv[k] = float(res[k].reshape(-1, order="F") @ D)
        out = np.array([xv[k] for k in self.all_keys]), res["Value"], res
        self._last_xvals, self._last_p = out, np.array(p_vec, dtype=np.float64, copy=True)      # (implicit_price_jacobian reads them)
        return out

    def __call__(self, p_vec) -> np.ndarray:
        cs = self.model.compspec
        T_pad = 1 + cs.max_lag + cs.max_lead
        xVals, value, _ = self.get_xVals(p_vec)
        self._last_value = value
        return np.tile(xVals[:, None], (1, T_pad))

    def batch(self, p_mat):
        """`get_xVals` for K price vectors through one hank_ss_batch per 64 of them: p_mat (n_free, K) -> (xVals (n_v, K), values
        (n_a, n_e, K), policies (n_a, n_e, K), status (K,) int32). The value loops, the lotteries, the power methods and the
        aggregation of every heterogeneous key (output `vf.outputs.index(key)` of the device) run on the device for all K at once,
        warm-started from `_value_warm` / `_D_warm` when present. A column the device refuses, or whose 1 + r is not positive,
        has a non-zero status and unspecified values. The assembler's own warm state and `_last_xvals` stay as they were (the
        normalised distributions of the call are at `last_batch_D`, (G, K), its step counts at `last_batch_iters`, (K, 2)). Device
        VFI only."""
        if not self.vfi_on_device:
            raise ValueError("SSAssembler.batch needs the device VFI (hank_ss_batch): there is no host form of it")
        from .BackwardIteration import ensure_het_outputs, het_output_count, household_block
        from .hip import HANK_ERR_DOMAIN
        model = self.model
        vf = model.value_fn
        P = np.asarray(p_mat, dtype=np.float64)
        if P.ndim == 1:
            P = P[:, None]
        K = P.shape[1]
        het_keys = vars_of_type(model, "heterogeneous")
        outs = tuple(vf.outputs)
        missing = [k for k in het_keys if k not in outs]
        if missing:
            raise ValueError(f"SSAssembler.batch: the device block does not serve the heterogeneous variables {missing}")
        hb = household_block(model)
        n_out = het_output_count(model, het_keys)
        ensure_het_outputs(hb, n_out)
        xv = {k: np.zeros(K) for k in self.all_keys}
        for i, k in enumerate(self.free_keys):
            xv[k] = P[i].copy()
        for k, v in self.ss_spec.fixed.items():
            xv[k] = np.full(K, float(v))
        xhh = np.stack([xv[k] for k in vf.household_inputs], axis=0)                  # (n_hh, K)
        ok = 1.0 + xhh[0] > 0.0 if vf.household_inputs[0] == "r" else np.ones(K, dtype=bool)
        n_a, n_e = self.endog_dim.n, self.n_exog
        values, policies = np.ones((n_a, n_e, K), order="F"), np.zeros((n_a, n_e, K), order="F")
        D = np.zeros((n_a * n_e, K), order="F")
        aggs = np.zeros((n_out, K))
        status = np.where(ok, 0, HANK_ERR_DOMAIN).astype(np.int32)
        iters_all = np.zeros((K, 2), dtype=np.int32)
        cols = np.flatnonzero(ok)
        for c0 in range(0, len(cols), 64):                   # (the library takes up to 64 scenarios per call)
            cc = cols[c0:c0 + 64]
            a, v, pol, d, iters, st = hb.ss_batch(xhh[:, cc], self.vfi_tol, n_het=n_out, value0=self._value_warm,
                                                  D0=getattr(self, "_D_warm", None), check=False)
            aggs[:, cc], values[:, :, cc], policies[:, :, cc], D[:, cc], status[cc], iters_all[cc] = a, v, pol, d, st, iters
            self.vfi_steps += int(iters[:, 0].sum())
        for k in het_keys:
            xv[k] = aggs[outs.index(k)]
        self.last_batch_D, self.last_batch_iters = D, iters_all
        return np.stack([xv[k] for k in self.all_keys], axis=0), values, policies, status


def implicit_price_jacobian(asm: SSAssembler, p_vec) -> np.ndarray:
    """dF/dp at the price iterate whose steady state `asm` has just solved (its last get_xVals), without another fixed point:
    what ForwardDiff.jacobian(F, p) (SteadyState.jl:195) carries through the VFI (:132-141) and invariant_dist
    (ForwardIteration.jl:446-530). One hank_primal at the constant path with the iterate's (V, D) as both boundaries, one
    hank_ss_jvp over the free household inputs (d aggregates / d prices through V and D), composed with the residual layer's own
    partials — central differences of `Residuals` alone, which is closed-form host code."""
    from .BackwardIteration import ensure_het_outputs, het_output_count, household_block
    model = asm.model
    vf = model.value_fn
    het_keys = vars_of_type(model, "heterogeneous")
    outs = tuple(vf.outputs)
    missing = [k for k in het_keys if k not in outs]
    if missing:
        raise ValueError(f"price_jacobian='implicit': the device block does not serve the heterogeneous variables {missing}")
    xVals, value, _ = asm._last_xvals
    xv = dict(zip(asm.all_keys, xVals))
    hb = household_block(model)
    n_out = het_output_count(model, het_keys)
    ensure_het_outputs(hb, n_out)
    hb.set_boundary(value, asm._D_warm)
    hb.primal(np.tile(np.array([xv[k] for k in vf.household_inputs])[:, None], (1, hb.P)))
    dx = np.zeros((hb.n_hh, asm.n_free))
    for k, name in enumerate(vf.household_inputs):
        if name in asm.free_keys:
            dx[k, asm.free_keys.index(name)] = 1.0
    dagg = hb.ss_jvp(dx, n_het=n_out)[0]                              # (n_out, n_free)
    n_v = len(asm.all_keys)
    dX = np.zeros((n_v, asm.n_free))                                  # d xVals / d p
    for i, k in enumerate(asm.all_keys):
        if k in asm.free_keys:
            dX[i, asm.free_keys.index(k)] = 1.0
        elif k in het_keys:
            dX[i] = dagg[outs.index(k)]
    cs = model.compspec
    T_pad = 1 + cs.max_lag + cs.max_lead
    X = np.tile(np.asarray(xVals, dtype=np.float64)[:, None], (1, T_pad))
    R = []
    for i in range(n_v):
        h = 1e-6 * max(1.0, abs(xVals[i]))
        Xp, Xm = X.copy(), X.copy()
        Xp[i] += h
        Xm[i] -= h
        R.append((Residuals(Xp, model) - Residuals(Xm, model)) / (2 * h))
    return np.stack(R, axis=1) @ dX


def _residuals_batch(asm: SSAssembler, p_mat):
    """(residuals (n_res, K), values (n_a, n_e, K), D (G, K)) of `asm.batch(p_mat)`; a failed scenario's column is inf"""
    xVals, values, _, status = asm.batch(p_mat)
    cs = asm.model.compspec
    T_pad = 1 + cs.max_lag + cs.max_lead
    out = None
    for k in range(xVals.shape[1]):
        if status[k] != 0:
            continue
        z = np.asarray(Residuals(np.tile(xVals[:, k][:, None], (1, T_pad)), asm.model), dtype=np.float64)
        if out is None:
            out = np.full((len(z), xVals.shape[1]), np.inf)
        out[:, k] = z
    if out is None:
        out = np.full((asm.n_free, xVals.shape[1]), np.inf)
    return out, values, asm.last_batch_D


def residuals_batch(asm: SSAssembler, p_mat) -> np.ndarray:
    """F(p) = Residuals(asm(p)) at K price vectors at once: p_mat (n_free, K) -> (n_res, K), the household side of every column in
    one hank_ss_batch (`SSAssembler.batch`), the residual layer per column on the host. A column the device refuses, or whose
    1 + r is not positive, comes back as a column of inf, as `NewtonRaphson.residuals_batch` does."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return _residuals_batch(asm, p_mat)[0]


def first_acceptable(norms, z_norm):
    """the step-halving rule of find_ss on a batch of trials: the first j whose residual norm is finite and <= z_norm (the trial the
    sequential loop would have stopped at), or None when no trial is acceptable. inf and nan entries are skipped."""
    for j, nj in enumerate(norms):
        if np.isfinite(nj) and nj <= z_norm:
            return j
    return None


@host_algebra
def find_ss(model: SequenceModel, ss_spec, label: str, verbose: bool = False, vfi_tol=None, vfi: str = "auto",
            price_jacobian: str = "fd", batch: bool = False) -> SteadyState:
    """Newton–Raphson on the free endogenous variables with step halving (SteadyState.jl:184-233). price_jacobian: "fd" — forward
    differences, one more steady state per free price — or "implicit" — the derivatives through the steady state from the device
    (`implicit_price_jacobian`: no further fixed point; needs the device VFI, no fallback). batch=True (device VFI only): the
    forward-difference columns of an iterate run as ONE hank_ss_batch, and so do its trials p - 2^-j step, j = 0..5, of which the
    first acceptable one is taken — the sequential rule's choice; when none is, the halving goes on one trial at a time."""
    from .NewtonRaphson import warm_linear_solver
    from .GeneralStructures import vars_of_type
    if price_jacobian not in ("fd", "implicit"):
        raise ValueError(f"price_jacobian must be 'fd' or 'implicit' (got {price_jacobian!r})")
    warm_linear_solver(len(vars_of_type(model, "endogenous")) * (model.compspec.T - 1))      # (library start-up behind this solve)
    asm = SSAssembler(model, ss_spec, vfi_tol, vfi)
    if price_jacobian == "implicit" and not asm.vfi_on_device:
        raise ValueError("price_jacobian='implicit' needs the device (hank_ss_jvp at the record of hank_primal) and the device VFI: "
                         "there is no host form of it" + (" (vfi='host' was asked for)" if vfi == "host" else ""))
    if batch and not asm.vfi_on_device:
        raise ValueError("batch=True needs the device VFI (hank_ss_batch runs the value loops of all trials on the device): "
                         "there is no host form of it" + (" (vfi='host' was asked for)" if vfi == "host" else ""))
    asm.newton_iterations = 0
    batches = 0

    def F(p):
        return Residuals(asm(p), model)

    def safe_eval(q):
        try:
            z = F(q)
            return z if np.all(np.isfinite(z)) else np.full(len(z), np.inf)
        except (ValueError, FloatingPointError):
            return np.full(asm.n_free, np.inf)

    p = np.array([ss_spec.guesses.get(k, 1.0) for k in asm.free_keys], dtype=np.float64)
    ε = model.compspec.ε
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        z = F(p)
        it, max_iter = 0, 100
        while np.linalg.norm(z) > ε and it < max_iter:
            if verbose:
                print(f"  [{label}] Iteration {it}: residual norm = {np.linalg.norm(z)}")
            asm._value_warm = getattr(asm, "_last_value", None)   # warm-start the inner VFI
            J = np.empty((len(z), asm.n_free))
            if price_jacobian == "implicit":
                if asm._last_p is None or not np.array_equal(asm._last_p, p):      # (a halved step's last evaluation was refused)
                    F(p)
                J = implicit_price_jacobian(asm, p)
            elif batch:
                h = 1e-6 * np.maximum(1.0, np.abs(p))
                Zq = _residuals_batch(asm, p[:, None] + np.diag(h))[0]
                batches += 1
                if not np.all(np.isfinite(Zq)):
                    raise ValueError(f"find_ss [{label}]: a forward-difference column of the batch has no finite residual")
                J = (Zq - z[:, None]) / h[None, :]
            else:
                for j in range(asm.n_free):
                    h = 1e-6 * max(1.0, abs(p[j]))
                    q = p.copy()
                    q[j] += h
                    J[:, j] = (F(q) - z) / h
            step = np.linalg.solve(J, z)
            η, z_norm = 1.0, np.linalg.norm(z)
            if batch:
                etas = 0.5 ** np.arange(6)
                P_try = p[:, None] - step[:, None] * etas[None, :]
                Zt, Vt, Dt = _residuals_batch(asm, P_try)
                batches += 1
                j = first_acceptable([np.linalg.norm(Zt[:, q]) for q in range(6)], z_norm)
                if j is None:                       # the sequential halving goes on from j = 6
                    η, p_new, z_new = etas[5], P_try[:, 5], np.full(len(z), np.inf)
                else:                               # the accepted trial's fixed point warm-starts the next iterate's
                    η, p_new, z_new = etas[j], P_try[:, j], Zt[:, j]
                    asm._last_value, asm._D_warm = Vt[:, :, j], Dt[:, j]
            else:
                p_new = p - η * step
                z_new = safe_eval(p_new)
            while (not np.isfinite(np.linalg.norm(z_new))) or np.linalg.norm(z_new) > z_norm:
                η /= 2
                if not η > 1e-8:
                    break
                p_new = p - η * step
                z_new = safe_eval(p_new)
            p, z = p_new, z_new
            it += 1
            asm.newton_iterations = it
    if it == max_iter:
        import warnings
        warnings.warn(f"find_ss [{label}]: did not converge in {max_iter} iterations (residual norm: {np.linalg.norm(z)})")
    asm._value_warm = getattr(asm, "_last_value", None)
    xVals, ss_value, _ = asm.get_xVals(p)
    vars_ = {k: float(v) for k, v in zip(asm.all_keys, xVals)}
    # one more value-function call at the converged value for clean policies (:222-225)
    if asm.vfi_on_device:
        from .BackwardIteration import household_block
        _, pol = household_block(model).backward_step(ss_value, [vars_[k] for k in model.value_fn.household_inputs])
        res = {asm.endog_dim.policy_var: pol, "Value": ss_value}       # (the converged value IS the Value key)
        for k in vars_of_type(model, "heterogeneous"):
            if k not in res:
                res[k] = model.value_fn.derived_policy(k, pol, vars_, model)
    else:
        res = model.value_fn.host_steady_state_step(ss_value, vars_, model)
        for k in vars_of_type(model, "heterogeneous"):
            if k not in res:
                res[k] = model.value_fn.derived_policy(k, res[asm.endog_dim.policy_var], vars_, model)
    het_keys = vars_of_type(model, "heterogeneous")
    policies = {k: res[k] for k in het_keys}
    Λ_endog = make_endogenous_transition(policies[asm.endog_dim.policy_var], asm.endog_dim, asm.n_exog)
    Λss = (asm.Λ_exog @ Λ_endog).tocsc()
    if asm.vfi_on_device and asm.endog_dim.n * asm.n_exog > 4000:
        from .BackwardIteration import household_block
        D, _ = household_block(model).stationary_dist(policies[asm.endog_dim.policy_var], getattr(asm, "_D_warm", None))
    else:
        D = invariant_dist(Λss.T, D0=getattr(asm, "_D_warm", None))
    ss = SteadyState(vars_, policies, Λss, D, ss_value)
    # how the solve went (scripts and tests compare the two price Jacobians): the assembler's counters at the end
    ss.solve_info = {"price_jacobian": price_jacobian, "vfi_steps": asm.vfi_steps, "newton_iterations": asm.newton_iterations,
                     "residual_norm": float(np.linalg.norm(z)), "batches": batches}
    return ss


def get_SteadyStates(model: SequenceModel, verbose: bool = False, vfi_tol=None, vfi: str = "auto", price_jacobian: str = "fd", batch: bool = False):
    """both steady states (SteadyState.jl:245-259); one solve when the specs are the same object. price_jacobian, batch: see find_ss."""
    ss_initial = find_ss(model, model.ss_initial, "initial", verbose, vfi_tol, vfi, price_jacobian, batch)
    if model.ss_initial is model.ss_ending:
        return ss_initial, ss_initial
    return ss_initial, find_ss(model, model.ss_ending, "ending", verbose, vfi_tol, vfi, price_jacobian, batch)
