"""Newton–Raphson for the perfect-foresight path — Python mirror of NewtonRaphson.jl (Boehl 2021).

Same call surface (`NewtonRaphsonHANK(x_0, J̅, exog_paths, mod, ss_initial, ss_ending; ε)`,
`y_Iteration(...)`); the hot path inside `fullFunction` — BackwardIteration → ForwardIteration —
runs on the GPU. One difference in *cost*, not in results: the reference re-runs the whole primal
pipeline inside every JVP (NewtonRaphson.jl:95, GeneralStructures.jl:546-547); here the primal
sweep at x is recorded once by the Float64 call `fullFunction(x)` (:91) and every JVP of the inner
loop reuses that linearisation (hank_jvp).
"""
from __future__ import annotations

import numpy as np
import scipy.sparse.linalg as spla

from .Aggregation import Residuals
from .BackwardIteration import BackwardIteration, ensure_het_outputs, household_block, household_inputs
from .dual import Dual
from .ForwardIteration import ForwardIteration
from .GeneralStructures import JVP, SequenceModel, assemble_full_xMat, vars_of_type
from ._threads import host_algebra


def make_fullFunction(exog_paths, mod: SequenceModel, ss_initial, ss_ending):
    """the closure of y_Iteration (NewtonRaphson.jl:77-83)."""

    def fullFunction(x_Vec):
        policy_seqs = BackwardIteration(x_Vec, exog_paths, mod, ss_ending, ss_initial=ss_initial)
        agg_seqs = ForwardIteration(policy_seqs, mod, ss_initial)
        padded_xMat = assemble_full_xMat(x_Vec, agg_seqs, exog_paths, mod, ss_initial, ss_ending)
        return Residuals(padded_xMat, mod)

    # what `VJP(fullFunction, x, ȳ)` differentiates: the linearisation at x, which knows its transpose
    fullFunction.linearize = lambda x: LinearizedFunction(x, exog_paths, mod, ss_initial, ss_ending)
    return fullFunction


class LinearizedFunction:
    """F(x) evaluated once + cheap J(x)·y products at that fixed x (the y-iteration's access pattern,
    NewtonRaphson.jl:91-105). Tangent batches (n, N) go through ONE hank_jvp."""

    exact_residual_layer = False        # True: J(x)·y through the compiled equations under a Dual at every call (tests compare the two)
    het_in_sweep = False                # True: a model that reads Value / UCE (device outputs >= 2) takes every output's tangent from ONE
                                        # hank_jvp_het instead of hank_jvp + hank_get_het_outputs; the two differ by the rounding of sums

    def __init__(self, x, exog_paths, mod: SequenceModel, ss_initial, ss_ending, discount_path=None, income_path=None, borrow_path=None):
        """discount_path: beta_t (P,), the discount factor of period t's Euler equation (HouseholdBlock.set_discount_path; not in the
        reference, which reads beta from the model's parameters); None: the model's constant. The path is set on the model's
        context before the primal is recorded, and restored with the record when another user of the context changed it.
        income_path: y (n_e, P), additive income by productivity state (HouseholdBlock.set_income_path; not in the reference either),
        handled in the same way; a model that reads Value or UCE is not served at one.
        borrow_path: amin_t (P,), the borrowing limit of period t's choice (HouseholdBlock.set_borrow_path; not in the reference, which
        reads borrow_cons from the model's parameters), handled in the same way. The three exclude each other."""
        self.x = np.asarray(x, dtype=np.float64)
        self.discount_path = None if discount_path is None else np.ascontiguousarray(discount_path, dtype=np.float64)
        self.income_path = None if income_path is None else np.asfortranarray(income_path, dtype=np.float64)
        self.borrow_path = None if borrow_path is None else np.ascontiguousarray(borrow_path, dtype=np.float64)
        if self.discount_path is not None and self.income_path is not None:
            raise ValueError("discount_path and income_path exclude each other")
        if self.borrow_path is not None and (self.discount_path is not None or self.income_path is not None):
            raise ValueError("borrow_path excludes discount_path and income_path")
        self.mod, self.exog_paths, self.ss_initial, self.ss_ending = mod, exog_paths, ss_initial, ss_ending
        self.hb = household_block(mod)
        xhh, _ = household_inputs(self.x, exog_paths, mod)
        self._xhh = xhh
        het = vars_of_type(mod, "heterogeneous")
        self.het = het
        outs = tuple(mod.value_fn.outputs)
        self._out_idx = [outs.index(k) for k in het]        # device output of each heterogeneous variable (hank_get_het_outputs)
        self._n_out = 1 + max(self._out_idx)              # outputs the device serves: up to the last one listed (hank_set_het_outputs)
        if self.income_path is not None and self._n_out > 2:
            raise ValueError(f"income_path: the heterogeneous variables {het} reach {outs[self._n_out - 1]!r} (device output >= 2), which the "
                             "device rebuilds from the inputs: it is not served at an income path")
        self._record_primal()
        self._xMat = assemble_full_xMat(self.x, {k: self.aggs[:, j] for k, j in zip(het, self._out_idx)}, exog_paths, mod, ss_initial, ss_ending)
        self.Fx = Residuals(self._xMat, mod)
        self._Rx = self._Ragg = None        # the residual layer's linearisation at this x, built at the first jvp

    def _linearise_residuals(self):
        """∂R/∂x and ∂R/∂agg at this x as sparse maps, from ONE evaluation of the compiled equations under a Dual: x — and with
        it the residual layer's linearisation — is fixed for the whole y-iteration (NewtonRaphson.jl:91-111), so the ≈ 21 inner
        iterations need not re-seed a Dual and re-evaluate the equations under it each time (Aggregation.jl:20-22,
        GeneralStructures.jl:329-377: the padded matrix is a selection of x, the aggregates and constants). Direction
        (row r, colour k) perturbs variable r in every padded column c with c mod W == k; the W = 1 + max_lag + max_lead columns
        a period's equations read have distinct colours, so each direction is one entry of that period's Jacobian block."""
        import scipy.sparse as sp
        from .GeneralStructures import var_names
        mod, cs = self.mod, self.mod.compspec
        P, n_v, n_endog, max_lag, max_lead = cs.T - 1, cs.n_v, cs.n_endog, cs.max_lag, cs.max_lead
        W = 1 + max_lag + max_lead
        T_pad = P + max_lag + max_lead
        n_eq = len(mod.equations)
        xp = np.zeros((n_v, T_pad, n_v * W))
        cols = np.arange(T_pad)
        for r in range(n_v):
            xp[r, cols, r * W + cols % W] = 1.0
        res = Residuals(Dual(self._xMat, xp), mod)
        Pm = np.asarray(res.p).reshape(P, n_eq, n_v, W)                   # [t, q, r, colour]: rows are ordered q + n_eq t, directions r W + colour
        keys = var_names(mod)
        endog = {keys.index(k): j for j, k in enumerate(vars_of_type(mod, "endogenous"))}
        hetr = {keys.index(k): j for j, k in enumerate(self.het)}
        rx, cx, vx, ra, ca, va = [], [], [], [], [], []
        t = np.arange(P)
        for k in range(W):
            c = t + (k - t) % W                   # the padded column of colour k inside period t's window [t, t + W)
            s_ = c - max_lag                      # ... as a transition period (boundary columns are constants)
            ok = (s_ >= 0) & (s_ < P)
            for r in range(n_v):
                if r not in endog and r not in hetr:
                    continue                      # exogenous paths carry no tangent
                for q in range(n_eq):
                    v = Pm[:, q, r, k]
                    nz = ok & (v != 0.0)
                    if not nz.any():
                        continue
                    rows = q + n_eq * t[nz]
                    if r in endog:
                        rx.append(rows); cx.append(endog[r] + n_endog * s_[nz]); vx.append(v[nz])
                    else:
                        ra.append(rows); ca.append(hetr[r] * P + s_[nz]); va.append(v[nz])
        cat = lambda L, dt: np.concatenate(L) if L else np.zeros(0, dtype=dt)
        self._Rx = sp.csr_matrix((cat(vx, float), (cat(rx, int), cat(cx, int))), shape=(n_eq * P, n_endog * P))
        self._Ragg = sp.csr_matrix((cat(va, float), (cat(ra, int), cat(ca, int))), shape=(n_eq * P, len(self.het) * P))

    def _record_primal(self):
        """(re-)run the Float64 sweep at x on the model's device context and take ownership of its record: the
        context is shared by everything that touches this model, so the generation counter says whose primal
        it currently holds (BackwardIteration and other linearisations bump it too)."""
        hb = self.hb
        hb.set_boundary(self.ss_ending.value, self.ss_initial.D)
        differs = lambda cur, want: (cur is None) != (want is None) or (want is not None and not np.array_equal(cur, want))
        # (the context is shared: a linearisation without a path clears another's; the paths exclude each other, so what has to
        # go is cleared before what has to come is set)
        paths = [("discount_path", self.discount_path), ("income_path", self.income_path), ("borrow_path", self.borrow_path)]
        for name, want in sorted(paths, key=lambda q: q[1] is not None):
            if differs(getattr(hb, name, None), want):
                getattr(hb, "set_" + name)(want)
        self.agg = hb.primal(self._xhh)
        if self._n_out > 2:
            ensure_het_outputs(hb, self._n_out)
        self.aggs = self.agg[:, None] if self._n_out == 1 else hb.het_outputs(self._n_out)[0]      # (P, outputs)
        hb._generation = getattr(hb, "_generation", 0) + 1
        hb._last = None          # an older PolicySequences must not take ForwardIteration's fused shortcut
        self._generation = hb._generation

    def jvp(self, y, pad_to: int | None = None):
        """J(x)·y for one tangent (n,) or a batch (n, N). Directions that do not move the household inputs
        (unit tangents in Y or KS, say) are not sent to the GPU — their household partials are zero; `pad_to`
        rounds the device batch up to a multiple (zero columns) so that repeated calls reuse one workspace."""
        y = np.asarray(y, dtype=np.float64)
        single = y.ndim == 1
        xd = Dual.seed(self.x, y[:, None] if single else y)
        _, dxhh = household_inputs(xd, self.exog_paths, self.mod)
        dxhh = np.asarray(dxhh, dtype=np.float64)
        if dxhh.ndim == 2:
            dxhh = dxhh[:, :, None]
        N = dxhh.shape[2]
        nz = np.flatnonzero(np.any(dxhh != 0.0, axis=(0, 1)))
        dagg = np.zeros((dxhh.shape[1], N))
        daggs = dagg[:, None, :] if self._n_out == 1 else np.zeros((dxhh.shape[1], self._n_out, N))      # (P, outputs, N)
        if len(nz):
            if getattr(self.hb, "_generation", None) != self._generation:
                # another linearisation / BackwardIteration used the model's context since: its record is not
                # this x's any more — restore ours (bit-identical: same kernels, same inputs) instead of
                # silently returning J(x_other)·y
                self._record_primal()
            sub = dxhh[:, :, nz]
            if pad_to and len(nz) % pad_to:
                padded = np.zeros(sub.shape[:2] + (-(-len(nz) // pad_to) * pad_to,))
                padded[:, :, :len(nz)] = sub
                sub = padded
            in_sweep = self.het_in_sweep and self._n_out > 2
            if in_sweep:
                ensure_het_outputs(self.hb, self._n_out)
                daggs[:, :, nz] = self.hb.jvp_het(sub, n_het=self._n_out)[:, :, :len(nz)]
            else:
                dagg[:, nz] = self.hb.jvp(sub)[:, :len(nz)]
            if self._n_out > 1 and not in_sweep:
                if self._n_out > 2:
                    ensure_het_outputs(self.hb, self._n_out)
                daggs[:, :, nz] = self.hb.het_outputs(self._n_out, sub)[1][:, :, :len(nz)]
        if self.exact_residual_layer:           # the reference's way: re-evaluate the equations under the Dual every time
            agg = {k: Dual(self.aggs[:, j], np.ascontiguousarray(daggs[:, j, :])) for k, j in zip(self.het, self._out_idx)}
            res = Residuals(assemble_full_xMat(xd, agg, self.exog_paths, self.mod, self.ss_initial, self.ss_ending), self.mod)
            return res.p[:, 0].copy() if single else res.p.copy()
        if self._Rx is None:
            self._linearise_residuals()
        Y = y[:, None] if single else y
        out = self._Rx @ Y + self._Ragg @ np.concatenate([daggs[:, j, :] for j in self._out_idx], axis=0)     # rows: het variable, period
        return out[:, 0].copy() if single else out


    def vjp(self, ȳ):
        """J(x)ᵀ·ȳ for one cotangent (n,) or a batch (n, M): the transpose of `jvp`, layer by layer — `_Raggᵀ` (the residual
        layer's dependence on the aggregates) → ONE hank_vjp (the reverse rules of ForwardIteration.jl:339-420 and of the
        backward loop) → the transpose of `household_inputs` (a selection of rows of x) — plus `_Rxᵀ`. Cotangent columns that
        put no weight on any aggregate are not sent to the GPU."""
        if self._n_out > 2:
            raise NotImplementedError(
                f"LinearizedFunction.vjp: the heterogeneous variables {self.het} reach {self.mod.value_fn.outputs[self._n_out - 1]!r} "
                "(device output >= 2), which is not affine in the policy: hank_vjp carries cotangents on the policy variable and on consumption only "
                "(vjp_het carries them all)")
        return self._vjp(ȳ, False)

    def vjp_het(self, ȳ):
        """`vjp` for every model: the same layers, with ONE hank_vjp_het in the middle when the heterogeneous variables reach
        Value or UCE (device outputs >= 2, not affine in the policy). With at most two device outputs it goes through hank_vjp:
        the same bits as `vjp`."""
        return self._vjp(ȳ, self._n_out > 2)

    def _vjp(self, ȳ, het: bool):
        ȳ = np.asarray(ȳ, dtype=np.float64)
        single = ȳ.ndim == 1
        Yb = ȳ[:, None] if single else ȳ
        if self._Rx is None:
            self._linearise_residuals()
        cs = self.mod.compspec
        P, M = cs.T - 1, Yb.shape[1]
        out = np.asarray(self._Rx.T @ Yb)
        ab = np.asarray(self._Ragg.T @ Yb).reshape(len(self.het), P, M)          # rows: het variable, period
        agg_bar = np.zeros((P, self._n_out, M))
        for j, o in enumerate(self._out_idx):
            agg_bar[:, o, :] += ab[j]
        nz = np.flatnonzero(np.any(agg_bar != 0.0, axis=(0, 1)))
        if len(nz):
            if getattr(self.hb, "_generation", None) != self._generation:
                self._record_primal()           # (the same generation check as jvp: the context holds another x's record)
            if het:
                ensure_het_outputs(self.hb, self._n_out)
                xb = self.hb.vjp_het(agg_bar[:, :, nz], self._n_out)
            else:
                xb = self.hb.vjp(agg_bar[:, :, nz], self._n_out)                 # (n_hh, P, len(nz))
            endog_keys = vars_of_type(self.mod, "endogenous")
            for k, name in enumerate(self.mod.value_fn.household_inputs):
                if name in endog_keys:          # exogenous inputs carry no cotangent back to x; x is (n_endog, P) column-major
                    out[np.ix_(endog_keys.index(name) + cs.n_endog * np.arange(P), nz)] += xb[k]
        return out[:, 0].copy() if single else out

    def _own_record(self):
        if getattr(self.hb, "_generation", None) != self._generation:
            self._record_primal()               # (the same generation check as jvp: the context holds another x's record)
        if self._n_out > 2:
            ensure_het_outputs(self.hb, self._n_out)

    def jvp_boundary(self, dV=None, dD=None):
        """∂F/∂(V_P, D_0)·(dV, dD) at this x: the residuals' tangent under seeds on the terminal marginal value `ss_ending.value`
        (BackwardIteration.jl:85) and on the initial distribution `ss_initial.D` (ForwardIteration.jl:293), x held fixed. dV, dD:
        (n_a, n_e) or (n_a, n_e, N), either may be None (zeros). `_Ragg` composed with ONE boundary product of the block:
        hank_jvp_het when the heterogeneous variables reach Value or UCE, hank_jvp_boundary (+ hank_get_het_outputs) otherwise."""
        given = [np.asarray(v) for v in (dV, dD) if v is not None]
        if not given:
            raise ValueError("at least one of dV, dD must be given")
        single = given[0].ndim == 2
        if self._Rx is None:
            self._linearise_residuals()
        self._own_record()
        hb = self.hb
        N = 1 if single else given[0].shape[2]
        if self._n_out > 2:
            daggs = hb.jvp_het(None, dV, dD, n_het=self._n_out)
        else:
            d0 = hb.jvp_boundary(None, dV, dD)
            daggs = d0[:, None, :] if self._n_out == 1 else hb.het_outputs(2, np.zeros((hb.n_hh, hb.P, N)))[1]
        out = self._Ragg @ np.concatenate([daggs[:, j, :] for j in self._out_idx], axis=0)
        return out[:, 0].copy() if single else out

    def vjp_boundary(self, ȳ):
        """the transpose of `jvp_boundary`: ȳ (n,) or (n, M) -> (value_end_bar, D_init_bar), each (n_a, n_e) or (n_a, n_e, M) —
        the gradient of ȳ·F with respect to the ending steady state's marginal value and the initial distribution, from ONE pair
        of transposed sweeps (hank_vjp_het_boundary when Value or UCE are read, hank_vjp_boundary otherwise)."""
        ȳ = np.asarray(ȳ, dtype=np.float64)
        single = ȳ.ndim == 1
        Yb = ȳ[:, None] if single else ȳ
        if self._Rx is None:
            self._linearise_residuals()
        P, M = self.mod.compspec.T - 1, Yb.shape[1]
        ab = np.asarray(self._Ragg.T @ Yb).reshape(len(self.het), P, M)
        agg_bar = np.zeros((P, self._n_out, M))
        for j, o in enumerate(self._out_idx):
            agg_bar[:, o, :] += ab[j]
        self._own_record()
        if self._n_out > 2:
            _, vb, db = self.hb.vjp_het_boundary(agg_bar, self._n_out)
        else:
            _, vb, db = self.hb.vjp_boundary(agg_bar, self._n_out)
        return (vb[:, :, 0].copy(), db[:, :, 0].copy()) if single else (vb, db)

    def _shock_ready(self):
        if self._Rx is None:
            self._linearise_residuals()
        self._own_record()

    def jvp_shock(self, dbeta):
        """∂F/∂beta · dbeta at this x: the residuals' tangent under a direction dbeta (P,) or (P, N) of the discount-factor path, x
        held fixed — `_Ragg` composed with ONE hank_jvp_shock (+ hank_get_het_outputs: beta has no direct term in any output)."""
        db = np.asarray(dbeta, dtype=np.float64)
        single = db.ndim == 1
        db = db[:, None] if single else db
        self._shock_ready()
        hb = self.hb
        d0 = hb.jvp_shock(None, db)
        daggs = d0[:, None, :] if self._n_out == 1 else hb.het_outputs(self._n_out, np.zeros((hb.n_hh, hb.P, db.shape[1])))[1]
        out = self._Ragg @ np.concatenate([daggs[:, j, :] for j in self._out_idx], axis=0)
        return out[:, 0].copy() if single else out

    def vjp_shock(self, ȳ):
        """the transpose of `jvp_shock`: ȳ (n,) or (n, M) -> beta_bar (P,) or (P, M), the gradient of ȳ·F with respect to the
        discount-factor path, from ONE hank_vjp_shock."""
        ȳ = np.asarray(ȳ, dtype=np.float64)
        single = ȳ.ndim == 1
        Yb = ȳ[:, None] if single else ȳ
        self._shock_ready()
        P, M = self.mod.compspec.T - 1, Yb.shape[1]
        ab = np.asarray(self._Ragg.T @ Yb).reshape(len(self.het), P, M)
        agg_bar = np.zeros((P, self._n_out, M))
        for j, o in enumerate(self._out_idx):
            agg_bar[:, o, :] += ab[j]
        _, bb = self.hb.vjp_shock(agg_bar, self._n_out)
        return bb[:, 0].copy() if single else bb

    def jvp_borrow(self, damin):
        """∂F/∂amin · damin at this x: the residuals' tangent under a direction damin (P,) or (P, N) of the borrowing-limit path, x
        held fixed — `_Ragg` composed with ONE hank_jvp_borrow (+ hank_get_het_outputs: the limit has no direct term in any output)."""
        da = np.asarray(damin, dtype=np.float64)
        single = da.ndim == 1
        da = da[:, None] if single else da
        self._shock_ready()
        hb = self.hb
        d0 = hb.jvp_borrow(None, da)
        daggs = d0[:, None, :] if self._n_out == 1 else hb.het_outputs(self._n_out, np.zeros((hb.n_hh, hb.P, da.shape[1])))[1]
        out = self._Ragg @ np.concatenate([daggs[:, j, :] for j in self._out_idx], axis=0)
        return out[:, 0].copy() if single else out

    def vjp_borrow(self, ȳ):
        """the transpose of `jvp_borrow`: ȳ (n,) or (n, M) -> amin_bar (P,) or (P, M), the gradient of ȳ·F with respect to the
        borrowing-limit path, from ONE hank_vjp_borrow."""
        ȳ = np.asarray(ȳ, dtype=np.float64)
        single = ȳ.ndim == 1
        Yb = ȳ[:, None] if single else ȳ
        self._shock_ready()
        P, M = self.mod.compspec.T - 1, Yb.shape[1]
        ab = np.asarray(self._Ragg.T @ Yb).reshape(len(self.het), P, M)
        agg_bar = np.zeros((P, self._n_out, M))
        for j, o in enumerate(self._out_idx):
            agg_bar[:, o, :] += ab[j]
        _, bb = self.hb.vjp_borrow(agg_bar, self._n_out)
        return bb[:, 0].copy() if single else bb

    def jvp_income(self, dy):
        """∂F/∂y · dy at this x: the residuals' tangent under a direction dy (n_e, P) or (n_e, P, N) of the income path, x held fixed
        — `_Ragg` composed with ONE hank_jvp_income and hank_get_het_outputs_income (y has a direct term in consumption)."""
        d = np.asarray(dy, dtype=np.float64)
        single = d.ndim == 2
        d = d[:, :, None] if single else d
        self._shock_ready()
        hb = self.hb
        d0 = hb.jvp_income(None, d)
        daggs = d0[:, None, :] if self._n_out == 1 else hb.het_outputs(self._n_out, None, dy=d)[1]
        out = self._Ragg @ np.concatenate([daggs[:, j, :] for j in self._out_idx], axis=0)
        return out[:, 0].copy() if single else out

    def vjp_income(self, ȳ):
        """the transpose of `jvp_income`: ȳ (n,) or (n, M) -> y_bar (n_e, P) or (n_e, P, M), the gradient of ȳ·F with respect to the
        income path, from ONE hank_vjp_income."""
        ȳ = np.asarray(ȳ, dtype=np.float64)
        single = ȳ.ndim == 1
        Yb = ȳ[:, None] if single else ȳ
        self._shock_ready()
        P, M = self.mod.compspec.T - 1, Yb.shape[1]
        ab = np.asarray(self._Ragg.T @ Yb).reshape(len(self.het), P, M)
        agg_bar = np.zeros((P, self._n_out, M))
        for j, o in enumerate(self._out_idx):
            agg_bar[:, o, :] += ab[j]
        _, yb = self.hb.vjp_income(agg_bar, self._n_out)
        return yb[:, :, 0].copy() if single else yb

    def residual_income_jacobian(self, J_y):
        """∂F/∂y (n, n_e P), column e + n_e s the income of state e in period s (the column-major vec of y (n_e, P)), from the
        household block's J_y (n_out, P, n_e, P) of `SteadyStateJacobian.income_jacobian`: `_Ragg` composed with the rows of the
        heterogeneous variables the equations read."""
        if self._Rx is None:
            self._linearise_residuals()
        J = np.asarray(J_y)
        P, n_e = J.shape[1], J.shape[2]
        rows = np.concatenate([J[j].transpose(0, 2, 1).reshape(P, P * n_e) for j in self._out_idx], axis=0)      # [t, s n_e + e]
        return np.asarray(self._Ragg @ rows)

    def residual_shock_jacobian(self, J_beta):
        """∂F/∂beta (n, P) from the household block's J_beta (n_out, P, P) of `SteadyStateJacobian.shock_jacobian`: `_Ragg` composed
        with the rows of the heterogeneous variables the equations read."""
        if self._Rx is None:
            self._linearise_residuals()
        return np.asarray(self._Ragg @ np.concatenate([np.asarray(J_beta)[j] for j in self._out_idx], axis=0))

    def residual_borrow_jacobian(self, J_amin):
        """∂F/∂amin (n, P) from the household block's J_amin (n_out, P, P) of `SteadyStateJacobian.borrow_jacobian`: `_Ragg` composed
        with the rows of the heterogeneous variables the equations read."""
        return self.residual_shock_jacobian(J_amin)

    def as_linear_operator(self):
        """J(x) as a scipy.sparse.linalg.LinearOperator with both products: matvec / matmat = `jvp`, rmatvec / rmatmat = `vjp`
        (`vjp_het` for a model whose heterogeneous variables reach Value or UCE) — LSQR / LSMR, BiCG, QMR and every other user of
        the transpose."""
        n = len(self.x)
        vjp = self.vjp_het if self._n_out > 2 else self.vjp
        col = lambda f: (lambda v: f(np.asarray(v, dtype=np.float64).reshape(-1)))
        mat = lambda f: (lambda V: f(np.asarray(V, dtype=np.float64)))
        return spla.LinearOperator((len(self.Fx), n), matvec=col(self.jvp), matmat=mat(self.jvp), rmatvec=col(vjp), rmatmat=mat(vjp),
                                   dtype=np.float64)


def _gmres(J, b, x0):
    """IterativeSolvers.gmres!(x, A, b) defaults: restart = min(20, n), reltol = sqrt(eps),
    warm start from x (NewtonRaphson.jl:97-98). `maxiter` there counts Krylov steps, scipy's counts
    restart cycles."""
    n = len(b)
    restart = min(20, n)
    x, _ = spla.gmres(J, b, x0=x0, rtol=np.sqrt(np.finfo(float).eps), atol=0.0, restart=restart,
                      maxiter=max(1, n // restart))
    return x


_LU_CACHE = []          # [(J, lu)]: holds the factored matrix itself — an id() alone can be recycled by a new J̅


def _lu_solver(J):
    """J̅ obtained from batched JVPs is a dense n x n matrix (n ≈ 1.2k): one LU factorisation, reused
    by every inner and outer iteration, replaces the two GMRES solves per inner iteration — same
    J̅⁻¹·b up to rounding, milliseconds instead of seconds on the host. (A deviation from
    NewtonRaphson.jl:97-98, which runs two warm-started gmres! solves: `linear_solver="gmres"` is that branch.)"""
    import scipy.linalg as sla
    if not (_LU_CACHE and _LU_CACHE[0][0] is J):
        A = J.toarray() if hasattr(J, "toarray") else np.asarray(J)
        _LU_CACHE[:] = [(J, sla.lu_factor(A))]
    lu = _LU_CACHE[0][1]
    return lambda b: sla.lu_solve(lu, b)


_INV_CACHE = []         # [(J, apply)]
_WARM = {"done": False}


def warm_linear_solver(n_unknowns: int):
    """The device linear-algebra libraries behind `_device_inverse_solver` (rocSOLVER / rocBLAS through torch) take 0.15-0.35 s to
    start the first time a process uses them (scripts/dev_inv_cost.py): shared objects and code objects being loaded. A model with
    >= 2 000 unknowns will need them, so `find_ss` calls this BEFORE its own solve begins: one small inverse and one product on the
    device, synchronously. (Round 4 ran it in a background thread beside the solve. The steady state's inner fixed points are
    persistent sweeps that assume the process has the GPU to itself — a library kernel that lands between their workgroups can
    keep a group from forming, and the context then moves to the per-period launches for good, silently: hank_stats' `fallbacks`.
    The start-up is paid once per process either way; here it can no longer cost a schedule.) Idempotent; a no-op without a GPU."""
    if n_unknowns < 2000 or _WARM["done"]:
        return
    _WARM["done"] = True
    try:
        import torch
        if torch.cuda.is_available():
            A = torch.eye(512, dtype=torch.float64, device="cuda") + 0.001
            (torch.linalg.inv(A) @ A[:, :1]).cpu()
            torch.cuda.synchronize()
    except Exception:       # noqa: BLE001 - a warm-up must never fail a solve
        pass


def release_linear_solver():
    """drop the factorisations kept for a J̅ (the host LU and the device inverse: n² fp64 in HBM, 97 MB at n = 3 493).
    NewtonRaphsonHANK calls it when it returns; a caller that drives y_Iteration itself calls it when done with a J̅."""
    _LU_CACHE[:] = []
    _INV_CACHE[:] = []


def _device_inverse_solver(J, device=None):
    """J̅⁻¹·b as ONE dense matrix-vector product on the GPU (a library GEMV: torch → rocBLAS) with the explicit inverse, formed once
    per J̅ (torch.linalg.inv on the device): at the one-asset HANK size (n = 3 493) the host's two triangular solves read 97 MB per
    inner iteration and took as long as the device's tangent sweeps (2.1 ms against 2.9 ms, scripts/dev_profile_newton.py). J̅⁻¹
    is a preconditioner here — the fixed point of the y-iteration is J(x)⁻¹F(x) whatever its accuracy. Returns None without a GPU."""
    try:
        import torch
        if not torch.cuda.is_available():
            return None
    except Exception:       # noqa: BLE001
        return None
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))       # the MODEL's GPU (hank_create_on), not torch's current one
    if not (_INV_CACHE and _INV_CACHE[0][0] is J and _INV_CACHE[0][2] == dev):
        import time
        t0 = time.perf_counter()
        A = J.toarray() if hasattr(J, "toarray") else np.asarray(J)
        Ainv = torch.linalg.inv(torch.from_numpy(np.ascontiguousarray(A, dtype=np.float64)).to(dev))
        (Ainv[:1] @ Ainv[:, :1]).cpu()      # the first product of a process also loads rocBLAS: count it with the set-up, not with an iteration
        # once per J̅ (and, the first time in a process, the linear-algebra libraries' own start-up: 0.15-0.35 s against 40 ms warm at
        # n = 3 493, scripts/dev_inv_cost.py): reported next to the solve times, examples/solve_hank.py
        y_Iteration.setup_s = getattr(y_Iteration, "setup_s", 0.0) + (time.perf_counter() - t0)

        def apply(b, Ainv=Ainv, dev=dev):
            return (Ainv @ torch.from_numpy(np.ascontiguousarray(b, dtype=np.float64)).to(dev)).cpu().numpy()

        _INV_CACHE[:] = [(J, apply, dev)]
    return _INV_CACHE[0][1]


@host_algebra
def y_Iteration(J̅, x, y0, exog_paths, mod: SequenceModel, ss_initial, ss_ending, *, precond=None,
                α: float | None = None, γ: float = 1.5, ε: float = 1e-9, verbose: bool = False, max_inner: int = 10_000,
                linear_solver: str = "auto", inner: str = "fixed_point", discount_path=None, income_path=None, borrow_path=None):
    """inner iteration for the search direction y with J(x)·y = F(x) (NewtonRaphson.jl:65-114).

    inner="fixed_point" (default, the reference): y ← y + α·J̅⁻¹(F(x) − J(x)·y). The reference accepts α (:72) and
    overrides it with 0.5 (:102): `α=None` is that; a value passed here is honoured (α = 1 is the undamped iteration).
    inner="krylov" (opt-in, not in the reference): GMRES on J(x) with J̅⁻¹ as right preconditioner — the same fixed point
    (the exact Newton step) in a handful of JVPs instead of the ≈ 21 that α = 0.5 needs to contract 1e-9 by halves."""
    lin = LinearizedFunction(x, exog_paths, mod, ss_initial, ss_ending, discount_path=discount_path, income_path=income_path, borrow_path=borrow_path)
    y_Iteration.last_Fx = lin.Fx            # F(x) of this linearisation: the step rule's ‖F(x)‖ (NewtonRaphsonHANK, step="backtrack")
    y = np.asarray(y0, dtype=np.float64)
    n = len(y)
    y_old, M, R = np.ones(n), np.ones(n), np.ones(n)
    Fx = lin.Fx
    i = 1
    solve = None
    if linear_solver in ("auto", "device") and len(y) >= 2000:      # (below that the host's LU solve takes a tenth of a millisecond)
        solve = _device_inverse_solver(J̅, getattr(lin.hb, "device", None))
    if solve is None and linear_solver in ("auto", "lu", "device"):
        solve = _lu_solver(J̅)
    if inner == "krylov":
        count = [0]

        def matvec(v):
            count[0] += 1
            return lin.jvp(np.asarray(v, dtype=np.float64).ravel())

        Pinv = spla.LinearOperator((n, n), matvec=(solve if solve is not None else (lambda b: _gmres(J̅, b, np.zeros(n)))), dtype=np.float64)
        A = spla.LinearOperator((n, n), matvec=matvec, dtype=np.float64)
        # right-preconditioned: J(x) J̅⁻¹ z = F(x), y = J̅⁻¹ z; J(x) J̅⁻¹ ≈ I near the steady state. Stop when the linear residual is
        # below ε relative to ‖F(x)‖ and below 1e-3 ε absolutely (the outer loop's ‖y‖ ≤ ε test then sees a converged step)
        AP = spla.LinearOperator((n, n), matvec=lambda z: matvec(Pinv.matvec(z)), dtype=np.float64)
        z, info = spla.gmres(AP, Fx, rtol=min(1e-10, ε), atol=1e-3 * ε, restart=min(30, n), maxiter=max(1, max_inner // 30))
        y = Pinv.matvec(z)
        if info != 0:       # not converged within maxiter (or a breakdown): the step is still a descent direction of the preconditioned
            import warnings  # system, but the caller must know it is not the Newton step
            warnings.warn(f"y_Iteration(inner='krylov'): GMRES returned info={info} after {count[0]} JVPs; "
                          f"‖F − J y‖ = {np.linalg.norm(Fx - lin.jvp(y)):.3e}", RuntimeWarning, stacklevel=2)
        y_Iteration.last_jvp_count = count[0]
        y_Iteration.total_jvps = getattr(y_Iteration, "total_jvps", 0) + count[0]
        if verbose:
            print(f"y_Iteration (krylov): {count[0]} JVPs, info={info}, ‖F − J y‖={np.linalg.norm(Fx - lin.jvp(y))}")
        return y
    if inner != "fixed_point":
        raise ValueError(f"unknown inner iteration {inner!r} (fixed_point | krylov)")
    step = 0.5 if α is None else float(α)
    while ε < np.linalg.norm(y - y_old) and i < max_inner:
        Λxy = lin.jvp(y)
        if solve is not None:
            R = solve(Fx - Λxy)
            M = solve(Λxy) if verbose else M       # only feeds the printed Rayleigh quotient (:101, :108-110)
        else:
            R = _gmres(J̅, Fx - Λxy, R)
            M = _gmres(J̅, Λxy, M)
        with np.errstate(divide="ignore", invalid="ignore"):      # printed only (:101, :108-110); NaN at y = 0 like Julia
            ray = np.divide(y @ M, y @ y) if verbose else np.nan
        y_old = y
        y = y_old + step * R
        i += 1
        if verbose and i % 10 == 0:
            print(f"y_Iteration {i}: α={step}  ‖y−y_old‖={np.linalg.norm(y - y_old)}  ray={ray}")
    y_Iteration.last_jvp_count = i - 1
    y_Iteration.total_jvps = getattr(y_Iteration, "total_jvps", 0) + i - 1
    return y


class StepRuleError(RuntimeError):
    """no trial step of the backtracking rule lowers ‖F‖ (every trial failed on the device, or y is no descent direction)."""


def backtrack(norms2, f0_2, c1: float = 1e-4) -> int:
    """the step rule of NewtonRaphsonHANK(step="backtrack") as a pure function: norms2[j] = ‖F(x − 2^-j y)‖² of the trials
    j = 0, 1, …, f0_2 = ‖F(x)‖². -> the first j with norms2[j] ≤ (1 − 2 c1 2^-j) f0_2 — Armijo's condition on ½‖F‖² along a Newton
    direction y (J y = F: the directional derivative of ½‖F‖² at α = 0 is −‖F‖²). When no trial passes: the trial of the smallest
    norm, if that is below ‖F(x)‖; otherwise StepRuleError. Entries that are not finite (a scenario the device refused) are
    skipped."""
    n2 = np.asarray(norms2, dtype=np.float64).reshape(-1)
    ok = np.isfinite(n2)
    for j in range(n2.size):
        if ok[j] and n2[j] <= (1.0 - 2.0 * c1 * 2.0 ** -j) * f0_2:
            return j
    if ok.any():
        j = int(np.argmin(np.where(ok, n2, np.inf)))
        if n2[j] < f0_2:
            return j
    raise StepRuleError(f"backtrack: none of the {n2.size} trial steps lowers ‖F‖² = {f0_2:.6e} (trials: {n2.tolist()})")


def residuals_batch(xs, exog_paths, mod: SequenceModel, ss_initial, ss_ending):
    """fullFunction (NewtonRaphson.jl:77-83) at K points at once: xs (n, K) -> (n_res, K). The household block of every column
    runs in ONE hank_primal_batch (K paths through one chain of launches, at the model's count of device outputs); the padded
    matrix and the residuals are assembled per column on the host. The context's recorded primal stays as it was, so a
    linearisation at another x keeps serving its JVPs. A column the device refuses (its status is not HANK_OK), or whose 1 + r is
    not positive somewhere, comes back as a column of inf."""
    xs = np.asarray(xs, dtype=np.float64)
    if xs.ndim == 1:
        xs = xs[:, None]
    K = xs.shape[1]
    hb = household_block(mod)
    het = vars_of_type(mod, "heterogeneous")
    outs = tuple(mod.value_fn.outputs)
    out_idx = [outs.index(k) for k in het]
    n_out = 1 + max(out_idx)
    xhh = np.stack([household_inputs(xs[:, k], exog_paths, mod)[0] for k in range(K)], axis=2)        # (n_hh, P, K)
    before = hb._boundary
    hb.set_boundary(ss_ending.value, ss_initial.D)
    if before is None or not (np.array_equal(before[0], hb._boundary[0]) and np.array_equal(before[1], hb._boundary[1])):
        hb._generation = getattr(hb, "_generation", 0) + 1      # a new boundary: the record is gone, whoever held it re-records
        hb._last = None
    if n_out > 2:
        ensure_het_outputs(hb, n_out)
    ok = np.ones(K, dtype=bool)
    if mod.value_fn.household_inputs[0] == "r":
        ok = np.all(1.0 + xhh[0] > 0.0, axis=0)
    out = np.full((len(mod.equations) * (mod.compspec.T - 1), K), np.inf)
    cols = np.flatnonzero(ok)
    for c0 in range(0, len(cols), 64):                   # (the library takes up to 64 scenarios per call)
        chunk = cols[c0:c0 + 64]
        aggs, status = hb.primal_batch(xhh[:, :, chunk], n_het=n_out, check=False)
        for j, k in enumerate(chunk):
            if status[j] != 0:
                continue
            agg = {name: aggs[:, o, j] for name, o in zip(het, out_idx)}
            out[:, k] = Residuals(assemble_full_xMat(xs[:, k], agg, exog_paths, mod, ss_initial, ss_ending), mod)
    return out


@host_algebra
def NewtonRaphsonHANK(x_0, J̅, exog_paths, mod: SequenceModel, ss_initial, ss_ending, *, ε: float = 1e-9,
                      verbose: bool = False, linear_solver: str = "auto", inner: str = "fixed_point", α: float | None = None,
                      step: str = "full", n_trial: int = 6, c1: float = 1e-4, discount_path=None, income_path=None, borrow_path=None):
    """outer Newton loop (NewtonRaphson.jl:27-46): x ← x − y until ‖y‖ ≤ ε or 100 iterations. `inner` / `α`: see y_Iteration
    (defaults = the reference's damped fixed point).

    step="full" (default, the reference): the full Newton step, unconditionally. step="backtrack" (not in the reference, whose
    alphaUpdate is a stub, NewtonRaphson.jl:117-120): after each y_Iteration the trials x − 2^-j y, j = 0 .. n_trial-1, are
    evaluated in ONE `residuals_batch` and `backtrack` picks the step; ‖F(x)‖ is the linearisation's own (`y_Iteration.last_Fx`),
    not one more primal. A direction already below ε (the loop's last) is taken whole, without trials: at that size the trials differ
    by the inner loop's own tolerance and say nothing. `NewtonRaphsonHANK.step_sizes` lists the accepted α, `.residual_norms` ‖F‖ at every iterate.

    discount_path: beta_t (P,) (`LinearizedFunction`): the transition under a path of the discount factor. J̅ is still the
    steady-state Jacobian: take it before the path is set, or on a clone of the context without one.
    income_path: y (n_e, P) (`LinearizedFunction`): the transition under a path of income by productivity state, under the same rules.
    borrow_path: amin_t (P,) (`LinearizedFunction`): the transition under a path of the borrowing limit, under the same rules."""
    if step not in ("full", "backtrack"):
        raise ValueError(f"unknown step rule {step!r} (full | backtrack)")
    if income_path is not None and step == "backtrack":
        raise ValueError("step='backtrack' evaluates its trials with hank_primal_batch, which is defined at one income process: use step='full' with an income_path")
    if borrow_path is not None and step == "backtrack":
        raise ValueError("step='backtrack' evaluates its trials with hank_primal_batch, which is defined at one borrowing limit: use step='full' with a borrow_path")
    if discount_path is not None and step == "backtrack":
        raise ValueError("step='backtrack' evaluates its trials with hank_primal_batch, which is defined at one discount factor: use step='full' with a discount_path")
    x = np.asarray(x_0, dtype=np.float64)
    y = x.copy()
    i = 1
    NewtonRaphsonHANK.step_sizes, NewtonRaphsonHANK.residual_norms = [], []
    try:
        while ε < np.linalg.norm(y) and i < 100:
            y = y_Iteration(J̅, x, y, exog_paths, mod, ss_initial, ss_ending, verbose=verbose, linear_solver=linear_solver, inner=inner, α=α,
                            discount_path=discount_path, income_path=income_path, borrow_path=borrow_path)
            if step == "full":
                x = x - y
            elif not ε < np.linalg.norm(y):         # a step below the tolerance ends the loop: taken whole, as the reference takes it
                x = x - y
                NewtonRaphsonHANK.step_sizes.append(1.0)
                NewtonRaphsonHANK.residual_norms[len(NewtonRaphsonHANK.step_sizes) - 1:] = [float(np.linalg.norm(y_Iteration.last_Fx))]
            else:
                f0_2 = float(np.sum(np.asarray(y_Iteration.last_Fx, dtype=np.float64) ** 2))
                alphas = 2.0 ** -np.arange(int(n_trial), dtype=np.float64)
                xs = x[:, None] - y[:, None] * alphas[None, :]
                n2 = np.sum(residuals_batch(xs, exog_paths, mod, ss_initial, ss_ending) ** 2, axis=0)
                j = backtrack(n2, f0_2, c1)
                x = np.ascontiguousarray(xs[:, j])
                NewtonRaphsonHANK.step_sizes.append(float(alphas[j]))
                NewtonRaphsonHANK.residual_norms[len(NewtonRaphsonHANK.step_sizes) - 1:] = [float(np.sqrt(f0_2)), float(np.sqrt(n2[j]))]
            i += 1
            if verbose:
                print(f"Iteration: {i}, norm(y): {np.linalg.norm(y)}" + (f", α: {NewtonRaphsonHANK.step_sizes[-1]}" if step != "full" else ""))
    finally:
        release_linear_solver()         # (the factorisations of J̅ live for one solve, not for the life of the process)
    NewtonRaphsonHANK.iterations = i - 1
    return x
