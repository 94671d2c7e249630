#!/usr/bin/env python
"""The RunMain.jl sequence (RunMain.jl:35-55, as intended — SURVEY.md §3.1) on the MI355X build:

    YAML -> model -> steady state (host) -> J̅ (its Toeplitz structure from n_hh backward tangent sweeps on the GPU; or n unit tangents)
         -> NewtonRaphsonHANK (Boehl y-iteration; one hank_jvp per inner iteration) -> converged path

    python examples/solve_transition.py [--n-a 500 --n-e 4 --T 300 --shock 0.01]

`--shock 0.8` is RunMain's own Z_t = 1 + 0.8^t (an 80 % TFP jump; may not converge with the
reference's fixed damping α = 0.5 — SURVEY.md App. B item 5)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def solve(n_a=500, n_e=4, T=300, shock=0.01, eps=1e-9, verbose=False, cold=False, inner="fixed_point", jacobian="toeplitz", step="full", with_model=False):
    """with_model=True: -> (report, x, model, steady state) instead of (report, x). step="backtrack": Newton with the backtracking step rule (the trial steps of an iteration in ONE hank_primal_batch). cold=True: the steady state is solved here from the YAML guesses (value iteration and stationary distribution on
    the device where one is present) instead of coming from the test fixtures' cache."""
    import hank_amd as h
    import hank_amd.parallel  # noqa: F401  (pulls in torch before the clocks start)
    from conftest import ks_setup
    t0 = time.perf_counter()
    if cold:
        ov = {"T": T, "dimensions": {"wealth": {"n": n_a}, "productivity": {"n": n_e}}}
        m = h.build_model_from_yaml(str(ROOT / "examples" / "krusell_smith.yaml"), overrides=ov)
        ss, _ = h.get_SteadyStates(m)
    else:
        m, ss, _ = ks_setup(n_a, n_e, T)
    t_ss = time.perf_counter() - t0
    P = T - 1
    Z = 1.0 + shock * 0.8 ** np.arange(1, P + 1)                       # RunMain.jl:22-23
    x0 = np.tile(np.array([ss.vars[k] for k in ("Y", "KS", "r", "w")]), P)   # SteadyState.jl:277-278
    t0 = time.perf_counter()
    J = h.getSteadyStateJacobian(ss, m, method=jacobian)
    t_jac = time.perf_counter() - t0
    h.y_Iteration.total_jvps = 0
    h.y_Iteration.setup_s = 0.0
    t0 = time.perf_counter()
    x = h.NewtonRaphsonHANK(x0, J, {"Z": Z}, m, ss, ss, ε=eps, verbose=verbose, inner=inner, step=step)
    t_newton = time.perf_counter() - t0
    lin = h.LinearizedFunction(x, {"Z": Z}, m, ss, ss)
    out = {"grid": f"{n_a}x{n_e}", "T": T, "shock": f"Z_t = 1 + {shock}*0.8^t", "steady_state_s": round(t_ss, 3),
            "ss_jacobian_s": round(t_jac, 3), "newton_s": round(t_newton, 3), "preconditioner_setup_s": round(h.y_Iteration.setup_s, 3),
            "newton_iterations": h.NewtonRaphsonHANK.iterations, "jvps": h.y_Iteration.total_jvps, "residual_norm": float(np.linalg.norm(lin.Fx)),
            "wall_to_converged_path_s": round(t_jac + t_newton, 3), "steady_state": "cold start" if cold else "cached",
            "inner": inner, "jacobian": jacobian, **({"step": step, "step_sizes": list(h.NewtonRaphsonHANK.step_sizes)} if step != "full" else {})}
    return (out, x, m, ss) if with_model else (out, x)


def group_report(x, m, ss, Z, cuts):
    """Who moves along the converged path x: the wealth groups cut at the steady-state CDF points `cuts` (0.5 0.9: the bottom half,
    the next 40 %, the top decile; `hank_amd.groups.wealth_groups`, fixed by wealth level), each with its mass, savings and
    consumption (hank_set_group_outputs / hank_get_group_outputs on a context of its own). Per group: the steady-state level, the
    peak deviation along the path, and the largest gap between that nonlinear path and the linear response J_group · dx of the
    household inputs' deviation (`SteadyStateJacobian.group_jacobian`: hank_fake_news_group)."""
    from hank_amd.BackwardIteration import household_block, household_inputs
    from hank_amd.groups import wealth_groups
    from hank_amd.SteadyStateJacobian import group_jacobian
    P = m.compspec.T - 1
    edges = [0.0, *[float(c) for c in cuts], 1.0]
    wd, pd_ = m.heterogeneity["wealth"], m.heterogeneity["productivity"]
    Wg = wealth_groups(ss.D, wd.grid.size, pd_.grid.size, edges)
    K = Wg.shape[1]
    hb = household_block(m).clone()
    hb.set_boundary(ss.value, ss.D)
    hb.set_group_outputs(np.concatenate([Wg, Wg, Wg], axis=1), np.repeat([hb.GROUP_MASS, hb.GROUP_POLICY, hb.GROUP_CONS], K))
    x_ss = np.tile(np.array([ss.vars[k] for k in ("Y", "KS", "r", "w")]), P)
    xhh_ss = np.asarray(household_inputs(x_ss, {"Z": np.ones(P)}, m)[0])
    xhh = np.asarray(household_inputs(x, {"Z": Z}, m)[0])
    hb.primal(xhh_ss)
    Y_ss = hb.group_outputs()[0]
    J = group_jacobian(hb)                                              # (3 K, P, n_hh, P)
    hb.primal(xhh)
    dY = hb.group_outputs()[0] - Y_ss                                   # (P, 3 K)
    lin = np.einsum("ktis,is->tk", J, xhh - xhh_ss)
    hb.close()

    def one(k):
        return {"steady_state": float(Y_ss[0, k]), "peak_deviation": float(dY[np.argmax(np.abs(dY[:, k])), k]),
                "linear_peak_deviation": float(lin[np.argmax(np.abs(lin[:, k])), k]), "max_gap_to_linear": float(np.abs(dY[:, k] - lin[:, k]).max())}

    return {"edges": edges, "groups": [{"cdf": [edges[g], edges[g + 1]], "mass": one(g), "savings": one(K + g), "consumption": one(2 * K + g)}
                                       for g in range(K)],
            "max_gap_to_linear": float(np.abs(dY - lin).max())}


def group_gradient(x, m, ss, Z, cuts):
    """The gradient of the distributional criterion L = ½ Σ_g Σ_t (C^g_t − C^g_ss)², C^g the consumption of wealth group g
    (`group_report`'s groups under GROUP_CONS), with respect to the n_hh·P household inputs at the converged path x: ONE
    hank_vjp_group with the cotangents C^g_t − C^g_ss, where the forward route takes n_hh·P tangent columns. Printed beside a central
    difference of L (`primal` + `group_outputs()`) at three coordinates."""
    from hank_amd.BackwardIteration import household_block, household_inputs
    from hank_amd.groups import wealth_groups
    P = m.compspec.T - 1
    edges = [0.0, *[float(c) for c in cuts], 1.0]
    wd, pd_ = m.heterogeneity["wealth"], m.heterogeneity["productivity"]
    Wg = wealth_groups(ss.D, wd.grid.size, pd_.grid.size, edges)
    hb = household_block(m).clone()
    hb.set_boundary(ss.value, ss.D)
    hb.set_group_outputs(Wg, hb.GROUP_CONS)
    x_ss = np.tile(np.array([ss.vars[k] for k in ("Y", "KS", "r", "w")]), P)
    xhh_ss = np.asarray(household_inputs(x_ss, {"Z": np.ones(P)}, m)[0])
    xhh = np.asarray(household_inputs(x, {"Z": Z}, m)[0])
    hb.primal(xhh_ss)
    C_ss = hb.group_outputs()[0]

    def loss(xh):
        hb.primal(xh)
        return 0.5 * float(np.sum((hb.group_outputs()[0] - C_ss) ** 2))

    L = loss(xhh)
    grad = hb.vjp_group(hb.group_outputs()[0] - C_ss)[:, :, 0]          # (n_hh, P)
    checks = []
    for i, t in ((0, 0), (1, P // 2), (0, P - 1)):
        h = 1e-6 * max(1.0, abs(xhh[i, t]))
        e = np.zeros_like(xhh); e[i, t] = h
        fd = (loss(xhh + e) - loss(xhh - e)) / (2 * h)
        checks.append({"input": i, "period": t, "vjp_group": float(grad[i, t]), "central_difference": fd})
    hb.close()
    return {"edges": edges, "loss": L, "gradient_norm": float(np.linalg.norm(grad)), "checks": checks}


def scale_family(n_a=500, n_e=4, T=300, shock=0.01, scales=(0.5, 1.0, 2.0, -1.0), eps=1e-9, max_rounds=100):
    """The nonlinear responses to the shock at several multiples, solved in LOCKSTEP: scenario k has the path Z_t = 1 + scales[k]·
    shock·0.8^t and its own iterate x_k, and every round evaluates F(x_k) of all scenarios from ONE
    hank_primal_batch, then steps each unconverged one by the chord rule x_k ← x_k − J̅⁻¹F(x_k) (J̅ the steady-state Jacobian,
    factored once: a round costs one batch, no tangent sweep; the rule converges linearly where ‖I − J̅⁻¹J(x)‖ < 1, the regime of
    these shocks). A converged scenario (‖step‖ ≤ eps) keeps its x. The first round from the steady state IS the first-order
    solution x_ss − J̅⁻¹F(x_ss; Z_k): each peak response is printed beside it."""
    import hank_amd as h
    from conftest import ks_setup
    from hank_amd.Aggregation import Residuals
    from hank_amd.BackwardIteration import ensure_het_outputs, household_block, household_inputs
    from hank_amd.GeneralStructures import assemble_full_xMat, vars_of_type
    from hank_amd.NewtonRaphson import _lu_solver, release_linear_solver
    m, ss, _ = ks_setup(n_a, n_e, T)
    P, K = T - 1, len(scales)
    names = ("Y", "KS", "r", "w")
    Zs = [{"Z": 1.0 + sc * shock * 0.8 ** np.arange(1, P + 1)} for sc in scales]
    x_ss = np.tile(np.array([ss.vars[k] for k in names]), P)
    solve_J = _lu_solver(h.getSteadyStateJacobian(ss, m))
    hb = household_block(m)
    hb.set_boundary(ss.value, ss.D)
    het = vars_of_type(m, "heterogeneous")
    out_idx = [tuple(m.value_fn.outputs).index(k) for k in het]
    n_out = 1 + max(out_idx)
    if n_out > 2:
        ensure_het_outputs(hb, n_out)
    xs = np.tile(x_ss[:, None], (1, K))
    done, first, rounds = np.zeros(K, dtype=bool), None, 0
    t0 = time.perf_counter()
    try:
        while not done.all() and rounds < max_rounds:
            xhh = np.stack([household_inputs(xs[:, k], Zs[k], m)[0] for k in range(K)], axis=2)
            aggs, _ = hb.primal_batch(xhh, n_het=n_out)                 # ONE batch per round (a failing scenario raises)
            for k in np.flatnonzero(~done):
                agg = {name: aggs[:, o, k] for name, o in zip(het, out_idx)}
                y = solve_J(Residuals(assemble_full_xMat(xs[:, k], agg, Zs[k], m, ss, ss), m))
                xs[:, k] -= y
                done[k] = np.linalg.norm(y) <= eps
            first = xs.copy() if first is None else first
            rounds += 1
    finally:
        release_linear_solver()
    wall = time.perf_counter() - t0

    def peaks(x):
        d = x.reshape(len(names), P, order="F") - np.array([ss.vars[k] for k in names])[:, None]
        return {k: float(d[j, np.argmax(np.abs(d[j]))]) for j, k in enumerate(names)}

    return {"grid": f"{n_a}x{n_e}", "T": T, "shock": f"Z_t = 1 + s*{shock}*0.8^t", "scales": list(scales), "rounds": rounds, "primal_batches": rounds,
            "converged": done.tolist(), "lockstep_s": round(wall, 3),
            "peak_response": {str(sc): {"nonlinear": peaks(xs[:, k]), "first_order": peaks(first[:, k])} for k, sc in enumerate(scales)}}


def gradient(n_a=500, n_e=4, T=300, shock=0.01, chunk=256):
    """The gradient of the merit function ½‖F(x)‖² at the Newton starting point (the steady state repeated, where F ≠ 0 under
    the shock): ∇ = J(x)ᵀ F(x). Reverse mode: ONE hank_vjp at M = 1 (`LinearizedFunction.vjp`). Forward mode: the n unit
    tangents, of which n_hh·P move the household inputs and reach the device (hank_jvp in batches of `chunk`). Prints both
    times and their agreement."""
    import hank_amd as h
    import hank_amd.parallel  # noqa: F401
    from conftest import ks_setup
    m, ss, _ = ks_setup(n_a, n_e, T)
    P = T - 1
    Z = 1.0 + shock * 0.8 ** np.arange(1, P + 1)
    x0 = np.tile(np.array([ss.vars[k] for k in ("Y", "KS", "r", "w")]), P)
    lin = h.LinearizedFunction(x0, {"Z": Z}, m, ss, ss)
    n = x0.size
    lin.vjp(lin.Fx); lin.jvp(np.eye(n)[:, :chunk])                      # warm-up: workspaces, graphs, the residual layer's linearisation
    t0 = time.perf_counter()
    g_rev = lin.vjp(lin.Fx)
    t_rev = time.perf_counter() - t0
    t0 = time.perf_counter()
    g_fwd = np.concatenate([lin.Fx @ lin.jvp(np.eye(n)[:, c0:c0 + chunk]) for c0 in range(0, n, chunk)])
    t_fwd = time.perf_counter() - t0
    return {"grid": f"{n_a}x{n_e}", "T": T, "unknowns": n, "merit": 0.5 * float(lin.Fx @ lin.Fx), "gradient_norm": float(np.linalg.norm(g_rev)),
            "reverse_s": round(t_rev, 5), "reverse_vjps": 1, "forward_s": round(t_fwd, 5), "forward_jvp_columns": lin.hb.n_hh * P,
            "max_abs_difference_over_max": float(np.max(np.abs(g_rev - g_fwd)) / np.max(np.abs(g_fwd)))}


def boundary_gradient(n_a=500, n_e=4, T=300, shock=0.01, seed=0):
    """The gradient of the merit function ½‖F(x)‖² with respect to the BOUNDARY (V_T, D_0) — the terminal marginal value
    `ss_end.value` (BackwardIteration.jl:85) and the initial distribution `ss_initial.D` (ForwardIteration.jl:293) — at the Newton
    starting point, from ONE hank_vjp_boundary: F reaches the boundary through the household aggregates alone, so the cotangent
    of the aggregates is the residual layer's `∂R/∂agg`ᵀ F. Printed next to its inner product with two random boundary
    directions (dV, dD) taken forward through hank_jvp_boundary: ⟨∇_V, dV⟩ + ⟨∇_D, dD⟩ = ⟨F, ∂R/∂agg · J_b (dV, dD)⟩."""
    import hank_amd as h
    import hank_amd.parallel  # noqa: F401
    from conftest import ks_setup
    m, ss, _ = ks_setup(n_a, n_e, T)
    P = T - 1
    Z = 1.0 + shock * 0.8 ** np.arange(1, P + 1)
    x0 = np.tile(np.array([ss.vars[k] for k in ("Y", "KS", "r", "w")]), P)
    lin = h.LinearizedFunction(x0, {"Z": Z}, m, ss, ss)
    if lin._n_out > 2:
        raise NotImplementedError("boundary derivatives cover the policy variable and consumption only")
    lin._linearise_residuals()
    hb, n_out = lin.hb, lin._n_out
    ab = np.asarray(lin._Ragg.T @ lin.Fx).reshape(len(lin.het), P)              # rows: het variable, period
    agg_bar = np.zeros((P, n_out, 1))
    for j, o in enumerate(lin._out_idx):
        agg_bar[:, o, 0] += ab[j]
    t0 = time.perf_counter()
    _, g_V, g_D = hb.vjp_boundary(agg_bar, n_out)
    t_rev = time.perf_counter() - t0
    rng = np.random.default_rng(seed)
    dV = rng.standard_normal((hb.n_a, hb.n_e, 2)) * np.abs(np.asarray(ss.value))[:, :, None]
    dD = rng.standard_normal((hb.n_a, hb.n_e, 2)) / hb.G
    t0 = time.perf_counter()
    dagg = hb.jvp_boundary(None, dV, dD)                                        # (P, 2)
    daggs = dagg[:, None, :] if n_out == 1 else hb.het_outputs(n_out, np.zeros((hb.n_hh, P, 2)))[1]
    t_fwd = time.perf_counter() - t0
    dF = lin._Ragg @ np.concatenate([daggs[:, o, :] for o in lin._out_idx], axis=0)
    fwd = lin.Fx @ dF
    rev = np.einsum("ae,aen->n", g_V[:, :, 0], dV) + np.einsum("ae,aen->n", g_D[:, :, 0], dD)
    return {"grid": f"{n_a}x{n_e}", "T": T, "merit": 0.5 * float(lin.Fx @ lin.Fx), "boundary_unknowns": 2 * hb.G,
            "gradient_norm_value_end": float(np.linalg.norm(g_V)), "gradient_norm_D_init": float(np.linalg.norm(g_D)),
            "reverse_s": round(t_rev, 5), "reverse_vjps": 1, "forward_s": round(t_fwd, 5),
            "directional_derivatives_reverse": [float(v) for v in rev], "directional_derivatives_forward": [float(v) for v in fwd],
            "max_abs_difference_over_max": float(np.max(np.abs(rev - fwd)) / np.max(np.abs(fwd)))}


def ss_gradient(n_a=200, n_e=3, T=150, Z_end=1.03, seed=0):
    """The chain from the transition path's merit function back to what moves the ENDING steady state, in the two-steady-state
    scenario: the gradient of ½‖F(x)‖² at the Newton starting point with respect to the ending steady state's household prices
    (r, w), through the terminal marginal value V_T = V_ss(r, w) (BackwardIteration.jl:85; SteadyState.jl:132-141). Reverse mode:
    ONE hank_vjp_het_boundary (value_end_bar), one primal at the ending steady path, ONE hank_ss_vjp(value_bar = value_end_bar).
    Printed beside a central difference in one random direction of (r, w): V_T re-solved by the device VFI at both ends, the
    merit function re-evaluated with it (everything else of the boundary held fixed)."""
    import dataclasses
    import hank_amd as h
    import hank_amd.parallel  # noqa: F401
    from hank_amd.BackwardIteration import ensure_het_outputs
    ov = {"T": T, "dimensions": {"wealth": {"n": n_a}, "productivity": {"n": n_e}},
          "steady_states": {"ending": {"fixed": {"Z": Z_end}, "guesses": {"r": 0.04, "w": 1.0, "Y": 1.5, "KS": 3.5}}}}
    m = h.build_model_from_yaml(str(ROOT / "examples" / "krusell_smith.yaml"), overrides=ov)
    ss_i, ss_e = h.get_SteadyStates(m, vfi_tol=1e-13)
    P = T - 1
    Z = np.full(P, float(Z_end))
    x0 = np.tile(np.array([ss_e.vars[k] for k in ("Y", "KS", "r", "w")]), P)
    names = m.value_fn.household_inputs
    xe = np.array([ss_e.vars[k] for k in names])

    def merit(ss_end):
        lin = h.LinearizedFunction(x0, {"Z": Z}, m, ss_i, ss_end)
        return 0.5 * float(lin.Fx @ lin.Fx), lin

    f0, lin = merit(ss_e)
    lin._linearise_residuals()
    hb, n_out = lin.hb, lin._n_out
    ab = np.asarray(lin._Ragg.T @ lin.Fx).reshape(len(lin.het), P)
    agg_bar = np.zeros((P, n_out, 1))
    for j, o in enumerate(lin._out_idx):
        agg_bar[:, o, 0] += ab[j]
    ensure_het_outputs(hb, n_out)
    t0 = time.perf_counter()
    _, g_V, _ = hb.vjp_het_boundary(agg_bar, n_out, value_end=True, D_init=False)      # d merit / d V_T
    hb.set_boundary(ss_e.value, ss_e.D)                                                   # the ending steady state's own record
    hb.primal(np.tile(xe[:, None], (1, P)))
    g_x, iters = hb.ss_vjp(value_bar=g_V, n_het=n_out)                                     # ... carried back to (r, w)
    t_rev = time.perf_counter() - t0
    d = np.random.default_rng(seed).standard_normal(len(names))
    d /= np.linalg.norm(d)
    hstep, f = 1e-6, []
    for sgn in (1.0, -1.0):
        v, _, _, _ = hb.vfi(ss_e.value, xe + sgn * hstep * d, 1e-13, 20_000)
        f.append(merit(dataclasses.replace(ss_e, value=v))[0])
    fd = (f[0] - f[1]) / (2 * hstep)
    rev = float(g_x[:, 0] @ d)
    return {"grid": f"{n_a}x{n_e}", "T": T, "shock": f"Z: 1 -> {Z_end} for good", "merit": f0, "household_prices": list(names),
            "gradient_wrt_ending_prices_through_V_T": [float(v) for v in g_x[:, 0]], "ss_vjp_steps_nu_lambda": list(iters),
            "reverse_s": round(t_rev, 5), "direction": [float(v) for v in d], "directional_derivative_reverse": rev,
            "directional_derivative_central_difference": fd, "relative_difference": abs(rev - fd) / max(abs(fd), 1e-300)}


def ss_curve(var, lo, hi, K, n_a=500, n_e=4, T=300):
    """The steady state's household side along a line in the free prices — `var` from lo to hi in K points, the other free prices at
    the YAML's guesses — from ONE hank_ss_batch (`SSAssembler.batch`): per point the heterogeneous aggregates (the asset-supply
    curve A(r) for var = r: what brackets a market-clearing rate when the guesses are poor), the residual norm and the value
    steps. No price Newton runs."""
    import hank_amd as h
    from hank_amd.Aggregation import Residuals
    from hank_amd.GeneralStructures import vars_of_type
    from hank_amd.SteadyState import SSAssembler
    ov = {"T": T, "dimensions": {"wealth": {"n": n_a}, "productivity": {"n": n_e}}}
    m = h.build_model_from_yaml(str(ROOT / "examples" / "krusell_smith.yaml"), overrides=ov)
    asm = SSAssembler(m, m.ss_initial, None, "device")
    if var not in asm.free_keys:
        raise SystemExit(f"--ss-curve: {var} is not a free price of the steady state (free: {', '.join(asm.free_keys)})")
    if not 1 <= K <= 64:
        raise SystemExit("--ss-curve: K must be 1..64 (one batch)")
    p = np.tile(np.array([m.ss_initial.guesses.get(k, 1.0) for k in asm.free_keys], dtype=np.float64)[:, None], (1, K))
    line = np.linspace(lo, hi, K)
    p[asm.free_keys.index(var)] = line
    t0 = time.perf_counter()
    xVals, _, _, status = asm.batch(p)
    wall = time.perf_counter() - t0
    hb = h.household_block(m)
    iters, ms = asm.last_batch_iters, hb.last_ss_batch_timings()
    cs = m.compspec
    T_pad = 1 + cs.max_lag + cs.max_lead
    het = vars_of_type(m, "heterogeneous")
    points = []
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in range(K):
            ok = status[k] == 0
            z = Residuals(np.tile(xVals[:, k][:, None], (1, T_pad)), m) if ok else None
            points.append({var: float(line[k]), "status": int(status[k]),
                           **({name: float(xVals[asm.all_keys.index(name), k]) for name in het} if ok else {}),
                           "residual_norm": float(np.linalg.norm(z)) if ok else None,
                           "value_steps": int(iters[k, 0]), "distribution_iterations": int(iters[k, 1])})
    return {"grid": f"{n_a}x{n_e}", "line": {"var": var, "lo": lo, "hi": hi, "K": K}, "batches": 1, "wall_s": round(wall, 4),
            "value_loops_ms": round(ms[0], 3), "distribution_loops_ms": round(ms[1], 3), "points": points}


def solve_permanent(n_a=200, n_e=3, T=150, Z_end=1.03, eps=1e-9, verbose=False):
    """The two-steady-state scenario of the reference YAML (`ending:` block, KrusellSmith.yaml:109-116): TFP moves
    to Z_end for good in period 1. The path starts from the initial steady state (KS_0, D_0 = ss_initial), the terminal
    value is the ending steady state's (BackwardIteration.jl:85), Newton starts at the ending steady state repeated and
    uses the sequence-space Jacobian there."""
    import hank_amd as h
    import hank_amd.parallel  # noqa: F401
    ov = {"T": T, "dimensions": {"wealth": {"n": n_a}, "productivity": {"n": n_e}},
          "steady_states": {"ending": {"fixed": {"Z": Z_end}, "guesses": {"r": 0.04, "w": 1.0, "Y": 1.5, "KS": 3.5}}}}
    m = h.build_model_from_yaml(str(ROOT / "examples" / "krusell_smith.yaml"), overrides=ov)
    t0 = time.perf_counter()
    ss_i, ss_e = h.get_SteadyStates(m)
    t_ss = time.perf_counter() - t0
    P = T - 1
    Z = np.full(P, float(Z_end))
    x0 = np.tile(np.array([ss_e.vars[k] for k in ("Y", "KS", "r", "w")]), P)
    t0 = time.perf_counter()
    J = h.getSteadyStateJacobian(ss_e, m)
    x = h.NewtonRaphsonHANK(x0, J, {"Z": Z}, m, ss_i, ss_e, ε=eps, verbose=verbose)
    t_solve = time.perf_counter() - t0
    lin = h.LinearizedFunction(x, {"Z": Z}, m, ss_i, ss_e)
    return {"grid": f"{n_a}x{n_e}", "T": T, "shock": f"Z: 1 -> {Z_end} for good", "steady_states_s": round(t_ss, 3),
            "newton_iterations": h.NewtonRaphsonHANK.iterations, "residual_norm": float(np.linalg.norm(lin.Fx)),
            "wall_to_converged_path_s": round(t_solve, 3), "KS_start": ss_i.vars["KS"], "KS_end": ss_e.vars["KS"],
            "KS_path_first_last": [float(x.reshape(4, P, order="F")[1, 0]), float(x.reshape(4, P, order="F")[1, -1])]}, x, ss_i, ss_e


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-a", type=int, default=500)
    ap.add_argument("--n-e", type=int, default=4)
    ap.add_argument("--T", type=int, default=300)
    ap.add_argument("--shock", type=float, default=0.01)
    ap.add_argument("--permanent", type=float, default=None, metavar="Z_END", help="two-steady-state scenario: Z jumps to Z_END for good")
    ap.add_argument("--verbose", action="store_true")
    ap.add_argument("--cold", action="store_true", help="solve the steady state from the YAML guesses (no fixture)")
    ap.add_argument("--inner", default="fixed_point", choices=["fixed_point", "krylov"], help="y-iteration: the reference's damped fixed point or GMRES on J(x) preconditioned by the steady-state Jacobian")
    ap.add_argument("--jacobian", default="toeplitz", choices=["toeplitz", "columns"])
    ap.add_argument("--step", default="full", choices=["full", "backtrack"], help="Newton's step rule: the reference's full step, or backtracking on ½‖F‖² with the trial steps x − 2^-j y in one hank_primal_batch")
    ap.add_argument("--scale", default=None, metavar="S1,S2,...", help="the nonlinear responses to the shock at these multiples (e.g. 0.5,1,2,-1), solved in lockstep from ONE hank_primal_batch per round; each peak response beside the first-order one from J̅")
    ap.add_argument("--gradient", action="store_true", help="the gradient of ½‖F(x)‖² at the starting point: one hank_vjp against n_hh·P JVP columns")
    ap.add_argument("--boundary-gradient", action="store_true", help="the gradient of ½‖F(x)‖² with respect to the boundary (V_T, D_0) at the starting point: one hank_vjp_boundary, checked against two hank_jvp_boundary directions")
    ap.add_argument("--ss-curve", nargs=4, default=None, metavar=("VAR", "LO", "HI", "K"), help="the steady state's household side along a line in the free prices (VAR from LO to HI in K points, the others at the YAML's guesses) from ONE hank_ss_batch: the heterogeneous aggregates, the residual norm and the value steps per point")
    ap.add_argument("--groups", nargs="+", type=float, default=None, metavar="CDF", help="after the converged path: the wealth groups cut at these steady-state CDF points (0.5 0.9: bottom half, next 40 %%, top decile) — each group's mass, savings and consumption deviation, and the largest gap between the nonlinear path and the linear response J_group · dx")
    ap.add_argument("--group-gradient", action="store_true", help="with --groups: the gradient of ½ Σ (C^g_t − C^g_ss)² over the groups' consumption paths with respect to the household inputs at the converged path, from ONE hank_vjp_group, beside a central difference at three coordinates")
    ap.add_argument("--ss-gradient", action="store_true", help="with --permanent: the gradient of ½‖F(x)‖² with respect to the ending steady state's household prices through V_T (hank_vjp_het_boundary, then hank_ss_vjp), beside a central difference in one random direction")
    a = ap.parse_args()
    if a.group_gradient and not a.groups:
        ap.error("--group-gradient requires --groups")
    import os
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    if world > 1:       # under torch.distributed.run: the Jacobian assembly is shared out over the ranks (one GPU each)
        import torch
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", torch.cuda.current_device()))
    if a.ss_curve:
        out = ss_curve(a.ss_curve[0], float(a.ss_curve[1]), float(a.ss_curve[2]), int(a.ss_curve[3]), a.n_a, a.n_e, a.T)
    elif a.scale:
        out = scale_family(a.n_a, a.n_e, a.T, a.shock, tuple(float(v) for v in a.scale.split(",")))
    elif a.boundary_gradient:
        out = boundary_gradient(a.n_a, a.n_e, a.T, a.shock)
    elif a.gradient:
        out = gradient(a.n_a, a.n_e, a.T, a.shock)
    elif a.ss_gradient:
        out = ss_gradient(a.n_a, a.n_e, a.T, a.permanent if a.permanent is not None else 1.03)
    elif a.permanent is not None:
        out = solve_permanent(a.n_a, a.n_e, a.T, a.permanent, verbose=a.verbose)[0]
    else:
        out, x, m, ss = solve(a.n_a, a.n_e, a.T, a.shock, verbose=a.verbose, cold=a.cold, inner=a.inner, jacobian=a.jacobian, step=a.step, with_model=True)
        if a.groups:
            out["group_outputs"] = group_report(x, m, ss, 1.0 + a.shock * 0.8 ** np.arange(1, a.T), a.groups)
            if a.group_gradient:
                out["group_gradient"] = group_gradient(x, m, ss, 1.0 + a.shock * 0.8 ** np.arange(1, a.T), a.groups)
    out["n_gpus"] = world
    if rank == 0:
        print(json.dumps(out))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()

