#!/usr/bin/env python
"""Timings of hank_primal_batch against K sequential hank_primal, reported, not gated.

    python scripts/dev_primal_batch.py [--small] [--solve] > profiles/primal_batch.log

Per grid (Krusell-Smith 2000x11, T = 300 at its steady state, and 1000x7, T = 500 at cases.shape's cheap boundary; --small: 50x2 and
70x3, T = 12) and K in {1, 2, 4, 8, 16, 32}: the HIP-event times of the batch's backward and forward chains (hank_last_batch_timings),
medians of 5 calls after a warm-up, beside the yardsticks — K x the time of ONE hank_primal in the same process, on the default
schedule (the persistent sweeps) and on HANK_SCHEDULE=launch (the per-period launches): the sum of primal_backward and
primal_forward of hank_last_timings, medians of 5 after a warm-up. The yardsticks are the existing entries, never the batch. The
scenarios are geometric deviations from the constant path, one size and decay per scenario. --solve: the wall time of
examples/solve_transition.py's Newton solve on the headline grid with step="backtrack" against step="full"."""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

KS = (1, 2, 4, 8, 16, 32)


def scenarios(base, amp, P, K):
    t = np.arange(P)
    return np.stack([base[:, None] + (-1.0) ** k * (0.25 + 0.75 * k / max(K - 1, 1)) * amp[:, None] * (0.5 + 0.4 * k / max(K - 1, 1)) ** t[None, :] for k in range(K)], axis=2)


def primal_ms(hb, x):
    ts = []
    for it in range(6):
        hb.primal(x)
        t = hb.last_timings()
        if it:
            ts.append(t["primal_backward"]["ms"] + t["primal_forward"]["ms"])
    return statistics.median(ts)


def grid(hank, name, m, V, D, base, amp):
    import cases
    P = m.compspec.T - 1
    x1 = scenarios(base, amp, P, 2)[:, :, 1]
    yard = {}
    for sched in (None, "launch"):
        hb = cases.block(hank, m, sched)
        hb.set_boundary(V, D)
        yard[sched] = primal_ms(hb, x1)
        fam = hb.stats()["schedule"]
        hb.close()
        print(f"{name}: one hank_primal, HANK_SCHEDULE={sched or 'default'} (schedule {fam}): {yard[sched]:.3f} ms (backward + forward, median of 5)")
    hb = cases.block(hank, m, None)
    hb.set_boundary(V, D)
    print(f"\n{name}: G = {hb.G}, P = {P}, {-(-hb.n_a // 32)} row blocks per scenario and period")
    print("| K | backward ms | forward ms | batch ms | K x persistent primal ms | K x launch primal ms | batch / K persistent | batch / K launch | ms per scenario |")
    print("|---|---|---|---|---|---|---|---|---|")
    for K in KS:
        xs = scenarios(base, amp, P, K)
        tb, tf = [], []
        for it in range(6):
            _, status = hb.primal_batch(xs)
            assert not status.any(), status
            b, f = hb.last_batch_timings()
            if it:
                tb.append(b); tf.append(f)
        b, f = statistics.median(tb), statistics.median(tf)
        print(f"| {K} | {b:.3f} | {f:.3f} | {b + f:.3f} | {K * yard[None]:.3f} | {K * yard['launch']:.3f} | {(b + f) / (K * yard[None]):.2f} | {(b + f) / (K * yard['launch']):.2f} | {(b + f) / K:.3f} |")
    hb.close()


def solve(hank, m, ss):
    """the Newton solve of examples/solve_transition.py at a 1 % TFP shock, both step rules, wall time of the second of two solves"""
    P = m.compspec.T - 1
    Z = 1.0 + 0.01 * 0.8 ** np.arange(1, P + 1)
    x0 = np.tile(np.array([ss.vars[k] for k in ("Y", "KS", "r", "w")]), P)
    J = hank.getSteadyStateJacobian(ss, m)
    print("\n| step rule | wall s (second solve) | outer iterations | accepted steps |")
    print("|---|---|---|---|")
    for step in ("full", "backtrack"):
        for it in range(2):
            t0 = time.perf_counter()
            hank.NewtonRaphsonHANK(x0, J, {"Z": Z}, m, ss, ss, ε=1e-9, step=step)
            dt = time.perf_counter() - t0
        print(f"| {step} | {dt:.3f} | {hank.NewtonRaphsonHANK.iterations} | {hank.NewtonRaphsonHANK.step_sizes} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--solve", action="store_true")
    a = ap.parse_args()
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    import cases
    import hank_amd as hank
    from conftest import ks_setup
    if not hank.hip.device_available():
        sys.exit("no gfx950 device: nothing is measured")
    m, ss, _ = ks_setup(*((50, 2, 12) if a.small else (2000, 11, 300)))
    r, w = ss.vars["r"], ss.vars["w"]
    grid(hank, f"Krusell-Smith {m.heterogeneity['wealth'].grid.size}x{m.heterogeneity['productivity'].grid.size}, T = {m.compspec.T}", m, np.asarray(ss.value), np.asarray(ss.D),
         np.array([r, w]), np.array([0.004, 0.01 * w]))
    m2, V2, D2, xhh2, _ = cases.shape(*((70, 3, 12) if a.small else (1000, 7, 500)))
    r2, w2 = xhh2[0, 0] - 0.004 * 0.8, xhh2[1, 0] / (1.0 + 0.01 * 0.8)
    grid(hank, f"Krusell-Smith {m2.heterogeneity['wealth'].grid.size}x{m2.heterogeneity['productivity'].grid.size}, T = {m2.compspec.T} (cheap boundary)", m2, V2, D2,
         np.array([r2, w2]), np.array([0.004, 0.01 * w2]))
    if a.solve:
        solve(hank, m, ss)


if __name__ == "__main__":
    main()
