#!/usr/bin/env python
"""Timings of hank_ss_batch against K single steady-state solves, reported, not gated.

    python scripts/dev_ss_batch.py [--small] [--no-find-ss] > profiles/ss_batch.log

Per grid (Krusell-Smith 2000x11 and one-asset HANK 1000x7; --small: 50x2 and 30x3) and K in {1, 2, 4, 8, 16, 32, 64}: the
household side of the steady state from a cold start (value ones, D uniform, vfi_tol 1e-11, the power method's defaults) at K price
vectors whose r spreads evenly over +-20 % around the steady state's, the other inputs at the steady state. The scenarios of a
batch of K are a subset of the 64 of the widest one, so that every yardstick is measured once per scenario.

The batch: the HIP-event times of its value loops and distribution loops (hank_last_ss_batch_timings) and the wall time of the
call, medians of 5 calls after a warm-up. The yardsticks, from the same process: the wall time of ONE hank_vfi followed by ONE
hank_stationary_dist per scenario, medians of 5 after a warm-up, summed over the batch's scenarios — on the default schedule (the
persistent launches k_xvfi / k_xstat) and on HANK_SCHEDULE=launch (the per-step launches). The yardsticks are the existing entries,
never the batch. Wall time against wall time decides "wins": all three include their allocations and copies.

Then find_ss on krusell_smith.yaml at 2000x11 with and without batch=True: wall time, vfi_steps, newton_iterations."""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

KS = (1, 2, 4, 8, 16, 32, 64)
TOL = 1e-11
REPS = 5


def subset(K):
    """the scenarios of a batch of K among the 64: evenly spread, both ends included from K = 2"""
    return [32] if K == 1 else [int(round(q)) for q in np.linspace(0, 63, K)]


def single_ms(hb, shape, xs):
    """per scenario: median wall ms of hank_vfi from ones + hank_stationary_dist from uniform, REPS after a warm-up; the step counts"""
    ms, steps = np.zeros(xs.shape[1]), []
    for k in range(xs.shape[1]):
        ts = []
        for it in range(REPS + 1):
            t0 = time.perf_counter()
            _, pol, n_v, _ = hb.vfi(np.ones(shape), xs[:, k], TOL)
            _, n_d = hb.stationary_dist(pol)
            if it:
                ts.append(1e3 * (time.perf_counter() - t0))
        ms[k] = statistics.median(ts)
        steps.append((n_v, n_d))
    return ms, steps


def grid(hank, name, m, base):
    import cases
    n_a, n_e = m.heterogeneity["wealth"].grid.size, m.heterogeneity["productivity"].grid.size
    xs = np.tile(base[:, None], (1, 64))
    xs[0] = base[0] * np.linspace(0.8, 1.2, 64)
    yard, steps = {}, None
    for sched in (None, "launch"):
        hb = cases.block(hank, m, sched)
        yard[sched], st = single_ms(hb, (n_a, n_e), xs)
        fam = hb.stats()["schedule"]
        hb.close()
        steps = steps or st
        print(f"{name}: single solves, HANK_SCHEDULE={sched or 'default'} (schedule {fam}): {yard[sched].min():.2f} .. {yard[sched].max():.2f} ms per scenario "
              f"(median {np.median(yard[sched]):.2f}), value steps {min(s[0] for s in st)} .. {max(s[0] for s in st)}, "
              f"distribution iterations {min(s[1] for s in st)} .. {max(s[1] for s in st)}", flush=True)
    hb = cases.block(hank, m, None)
    print(f"\n{name}: G = {hb.G}, {-(-n_a // 32)} row blocks per scenario, r = {base[0]:.5f} x (0.8 .. 1.2)")
    print("| K | value loops ms | distribution loops ms | batch wall ms | K persistent singles ms | K launch singles ms | batch / persistent | batch / launch "
          "| batch ms per scenario | value steps (max) | distribution iterations (max) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    wins = {None: None, "launch": None}
    for K in KS:
        ks = subset(K)
        tv, td, tw = [], [], []
        for it in range(REPS + 1):
            t0 = time.perf_counter()
            _, _, _, _, iters, status = hb.ss_batch(xs[:, ks], TOL)
            w = 1e3 * (time.perf_counter() - t0)
            assert not status.any(), status
            v, d = hb.last_ss_batch_timings()
            if it:
                tv.append(v); td.append(d); tw.append(w)
        v, d, w = statistics.median(tv), statistics.median(td), statistics.median(tw)
        yp, yl = yard[None][ks].sum(), yard["launch"][ks].sum()
        for sched, y in ((None, yp), ("launch", yl)):
            if w < y and wins[sched] is None:
                wins[sched] = K
            elif w >= y:
                wins[sched] = None
        print(f"| {K} | {v:.2f} | {d:.2f} | {w:.2f} | {yp:.2f} | {yl:.2f} | {w / yp:.2f} | {w / yl:.2f} | {w / K:.2f} | {iters[:, 0].max()} | {iters[:, 1].max()} |", flush=True)
    hb.close()
    for sched in (None, "launch"):
        what = "the persistent singles" if sched is None else "the launched singles"
        print(f"{name}: the batch beats {what} " + (f"from K = {wins[sched]} on" if wins[sched] else "at no K up to 64 (or not from some K on)"))
    print(flush=True)


def find_ss_table(hank, n_a, n_e, T):
    import importlib
    S = importlib.import_module("hank_amd.SteadyState")
    ov = {"T": T, "dimensions": {"wealth": {"n": n_a}, "productivity": {"n": n_e}}}
    print(f"find_ss, krusell_smith.yaml at {n_a}x{n_e}, device VFI, from the YAML guesses (second of two solves)")
    print("| batch | wall s | vfi_steps | newton_iterations | batches | residual norm |")
    print("|---|---|---|---|---|---|")
    for batch in (False, True):
        for it in range(2):
            m = hank.build_model_from_yaml(str(ROOT / "examples" / "krusell_smith.yaml"), overrides=ov)
            t0 = time.perf_counter()
            ss = S.find_ss(m, m.ss_initial, "initial", vfi="device", batch=batch)
            dt = time.perf_counter() - t0
        si = ss.solve_info
        print(f"| {batch} | {dt:.3f} | {si['vfi_steps']} | {si['newton_iterations']} | {si['batches']} | {si['residual_norm']:.3e} |", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-find-ss", action="store_true")
    a = ap.parse_args()
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    import hank_amd as hank
    from conftest import ks_setup
    from examples.solve_hank import build
    if not hank.hip.device_available():
        sys.exit("no gfx950 device: nothing is measured")
    ks = (50, 2, 12) if a.small else (2000, 11, 300)
    m, ss, _ = ks_setup(*ks)
    grid(hank, f"Krusell-Smith {ks[0]}x{ks[1]}", m, np.array([ss.vars["r"], ss.vars["w"]]))
    hk = (30, 3, 10) if a.small else (1000, 7, 10)
    m2, ss2 = build(*hk)
    grid(hank, f"one-asset HANK {hk[0]}x{hk[1]}", m2, np.array([ss2.vars["r"], ss2.vars["om"], ss2.vars["Tr"]]))
    if not a.no_find_ss:
        find_ss_table(hank, *ks)


if __name__ == "__main__":
    main()
