#!/usr/bin/env python
"""dev: what the first hank_jvp directly behind a one-pass persistent Dual pass costs (MI355X, the benched shape 2000x11, T = 300).

    python scripts/dev_jvp_after_dual.py [--reps 10] [--tangents 32]

The lean front of that pass (k_xdual_front, HANK_XDUAL_FRONT=1) leaves lo, lw, ig and start of the lottery record unwritten; the
first reader pays one k_lottery (ensure_lottery) next to the k_xlwg_build it has always paid. Per repetition: hank_primal_jvp_dev,
then two hank_jvp_dev at that record, each timed by a host clock around a stream synchronisation and by hank_last_timings (the
tangent sweeps alone, which leave the deferred launches out). Run it once per library / knob (HANK_HIP_LIB, HANK_XDUAL_FRONT) and
compare the printed JSON lines."""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tangents", type=int, default=32)
    a = ap.parse_args()
    import torch
    import hank_amd as h
    from bench import WORKLOADS, load_or_solve_ss
    from conftest import ks_paths

    wl = WORKLOADS["ks_2000x11_T300_N32"]
    m, ss = load_or_solve_ss(wl["n_a"], wl["n_e"], wl["T"])
    P, N = wl["T"] - 1, a.tangents
    x, _ = ks_paths(m, ss, "x1", 0.01)
    dev = torch.device("cuda", 0)
    hb = h.household_block(m)
    hb.set_boundary(ss.value, ss.D)
    rng = np.random.default_rng(1000)
    d_x = torch.from_numpy(np.asfortranarray(x[2:4]).reshape(-1, order="F").copy()).to(dev)
    d_dx = torch.from_numpy(rng.standard_normal(2 * P * N)).to(dev)
    d_agg = torch.empty(P, dtype=torch.float64, device=dev)
    d_dagg = torch.empty(P * N, dtype=torch.float64, device=dev)
    first, second, sweeps = [], [], []
    for rep in range(a.reps + 2):
        hb.primal_jvp_dev(d_x.data_ptr(), d_dx.data_ptr(), N, d_agg.data_ptr(), d_dagg.data_ptr())
        hb.sync()
        t0 = time.perf_counter()
        hb.jvp_dev(d_dx.data_ptr(), N, d_dagg.data_ptr())
        hb.sync()
        t1 = time.perf_counter()
        tm = hb.last_timings()
        hb.jvp_dev(d_dx.data_ptr(), N, d_dagg.data_ptr())
        hb.sync()
        t2 = time.perf_counter()
        if rep >= 2:      # (the first repetitions allocate the workspace of this width)
            first.append(1e3 * (t1 - t0)); second.append(1e3 * (t2 - t1))
            sweeps.append(tm["tangent_backward"]["ms"] + tm["tangent_forward"]["ms"])
    hb.check()
    print(json.dumps({"lib": os.path.basename(os.environ.get("HANK_HIP_LIB", "tree")), "HANK_XDUAL_FRONT": os.environ.get("HANK_XDUAL_FRONT"), "N": N, "reps": a.reps,
                      "first_jvp_after_dual_ms": {"median": float(np.median(first)), "min": min(first), "max": max(first)},
                      "second_jvp_ms": {"median": float(np.median(second)), "min": min(second), "max": max(second)},
                      "first_jvp_sweeps_ms_last_timings": float(np.median(sweeps)), "fallbacks": hb.stats()["fallbacks"]}))


if __name__ == "__main__":
    main()
