#!/usr/bin/env python
"""dev: the cost of the non-affine heterogeneous outputs (Value, UCE; csrc/hank_hetx.h). Times hank_primal_jvp followed by
hank_get_het_outputs at 2000x11, T=300 for N in {1, 32, 256} with n_het = 2 (today's outputs) and n_het = 3 (+ Value), and the
one-asset HANK at 1000x7, T=500 with n_het = 4 (+ Value, UCE). Medians of --reps timed calls after one warm-up; the memo is
switched off so that every call runs the Dual pass. Output: one line per configuration (profiles/r06_het_outputs.log)."""
import argparse
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch

torch.cuda.init()
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
os.environ["HANK_PRIMAL_MEMO"] = "0"
from conftest import ks_paths, ks_setup  # noqa: E402


def block(m):
    import hank_amd as h
    wd, pd_ = m.heterogeneity["wealth"], m.heterogeneity["productivity"]
    return h.HouseholdBlock(wd.grid, pd_.grid, pd_.transition, m.params.β, m.params.γ, m.params.borrow_cons, m.compspec.T,
                            m.value_fn.value_fn_id)


def timed(hb, x, y, n_het, reps):
    hb.set_het_outputs(max(n_het, 2))

    def one():
        t0 = time.perf_counter()
        hb.primal_jvp(x, y)
        t1 = time.perf_counter()
        hb.het_outputs(n_het, y)
        return t1 - t0, time.perf_counter() - t1

    one()
    ts = np.array([one() for _ in range(reps)]) * 1e3
    return np.median(ts[:, 0]), np.median(ts[:, 1]), ts.sum(axis=1).std()


ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
a = ap.parse_args()
print("config | primal_jvp ms | het_outputs ms | total ms | spread (std of totals) ms | family", flush=True)
m, ss, _ = ks_setup(2000, 11, 300)
P = m.compspec.T - 1
x, _ = ks_paths(m, ss, "x1", 0.05)
hb = block(m)
hb.set_boundary(ss.value, ss.D)
for N in (1, 32, 256):
    y = np.random.default_rng(1).standard_normal((2, P, N))
    for n_het in (2, 3):
        pj, ho, sd = timed(hb, x[2:4], y, n_het, a.reps)
        print(f"KS 2000x11 T=300 N={N} n_het={n_het} | {pj:.2f} | {ho:.2f} | {pj + ho:.2f} | {sd:.2f} | {hb.info()['last_tangent_family_name']}", flush=True)
hb.close()

from examples.solve_hank import build  # noqa: E402
m, ss = build(1000, 7, 500, "one_asset_hank_goods.yaml")
P = m.compspec.T - 1
t = np.arange(P)
x = np.stack([ss.vars["r"] + 0.002 * 0.8 ** t, ss.vars["om"] * (1 + 0.01 * 0.7 ** t), ss.vars["Tr"] * (1 - 0.02 * 0.9 ** t)])
hb = block(m)
hb.set_boundary(ss.value, ss.D)
for N in (1, 32):
    y = np.random.default_rng(2).standard_normal((3, P, N))
    for n_het in (2, 4):
        pj, ho, sd = timed(hb, x, y, n_het, a.reps)
        print(f"HANK 1000x7 T=500 N={N} n_het={n_het} | {pj:.2f} | {ho:.2f} | {pj + ho:.2f} | {sd:.2f} | {hb.info()['last_tangent_family_name']}", flush=True)
hb.close()
