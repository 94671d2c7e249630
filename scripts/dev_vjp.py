#!/usr/bin/env python
"""dev: hank_vjp against its yardstick. A VJP batch moves the same algorithmic bytes as a JVP batch of the same width, so the
yardstick is the launch family's hank_jvp (HANK_SCHEDULE=launch) at a recorded primal: hank_last_timings' tangent backward +
forward sweep against hank_last_vjp_timings' Sweep A + Sweep B, same process, alternating, medians of 5 after warm-up, at
Krusell-Smith 2000x11, T=300 for M = N in {1, 32, 256} and at the one-asset HANK 1000x7, T=500, M = 32.

    python scripts/dev_vjp.py [--log profiles/vjp.log] [--trace]      --trace: one short run for a kernel trace (no timing table)
"""
import argparse
import os
import sys
from pathlib import Path

import numpy as np
import torch

torch.cuda.init()       # before libhank_hip loads its HIP runtime (the other order leaves torch without a device)

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import hank_amd as h  # noqa: E402
from conftest import ks_paths, ks_setup  # noqa: E402


def block(m):
    os.environ["HANK_SCHEDULE"] = "launch"
    wd, pd_ = m.heterogeneity["wealth"], m.heterogeneity["productivity"]
    hb = h.HouseholdBlock(wd.grid, pd_.grid, pd_.transition, m.params.β, m.params.γ, m.params.borrow_cons, m.compspec.T, m.value_fn.value_fn_id)
    os.environ.pop("HANK_SCHEDULE", None)
    return hb


def cases():
    m, ss, _ = ks_setup(2000, 11, 300)
    x, _ = ks_paths(m, ss, "x1", 0.01)
    yield "KS 2000x11 T=300", m, ss, x[2:4], (1, 32, 256)
    from examples.solve_hank import build
    m, ss = build(1000, 7, 500)
    t = np.arange(m.compspec.T - 1)
    x = np.stack([ss.vars["r"] + 0.002 * 0.8 ** t, ss.vars["om"] * (1 + 0.01 * 0.7 ** t), ss.vars["Tr"] * (1 - 0.02 * 0.9 ** t)])
    yield "HANK 1000x7 T=500", m, ss, x, (32,)


def measure(out, trace=False):
    for name, m, ss, x, widths in cases():
        hb = block(m)
        hb.set_boundary(ss.value, ss.D)
        hb.primal(x)
        P, rng = hb.P, np.random.default_rng(0)
        for M in widths:
            y, yb = rng.standard_normal((hb.n_hh, P, M)), rng.standard_normal((P, 1, M))
            jv, vj = [], []
            for k in range(1 if trace else 7):          # two warm-up rounds (allocation, graph capture), five timed
                dagg = hb.jvp(y)
                t = hb.last_timings()
                xbar = hb.vjp(yb, 1)
                v = hb.last_vjp_timings()
                if k >= 2:
                    jv.append((t["tangent_backward"]["ms"], t["tangent_forward"]["ms"]))
                    vj.append((v["sweep_a"]["ms"], v["sweep_b"]["ms"]))
            if trace:
                continue
            pair = abs(np.sum(yb[:, 0, :] * dagg) - np.sum(xbar * y)) / np.sum(np.abs(xbar * y))
            jb, jf = np.median(jv, axis=0)
            va, vb = np.median(vj, axis=0)
            line = (f"{name} M=N={M}: jvp back {jb:.3f} + fwd {jf:.3f} = {jb + jf:.3f} ms | vjp A {va:.3f} + B {vb:.3f} = {va + vb:.3f} ms | "
                    f"ratio {(va + vb) / (jb + jf):.2f} | <ybar, J y> vs <xbar, y>: {pair:.1e}")
            print(line, flush=True)
            out.append(line)
        hb.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=str(ROOT / "profiles" / "vjp.log"))
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    lines = []
    measure(lines, a.trace)
    if not a.trace:
        Path(a.log).write_text("\n".join(lines) + "\n")
