#!/usr/bin/env python
"""dev: hank_jvp_boundary and hank_vjp_boundary against their yardsticks. The boundary products run the launch family's sweeps
with three state-sized arrays more per sweep (the seed's layout change and its contraction, or the export of a state), so the
byte model predicts 1 + 3 / P of the yardstick: hank_jvp under HANK_SCHEDULE=launch (hank_last_timings' tangent backward +
forward sweep) and hank_vjp (hank_last_vjp_timings' Sweep A + Sweep B), same process, same record, alternating, medians of 5
after warm-up; the yardstick is run twice per round (before and after the boundary product) for its spread. Krusell-Smith
2000x11, T=300, widths 1, 32, 256.

    python scripts/dev_boundary.py [--log profiles/boundary.log]
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


def measure(out, n_a=2000, n_e=11, T=300, widths=(1, 32, 256)):
    m, ss, _ = ks_setup(n_a, n_e, T)
    x, _ = ks_paths(m, ss, "x1", 0.01)
    hb = block(m)
    hb.set_boundary(ss.value, ss.D)
    hb.primal(x[2:4])
    P, rng = hb.P, np.random.default_rng(0)
    out.append(f"KS {n_a}x{n_e} T={T}: byte model 1 + 3/P = {1 + 3 / P:.4f}")
    for W in widths:
        y, yb = rng.standard_normal((hb.n_hh, P, W)), rng.standard_normal((P, 1, W))
        dV = rng.standard_normal((hb.n_a, hb.n_e, W)) * np.abs(np.asarray(ss.value))[:, :, None]
        dD = rng.uniform(0, 1, (hb.n_a, hb.n_e, W)) / hb.G
        tan = lambda: sum(hb.last_timings()[k]["ms"] for k in ("tangent_backward", "tangent_forward"))      # noqa: E731
        halves = lambda: [hb.last_timings()[k]["ms"] for k in ("tangent_backward", "tangent_forward")]          # noqa: E731
        cot = lambda: sum(hb.last_vjp_timings()[k]["ms"] for k in ("sweep_a", "sweep_b"))                   # noqa: E731
        rows = []
        for k in range(7):          # two warm-up rounds (allocation, graph capture), five timed
            hb.jvp(y); j1 = tan(); h1 = halves()
            dagg = hb.jvp_boundary(y, dV, dD); jb = tan(); hb_ = halves()
            hb.jvp(y); j2 = tan()
            hb.vjp(yb, 1); v1 = cot()
            xb, Vb, Db = hb.vjp_boundary(yb, 1); vb = cot()
            hb.vjp(yb, 1); v2 = cot()
            if k >= 2:
                rows.append((j1, jb, j2, v1, vb, v2, *h1, *hb_))
        j1, jb, j2, v1, vb, v2, b1, f1, bb, fb = np.median(rows, axis=0)
        lhs = np.sum(yb[:, 0, :] * dagg)
        rhs = np.sum(xb * y) + np.sum(Vb * dV) + np.sum(Db * dD)
        line = (f"N=M={W}: jvp {j1:.3f} / {j2:.3f} ms (spread {abs(j1 - j2) / min(j1, j2):.1%}), jvp_boundary {jb:.3f} ms, ratio {jb / (0.5 * (j1 + j2)):.3f} (backward {b1:.3f} -> {bb:.3f}, forward {f1:.3f} -> {fb:.3f}) | "
                f"vjp {v1:.3f} / {v2:.3f} ms (spread {abs(v1 - v2) / min(v1, v2):.1%}), vjp_boundary {vb:.3f} ms, ratio {vb / (0.5 * (v1 + v2)):.3f} | "
                f"<ybar, J (y, dV, dD)> vs <(xbar, Vbar, Dbar), (y, dV, dD)>: {abs(lhs - rhs) / abs(lhs):.1e}")
        print(line, flush=True)
        out.append(line)
    hb.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=str(ROOT / "profiles" / "boundary.log"))
    a = ap.parse_args()
    lines = []
    measure(lines)
    Path(a.log).write_text("\n".join(lines) + "\n")
