#!/usr/bin/env python
"""dev: hank_vjp_het against its yardstick. The extra outputs (Value, UCE) add 16 bytes per point, period, column block and
output to Sweep A's 44 B of record + 24 M B of state and p̄, and nothing to Sweep B, so the yardstick is hank_vjp at n_het = 2 on
the same record and width: hank_last_vjp_timings of both, same process, alternating, medians of 5 after warm-up, at
Krusell-Smith 2000x11, T=300, n_het = 3 for M in {1, 32, 256} and at the one-asset HANK 1000x7, T=500, n_het = 4, M = 32. The
yardstick runs twice per round: the spread between its two medians is printed next to the ratio. Also the once-per-record cost of
k_hx_record (the first hank_vjp_het after a primal against the second, host clock around a synchronous call).

    python scripts/dev_vjp_het.py [--log profiles/vjp_het.log]
"""
import argparse
import os
import sys
import time
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
    yield "KS 2000x11 T=300", m, ss, x[2:4], 3, (1, 32, 256)
    from examples.solve_hank import build
    m, ss = build(1000, 7, 500)
    t = np.arange(m.compspec.T - 1)
    x = np.stack([ss.vars["r"] + 0.002 * 0.8 ** t, ss.vars["om"] * (1 + 0.01 * 0.7 ** t), ss.vars["Tr"] * (1 - 0.02 * 0.9 ** t)])
    yield "HANK 1000x7 T=500", m, ss, x, 4, (32,)


def byte_model(M, NX):
    return (44 + 24 * M + 16 * NX) / (44 + 24 * M)


def measure(out):
    for name, m, ss, x, n_het, widths in cases():
        hb = block(m)
        hb.set_boundary(ss.value, ss.D)
        hb.set_het_outputs(n_het)
        hb.primal(x)
        P, rng = hb.P, np.random.default_rng(0)
        for M in widths:
            yb = rng.standard_normal((P, n_het, M))
            y2 = np.ascontiguousarray(yb[:, :2, :])
            base, base2, het = [], [], []
            for k in range(7):                          # two warm-up rounds (allocation, graph capture), five timed
                hb.vjp(y2, 2); a = hb.last_vjp_timings()
                hb.vjp_het(yb, n_het); v = hb.last_vjp_timings()
                hb.vjp(y2, 2); b = hb.last_vjp_timings()
                if k >= 2:
                    base.append((a["sweep_a"]["ms"], a["sweep_b"]["ms"]))
                    het.append((v["sweep_a"]["ms"], v["sweep_b"]["ms"]))
                    base2.append((b["sweep_a"]["ms"], b["sweep_b"]["ms"]))
            (a0, b0), (a1, b1), (ah, bh) = np.median(base, axis=0), np.median(base2, axis=0), np.median(het, axis=0)
            line = (f"{name} M={M} n_het={n_het}: hank_vjp A {a0:.3f} + B {b0:.3f} ms (again: A {a1:.3f} + B {b1:.3f}; spread A {abs(a1 - a0) / a0:.1%}, "
                    f"B {abs(b1 - b0) / b0:.1%}) | hank_vjp_het A {ah:.3f} + B {bh:.3f} ms | Sweep A ratio {ah / a0:.3f} (byte model "
                    f"{byte_model(M, n_het - 2):.3f}) | Sweep B ratio {bh / b0:.3f}")
            print(line, flush=True)
            out.append(line)
        # k_hx_record once per record: the first hank_vjp_het after a primal against the second
        M = widths[-1] if 32 not in widths else 32
        yb = rng.standard_normal((P, n_het, M))
        firsts, seconds = [], []
        for _ in range(5):
            hb.primal(x); hb.sync()
            hb.vjp(np.ascontiguousarray(yb[:, :2, :]), 2)                # (Sweep B's segment starts are rebuilt here, not in the timed call)
            t0 = time.perf_counter(); hb.vjp_het(yb, n_het); t1 = time.perf_counter(); hb.vjp_het(yb, n_het); t2 = time.perf_counter()
            firsts.append(t1 - t0); seconds.append(t2 - t1)
        line = (f"{name} M={M}: first hank_vjp_het after a primal {1e3 * np.median(firsts):.3f} ms, second {1e3 * np.median(seconds):.3f} ms (host clock): "
                f"k_hx_record ({n_het - 2 if n_het < 4 else 2} outputs) ~ {1e3 * (np.median(firsts) - np.median(seconds)):.3f} ms")
        print(line, flush=True)
        out.append(line)
        hb.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=str(ROOT / "profiles" / "vjp_het.log"))
    a = ap.parse_args()
    lines = []
    measure(lines)
    Path(a.log).write_text("\n".join(lines) + "\n")
