#!/usr/bin/env python
"""dev: the Toeplitz J̅ of every heterogeneous output (hank_fake_news_het, csrc/hank_jacobian.h). Medians of --reps timed calls
after one warm-up, all in one process:
  1. hank_fake_news against hank_fake_news_het(n) for n = 1 .. the family's maximum, at a stationary primal: KS 2000x11, T=300
     and the one-asset HANK 1000x7, T=500;
  2. getSteadyStateJacobian method="toeplitz" against method="columns" for the goods and the sticky-wage one-asset HANK at
     1000x7, T=500, and for Krusell-Smith with heterogeneous: [KD, Value] at 2000x11, T=300 (with max |Jt - Jc| / max |Jc|).
--quick: one call of each device entry at the HANK size and no J̅ (the rocprofv3 kernel-trace run).
Output: one line per configuration (profiles/fake_news_het.log)."""
import argparse
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

torch.cuda.init()
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import hank_amd as h  # noqa: E402
from hank_amd.BackwardIteration import household_inputs  # noqa: E402
from conftest import ks_setup  # noqa: E402
from examples.solve_hank import build  # noqa: E402


def med(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def stationary_block(m, ss):
    P = m.compspec.T - 1
    x = np.tile(np.array([ss.vars[k] for k in h.vars_of_type(m, "endogenous")]), P)
    exog = {k: np.full(P, float(ss.vars[k])) for k in h.vars_of_type(m, "exogenous")}
    xhh = np.asarray(household_inputs(x, exog, m)[0])
    wd, pd_ = m.heterogeneity["wealth"], m.heterogeneity["productivity"]
    hb = h.HouseholdBlock(wd.grid, pd_.grid, pd_.transition, m.params.β, m.params.γ, m.params.borrow_cons, m.compspec.T,
                          m.value_fn.value_fn_id)
    hb.set_boundary(ss.value, ss.D)
    hb.primal(xhh)
    return hb


def device_entries(label, m, ss, reps):
    hb = stationary_block(m, ss)
    n_max = len(m.value_fn.outputs)
    if reps == 0:
        hb.fake_news(); hb.fake_news_het(n_max); torch.cuda.synchronize()
        print(f"{label} | one call of fake_news and fake_news_het({n_max})", flush=True)
        hb.close()
        return
    t0 = med(hb.fake_news, reps)
    print(f"{label} | hank_fake_news | {t0:.2f} ms", flush=True)
    for n in range(1, n_max + 1):
        tn = med(lambda: hb.fake_news_het(n), reps)
        print(f"{label} | hank_fake_news_het({n}) | {tn:.2f} ms | x{tn / t0:.2f} of hank_fake_news", flush=True)
    hb.close()


def jacobians(label, m, ss, reps):
    Jt = h.getSteadyStateJacobian(ss, m, method="toeplitz").toarray()
    Jc = h.getSteadyStateJacobian(ss, m, method="columns").toarray()
    err = np.max(np.abs(Jt - Jc)) / np.max(np.abs(Jc))
    tt = med(lambda: h.getSteadyStateJacobian(ss, m, method="toeplitz"), reps)
    tc = med(lambda: h.getSteadyStateJacobian(ss, m, method="columns"), reps)
    print(f"{label} | J̅ n={Jt.shape[0]} | toeplitz {tt:.1f} ms | columns {tc:.1f} ms | columns / toeplitz {tc / tt:.1f} | "
          f"max|Jt-Jc|/max|Jc| {err:.2e}", flush=True)


ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--quick", action="store_true")
a = ap.parse_args()
print(f"device: {torch.cuda.get_device_name(0)}; medians of {a.reps}", flush=True)

mw, ssw = build(1000, 7, 500, "one_asset_hank_wages.yaml")
if a.quick:
    device_entries("HANK wages 1000x7 T=500", mw, ssw, 0)
    sys.exit(0)
mk, ssk = ks_setup(2000, 11, 300)[:2]
device_entries("KS 2000x11 T=300", mk, ssk, a.reps)
device_entries("HANK wages 1000x7 T=500", mw, ssw, a.reps)
jacobians(f"HANK wages 1000x7 T=500 {list(h.vars_of_type(mw, 'heterogeneous'))}", mw, ssw, a.reps)
mg, ssg = build(1000, 7, 500, "one_asset_hank_goods.yaml")
jacobians(f"HANK goods 1000x7 T=500 {list(h.vars_of_type(mg, 'heterogeneous'))}", mg, ssg, a.reps)
src = (ROOT / "examples" / "krusell_smith.yaml").read_text()
line = '    - {name: "KD", description: "capital demand (aggregate household savings)"}\n'
with tempfile.TemporaryDirectory() as d:
    spec = Path(d) / "ks_value.yaml"
    spec.write_text(src.replace(line, line + '    - {name: "Value", description: "aggregate value"}\n'))
    mv = h.build_model_from_yaml(str(spec), overrides={"T": 300, "dimensions": {"wealth": {"n": 2000}, "productivity": {"n": 11}}})
ssv, _ = h.get_SteadyStates(mv)
jacobians("KS 2000x11 T=300 [KD, Value]", mv, ssv, a.reps)
