#!/usr/bin/env python
"""dev: what hank_jvp_het costs against the two calls it replaces.

    python scripts/dev_jvp_het.py [ks|hank ...]      log: profiles/jvp_het.log

Per shape and width, in ONE process, alternating, device-pointer forms, wall time to hank_sync, medians of 5 after warm-up:
  two calls / launch    hank_jvp under HANK_SCHEDULE=launch, then hank_get_het_outputs(n_het)          (the yardstick, run twice: its spread)
  two calls / default   the same pair with the default schedule's hank_jvp in front                     (what LinearizedFunction pays)
  hank_jvp_het          one call, unseeded; and seeded with dV_P and dD_0
and the TAN_FWD span of hank_jvp_het next to that of the launch family's hank_jvp: the price of the slots."""
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

torch.cuda.init()       # before libhank_hip loads its HIP runtime

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import hank_amd as h  # noqa: E402
import cases  # noqa: E402
from conftest import ks_paths, ks_setup  # noqa: E402

DEV = torch.device("cuda", 0)
REPS = 5


def dev(arr):
    return torch.from_numpy(np.asfortranarray(arr).reshape(-1, order="F").copy()).to(DEV)


def timed(hb, fn):
    t0 = time.perf_counter()
    fn()
    hb.sync()
    return 1e3 * (time.perf_counter() - t0)


def run(label, m, ss, x, n_het, Ns, log):
    V, D = np.asarray(ss.value), np.asarray(ss.D)
    hbs = {}
    for sched in ("launch", None):
        hb = cases.block(h, m, sched)
        hb.set_boundary(V, D); hb.set_het_outputs(n_het); hb.primal(x)
        hbs[sched] = hb
    hbL, hbD = hbs["launch"], hbs[None]
    P, nh, G = hbL.P, hbL.n_hh, hbL.G
    for N in Ns:
        rng = np.random.default_rng(N)
        d_y = dev(rng.standard_normal((nh, P, N)) * 1e-2)
        d_dV = dev(rng.standard_normal((G, N)) * np.abs(V).reshape(-1, order="F")[:, None])
        d_dD = dev(rng.uniform(0, 1, (G, N)) / G)
        d_o1 = torch.empty(P * N, dtype=torch.float64, device=DEV)
        d_o = torch.empty(P * n_het * N, dtype=torch.float64, device=DEV)

        def two(hb):
            hb.jvp_dev(d_y.data_ptr(), N, d_o1.data_ptr())
            hb.het_outputs_dev(n_het, d_y.data_ptr(), N, 0, d_o.data_ptr())
        paths = {
            "two calls / launch (a)": lambda: two(hbL),
            "hank_jvp_het": lambda: hbL.jvp_het_dev(n_het, d_y.data_ptr(), 0, 0, N, d_o.data_ptr()),
            "two calls / launch (b)": lambda: two(hbL),
            "two calls / default": lambda: two(hbD),
            "hank_jvp_het seeded": lambda: hbL.jvp_het_dev(n_het, d_y.data_ptr(), d_dV.data_ptr(), d_dD.data_ptr(), N, d_o.data_ptr()),
        }
        owner = {k: (hbD if "default" in k else hbL) for k in paths}
        for k, fn in paths.items():          # warm-up: workspaces, graphs, the record's f and f_c
            for _ in range(2):
                timed(owner[k], fn)
        ms = {k: [] for k in paths}
        spans = {}
        for _ in range(REPS):
            for k, fn in paths.items():
                ms[k].append(timed(owner[k], fn))
                if k in ("hank_jvp_het", "hank_jvp_het seeded"):
                    spans.setdefault(k, []).append(hbL.last_timings()["tangent_forward"]["ms"])
            hbL.jvp_dev(d_y.data_ptr(), N, d_o1.data_ptr()); hbL.sync()
            spans.setdefault("hank_jvp / launch", []).append(hbL.last_timings()["tangent_forward"]["ms"])
            hbL.jvp_boundary_dev(d_y.data_ptr(), d_dV.data_ptr(), d_dD.data_ptr(), N, d_o1.data_ptr()); hbL.sync()
            spans.setdefault("hank_jvp_boundary", []).append(hbL.last_timings()["tangent_forward"]["ms"])
        line = f"{label} n_het={n_het} N={N:4d} | " + " | ".join(f"{k} {statistics.median(v):7.3f} ms" for k, v in ms.items())
        line2 = f"{label} n_het={n_het} N={N:4d} | TAN_FWD span: " + " | ".join(f"{k} {statistics.median(v):7.3f} ms" for k, v in spans.items()) \
            + f" | family of the default hank_jvp: {hbD.info()['last_tangent_family_name']}"
        for ln in (line, line2):
            print(ln, flush=True)
            log.write(ln + "\n"); log.flush()
    for hb in hbs.values():
        hb.close()


if __name__ == "__main__":
    which = sys.argv[1:] or ["ks", "hank"]
    out = ROOT / "profiles" / "jvp_het.log"
    with open(os.environ.get("DEV_JVP_HET_LOG", out), "a") as log:
        if "ks" in which:
            m, ss, _ = ks_setup(2000, 11, 300)
            run("KS 2000x11 T=300", m, ss, np.ascontiguousarray(ks_paths(m, ss, "x1", 0.01)[0][2:4]), 3, (1, 32, 256), log)
        if "hank" in which:
            m, ss = cases.hank_economy(1000, 7, 500)
            run("HANK 1000x7 T=500", m, ss, cases.hank_x(ss, m.compspec.T - 1), 4, (1, 32), log)
