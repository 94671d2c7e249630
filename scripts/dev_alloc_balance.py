#!/usr/bin/env python
"""dev: every path of the host library that allocates or frees device memory, once, so that a HIP-API trace can count the calls
(the counts of two builds are compared: profiles/device_owner_alloc_balance.txt). Host-pointer entries and numpy only.
    rocprofv3 --hip-trace --stats -d OUT -- python scripts/dev_alloc_balance.py          (HANK_HIP_LIB selects the library)
1. tests/test_gpu_lifetime.py's churn: three cycles over the four schedules of create, every entry, close, close;
2. its eviction sequence under HANK_TAN_CACHE=1, every schedule: hank_jvp at N = 2, 3 and hank_vjp at M = 2, 3, four times each;
3. at a steady state (Krusell-Smith 50x2, T = 20; the default schedule and the launches): hank_fake_news, hank_fake_news_het (the
   workspace grows), the non-affine outputs (the record's f, f_c and S, allocated once per context; hx_slab's
   direction-dependent buffers, grown once), hank_vfi, hank_stationary_dist and the four granular steps."""
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import hank_amd as h  # noqa: E402
import cases as vc  # noqa: E402
from conftest import ks_setup  # noqa: E402
from test_gpu_lifetime import SCHEDULES, _inputs, _use_everything  # noqa: E402

m, V, D, xhh, _, y, yb = _inputs()
for cycle in range(3):
    for sched in SCHEDULES:
        hb = vc.block(h, m, sched)
        _use_everything(hb, V, D, xhh, y, yb)
        hb.close(); hb.close()
print("churn done")

os.environ["HANK_TAN_CACHE"] = "1"
for sched in SCHEDULES:
    hb = vc.block(h, m, sched)
    hb.set_boundary(V, D)
    hb.primal(xhh)
    n0 = hb.stats()["tangent_workspaces_allocated"]
    for _ in range(4):
        for n in (2, 3):
            hb.jvp(np.ascontiguousarray(y[:, :, :n]))
    for _ in range(4):
        for n in (2, 3):
            hb.vjp(np.ascontiguousarray(yb[:, :, :n]), 2)
    assert hb.stats()["tangent_workspaces_allocated"] == n0 + 16
    hb.close()
os.environ.pop("HANK_TAN_CACHE")
print("eviction done")

ms, ss, _ = ks_setup(50, 2, 20)
P = ms.compspec.T - 1
x0 = np.tile(np.array([[ss.vars["r"]], [ss.vars["w"]]]), (1, P))
rng = np.random.default_rng(0)
for sched in (None, "launch"):
    hb = vc.block(h, ms, sched)
    hb.set_boundary(ss.value, ss.D)
    hb.primal(x0)
    hb.fake_news()
    hb.set_het_outputs(3)
    hb.fake_news_het(3)
    y1, y4 = rng.standard_normal((2, P, 1)), rng.standard_normal((2, P, 4))
    hb.jvp(y1); hb.het_outputs(3, y1)
    hb.jvp(y4); hb.het_outputs(3, y4)
    xt = [ss.vars["r"], ss.vars["w"]]
    v, pol, it, _ = hb.vfi(np.ones((50, 2)), xt, 1e-9)
    Dst, steps = hb.stationary_dist(pol, tol=1e-12)
    hb.backward_step(v, xt)
    hb.backward_step_dual(v, rng.standard_normal((50, 2, 3)), xt, rng.standard_normal((2, 3)))
    hb.forward_step(pol, Dst)
    hb.forward_step_dual(pol, rng.standard_normal((50, 2, 3)), Dst, rng.standard_normal((50, 2, 3)))
    print(f"steady state ({sched}): vfi {it} steps, power method {steps} steps, stats {hb.stats()}")
    hb.close()
print("done")
