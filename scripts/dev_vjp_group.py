#!/usr/bin/env python
"""dev: the cost of cotangents on group outputs (hank_vjp_group; csrc/hank_adjoint.h: k_adj_dist_grp). Krusell-Smith 2000x11,
T=300, M=32, wealth groups under the three bases. Events on the context's stream around the device-pointer entries, two warm-ups,
the median of --reps timed calls; Sweep A and Sweep B from hank_last_vjp_timings of the last call. Lines:
  hank_vjp_group_dev at K in {4, 12, 32};
  hank_vjp_dev at n_het = 2: the same sweeps without groups, so the ratio is the price of the K loop;
  hank_vjp_het_dev at n_het = 3;
  the forward route to the same gradient of a criterion over (P, K) group paths: 19 batches (598 unit tangents, 32 per batch) of
  hank_jvp_dev + hank_get_group_outputs_dev at K = 12.
Output: profiles/vjp_group.log."""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

torch.cuda.init()
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
from conftest import ks_paths, ks_setup  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--out", default=str(ROOT / "profiles" / "vjp_group.log"))
a = ap.parse_args()

import hank_amd as h  # noqa: E402
from hank_amd.groups import wealth_groups  # noqa: E402

m, ss, _ = ks_setup(2000, 11, 300)
P, M, n_a, n_e = m.compspec.T - 1, 32, 2000, 11
x, _ = ks_paths(m, ss, "x1", 0.05)
wd, pd_ = m.heterogeneity["wealth"], m.heterogeneity["productivity"]
hb = h.HouseholdBlock(wd.grid, pd_.grid, pd_.transition, m.params.β, m.params.γ, m.params.borrow_cons, m.compspec.T, m.value_fn.value_fn_id)
dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(dev)
torch.cuda.set_stream(stream)
hb.set_stream(stream.cuda_stream)
hb.set_boundary(ss.value, ss.D)
hb.set_het_outputs(3)
hb.primal(x[2:4])
rng = np.random.default_rng(0)


def on_device(arr):
    return torch.from_numpy(np.asfortranarray(arr).reshape(-1, order="F").copy()).to(dev)


def timed(call, reps):
    """two warm-ups, then the median (and the spread) of `reps` calls bracketed by events on the context's stream -> ms"""
    for _ in range(2):
        call()
    hb.sync()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def groups(K):
    """K groups: K / 3 wealth groups (quantile edges) under MASS, POLICY and CONS; K = 4: four groups under CONS"""
    nb, bases = (4, [2]) if K == 4 else (K // 3, [0, 1, 2])
    Wg = wealth_groups(ss.D, n_a, n_e, tuple(np.linspace(0.0, 1.0, nb + 1)))
    W = np.concatenate([Wg] * len(bases) + ([Wg[:, :K - nb * len(bases)]] if K > nb * len(bases) else []), axis=1)
    base = np.concatenate([np.repeat(np.array(bases, dtype=np.int32), nb), np.full(K - nb * len(bases), 2, dtype=np.int32)])
    return W, base


lines = ["entry | median ms | min | max | Sweep A ms | Sweep B ms"]


def report(name, call, sweeps=True):
    med, lo, hi = timed(call, a.reps)
    hb.sync()
    t = hb.last_vjp_timings() if sweeps else None
    lines.append(f"{name} | {med:.2f} | {lo:.2f} | {hi:.2f} | " + (f"{t['sweep_a']['ms']:.2f} | {t['sweep_b']['ms']:.2f}" if t else "- | -"))
    print(lines[-1], flush=True)
    return med, t


d_x = torch.empty(2 * P * M, dtype=torch.float64, device=dev)
d_y2, d_y3 = on_device(rng.standard_normal((P, 2, M))), on_device(rng.standard_normal((P, 3, M)))
base_ms, base_t = report("hank_vjp_dev n_het=2 M=32", lambda: hb.vjp_dev(2, d_y2.data_ptr(), M, d_x.data_ptr()))
report("hank_vjp_het_dev n_het=3 M=32", lambda: hb.vjp_het_dev(3, d_y3.data_ptr(), M, d_x.data_ptr()))
grp = {}
for K in (4, 12, 32):
    W, base = groups(K)
    hb.set_group_outputs(W, base)
    d_g = on_device(rng.standard_normal((P, K, M)))
    grp[K] = report(f"hank_vjp_group_dev K={K} M=32", lambda: hb.vjp_group_dev(0, 0, d_g.data_ptr(), M, d_x.data_ptr()))
    report(f"hank_vjp_group_dev K={K} M=32 with agg_bar n_het=2", lambda: hb.vjp_group_dev(2, d_y2.data_ptr(), d_g.data_ptr(), M, d_x.data_ptr()))
# the forward route at K = 12: one batch of 32 tangents, times the 19 batches the 598 inputs take
W, base = groups(12)
hb.set_group_outputs(W, base)
d_dx = on_device(rng.standard_normal((2, P, M)))
d_da, d_dg = torch.empty(P * M, dtype=torch.float64, device=dev), torch.empty(P * 12 * M, dtype=torch.float64, device=dev)


def forward_batch():
    hb.jvp_dev(d_dx.data_ptr(), M, d_da.data_ptr())
    hb.group_outputs_dev(d_dx.data_ptr(), M, 0, d_dg.data_ptr())


fwd_ms, _ = report("hank_jvp_dev + hank_get_group_outputs_dev K=12 N=32 (one batch)", forward_batch, sweeps=False)
nb = -(-2 * P // M)
lines.append(f"forward route, {nb} batches: {nb * fwd_ms:.1f} ms; hank_vjp_group_dev K=12: {grp[12][0]:.2f} ms; ratio {nb * fwd_ms / grp[12][0]:.1f}")
for K in (4, 12, 32):
    lines.append(f"K={K}: whole call {grp[K][0] / base_ms:.2f} x hank_vjp_dev, Sweep A {grp[K][1]['sweep_a']['ms'] / base_t['sweep_a']['ms']:.2f} x hank_vjp_dev's")
print("\n".join(lines[-4:]), flush=True)
Path(a.out).parent.mkdir(parents=True, exist_ok=True)
Path(a.out).write_text("\n".join(lines) + "\n")
hb.set_stream(None)
hb.close()
