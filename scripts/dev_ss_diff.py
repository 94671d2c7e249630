#!/usr/bin/env python
"""Timings of hank_ss_jvp / hank_ss_vjp and of find_ss with the implicit price Jacobian, reported, not gated.

    python scripts/dev_ss_diff.py [--small] > profiles/ss_diff.log

Per economy (Krusell-Smith 2000x11 and the one-asset HANK 1000x7; --small: 50x2 and 30x3): steps and milliseconds of each of the
four loops at N = M = n_hh — medians of 5 calls after a warm-up, HIP events around each loop (hank_last_ss_timings: from before a
loop's first step to behind the synchronisation that fetched its last stop word) — beside the yardstick steps x (the launch
family's time per period), from hank_last_timings of a hank_jvp and hank_last_vjp_timings of a hank_vjp_het at the same width on the
same launch-schedule context. Then find_ss cold from the YAML guesses with price_jacobian = "implicit" against "fd"."""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def loops(hank, name, m, ss, x, n_het):
    import cases
    hb = cases.block(hank, m, "launch")
    hb.set_boundary(ss.value, ss.D)
    hb.set_het_outputs(n_het)
    P, n_hh = hb.P, hb.n_hh
    hb.primal(np.tile(np.asarray(x)[:, None], (1, P)))
    # the yardstick: one period of each launch-family sweep at this width
    rng = np.random.default_rng(0)
    y = rng.standard_normal((n_hh, P, n_hh)) * 1e-3
    yb = rng.standard_normal((P, n_het, n_hh))
    per = {k: [] for k in ("tangent_backward", "tangent_forward", "sweep_a", "sweep_b")}
    for it in range(6):
        hb.jvp(y)
        t = hb.last_timings()
        hb.vjp_het(yb, n_het)
        v = hb.last_vjp_timings()
        if it:
            for k in ("tangent_backward", "tangent_forward"):
                per[k].append(1e3 * t[k]["ms"] / t[k]["launches"])
            for k in ("sweep_a", "sweep_b"):
                per[k].append(1e3 * v[k]["ms"] / v[k]["launches"])
    us = {k: statistics.median(vv) for k, vv in per.items()}
    hb.primal(np.tile(np.asarray(x)[:, None], (1, P)))
    dx, ab = np.eye(n_hh), rng.standard_normal((n_het, n_hh))
    Vb, Db = rng.standard_normal((hb.G, n_hh)), rng.standard_normal((hb.G, n_hh))
    tj, tv = [], []
    for it in range(6):
        _, _, _, _, ij = hb.ss_jvp(dx, n_het=n_het)
        a = hb.last_ss_timings()
        _, iv = hb.ss_vjp(ab, Vb, Db, n_het=n_het)
        b = hb.last_ss_timings()
        if it:
            tj.append(a); tv.append(b)
    med = lambda ts, k: statistics.median(t[k] for t in ts)      # noqa: E731
    print(f"\n{name}: G = {hb.G}, N = M = n_hh = {n_hh}, n_het = {n_het}, tol 1e-13; launch family per period: backward tangent {us['tangent_backward']:.1f} us, "
          f"forward tangent {us['tangent_forward']:.1f} us, Sweep A {us['sweep_a']:.1f} us, Sweep B {us['sweep_b']:.1f} us")
    print("| loop | steps | ms (median of 5) | us per step | yardstick: steps x launch family per period, ms | ratio |")
    print("|---|---|---|---|---|---|")
    rows = (("JVP value (k_ss_back + check)", ij[0], med(tj, 0), us["tangent_backward"]), ("JVP distribution (k_ss_fwd + check, centring)", ij[1], med(tj, 1), us["tangent_forward"]),
            ("VJP lambda (k_ss_lam + check)", iv[1], med(tv, 1), us["sweep_a"]), ("VJP nu (k_ss_nu + check)", iv[0], med(tv, 0), us["sweep_b"]))
    for what, steps, ms, u in rows:
        print(f"| {what} | {steps} | {ms:.2f} | {1e3 * ms / steps:.2f} | {steps * u / 1e3:.2f} | {ms / (steps * u / 1e3):.2f} |")
    # the lambda loop centred once (the plain series) against re-centred every step, same cotangents, capped at 20 000 steps
    import os
    os.environ["HANK_SS_RECENTRE"] = "0"
    try:
        hb.ss_vjp(ab, Vb, Db, n_het=n_het, max_iter=20_000, check=False)
    finally:
        del os.environ["HANK_SS_RECENTRE"]
    once = hb.last_ss
    hb.ss_vjp(ab, Vb, Db, n_het=n_het, max_iter=20_000, check=False)
    print(f"lambda loop, g centred once (HANK_SS_RECENTRE=0): {once['iters'][1]} steps, last increment ratio {once['resid'][1]:.3e}; "
          f"re-centred every step: {hb.last_ss['iters'][1]} steps, {hb.last_ss['resid'][1]:.3e} (cap 20000, tol 1e-13; "
          f"|D_ss - Lambda D_ss| of the record: {np.abs(hb.dist_seq()[:, :, 0].reshape(-1, order='F') - np.asarray(ss.D).reshape(-1, order='F')).max():.2e})")
    hb.close()


def newton(hank, name, make_model, spec_of):
    print(f"\n{name}: find_ss cold from the YAML guesses")
    print("| price Jacobian | wall s | VFI steps | Newton iterations | residual norm |")
    print("|---|---|---|---|---|")
    out = {}
    for pj in ("fd", "implicit"):
        m = make_model()
        t0 = time.perf_counter()
        try:
            ss = hank.find_ss(m, spec_of(m), "initial", vfi="device", price_jacobian=pj)
        except Exception as e:      # noqa: BLE001  (reported, not gated)
            print(f"| {pj} | failed: {type(e).__name__}: {e} | | | |")
            continue
        el = time.perf_counter() - t0
        out[pj] = (el, ss)
        si = ss.solve_info
        print(f"| {pj} | {el:.2f} | {si['vfi_steps']} | {si['newton_iterations']} | {si['residual_norm']:.2e} |")
    if len(out) == 2:
        d = max(abs(out["fd"][1].vars[k] - out["implicit"][1].vars[k]) for k in out["fd"][1].vars)
        print(f"largest difference of a steady-state variable between the two: {d:.2e}; implicit / fd wall time {out['implicit'][0] / out['fd'][0]:.2f}"
              + ("" if out["implicit"][0] < out["fd"][0] else "  — implicit is NOT faster here; \"fd\" stays the default"))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    import hank_amd as hank
    import hank_amd.parallel  # noqa: F401
    import cases
    from conftest import ks_setup
    ks, hk = ((50, 2, 100), (30, 3, 40)) if a.small else ((2000, 11, 300), (1000, 7, 300))
    m, ss, _ = ks_setup(*ks)
    loops(hank, f"Krusell-Smith {ks[0]}x{ks[1]}", m, ss, [ss.vars["r"], ss.vars["w"]], 3)
    mh, ssh = cases.hank_economy(*hk, "one_asset_hank.yaml")
    loops(hank, f"one-asset HANK {hk[0]}x{hk[1]}", mh, ssh, [ssh.vars[k] for k in mh.value_fn.household_inputs], 4)
    ov = {"T": ks[2], "dimensions": {"wealth": {"n": ks[0]}, "productivity": {"n": ks[1]}}}
    newton(hank, f"Krusell-Smith {ks[0]}x{ks[1]}", lambda: hank.build_model_from_yaml(str(ROOT / "examples" / "krusell_smith.yaml"), overrides=ov), lambda mm: mm.ss_initial)

    def hank_model():
        from hank_amd import OneAssetHANK as oa
        ovh = {"T": hk[2], "dimensions": {"wealth": {"n": hk[0]}, "productivity": {"n": hk[1]}}}
        mm = hank.build_model_from_yaml(str(ROOT / "examples" / "one_asset_hank.yaml"), overrides=ovh)
        mm.params.B = oa.calibrate_bond_supply(mm)
        return mm

    newton(hank, f"one-asset HANK {hk[0]}x{hk[1]}", hank_model, lambda mm: mm.ss_initial)
