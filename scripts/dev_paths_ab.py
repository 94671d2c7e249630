#!/usr/bin/env python
"""dev: host overhead of the path entries — hank_jvp_shock_dev, hank_jvp_income_dev, hank_vjp_shock_dev, hank_vjp_income_dev — at
Krusell-Smith 2000x11, T = 300, N = M = 32 (n_het = 2), for one library or for two against each other (profiles/path_owner_ab.log).

    python scripts/dev_paths_ab.py                                   # the library in force (HANK_HIP_LIB, or the tree's): one JSON line
    python scripts/dev_paths_ab.py --ab PARENT.so [--rounds 3] [--log profiles/path_owner_ab.log]

One measurement: a context at a recorded primal, no path set; per entry 3 warm-up calls (allocation, graph capture), then BLOCKS
blocks of REPS calls. Per block: the time until the REPS asynchronous calls have returned (enqueue) and until the stream has drained
(wall), both per call, and the sweeps' milliseconds of the block's last call (hank_last_timings / hank_last_vjp_timings).
--ab: PARENT.so and the tree's library measured alternately, each round in a fresh process of its own; per entry and figure the
parent's spread (min .. max over all its blocks) and median and the change's median — the margin is the parent's own spread."""
import argparse
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
REPS, BLOCKS, N = 20, 5, 32


def measure():
    import torch
    torch.cuda.init()       # before libhank_hip loads its HIP runtime (the other order leaves torch without a device)
    sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
    import hank_amd as h
    from conftest import ks_paths, ks_setup
    m, ss, _ = ks_setup(2000, 11, 300)
    x, _ = ks_paths(m, ss, "x1", 0.01)
    hb = h.household_block(m)
    hb.set_boundary(ss.value, ss.D)
    hb.primal(np.asfortranarray(x[2:4]))
    P, ne, nh, dev = hb.P, hb.n_e, hb.n_hh, torch.device("cuda", 0)
    rand = lambda n: torch.randn(n, dtype=torch.float64, device=dev)      # noqa: E731
    empty = lambda n: torch.empty(n, dtype=torch.float64, device=dev)     # noqa: E731
    dx, db, dy, out = rand(nh * P * N) * 1e-2, rand(P * N) * 1e-2, rand(ne * P * N) * 1e-2, empty(P * N)
    yb, xbar, bbar, ybar = rand(P * 2 * N), empty(nh * P * N), empty(P * N), empty(ne * P * N)
    p = lambda t: t.data_ptr()      # noqa: E731
    tan = lambda: {k: v["ms"] for k, v in hb.last_timings().items() if k.startswith("tangent")}      # noqa: E731
    cot = lambda: {k: v["ms"] for k, v in hb.last_vjp_timings().items()}                             # noqa: E731
    entries = {
        "jvp_shock_dev": (lambda: hb.jvp_shock_dev(p(dx), p(db), N, p(out)), tan),
        "jvp_income_dev": (lambda: hb.jvp_income_dev(p(dx), p(dy), N, p(out)), tan),
        "vjp_shock_dev": (lambda: hb.vjp_shock_dev(2, p(yb), N, p(xbar), p(bbar)), cot),
        "vjp_income_dev": (lambda: hb.vjp_income_dev(2, p(yb), N, p(xbar), p(ybar)), cot),
    }
    res = {}
    for name, (call, sweeps) in entries.items():
        for _ in range(3):
            call()
        hb.check()
        blocks = []
        for _ in range(BLOCKS):
            t0 = time.perf_counter()
            for _ in range(REPS):
                call()
            t1 = time.perf_counter()
            hb.sync()
            t2 = time.perf_counter()
            blocks.append(dict(enqueue_ms=1e3 * (t1 - t0) / REPS, wall_ms=1e3 * (t2 - t0) / REPS, **sweeps()))
        res[name] = blocks
    hb.check()
    hb.close()
    print("PATHS_AB " + json.dumps(res), flush=True)


def child(lib):
    env = dict(os.environ)
    if lib:
        env["HANK_HIP_LIB"] = str(lib)
    else:
        env.pop("HANK_HIP_LIB", None)
    r = subprocess.run([sys.executable, __file__], env=env, capture_output=True, text=True, timeout=600)
    line = next((l for l in r.stdout.splitlines() if l.startswith("PATHS_AB ")), None)
    if r.returncode != 0 or line is None:
        sys.exit(f"measurement of {lib or 'the tree library'} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
    return json.loads(line[len("PATHS_AB "):])


def ab(parent, rounds, log):
    lines = [f"# scripts/dev_paths_ab.py --ab {Path(parent).name} --rounds {rounds}: KS 2000x11, T=300, N=M={N}, n_het=2; parent and change alternating, a fresh",
             f"# process per round; per block {REPS} calls, {BLOCKS} blocks per round after 3 warm-up calls; ms per call. spread: min .. max over the parent's own blocks"]
    runs = {"parent": [], "change": []}
    for r in range(rounds):
        for who, lib in (("parent", parent), ("change", None)):
            res = child(lib)
            runs[who].append(res)
            for name, blocks in res.items():
                lines.append(f"{who} round {r + 1} {name}: " + " | ".join(" ".join(f"{k}={v:.4f}" for k, v in b.items()) for b in blocks))
    lines.append("# summary: entry figure: parent spread min .. max, parent median, change median, change median inside the parent's spread")
    for name in runs["parent"][0]:
        for fig in runs["parent"][0][name][0]:
            pv = np.array([b[fig] for res in runs["parent"] for b in res[name]])
            cv = np.array([b[fig] for res in runs["change"] for b in res[name]])
            cm = float(np.median(cv))
            lines.append(f"{name} {fig}: parent {pv.min():.4f} .. {pv.max():.4f}, parent median {np.median(pv):.4f}, change median {cm:.4f}, "
                         f"inside {'yes' if pv.min() <= cm <= pv.max() else 'NO'}")
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if log:
        Path(log).write_text(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", metavar="PARENT.so", help="measure this library against the tree's")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--log")
    a = ap.parse_args()
    if a.ab:
        ab(a.ab, a.rounds, a.log)
    else:
        measure()
