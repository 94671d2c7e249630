#!/usr/bin/env python
"""dev: the timed quantities of the kernels built on the shared step bodies of csrc/hank_device.h, for one library per call, and the
comparison of two series of calls (profiles/shared_step_bodies.txt).

    HANK_HIP_LIB=/other/tree/libhank_hip.so python scripts/dev_time_bodies.py measure >> parent.jsonl      # alternate the two,
    python scripts/dev_time_bodies.py measure >> this.jsonl                                                 # five times each
    python scripts/dev_time_bodies.py compare parent.jsonl this.jsonl

measure, at the bench workload's grid (Krusell-Smith 2000x11, T = 300), one JSON line of medians over 5 calls after a warm-up:
    sweep_a / sweep_b of hank_vjp at M = 32 and M = 1 (hank_last_vjp_timings, ms);
    the two loops of hank_ss_vjp at M = 4, all three cotangents, at that grid's steady state (hank_last_ss_timings / iters, us per step);
    the two chains of hank_primal_batch at K = 8 (hank_last_batch_timings, ms).
compare: per quantity both series, their medians and the first series' spread (max - min); a quantity passes when the second
median is no higher than the first median plus that spread. Lines {"bench_ms_per_step": ...} (bench.py's result) may be mixed in."""
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def measure():
    import hank_amd as hank
    import cases
    from conftest import ks_paths, ks_setup
    m, ss, _ = ks_setup(2000, 11, 300)
    hb = cases.block(hank, m, None)
    hb.set_boundary(ss.value, ss.D)
    hb.set_het_outputs(3)
    P, G = hb.P, hb.G
    xp = np.ascontiguousarray(ks_paths(m, ss, "x1", 0.01)[0][2:4])
    xs = np.tile(np.array([ss.vars["r"], ss.vars["w"]])[:, None], (1, P))
    rng = np.random.default_rng(0)
    med = lambda v: statistics.median(v)      # noqa: E731
    out = {}
    hb.primal(xp)
    for M in (32, 1):
        yb = rng.standard_normal((P, 2, M))
        ts = []
        for it in range(6):
            hb.vjp(yb, 2)
            ts.append(hb.last_vjp_timings())
        for k in ("sweep_a", "sweep_b"):
            out[f"vjp_M{M}_{k}_ms"] = med(t[k]["ms"] for t in ts[1:])
    xb = np.stack([xp * (1.0 + 1e-4 * k) for k in range(8)], axis=2)
    ts = []
    for it in range(6):
        hb.primal_batch(xb, 3)
        ts.append(hb.last_batch_timings())
    out["batch_K8_backward_ms"], out["batch_K8_forward_ms"] = med(t[0] for t in ts[1:]), med(t[1] for t in ts[1:])
    hb.primal(xs)
    cot = (rng.standard_normal((3, 4)), rng.standard_normal((G, 4)), rng.standard_normal((G, 4)))
    ts = []
    for it in range(6):
        _, iters = hb.ss_vjp(*cot, n_het=3)
        ms = hb.last_ss_timings()
        ts.append((1e3 * ms[0] / iters[0], 1e3 * ms[1] / iters[1]))
    out["ss_vjp_M4_nu_us_per_step"], out["ss_vjp_M4_lambda_us_per_step"] = med(t[0] for t in ts[1:]), med(t[1] for t in ts[1:])
    out["ss_vjp_M4_iters"] = list(iters)
    hb.close()
    print(json.dumps(out), flush=True)


def compare(pa, pb):
    def series(p):
        s = {}
        for line in Path(p).read_text().splitlines():
            if line.startswith("{"):
                for k, v in json.loads(line).items():
                    if isinstance(v, (int, float)):
                        s.setdefault(k, []).append(float(v))
        return s
    a, b = series(pa), series(pb)
    bad = 0
    for k in a:
        if k not in b:
            continue
        ma, mb, spread = statistics.median(a[k]), statistics.median(b[k]), max(a[k]) - min(a[k])
        ok = mb <= ma + spread
        bad += not ok
        print(f"{k}\n    A {' '.join(f'{v:.4f}' for v in a[k])}\n    B {' '.join(f'{v:.4f}' for v in b[k])}\n"
              f"    median A {ma:.4f}, B {mb:.4f}; spread of A {spread:.4f}; B - A {mb - ma:+.4f}: {'passes' if ok else 'FAILS'}")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "measure":
        measure()
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
