#!/usr/bin/env python
"""dev: what every entry that runs a kernel built on the shared step bodies of csrc/hank_device.h returns, as bytes, so that two
builds of the library can be compared (profiles/shared_step_bodies.txt, profiles/shared_step_bodies_dump_cmp.txt).

    python scripts/dev_dump_bits.py prepare IN.npz                                    # no GPU
    HANK_HIP_LIB=/other/tree/libhank_hip.so python scripts/dev_dump_bits.py dump IN.npz A.npz
    python scripts/dev_dump_bits.py dump IN.npz B.npz
    python scripts/dev_dump_bits.py cmp A.npz B.npz                                   # exit status 1 if any byte differs

prepare: the suite's economies with their boundaries (tests/ss_diff_cases.py: steady states of the CPU oracle; tests/cases.py:
EDGE_GRIDS, deep clamped prefixes and flat tops), T <= 13. dump, per economy, same seeds under every library:
  hank_vjp, hank_vjp_het (every count of outputs), hank_vjp_het_boundary, each with the policy cotangent sequence: M = 1, 2, 3, 4, 7,
      16, 33, 34 on ks50x2 and hank30x3, M = 1, 4, 32, 33 on the EDGE_GRIDS economies
  hank_ss_vjp: M = 1, 2, 3, 7, 16, 32, 34 x {agg, value, D, all} on six economies, with iters and resid
  hank_ss_jvp: N = 1, 3, 4, 33, every count of outputs, on ks30x3 and hank30x3
  hank_primal under every forced schedule (and the default): aggregates, policies, distributions, every output, their tangents
      after hank_jvp at N = 3, and the Dual pass (hank_primal_jvp, whose lottery writes no segment records) on ks30x3, hank30x3, clamp
  hank_stationary_dist, hank_vfi from a perturbed value (ks30x3, hank30x3), hank_primal_batch (K = 1, 3, every count of outputs, policies), hank_jvp_het with both boundary seeds
An entry that raises leaves its message in place of its arrays."""
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

SS_NAMES = ("ks50x2", "ks30x3", "hank30x3", "clamp", "ks40x16", "gamma3")
VJP_WIDTHS = (1, 2, 3, 4, 7, 16, 33, 34)
EDGE_WIDTHS = (1, 4, 32, 33)
SS_VJP_WIDTHS = (1, 2, 3, 7, 16, 32, 34)
SS_JVP_WIDTHS = (1, 3, 4, 33)
MODES = {"agg": (1, 0, 0), "value": (0, 1, 0), "D": (0, 0, 1), "all": (1, 1, 1)}
SCHEDULES = (None, "launch", "xcd", "wide")


def prepare(path):
    import cases
    import ss_diff_cases as S
    out = {}

    def put(name, args, V, D, x, n_het):
        grid, z, Pi, beta, gamma, bc, T, vf = args
        out.update({f"{name}/grid": grid, f"{name}/z": z, f"{name}/Pi": Pi, f"{name}/prefs": np.array([beta, gamma, bc]),
                    f"{name}/ints": np.array([T, vf, n_het]), f"{name}/V": V, f"{name}/D": D, f"{name}/x": x})

    for name in SS_NAMES:
        c = S.case(name)
        put(name, c["args"], c["V"], c["D"], c["x"], c["n_het"])
    for name in cases.EDGE_GRIDS:
        ec = cases.raw_economy(name)
        put("edge-" + name, ec["args"], ec["V"], ec["D"], ec["x"], 3)
    np.savez(path, **{k: np.asarray(v, dtype=np.int64 if k.endswith("/ints") else np.float64) for k, v in out.items()})


class Economy:
    def __init__(self, g, name):
        f = lambda k: g[f"{name}/{k}"]      # noqa: E731
        T, vf, self.n_het = (int(v) for v in f("ints"))
        beta, gamma, bc = (float(v) for v in f("prefs"))
        self.name, self.args, self.V, self.D, self.x = name, (f("grid"), f("z"), f("Pi"), beta, gamma, bc, T, vf), f("V"), f("D"), f("x")

    def block(self, hank, schedule=None):
        import cases
        hb = cases.raw_block(hank, self.args, schedule)
        hb.set_boundary(self.V, self.D)
        hb.set_het_outputs(self.n_het)
        return hb

    def path(self, P, moving=True):
        """the household inputs (n_hh, P): the recorded path of an EDGE_GRIDS economy; else the steady state's prices, constant, or
        with a geometric deviation"""
        if self.x.ndim == 2:
            return self.x
        return self.x[:, None] * (1.0 + (0.01 * 0.8 ** np.arange(P) if moving else np.zeros(P)))


def dump(inputs, path):
    import hank_amd as hank
    g = np.load(inputs)
    out = {}

    def fail(key, e):
        out[f"{key}/error"] = np.frombuffer(f"{type(e).__name__}: {e}".encode(), dtype=np.uint8)

    def group(key, fn):
        try:
            for k, v in fn().items():
                out[f"{key}/{k}"] = np.asarray(v)
        except Exception as e:      # noqa: BLE001  (the message is the entry's output)
            fail(key, e)

    def vjps(ec, widths):
        print(f"{ec.name}: vjp", flush=True)
        hb = ec.block(hank)
        P = hb.P
        hb.primal(ec.path(P))
        for M in widths:
            rng = np.random.default_rng(M)
            for n_het in range(1, ec.n_het + 1):
                yb = rng.standard_normal((P, n_het, M))
                if n_het <= 2:
                    group(f"{ec.name}/vjp/M{M}/h{n_het}", lambda: {"xbar": hb.vjp(yb, n_het), "pbar": hb.policy_cotangent_seq(M)})
                group(f"{ec.name}/vjp_het/M{M}/h{n_het}", lambda: {"xbar": hb.vjp_het(yb, n_het), "pbar": hb.policy_cotangent_seq(M)})
            group(f"{ec.name}/vjp_het_boundary/M{M}",
                  lambda: dict(zip(("xbar", "Vbar", "Dbar", "pbar"), hb.vjp_het_boundary(yb, ec.n_het) + (hb.policy_cotangent_seq(M),))))
        hb.close()

    def steady(ec):
        print(f"{ec.name}: steady state", flush=True)
        hb = ec.block(hank)
        hb.primal(ec.path(hb.P, moving=False))
        n_hh = hb.n_hh
        for M in SS_VJP_WIDTHS:
            rng = np.random.default_rng(200 + M)
            cot = (rng.standard_normal((ec.n_het, M)), rng.standard_normal((hb.G, M)), rng.standard_normal((hb.G, M)))
            for mode, on in MODES.items():
                def one():
                    xbar, iters = hb.ss_vjp(*(c if w else None for c, w in zip(cot, on)), n_het=ec.n_het)
                    return {"xbar": xbar, "iters": iters, "resid": hb.last_ss["resid"]}
                group(f"{ec.name}/ss_vjp/M{M}/{mode}", one)
        if ec.name in ("ks30x3", "hank30x3"):
            for N in SS_JVP_WIDTHS:
                dx = np.random.default_rng(100 + N).standard_normal((n_hh, N))
                for n_het in range(1, ec.n_het + 1):
                    def one():
                        dagg, dV, dpol, dD, iters = hb.ss_jvp(dx, n_het=n_het)
                        return {"dagg": dagg, "dV": dV, "dpol": dpol, "dD": dD, "iters": iters, "resid": hb.last_ss["resid"]}
                    group(f"{ec.name}/ss_jvp/N{N}/h{n_het}", one)
        hb.close()

    def primals(ec):
        for sched in SCHEDULES:
            print(f"{ec.name}: primal under schedule {sched}", flush=True)
            key = f"{ec.name}/primal/{sched}"
            try:
                hb = ec.block(hank, sched)
            except Exception as e:      # noqa: BLE001
                fail(key, e)
                continue
            P, n_hh = hb.P, hb.n_hh
            xp = ec.path(P)
            y = np.random.default_rng(3).standard_normal((n_hh, P, 3)) * 1e-3
            group(key, lambda: {"agg": hb.primal(xp), "policy": hb.policy_seq(), "D": hb.dist_seq(), "het": hb.het_outputs(ec.n_het)[0]})
            group(key + "/jvp", lambda: dict(zip(("dagg", "het", "dhet"), (hb.jvp(y),) + hb.het_outputs(ec.n_het, y))))
            group(key + "/dual", lambda: dict(zip(("agg", "dagg", "policy", "D"), hb.primal_jvp(xp * 1.001, y) + (hb.policy_seq(), hb.dist_seq()))))
            if sched is None:
                def stat():
                    D, steps = hb.stationary_dist(hb.policy_seq()[:, :, 0], max_iter=20_000)
                    return {"D": D, "steps": steps}
                group(f"{ec.name}/stationary_dist", stat)
                if ec.name in ("ks30x3", "hank30x3"):
                    def vfi():
                        V, pol, steps, supnorm = hb.vfi(ec.V * 1.01, xp[:, 0], tol=1e-10, max_iter=5000)
                        return {"V": V, "policy": pol, "steps": steps, "supnorm": supnorm}
                    group(f"{ec.name}/vfi", vfi)
                for K in (1, 3):
                    xs = np.stack([xp * (1.0 + 0.001 * k) for k in range(K)], axis=2)
                    for n_het in range(1, ec.n_het + 1):
                        group(f"{ec.name}/primal_batch/K{K}/h{n_het}", lambda: dict(zip(("aggs", "status", "policies"), hb.primal_batch(xs, n_het, policy=True))))
                rng = np.random.default_rng(5)
                dv, dd = rng.standard_normal((hb.n_a, hb.n_e, 3)), rng.standard_normal((hb.n_a, hb.n_e, 3)) * 1e-3
                hb.primal(xp)
                group(f"{ec.name}/jvp_het", lambda: {"dagg": hb.jvp_het(y, dv, dd - dd.mean(axis=(0, 1)), n_het=ec.n_het)})
            hb.close()

    for name in ("ks50x2", "hank30x3"):
        vjps(Economy(g, name), VJP_WIDTHS)
    for name in sorted(k[:-5] for k in g.files if k.startswith("edge-") and k.endswith("/grid")):
        vjps(Economy(g, name), EDGE_WIDTHS)
    for name in SS_NAMES:
        steady(Economy(g, name))
    for name in ("ks30x3", "hank30x3", "clamp"):
        primals(Economy(g, name))
    np.savez(path, **out)
    errs = [k for k in out if k.endswith("/error")]
    print(f"{len(out)} arrays under {os.environ.get('HANK_HIP_LIB') or 'the tree library'} -> {path}; {len(errs)} entries raised")
    for k in errs:
        print(f"  {k}: {out[k].tobytes().decode()}")


def cmp(pa, pb):
    a, b = np.load(pa), np.load(pb)
    names = sorted(set(a.files) | set(b.files))
    lines, bad = [], 0
    for k in names:
        if k not in a.files or k not in b.files:
            lines.append(f"MISSING    {k}  only in {pa if k in a.files else pb}")
            bad += 1
            continue
        u, v = a[k], b[k]
        same = u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes()
        bad += not same
        note = ""
        if k.endswith("/error"):
            note = " " + u.tobytes().decode()
        elif k.endswith("/iters") or k.endswith("/steps"):
            note = f" {u.tolist()}"
        elif not same and u.shape == v.shape:
            note = f" max |a - b| {np.max(np.abs(u.astype(np.float64) - v.astype(np.float64))):.3e}"
        lines.append(f"{'identical' if same else 'DIFFERS  '}  {k}  {u.dtype}{list(u.shape)}{note}")
    print(f"# {len(names)} arrays dumped under two libraries, same driver script and inputs: {len(names) - bad} byte-identical, {bad} differ")
    print("\n".join(lines))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "prepare":
        prepare(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "dump":
        dump(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 4 and sys.argv[1] == "cmp":
        sys.exit(cmp(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
