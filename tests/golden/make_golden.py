"""Generates tests/golden/*.npz. The reference holds NO golden vectors for this path and cannot be
run here (no Julia), so these vectors are produced by the CPU oracle (oracle/hank_oracle.c) — they
freeze the restated semantics (regression anchor for the oracle, parity target for the HIP path);
they are not reference outputs ("parity unpinned" in that sense).

    python tests/golden/make_golden.py

`python tests/golden/make_golden.py ref` writes ref_cppdual_ops.npz instead: the outputs of the reference's own C++
dual classes (oracle/_ref, built by `make -C oracle ref` where the reference sources are present) on the inputs
tests/test_oracle_dual_vs_ref.py draws, so that test runs without the reference.
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
from conftest import ks_paths, ks_setup  # noqa: E402


def main():
    out = Path(__file__).resolve().parent
    m, ss, orc = ks_setup(30, 3, 25)
    P, N = m.compspec.T - 1, 3
    x, Z = ks_paths(m, ss, "x1", 0.05)
    rng = np.random.default_rng(2024)
    y = rng.standard_normal((4, P, N))
    xd = np.zeros((4, P, 1 + N)); xd[..., 0] = x; xd[..., 1:] = y
    st, F, agg = orc.ks_full_function(xd, Z, m.params.α, m.params.δ, ss.vars["KS"], ss.value, ss.D, N)
    assert st == 0
    xr = np.ascontiguousarray(xd[2]); xw = np.ascontiguousarray(xd[3])
    st, pol = orc.backward_iteration(xr, xw, ss.value, N)
    _, Dseq = orc.forward_iteration(pol, ss.D, N, return_D=True)
    wd, pd_ = m.heterogeneity["wealth"], m.heterogeneity["productivity"]
    np.savez_compressed(out / "ks_30x3_T25_N3.npz", a_grid=wd.grid, z_grid=pd_.grid, Pi=pd_.transition,
                        beta=m.params.β, gamma=m.params.γ, borrow_cons=m.params.borrow_cons, alpha=m.params.α,
                        delta=m.params.δ, T=m.compspec.T, ss_value=ss.value, ss_D=ss.D, KS_ss=ss.vars["KS"],
                        x=x, Z=Z, y=y, F=F, agg=agg, policy_seq=pol, D_last=Dseq[-1])

    # granular forward step: clamps, exact grid hits (searchsortedfirst ties), non-monotone policy
    grid = wd.grid
    pol_e = rng.uniform(-1.0, grid[-1] + 5.0, (30, 3))
    pol_e[0, 0] = grid[0]; pol_e[1, 0] = grid[5]; pol_e[2, 0] = grid[-1]; pol_e[3, 1] = grid[0] - 1.0
    pol_e[4, 2] = grid[-1] + 1.0; pol_e[5, 2] = 0.5 * (grid[3] + grid[4])
    dpol_e = rng.standard_normal((30, 3, N))
    Dp = rng.uniform(0, 1, (30, 3)); Dp /= Dp.sum()
    dDp = rng.standard_normal((30, 3, N)) * 1e-2
    Dn = orc.transition_step(np.concatenate([pol_e[..., None], dpol_e], -1), np.concatenate([Dp[..., None], dDp], -1), N)
    np.savez_compressed(out / "forward_step_edge_30x3_N3.npz", policy=pol_e, dpolicy=dpol_e, D_prev=Dp, dD_prev=dDp, D_new=Dn)
    print("golden written")


def ref_cppdual():
    """reference C++ dual ops on the inputs of tests/test_oracle_dual_vs_ref.py (same seeds, same draw order)."""
    import ctypes as C
    from oracle import oracle
    lib = oracle.ref_lib()
    assert lib is not None, "oracle/_ref not built"
    dp = C.POINTER(C.c_double)
    arrays = {}
    for N, fname in ((1, "ref_dual1_op"), (3, "ref_dual3_op")):
        f = getattr(lib, fname)
        rng = np.random.default_rng(7)
        xs, ys, outs = [], [], []
        for _ in range(200):
            x, y = rng.standard_normal(1 + N), rng.standard_normal(1 + N)
            o = np.empty((5, 1 + N))
            for rop in range(5):
                r = np.empty(1 + N)
                f(rop, x.ctypes.data_as(dp), y.ctypes.data_as(dp), r.ctypes.data_as(dp))
                o[rop] = r
            xs.append(x); ys.append(y); outs.append(o)
        arrays[f"binop_n{N}_x"], arrays[f"binop_n{N}_y"], arrays[f"binop_n{N}_out"] = np.array(xs), np.array(ys), np.array(outs)
    rng = np.random.default_rng(3)
    xs, outs = [], []
    for _ in range(100):
        x = np.array([rng.uniform(0.1, 5.0), rng.standard_normal()])
        r = np.empty(2)
        lib.ref_dual1_op(5, x.ctypes.data_as(dp), x.ctypes.data_as(dp), r.ctypes.data_as(dp))
        xs.append(x); outs.append(r)
    arrays["sqrt_n1_x"], arrays["sqrt_n1_out"] = np.array(xs), np.array(outs)
    x = np.arange(10, dtype=np.float64)
    g = np.empty(10)
    lib.ref_rosenbrock_grad1(x.ctypes.data_as(dp), 10, g.ctypes.data_as(dp))
    arrays["rosenbrock_grad1_x"], arrays["rosenbrock_grad1"] = x, g
    np.savez_compressed(Path(__file__).resolve().parent / "ref_cppdual_ops.npz", **arrays)
    print("ref_cppdual_ops.npz written")


if __name__ == "__main__":
    if sys.argv[1:] == ["ref"]:
        ref_cppdual()
    else:
        main()
