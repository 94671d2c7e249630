"""The CPU reference of the group outputs (hank_get_group_outputs), shared by tests/test_group_outputs_host.py and
tests/test_gpu_group_outputs.py: the oracle's own BackwardIteration, the c_grid of KrusellSmith.jl:79 as a policy, and
orc_forward_iteration_het, which dots every sequence it is handed with the same post-transition D_t (ForwardIteration.jl:303-307)
and pushes D with sequence 0 — so the savings policy comes first in the list and the weighted sequences W·1, W·a', W·c behind it.
Nothing is added to the reference's semantics: a weight is a constant factor on a policy sequence."""
import numpy as np

MASS, POLICY, CONS = 0, 1, 2
EDGES = (0.0, 0.2, 0.5, 0.9, 1.0)          # the wealth groups of the Krusell-Smith 130x3 case
_REFS = {}


def group_reference(orc, xhh, y, value, D, W, base):
    """agg (K, P), dagg (K, P, N) of the groups W (G, K) with bases base[K] at xhh (n_hh, P) under the partials y (n_hh, P, N <= 32;
    None: the values alone, dagg (K, P, 0)). Row 2 of xhh / y is the transfer path when n_hh > 2."""
    W = np.asarray(W, dtype=np.float64)
    base = np.broadcast_to(np.asarray(base), (W.shape[1],))
    (n, Nc, xd), = orc._seeded(xhh, y)
    xt = xd[2] if len(xd) > 2 else None
    st, pol = orc.backward_iteration(xd[0], xd[1], value, Nc, xt)
    assert st == 0, st
    ps = np.ascontiguousarray(pol.transpose(0, 2, 1, 3))        # [t][e][a][1+N]
    cons = orc._consumption(xd[0], xd[1], xt, ps, Nc)
    one = np.zeros_like(ps)
    one[..., 0] = 1.0                                           # MASS: value 1, zero partials
    f = {MASS: one, POLICY: ps, CONS: cons}
    seqs = [ps]                                                 # (sequence 0 pushes D)
    for k, b in enumerate(base):
        Wk = W[:, k].reshape(orc.n_e, orc.n_a)                  # pt = e n_a + ia -> [e][a]
        seqs.append(Wk[None, :, :, None] * f[int(b)])
    agg = orc._aggregate(seqs, D, Nc)[1:]
    return agg[..., 0], agg[..., 1:1 + n]


def ks_groups():
    """the twelve outputs of the Krusell-Smith 130x3 case: wealth groups at EDGES, every base. -> (W (G, 12), base (12,)), output
    3 b + g is group g under base b."""
    from conftest import ks_setup
    from hank_amd.groups import wealth_groups
    m, ss, _ = ks_setup(130, 3, 40)
    Wg = wealth_groups(ss.D, 130, 3, EDGES)
    K = Wg.shape[1]
    return np.concatenate([Wg, Wg, Wg], axis=1), np.repeat(np.array([MASS, POLICY, CONS], dtype=np.int32), K)


def ks_reference(N, seed=3):
    """(xhh (2, 39), y (2, 39, N), W, base, agg (12, 39), dagg (12, 39, N)) of the Krusell-Smith 130x3, T = 40 case on the x1 path
    (shock 0.05): computed once per width, shared, never written to. The oracle covers the first 32 columns; the directions
    behind them are combinations C (32, N - 32) of those 32 (coefficients N(0, 1) / sqrt(32): columns of the same size), so their
    reference follows by linearity, dagg[..., 32:] = dagg[..., :32] C."""
    key = ("ks130", N, seed)
    if key not in _REFS:
        from conftest import ks_paths, ks_setup
        m, ss, orc = ks_setup(130, 3, 40)
        x, _ = ks_paths(m, ss, "x1", 0.05)
        xhh = np.ascontiguousarray(x[2:4])
        rng = np.random.default_rng(seed)
        y = rng.standard_normal((2, xhh.shape[1], min(N, 32)))
        W, base = ks_groups()
        agg, dagg = group_reference(orc, xhh, y, ss.value, ss.D, W, base)
        if N > 32:
            C = rng.standard_normal((32, N - 32)) / np.sqrt(32.0)
            y, dagg = np.concatenate([y, y @ C], axis=2), np.concatenate([dagg, dagg @ C], axis=2)
        for a in (xhh, y, W, base, agg, dagg):
            a.setflags(write=False)
        _REFS[key] = (xhh, y, W, base, agg, dagg)
    return _REFS[key]


def nontrivial(agg, dagg, what=""):
    """every output's reference exceeds 1e-2 in value and 1e-1 in tangent (measured: >= 2e-2 and >= 1.4 on the Krusell-Smith case)"""
    for k in range(agg.shape[0]):
        va, vd = np.abs(agg[k]).max(), np.abs(dagg[k]).max()
        print(f"{what} output {k}: max |value| {va:.3e}, max |tangent| {vd:.3e}")
        assert va > 1e-2 and vd > 1e-1, (what, k, va, vd)
